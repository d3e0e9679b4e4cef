"""The observation kernels on junctions that are not a four-arm grid (tests/star_networks.py generates them).

On grid_6x6 and the bench grid every intersection has 12 roadLinks of one start lane each, at most 8 phases, 36 laneLinks, and no
lane ever holds more than about 40 vehicles: whole branches of laneFeatures, laneFlowTick and interFeatures
(csrc/hip/cfx_kernels.h) never run there.  Each network below exists for the branches named with it:

  star7  7 arms x 1 lane, arms of 300 / 150 / 60 / 800 / 300 / 25 / 300 m, a second signal S on arm 0
         interFeatures: 42 roadLinks = three trips of `m += kInterGroups` (the last a partial one); two mask words, so
         `mask[wd]` with wd = 1, `diff[wd * 32 + ..]` and interTables' `m / 32` packing; 12 phases at C beside 2 at S and 42
         roadLinks beside 2: the padding loops behind nRL and nPh see rows of different lengths.
         laneFeatures: the 800 m lane holds more than 64 vehicles — nReal = min(n, nFront) with n > K = 64, a walk that goes on
         behind the last front slot, more than four chunks; a 25 m lane.
         laneFlowTick: with the step counter moved far up, the lane's sum of `since` needs more than 32 bits
         (featShflXor64's high half, `(long long) f.step * left`).
  star5  5 arms of 1 / 2 / 3 / 5 / 2 lanes, arms of 300 / 300 / 700 / 300 / 120 m, the signal S on arm 0
         interFeatures: up to 5 in-lanes and 5 out-lanes per roadLink (the `inWaiting` loop over several in-lanes of one
         roadLink, lists longer than one entry), 126 laneLinks at C.
         laneFeatures / laneFlowTick: more than 64 vehicles on each of three parallel lanes; L = 28 lanes, a partial last block;
         the seed matters (every lane of the first road is a candidate), so a VectorEngine's environments differ.
  star3  3 arms of 18 / 1 / 2 lanes, intersection width 80
         interFeatures: in-lane and out-lane lists of 18 entries and 36 laneLinks in one roadLink: the second trip of the
         `j += kFeatGroup` loops.

Every oracle is one of the existing test modules' (built from the roadnet JSON and from getters that predate the features), fed
by the engine under test; the reference engine and the twin agree on these networks exactly (the first test), and the HIP engine
equals the twin state for state (the first gpu test) — the rest stands on those two.  Every test asserts that its run reached the
branch it is for: it fails rather than pass without having looked."""
import json
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_same_state, checkpoint_record, dump_json_exact

torch = pytest.importorskip("torch")

import star_networks  # noqa: E402
import test_intersection_features as ti  # noqa: E402
import test_lane_features as tf  # noqa: E402
import test_lane_flow as tl  # noqa: E402
import test_lane_fronts as tr  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_lane_flow import hip_engine  # noqa: E402

STARS = ("star7", "star5", "star3")
LAYOUTS = ("auto", "dense")


def star_config(workdir, name, layout="auto", seed=0):
    return star_networks.make(workdir, name, seed=seed, layout=layout)


# ------------------------------------------------------------------------------------------------- what a run must have reached
class StarSeen(ti.Seen):
    """Seen, and for star7: which roadLinks of C had vehicles on their in-lanes / inside the junction at a check, and whether
    the phase serving exactly the roadLinks >= 32 and the one serving only roadLinks < 32 ever showed different pressures."""

    def __init__(self, eng, name):
        super().__init__()
        self.name = name
        self.c = eng.intersection_ids().index("C")
        arms = star_networks.NETWORKS[name]["arms"]
        self.p_high, self.p_low = arms + 1, arms + 2  # (star_networks.phase_lists)
        self.m_in = self.m_inside = None
        self.pressures_differ = 0

    def add(self, want):
        super().add(want)
        row_in, row_inside = want["movement_in"][self.c] > 0, want["movement_inside"][self.c] > 0
        self.m_in = row_in if self.m_in is None else self.m_in | row_in
        self.m_inside = row_inside if self.m_inside is None else self.m_inside | row_inside
        hi, lo = (int(want["phase_pressure"][self.c, p]) for p in (self.p_high, self.p_low))
        self.pressures_differ += int(hi != ti.PAD and lo != ti.PAD and hi != lo)

    def check(self, phases_change=True):
        super().check(phases_change)
        if self.name != "star7":
            return
        for lo, hi in ((32, 42), (16, 32)):
            assert self.m_in[lo:hi].any(), "movement_in was zero in every checked row %d <= m < %d" % (lo, hi)
            assert self.m_inside[lo:hi].any(), "movement_inside was zero in every checked row %d <= m < %d" % (lo, hi)
        assert self.pressures_differ > 0, "the phase of the roadLinks >= 32 and the one of roadLinks < 32 never differed"


class StarLooked(tr.Looked):
    """Looked with the K = 64 condition, and whether the environments of a vector run ever held different lane counts."""

    def __init__(self):
        super().__init__(beyond_64=True)
        self.envs_differ = 0

    def at(self, lanes_per_env):
        super().at(lanes_per_env)
        counts = [[len(v) for v in lanes] for lanes in lanes_per_env]
        self.envs_differ += int(all(counts[a] != counts[b] for a in range(len(counts)) for b in range(a)) and len(counts) > 1)


def features_body(eng, steps, where):
    most = 0
    for s in range(steps):
        eng.next_step()
        if s % 50 == 49:
            tf.check_features(eng, tf.dict_oracle, "%s, step %d" % (where, s))
            most = max(most, int(eng.get_lane_vehicle_count_array().max()))
    assert most > 64, "no checked state had a lane with more than 64 vehicles (most: %d)" % most


# step numbers the snapshot is moved to, and what the fullest lane's sum of `since` must then exceed.  6 * 10^7: the sum of a
# lane with 72 vehicles or more needs a 33rd bit.  10^9: the sum exceeds 16 * 2^32, so the partial sums of the group's sixteen
# threads exceed 2^32 on average — the values that travel through the shuffles have a high half, not only their total.
LARGE_STEPS = ((60_000_000, 1 << 32), (1_000_000_000, 1 << 36))


def large_step_body(make, cfg, tmp_path, step, floor):
    eng = make(cfg)
    for s in range(300):
        eng.next_step()
    path = str(tmp_path / "star_snapshot.json")
    eng.snapshot().dump(path)
    with open(path) as f:
        doc = json.load(f)
    assert doc["step"] == 300
    doc["step"] = step
    dump_json_exact(doc, path)
    before = eng.get_lane_vehicles()
    eng.load_from_file(path)
    assert eng._scalars()["step"] == step and eng.get_lane_vehicles() == before
    eng.track_lane_flow(True)
    model = tl.Model(eng.lane_ids())
    model.baseline(eng.get_lane_vehicles(), step)
    since_sum = 0
    for s in range(60):
        eng.next_step()
        model.tick(eng.get_lane_vehicles(), eng.get_vehicle_speed(), step + s + 1)
        since_sum = max(since_sum, max(sum(r[0] for r in d.values()) for d in model.on))
        if s % 20 != 19:
            continue
        where = "step %d + %d" % (step, s + 1)
        want, got = model.outputs(), eng.observe_lane_flow_array()
        for k in tl.NAMES:
            assert got[k].dtype == tl.DTYPES[k] and np.array_equal(got[k], want[k]), "%s: %s differs" % (where, k)
        tr.check_fronts(eng, [tr.dict_lanes(eng, model, step + s + 1)], where, tracker=True, ks=(64,))
    assert since_sum > floor, "no lane's sum of since exceeded %d (most: %d)" % (floor, since_sum)
    assert want["left"].sum() > 0 and want["left_steps"].sum() > 0 and want["waiting_steps"].sum() > 0


def vector_star5(make_vec, make_single, workdir, layout="auto"):
    """Three environments of star5 in one VectorEngine, and the standalone engines with the seeds 0, 1 and 2."""
    singles = [make_single(star_config(workdir, "star5", layout, seed=e)) for e in range(3)]
    return make_vec(star_config(workdir, "star5", layout), 3), singles


def hip_vector_star5(mod, workdir, layout):
    """(VectorEngine reads the layout from the same config key as Engine but has no _layout(): hip_engine asserts it on the
    standalone engines, which are built from the same configs but for the seed.)"""
    return vector_star5(lambda c, n: mod.VectorEngine(c, n), lambda c: hip_engine(mod, c, layout), workdir, layout)


ENVS_NEVER_DIFFERED = "the three environments never held different lane counts at a check"


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
@pytest.mark.parametrize("name", STARS)
def test_star_reference_vs_twin(mod, workdir, ref_module, name):
    cfg = star_config(workdir, name)
    ref = ref_module.Engine(cfg, 1)
    tw = twin(mod, cfg)
    for s in range(500):
        ref.next_step()
        tw.next_step()
        if s % 10 == 9:
            assert checkpoint_record(tw) == checkpoint_record(ref), "%s step %d" % (name, s + 1)
    assert tw.get_vehicle_count() > 150 and tw._scalars()["finished_vehicle_count"] > 50
    assert ref.get_average_travel_time() == tw.get_average_travel_time()
    time.sleep(0.2)  # reference destructor race
    del ref


def test_layout_equals_the_roadnet_json(mod, workdir):
    for name in STARS:
        cfg = star_config(workdir, name)
        eng = twin(mod, cfg)
        tables = ti.Tables(eng, cfg)
        want, got = tables.layout(), eng.intersection_layout()
        assert sorted(got) == sorted(want), name
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, "%s: %s is %s %s" % (name, k, got[k].dtype, got[k].shape)
            assert np.array_equal(got[k], want[k]), "%s: %s differs" % (name, k)
        # the networks are what the module docstring says (from the JSON side)
        if name == "star7":
            assert (tables.M, tables.P) == (42, 12)
            assert {2, 42} <= set(want["n_roadlinks"].tolist()) and {2, 12} <= set(want["n_phases"].tolist())
            c = eng.intersection_ids().index("C")
            assert any(p and min(p) >= 32 for p in tables.phases[c]), "no phase serves only roadLinks >= 32"
            assert any(p and max(p) < 32 and len(p) > 1 for p in tables.phases[c])
        if name == "star5":
            assert want["in_lanes"].shape[-1] == 5 and want["out_lanes"].shape[-1] == 5 and len(eng.lane_ids()) == 28
            assert sum(len(rl["laneLinks"]) for it in ti.roadnet_of(cfg)["intersections"] if it["id"] == "C" for rl in it["roadLinks"]) == 126
        if name == "star3":
            assert want["in_lanes"].shape[-1] == 18 and want["out_lanes"].shape[-1] == 18
            assert max(len(rl["laneLinks"]) for it in ti.roadnet_of(cfg)["intersections"] for rl in it["roadLinks"]) == 36


@pytest.mark.parametrize("name", STARS)
def test_intersections_equal_the_oracle_twin(mod, workdir, name):
    cfg = star_config(workdir, name)
    eng = twin(mod, cfg)
    ti.run_against_oracle(eng, cfg, 300, 25, name, seen=StarSeen(eng, name))


@pytest.mark.parametrize("name", STARS)
def test_fronts_equal_the_dict_oracle_twin(mod, workdir, name):
    looked = StarLooked() if name != "star3" else None  # (star3's lanes stay below 64 vehicles)
    tr.run_against_dict_oracle(twin(mod, star_config(workdir, name)), 400, 25, name, tracker=True, fused=True, looked=looked)


@pytest.mark.parametrize("name", STARS)
def test_lane_flow_equals_the_model_twin(mod, workdir, name):
    eng = twin(mod, star_config(workdir, name))
    tl.run_against_model(eng, eng, 400, name)


@pytest.mark.parametrize("name", STARS)
def test_lane_features_equal_the_dict_oracle_twin(mod, workdir, name):
    eng = twin(mod, star_config(workdir, name))
    if name != "star3":
        features_body(eng, 350, name)
    else:  # (star3's lanes stay below 64 vehicles)
        for s in range(150):
            eng.next_step()
            if s % 50 == 49:
                tf.check_features(eng, tf.dict_oracle, "%s, step %d" % (name, s))
        assert eng.get_lane_vehicle_count_array().max() > 16


def test_vector_engine_equals_standalone_twins(mod, workdir):
    vec, singles = vector_star5(lambda c, n: mod.VectorEngine._with_backend(c, n, 1, TWIN_LIB), lambda c: twin(mod, c), workdir)
    looked = StarLooked()
    tr.vector_body(vec, singles, 300, 50, looked=looked)
    assert looked.envs_differ > 0, ENVS_NEVER_DIFFERED


@pytest.mark.parametrize("step, floor", LARGE_STEPS)
def test_large_step_numbers_twin(mod, workdir, tmp_path, step, floor):
    large_step_body(lambda cfg: twin(mod, cfg), star_config(workdir, "star7"), tmp_path, step, floor)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", STARS)
def test_hip_state_equals_twin(mod, workdir, name, layout):
    cfg = star_config(workdir, name, layout)
    eng, tw = hip_engine(mod, cfg, layout), twin(mod, cfg)
    for s in range(400):
        eng.next_step()
        tw.next_step()
        if s % 10 == 9:
            assert_same_state(eng, tw, "%s %s, step %d" % (name, layout, s + 1))
    assert eng.get_vehicle_count() > 150 and eng.get_lane_vehicle_count_array().max() > (64 if name != "star3" else 16)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", STARS)
def test_intersections_equal_the_oracle(mod, workdir, name, layout):
    cfg = star_config(workdir, name, layout)
    eng = hip_engine(mod, cfg, layout)
    ti.run_against_oracle(eng, cfg, 300, 25, "%s %s" % (name, layout), seen=StarSeen(eng, name))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tracker", [True, False])
@pytest.mark.parametrize("name", ["star7", "star5"])
def test_fronts_equal_the_dict_oracle(mod, workdir, name, tracker, layout):
    eng = hip_engine(mod, star_config(workdir, name, layout), layout)
    tr.run_against_dict_oracle(eng, 400, 25, "%s %s" % (name, layout), tracker=tracker, fused=tracker, looked=StarLooked())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["star7", "star5"])
def test_lane_features_equal_the_dict_oracle(mod, workdir, name, layout):
    features_body(hip_engine(mod, star_config(workdir, name, layout), layout), 350, "%s %s" % (name, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["star7", "star5"])
def test_lane_flow_equals_the_model(mod, workdir, name, layout):
    eng = hip_engine(mod, star_config(workdir, name, layout), layout)
    tl.run_against_model(eng, eng, 400, "%s %s" % (name, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("step, floor", LARGE_STEPS)
def test_large_step_numbers(mod, workdir, tmp_path, step, floor, layout):
    large_step_body(lambda cfg: hip_engine(mod, cfg, layout), star_config(workdir, "star7", layout), tmp_path, step, floor)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_vector_engine_fronts_equal_standalone(mod, workdir, layout):
    vec, singles = hip_vector_star5(mod, workdir, layout)
    looked = StarLooked()
    tr.vector_body(vec, singles, 300, 50, looked=looked)
    assert looked.envs_differ > 0, ENVS_NEVER_DIFFERED


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_vector_engine_tracker_columns_equal_standalone(mod, workdir, layout):
    vec, singles = hip_vector_star5(mod, workdir, layout)
    looked = StarLooked()
    tr.vector_tracker_body(vec, singles, 300, 50, looked=looked)
    assert looked.envs_differ > 0, ENVS_NEVER_DIFFERED
    assert "n > K" in looked.seen[64], "no environment had a lane with more than 64 vehicles at a check"
