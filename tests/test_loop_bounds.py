"""The device-tensor calls on both sides of the four constants that decide how often a loop of their kernels comes round
(cfx_kernels.h).  Two shapes, the smallest that straddle them:

  thin grid   generate_grid(300, 2), ONE Engine: 1204 intersections, 600 signalised, 89 of those at index >= 1024 (a 2 x 300
              grid is no use: its intersections from 1024 on are all virtual); 30 612 positions = 120 tiles of 256
  batch       grid_6x6 x 20, a VectorEngine: 1200 intersections, environment 17 straddles index 1024, 18 and 19 lie beyond
              it; 36 000 positions = 141 tiles.  The oracle is 20 standalone twins on seeds seed + r

  SET_BLOCK      k_set_phases_dense / k_set_tl_plan run as ONE workgroup of 1024 threads that strides over all intersections
                 of all environments: a second pass from 1025 on, which the verdict (atomicMin of the first offender) and
                 the apply loop both depend on
  TILE_SUM_LANES vehicleRows adds up the tile sums of k_vehicle_tile_sums 64 at a time: a second pass from 65 tiles on, a
                 third from 129
  PAD_ROWS       kRowPadRows: padding block j of kr_/kd_vehicle_rows and _poses owns rows [j, j + 1) * 2048 and skips those
                 below `count`
  STAGE_POINTS   kGeoStage, the fourth: tests/test_vehicle_poses.py has it, with the 16- and 17-point polylines

Every test asserts its shape first, from the engine.  Every test marked gpu has an unmarked sibling that runs the same body
with the twin in the HIP engine's place, which settles the shapes, seeds, step counts and preconditions on a machine without a
GPU.  (The signal plan is state only the device library keeps: the plan test's sibling runs the built twins alone, for the
preconditions, and the plan's rejection test has none.)  All comparisons are array_equal or ==."""
import time

import numpy as np
import pytest

from conftest import SHADOW_GPU, assert_same_state

torch = pytest.importorskip("torch")

import test_vehicle_poses as poses  # noqa: E402
import test_vehicle_rows as rows  # noqa: E402
from cityflow_amd.torch_io import VEHICLE_ROW_TILE  # noqa: E402
from test_device_tensors import host_apply, tensor_device, twin  # noqa: E402
from test_tl_plan import NAN, Plan, dev, durations_of, lights, on_device, one_plan_per_environment  # noqa: E402
from test_vector_many_envs import vec_default, vec_twin  # noqa: E402
from test_vehicle_rows import drivables, hip_network_engine  # noqa: E402

SET_BLOCK = 1024     # blockDim of k_set_phases_dense and of k_set_tl_plan, each launched as one workgroup
TILE_SUM_LANES = 64  # the lanes over which vehicleRows sums k_vehicle_tile_sums' results
PAD_ROWS = 2048      # kRowPadRows of kr_/kd_vehicle_rows and kr_/kd_vehicle_poses
assert VEHICLE_ROW_TILE == 256  # kRowTile

R = 20                    # environments of the batch
THIN = (300, 2)           # rows, columns of the thin grid
THIN_FLOW_INTERVAL = 2.0  # 604 flows; a lane admits a vehicle every 3 s, so a shorter interval only fills the buffers


def thin_config(scen, workdir, layout="auto", **config):
    if layout == "dense":
        config["cfx"] = {"layout": "dense"}
    return scen.generate_grid(THIN[0], THIN[1], workdir, flow_interval=THIN_FLOW_INTERVAL, **config)


def batch_config(scen, workdir, layout="auto", **config):
    if layout == "dense":
        config["cfx"] = {"layout": "dense"}
    return scen.materialize("grid_6x6", workdir, **config)


def thin_default(mod, layout="auto"):
    return lambda cfg: hip_network_engine(mod, cfg, layout)


def assert_shape(eng, single, envs, tiles_above):
    """The shape every test here stands on, from the engine (`single`: an Engine on one environment's network): returns the
    virtual mask of all intersections of all environments, in intersection_ids() order."""
    virtual = np.asarray(single._flat_net()["inter_virtual"]) != 0
    assert np.array_equal(virtual, single._phase_counts() < 0) and len(virtual) == len(single.intersection_ids())
    if eng is not None:  # (None: the standalone engines alone, `envs` of them)
        assert tuple(eng._tensor_shapes()[1]) == ((envs, len(virtual)) if envs > 1 else (len(virtual),))
        assert eng._drivable_counts() == single._drivable_counts()
    virtual = np.tile(virtual, envs)
    assert len(virtual) > SET_BLOCK, len(virtual)
    assert int((~virtual[SET_BLOCK:]).sum()) >= 8, "fewer than 8 signalised intersections at index >= %d" % SET_BLOCK
    n_tiles = -(-envs * drivables(single)[1] // VEHICLE_ROW_TILE)
    assert n_tiles > tiles_above, n_tiles
    return virtual


def flat_phases(engines):
    return np.concatenate([np.asarray(e._tl_state()[0]).reshape(-1) for e in engines])


def same_whole_state(eng, twins, where):
    """assert_same_state of an Engine; per environment the lane counts and every vehicle's speed of a VectorEngine."""
    if len(eng._tensor_shapes()[1]) == 1:
        return assert_same_state(eng, twins[0], where)
    counts = eng.get_lane_vehicle_count_array()
    for r, t in enumerate(twins):
        assert np.array_equal(counts[r], t.get_lane_vehicle_count_array()), "%s: env %d lane counts" % (where, r)
        assert eng.get_vehicle_speed(r) == t.get_vehicle_speed(), "%s: env %d vehicle speeds" % (where, r)


# --------------------------------------------------------------------------------- 1. set_tl_phases_tensor beyond one block
# Steps and seed: on the twins a call every third step of 75 changes the phase of every signalised intersection many times
# over; what matters is that vehicles have reached the junctions (some 25 steps), so that the lights decide who moves
PHASE_STEPS, PHASE_SEED = 75, 5


def phases_tensor(eng, want, dtype):
    return torch.from_numpy(np.ascontiguousarray(want.reshape(tuple(eng._tensor_shapes()[1])))).to(dtype).to(tensor_device(eng))


def phases_body(eng, twins, unset, virtual, where):
    """eng through set_tl_phases_tensor, the twins through set_tl_phases, in lockstep; `unset`: a twin of the last environment
    whose signals are never set."""
    n = len(virtual)
    envs = len(twins)
    n_phases = np.tile(twins[0]._phase_counts(), envs).astype(np.int64)
    assert (n_phases[~virtual] > 1).all() and virtual[:SET_BLOCK].any() and virtual[SET_BLOCK:].any()
    rng = np.random.default_rng(PHASE_SEED)
    changed, kept = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    calls = 0
    for s in range(PHASE_STEPS):
        if s % 3 == 0:
            want = rng.integers(0, 1 << 20, size=n) % np.maximum(n_phases, 1)
            want[rng.random(n) < 0.2] = -1
            want[virtual] = rng.choice([99, -5, 12345, -1, 0], size=int(virtual.sum()))  # ignored, whatever it is
            before = flat_phases(twins)
            eng.set_tl_phases_tensor(phases_tensor(eng, want, torch.int64 if calls % 2 else torch.int32))
            for r, t in enumerate(twins):
                host_apply(t, want.reshape(envs, -1)[r])
            after = flat_phases(twins)
            assert np.array_equal(flat_phases([eng]), after), "%s: phases differ right after the call at step %d" % (where, s)
            changed |= after != before
            kept |= ~virtual & (want == -1)
            calls += 1
        for e in [eng, unset] + twins:
            e.next_step()
        if s % 10 == 9 or s == PHASE_STEPS - 1:
            same_whole_state(eng, twins, "%s step %d" % (where, s))
    assert not changed[virtual].any()
    low, high = int(changed[:SET_BLOCK].sum()), int(changed[SET_BLOCK:].sum())
    print("%s: %d calls changed the phase of %d intersections below %d and of %d from it on" % (where, calls, low, SET_BLOCK, high))
    assert high >= 8 and low >= 8, (low, high)
    assert kept[:SET_BLOCK].any() and kept[SET_BLOCK:].any()
    assert twins[-1].get_vehicle_count() > 0
    assert (twins[-1].get_vehicle_speed() != unset.get_vehicle_speed()
            or not np.array_equal(twins[-1].get_lane_vehicle_count_array(), unset.get_lane_vehicle_count_array())), \
        where + ": the run equals one whose signals were never set"


def phase_rejections_body(eng, twins, virtual, where):
    envs, n = len(twins), len(virtual)
    I = n // envs
    ids = twins[0].intersection_ids()
    n_phases = np.tile(twins[0]._phase_counts(), envs).astype(np.int64)
    real = np.nonzero(~virtual)[0]
    lo, hi = int(real[real < SET_BLOCK][7]), int(real[real >= SET_BLOCK][5])

    def words(x):
        return ("'%s'" % ids[x % I], "not applied") + (("env %d" % (x // I),) if envs > 1 else ())

    def rejected(bad, x):
        before = flat_phases([eng])
        with pytest.raises(IndexError) as err:  # (the HIP engine raises at the call that waits; the twin's host path at once)
            eng.set_tl_phases_tensor(phases_tensor(eng, bad, torch.int32))
            eng.sync()
        for w in words(x) + ("phase %d" % bad[x],):
            assert w in str(err.value), "%s: %r lacks %r" % (where, str(err.value), w)
        assert np.array_equal(flat_phases([eng]), before), where + ": a rejected call changed a signal"

    def apply(want):
        eng.set_tl_phases_tensor(phases_tensor(eng, want, torch.int32))
        for r, t in enumerate(twins):
            host_apply(t, want.reshape(envs, -1)[r])
        got = flat_phases([eng])
        assert np.array_equal(got, flat_phases(twins))
        assert np.array_equal(got[~virtual], want[~virtual]), where + ": a valid call did not apply"

    for _ in range(10):
        for e in [eng] + twins:
            e.next_step()
    apply(np.where(virtual, 0, 1))
    good = np.where(virtual, 77, 2)  # a valid change at every signalised intersection, on both sides of SET_BLOCK
    bad = good.copy()
    bad[hi] = n_phases[hi] + 3
    rejected(bad, hi)  # the only offender is beyond the first pass
    bad[lo] = -7
    rejected(bad, lo)  # one offender on either side: the lower one is named
    bad[lo] = -1
    bad[hi] = n_phases[hi]
    rejected(bad, hi)  # (one past the last phase)
    apply(good)
    assert (flat_phases([eng])[real] == 2).all() and len(real[real < SET_BLOCK]) >= 8 and len(real[real >= SET_BLOCK]) >= 8
    for _ in range(10):
        for e in [eng] + twins:
            e.next_step()
    same_whole_state(eng, twins, where + " after the rejected calls")
    assert twins[-1].get_vehicle_count() > 0


def thin_phase_engines(mod, make, scen, workdir, layout, n_twins):
    cfg = thin_config(scen, workdir, layout, rlTrafficLight=True)
    eng = make(cfg)
    twins = [twin(mod, cfg) for _ in range(n_twins)]
    return eng, twins, assert_shape(eng, twins[0], 1, TILE_SUM_LANES)


def batch_phase_engines(mod, make_vec, scen, workdir, unset):
    vec = make_vec(batch_config(scen, workdir, rlTrafficLight=True), R)
    twins = [twin(mod, batch_config(scen, workdir, rlTrafficLight=True, seed=r)) for r in range(R + (1 if unset else 0))]
    if unset:
        twins[R] = twin(mod, batch_config(scen, workdir, rlTrafficLight=True, seed=R - 1))
    virtual = assert_shape(vec, twins[0], R, 2 * TILE_SUM_LANES)
    I = len(virtual) // R
    # environment 17 straddles it (the four entries below it are virtual: all its signals lie beyond, all of 16's before)
    assert 17 * I < SET_BLOCK < 18 * I and (~virtual[16 * I:17 * I]).any() and (~virtual[SET_BLOCK:18 * I]).any()
    return vec, twins, virtual


def thin_phases(mod, make, scen, workdir, layout):
    t0 = time.perf_counter()
    eng, twins, virtual = thin_phase_engines(mod, make, scen, workdir, layout, 2)
    phases_body(eng, twins[:1], twins[1], virtual, "thin grid %s" % layout)
    print("set_tl_phases_tensor thin grid %s: %.1f s" % (layout, time.perf_counter() - t0))


def batch_phases(mod, make_vec, scen, workdir):
    t0 = time.perf_counter()
    vec, twins, virtual = batch_phase_engines(mod, make_vec, scen, workdir, True)
    phases_body(vec, twins[:R], twins[R], virtual, "grid_6x6 x%d" % R)
    print("set_tl_phases_tensor grid_6x6 x%d: %.1f s" % (R, time.perf_counter() - t0))


def thin_phase_rejections(mod, make, scen, workdir):
    t0 = time.perf_counter()
    eng, twins, virtual = thin_phase_engines(mod, make, scen, workdir, "auto", 1)
    phase_rejections_body(eng, twins, virtual, "thin grid")
    print("set_tl_phases_tensor rejections thin grid: %.1f s" % (time.perf_counter() - t0))


def batch_phase_rejections(mod, make_vec, scen, workdir):
    t0 = time.perf_counter()
    vec, twins, virtual = batch_phase_engines(mod, make_vec, scen, workdir, False)
    phase_rejections_body(vec, twins, virtual, "grid_6x6 x%d" % R)
    print("set_tl_phases_tensor rejections grid_6x6 x%d: %.1f s" % (R, time.perf_counter() - t0))


def test_phases_thin_grid_twin_against_twin(mod, scen, workdir):
    thin_phases(mod, lambda cfg: twin(mod, cfg), scen, workdir, "auto")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_phases_thin_grid_beyond_one_block(mod, scen, workdir, layout):
    thin_phases(mod, thin_default(mod, layout), scen, workdir, layout)


def test_phases_batch_twin_against_twins(mod, scen, workdir):
    batch_phases(mod, vec_twin(mod), scen, workdir)


@pytest.mark.gpu
def test_phases_batch_beyond_one_block(mod, scen, workdir):
    batch_phases(mod, vec_default(mod), scen, workdir)


def test_phase_rejections_thin_grid_twin(mod, scen, workdir):
    thin_phase_rejections(mod, lambda cfg: twin(mod, cfg), scen, workdir)


@pytest.mark.gpu
def test_phase_rejections_thin_grid_beyond_one_block(mod, scen, workdir):
    thin_phase_rejections(mod, thin_default(mod), scen, workdir)


def test_phase_rejections_batch_twin(mod, scen, workdir):
    batch_phase_rejections(mod, vec_twin(mod), scen, workdir)


@pytest.mark.gpu
def test_phase_rejections_batch_beyond_one_block(mod, scen, workdir):
    batch_phase_rejections(mod, vec_default(mod), scen, workdir)


# -------------------------------------------------------------------- 2. set_tl_plan_tensor / get_tl_phase_durations_tensor
PLAN_STEPS = 120


def plan_engines(mod, scen, workdir, shape):
    """(config, plan, one plan per environment, twins BUILT with them, a twin of the last environment on the file's plan)"""
    if shape == "thin":
        cfg = thin_config(scen, workdir)
        plan = Plan(twin(mod, cfg), cfg)
        plans = [plan.other(3)]
        return cfg, plan, plans, [twin(mod, plan.built(plans[0], "bounds"))], twin(mod, cfg)
    cfg = batch_config(scen, workdir)
    plan = Plan(twin(mod, cfg), cfg)
    plans = [plan.other(k) for k in range(R)]
    assert len({T.tobytes() for T in plans}) > 8
    singles = [twin(mod, plan.built(plans[r], "bounds_env%d" % r, seed=r)) for r in range(R)]
    return cfg, plan, plans, singles, twin(mod, batch_config(scen, workdir, seed=R - 1))


def plan_body(mod, make, scen, workdir, shape):
    """make(cfg) -> the engine that is GIVEN the plans (None: the built twins alone)."""
    t0 = time.perf_counter()
    cfg, plan, plans, singles, on_file = plan_engines(mod, scen, workdir, shape)
    envs = len(singles)
    eng = make(cfg) if make is not None else None
    assert_shape(eng, singles[0], envs, TILE_SUM_LANES)
    last = (envs - 1) * plan.I  # the last environment's first intersection
    assert envs == 1 or last >= SET_BLOCK
    sequences = []

    def every_step(s, engines):
        on_file.next_step()
        sequences.append((lights(engines[-1])[0], lights(on_file)[0]))

    one_plan_per_environment(eng, singles, plan, plans, PLAN_STEPS, every_step)
    given, file = np.stack([a for a, _ in sequences]), np.stack([b for _, b in sequences])  # [steps, I] of the last environment
    beyond = [i for i in plan.real if last + i >= SET_BLOCK and not np.array_equal(given[:, i], file[:, i])]
    assert beyond, "no intersection from %d on ran through another phase sequence than the file plan's" % SET_BLOCK
    assert singles[-1].get_vehicle_count() > 0
    print("set_tl_plan_tensor %s: %d intersections from %d on left the file plan's sequence; %.1f s"
          % (shape, len(beyond), SET_BLOCK, time.perf_counter() - t0))


@pytest.mark.parametrize("shape", ["thin", "batch"])
def test_plan_preconditions_on_the_built_twins(mod, scen, workdir, shape):
    plan_body(mod, None, scen, workdir, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["thin", "batch"])
def test_plan_beyond_one_block(mod, scen, workdir, shape):
    make = (lambda cfg: on_device(thin_default(mod)(cfg))) if shape == "thin" else (lambda cfg: on_device(vec_default(mod)(cfg, R)))
    plan_body(mod, make, scen, workdir, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["thin", "batch"])
def test_plan_rejections_beyond_one_block(mod, scen, workdir, shape):
    """tests/test_vector_many_envs.py::test_a_rejection_names_an_env_beyond_64 with the offender at an intersection from
    SET_BLOCK on (in environment 18 or 19 of the batch): an invalid duration, an invalid phase, a negative phase_remain, a cycle
    shorter than a step, each among valid entries everywhere else.  None is applied anywhere, the message names the place, and
    where an intersection below SET_BLOCK holds an invalid duration in the same call the lower key wins."""
    t0 = time.perf_counter()
    cfg = thin_config(scen, workdir) if shape == "thin" else batch_config(scen, workdir)
    envs = 1 if shape == "thin" else R
    eng = on_device(thin_default(mod)(cfg) if shape == "thin" else vec_default(mod)(cfg, R))
    single = twin(mod, cfg)
    plan = Plan(single, cfg)
    I = plan.I
    virtual = assert_shape(eng, single, envs, TILE_SUM_LANES)
    real = np.nonzero(~virtual)[0]
    lo, hi = int(real[real < SET_BLOCK][7]), int(real[real >= SET_BLOCK][-3])
    (el, il), (e, i) = (lo // I, lo % I), (hi // I, hi % I)
    assert plan.count[i] > 3 and plan.count[il] > 3 and (envs == 1 or (e in (18, 19) and el < 17))
    give = lambda a, dtype=None: dev(eng, a if envs > 1 else a[0], dtype)  # noqa: E731
    shaped = lambda a: np.asarray(a).reshape((envs, I) + np.asarray(a).shape[(2 if envs > 1 else 1):])  # noqa: E731  [R, I, ...]

    def rejected(name, x, *want, **kwargs):
        eng.set_tl_plan_tensor(**kwargs)
        with pytest.raises(ValueError) as err:
            eng.sync() if name != "phase" else eng.get_lane_vehicle_count_array()  # (any call that waits for the device)
        msg = str(err.value)
        for w in want + ("'%s'" % plan.ids[x % I], "not applied") + (("env %d" % (x // I),) if envs > 1 else ()):
            assert w in msg, "%s: %r lacks %r" % (name, msg, w)
        return msg

    base = np.stack([plan.file()] * envs)
    for s in range(5):
        eng.next_step()
    before = [shaped(a) for a in lights(eng)]
    d = np.stack([plan.other(k) for k in range(envs)])
    p = np.full((envs, I), -1, dtype=np.int64)
    rem = np.full((envs, I), NAN)
    for x in real:
        p[x // I, x % I] = (x // I + x % I) % plan.count[x % I]
        rem[x // I, x % I] = 1.0 + 0.25 * ((x // I + x % I) % 8)
    bad = d.copy()
    bad[e, i, 3] = -1.0
    rejected("duration", hi, "durations", "phase 3", durations=give(bad), phase_remain=give(bad[:, :, 0]))
    bad_p = p.copy()
    bad_p[e, i] = plan.count[i]
    rejected("phase", hi, "phase", str(plan.count[i]), phase=give(bad_p))
    bad_rem = rem.copy()
    bad_rem[e, i] = -0.25
    rejected("phase_remain", hi, "phase_remain", "-0.25", phase_remain=give(bad_rem), durations=give(d))
    short = d.copy()
    short[e, i, :plan.count[i]] = 0.0
    short[e, i, 1] = 0.5
    assert "would sum to 0.5" in rejected("sum", hi, "durations", "sum", durations=give(short))  # (the interval is 1.0)
    short[el, il, 2] = -2.0  # ... and an invalid duration below SET_BLOCK in the same call: the lower key wins
    assert "sum" not in rejected("lower key", lo, "durations", "phase 2", "-2", durations=give(short), phase=give(p))
    after = [shaped(a) for a in lights(eng)]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the lights changed somewhere"
    assert np.array_equal(shaped(durations_of(eng)), base), "durations changed somewhere"
    # the corrected call applies everywhere, every environment and intersection with its own values
    d[e, i, 3] = 7.75
    eng.set_tl_plan_tensor(durations=give(d), phase=give(p), phase_remain=give(rem))
    eng.sync()
    assert np.array_equal(shaped(durations_of(eng)), d)
    ph, re = [shaped(a).reshape(-1) for a in lights(eng)]
    assert np.array_equal(ph[real], p.reshape(-1)[real]) and np.array_equal(re[real], rem.reshape(-1)[real])
    assert len({p.reshape(-1)[x] for x in real[real >= SET_BLOCK]}) > 2 and len({rem.reshape(-1)[x] for x in real[real >= SET_BLOCK]}) > 2
    print("set_tl_plan_tensor rejections %s: %.1f s" % (shape, time.perf_counter() - t0))


# ------------------------------------------------------------------ 3. observe_vehicles_tensor beyond 64 and 128 tile sums
class Held:
    """The row lengths of the issue in every compared state, and what the compared states contained."""

    def __init__(self, envs):
        self.envs, self.states = envs, []

    def lengths(self, eng, start, count, where):
        """(count + 5000, count, the largest 2048 k + 1 below count, 0) and the record of this state."""
        D = drivables(eng)[1]
        first = np.asarray(start).reshape(self.envs, D + 1)[:, :-1].reshape(-1)  # the first row of every position
        occupied = np.nonzero(np.diff(np.append(first, count)) > 0)[0]
        assert count > 2 * PAD_ROWS, "%s: only %d vehicles" % (where, count)
        cut = (count - 2) // PAD_ROWS * PAD_ROWS + 1
        assert cut < count <= cut + PAD_ROWS and cut % PAD_ROWS == 1
        # the last row that is kept, row cut - 1, is the first of padding block cut // PAD_ROWS's range; its position:
        cut_tile = int(np.searchsorted(first, cut - 1, side="right") - 1) // VEHICLE_ROW_TILE
        assert cut_tile > TILE_SUM_LANES, "%s: the cut at row %d lies in tile %d" % (where, cut, cut_tile)
        long = count + 5000
        wholly = [j for j in range(-(-long // PAD_ROWS)) if j * PAD_ROWS >= count]  # blocks that hold nothing but padding
        assert len(wholly) >= 2 and count % PAD_ROWS != 0 and count // PAD_ROWS >= 2  # ... one straddles count, two lie below it
        self.states.append((where, count, int((occupied >= TILE_SUM_LANES * VEHICLE_ROW_TILE).sum()),
                            int((occupied >= 2 * TILE_SUM_LANES * VEHICLE_ROW_TILE).sum()), cut, cut_tile))
        return long, count, cut, 0

    def enough(self, where):
        for state in self.states:
            print("%s: count %d, occupied drivables beyond tile 64: %d, beyond tile 128: %d, cut at N = %d in tile %d" % state)
        assert self.states and all(s[2] > 0 for s in self.states), where + ": no vehicle beyond the 64th tile"
        assert self.envs == 1 or all(s[3] > 0 for s in self.states), where + ": no vehicle beyond the 128th tile"


def check_lengths(eng, want, lengths, groups, where):
    """want: outputs that were held against the oracle at one length; every group of outputs at every length equals them cut
    or padded, and every element of every tensor, pre-filled with FILL, is written."""
    count = int(want["count"])
    for n_rows in lengths:
        for names in groups:
            t = poses.tensors(eng, n_rows, names)
            eng.observe_vehicles_tensor(**t)
            cut = poses.at_length({k: v[:count] if k in poses.ALL else v for k, v in want.items()}, n_rows, [k for k in names if k in poses.ALL])
            for k in names:
                poses.same(t[k], cut[k] if k in cut else want[k], "%s, N = %d, %d outputs: %s" % (where, n_rows, len(names), k))


# The batch, (steps, every): on the twins 4800, 9120 and 13 440 vehicles at steps 28, 56 and 84, the cut in tiles 119, 121, 126.
# The thin grid, the compared steps: under its file's plan the 600 row flows cross their junctions together in the first 30 s
# and then wait 110 s for the next green, so the laneLinks beyond tile 64 (the lanes end in tile 35) stand empty in most
# states; with rlTrafficLight and no phase ever set the signals hold phase 0, the rows flow on, and at these steps the twin
# has the cut in tiles 101, 117 and 75 (8456, 10 268 and 10 872 vehicles, 790 occupied laneLinks beyond tile 64).
BATCH_ROWS = (84, 28)
THIN_ROWS = (42, 50, 52)


def batch_rows(mod, make_vec, scen, workdir, layout, body):
    t0 = time.perf_counter()
    vec = make_vec(batch_config(scen, workdir, layout), R)
    singles = [twin(mod, batch_config(scen, workdir, seed=r)) for r in range(R)]
    assert_shape(vec, singles[0], R, 2 * TILE_SUM_LANES)
    held = Held(R)
    where = "grid_6x6 x%d %s %s" % (R, layout, body.__name__)
    names = rows.ROWS if body is rows else ("drivable", "env", "distance", "speed") + poses.POSES
    groups = (names + ("start", "count"),) + ((poses.POSES,) if body is poses else ())

    def extra(vec, got, total, at):
        check_lengths(vec, got, held.lengths(vec, got["start"], total, at), groups, at)

    body.vector_body(vec, singles, BATCH_ROWS[0], BATCH_ROWS[1], where, extra=extra)
    assert len(held.states) == BATCH_ROWS[0] // BATCH_ROWS[1]
    held.enough(where)
    print("observe_vehicles_tensor %s: %.1f s" % (where, time.perf_counter() - t0))


def thin_rows(mod, make, scen, workdir, layout):
    t0 = time.perf_counter()
    eng = make(thin_config(scen, workdir, layout, rlTrafficLight=True))
    assert_shape(eng, eng, 1, TILE_SUM_LANES)
    held = Held(1)
    for s in range(1, max(THIN_ROWS) + 1):
        eng.next_step()
        if s not in THIN_ROWS:
            continue
        where = "thin grid %s step %d" % (layout, s)
        want = rows.state_rows(eng)
        rows.check_array(eng, want, where)
        host = eng.observe_vehicles_array(poses=True)  # the host form: the state's rows and the poses worked out on the host
        for k in want:
            rows.same(host[k], want[k], "%s: host form with poses, %s" % (where, k))
        lengths = held.lengths(eng, want["start"], int(want["count"]), where)
        rows.check_tensors(eng, want, where, lengths)
        poses.check_tensors(eng, host, where, lengths)  # all thirteen row outputs with start and count, then the six alone
    rows.cross_check_ids(eng, want, where)
    assert len(held.states) == len(THIN_ROWS)
    held.enough("thin grid " + layout)
    print("observe_vehicles_tensor thin grid %s: %.1f s" % (layout, time.perf_counter() - t0))


@pytest.mark.parametrize("body", [rows, poses], ids=["rows", "poses"])
def test_rows_batch_twin_against_twins(mod, scen, workdir, body):
    batch_rows(mod, vec_twin(mod), scen, workdir, "auto", body)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("body", [rows, poses], ids=["rows", "poses"])
def test_rows_batch_beyond_128_tiles(mod, scen, workdir, body, layout):
    def make_vec(cfg, n):
        vec = vec_default(mod)(cfg, n)
        assert SHADOW_GPU or (vec._vehicle_rows_device() and vec._vehicle_poses_device())
        return vec
    batch_rows(mod, make_vec, scen, workdir, layout, body)


def test_rows_thin_grid_twin(mod, scen, workdir):
    thin_rows(mod, lambda cfg: twin(mod, cfg), scen, workdir, "auto")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_rows_thin_grid_beyond_64_tiles(mod, scen, workdir, layout):
    def make(cfg):
        eng = hip_network_engine(mod, cfg, layout)
        assert SHADOW_GPU or eng._vehicle_poses_device()
        return eng
    thin_rows(mod, make, scen, workdir, layout)
