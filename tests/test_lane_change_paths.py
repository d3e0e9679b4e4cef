"""The fallback paths of the lane-change schedule walk (k_lc_schedule / k_lc_insert, csrc/hip/cfx_lc_kernels.h).

The walk has a fast path sized for three-lane grid roads of 300 m and a fallback behind each capacity; the grids of
tests/test_lane_change.py never leave the fast path.  The star junctions below (tests/star_networks.py, "laneChange": true) do:

  star3  in_0 / out_0 have 18 lanes: more than kLcSchedLanes = 8, the walk reads global memory (`staged` false) ...
  long5  ... and so it does on in_0 and in_3 (5 lanes) once they hold more than kLcSchedStage = 384 slots; before that in_0 is
         staged, but its 28 segments are more than kLcSchedSegs = 24: the table of segment runs is off (`sRunsOff`) and every
         neighbour search builds its segments by bisection
  wide3  a 9-lane road whose candidates share few target lanes: lanes that get two shadows in one step (`runs` false, the
         earlier shadow merged into the segment, the `seq` rules of two shadows before one anchor), a dozen candidates and
         up to 11 new shadows on one road in one step

Natural traffic never exceeds kLcRoadCand = 64 candidates or kLcRoadInserts = 32 new shadows on one road, so two builds of the
HIP library with those capacities made small (cityflow_amd/build.py HIP_VARIANTS) stand in: `cand4` takes the `tooMany` walk
wherever a road has more than 4 candidates and must still equal the twin, which has no such capacity; `ins2` must refuse a
third shadow on one road with CFX_ERR_CAPACITY, never cut silently.

The oracle is the CPU twin; the reference engine and the twin agree exactly on the three networks (the first test).  Every
engine test keeps a record of what its run reached, taken from the twin's lane lists between steps, and fails if the path it
is for was not reached; test_twin_runs_reach_every_path checks the same conditions on the twin alone, so that a failure on the
device can only be the kernel's."""
import json
import math
import os

import numpy as np
import pytest

import conftest
from conftest import REF_DIR, TWIN_LIB

torch = pytest.importorskip("torch")

import star_networks  # noqa: E402
from test_lane_change import _state, lcp  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_lane_flow import hip_engine  # noqa: E402

CFX_LC_SHADOW, CFX_LC_CHANGING = 1, 4  # include/cityflow_amd.h
SCALARS = ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time", "vehicle_steps")
STAGE_SLOTS, STAGE_LANES, STAGE_SEGS = 384, 8, 24  # kLcSchedStage, kLcSchedLanes, kLcSchedSegs


def lc_config(workdir, name, seed=0):
    return star_networks.make(workdir, name, seed=seed, lane_change=True)


def variant_lib(name):
    """A small-capacity build of the HIP library; not to be had from a twin that stands in for the device."""
    if conftest.SHADOW_GPU:
        pytest.skip("a capacity of the device code: the twin has none")
    from cityflow_amd import build
    path = build.hip_variant_target(name)
    assert os.path.exists(path), path + " was not built"
    return path


def checked(s):
    """States are compared after every step for the first 100 steps, then after every 5th."""
    return s < 100 or s % 5 == 4


def assert_equals_twin(eng, tw, b, where):
    """Every field of _vehicle_state() (the lc_* ones included), the lane counts and the scalars; b = _state(tw)."""
    a = _state(eng)
    assert a.keys() == b.keys() and "lc_flags" in a, where
    for k in a:
        assert a[k].shape == b[k].shape, "%s: %s count differs (%s vs %s)" % (where, k, a[k].shape, b[k].shape)
        assert np.array_equal(a[k], b[k]), "%s: %s differs" % (where, k)
    assert np.array_equal(eng.get_lane_vehicle_count_array(), tw.get_lane_vehicle_count_array()), where + ": lane counts"
    sa, sb = eng._scalars(), tw._scalars()
    for k in SCALARS:
        assert sa[k] == sb[k], "%s: scalar %s differs (%r vs %r)" % (where, k, sa[k], sb[k])


class Reach:
    """What a run reached, from the twin's get_lane_vehicles() between steps and its states at the checks."""

    def __init__(self, tw):
        net = tw._flat_net()
        road_ids, lane_ids = list(net["road_ids"]), list(net["lane_ids"])
        self.lane_road = np.asarray(net["lane_road"])
        self.n_lanes = len(lane_ids)
        self.road_ids = road_ids
        self.road_of = {lane_ids[l]: road_ids[int(self.lane_road[l])] for l in range(self.n_lanes)}
        self.road_lanes = {r: sum(1 for x in self.road_of.values() if x == r) for r in road_ids}
        self.prev = tw.get_lane_vehicles()
        # one record per new shadow: (step, road, lane, the road's vehicles before the step, ... after it)
        self.shadows = []
        self.double_steps = {}    # step -> the lanes that got at least 2 new shadows
        self.adjacent_steps = 0   # ... steps in which two of them are neighbours in the lane's list
        self.most_on_a_road = 0   # new shadows on one road in one step
        self.first_over = {}      # n -> the first step in which one road got more than n new shadows
        self.candidates = {}      # checked step -> {road: candidates of that step's walk, at least}

    def _road_vehicles(self, lanes):
        out = dict.fromkeys(self.road_ids, 0)
        for lane, ids in lanes.items():
            if lane in self.road_of:
                out[self.road_of[lane]] += len(ids)
        return out

    def _road_changing(self, lanes):
        """{road: its real vehicles in the middle of a change}: those whose "<id>_shadow" is on a lane of the same road"""
        road = {v: self.road_of[lane] for lane, ids in lanes.items() if lane in self.road_of for v in ids}
        out = {}
        for v, r in road.items():
            if v.endswith("_shadow") and road.get(v[:-len("_shadow")]) == r:
                out[r] = out.get(r, 0) + 1
        return out

    def step(self, s, lanes):
        """lanes: the twin's get_lane_vehicles() after step s."""
        old = {v for ids in self.prev.values() for v in ids if v.endswith("_shadow")}
        before, after = self._road_vehicles(self.prev), self._road_vehicles(lanes)
        per_road, adjacent = {}, False
        for lane, ids in lanes.items():
            new = [i for i, v in enumerate(ids) if v.endswith("_shadow") and v not in old]
            if not new:
                continue
            road = self.road_of[lane]
            per_road[road] = per_road.get(road, 0) + len(new)
            for _ in new:
                self.shadows.append((s, road, lane, before[road], after[road]))
            if len(new) >= 2:
                self.double_steps.setdefault(s, []).append(lane)
                adjacent = adjacent or any(b - a == 1 for a, b in zip(new, new[1:]))
        self.adjacent_steps += int(adjacent)
        most = max(per_road.values(), default=0)
        self.most_on_a_road = max(self.most_on_a_road, most)
        if most > 2 and 2 not in self.first_over:
            self.first_over[2] = s
        # The candidates of this step's walk on a road are at least: the real vehicles that were changing on it when the step
        # began (k_lc_plan: `changing` keeps the signal and stays a candidate) and the parents of its new shadows (lcPlanChange
        # held for each, and none of them was changing before).
        if checked(s):
            was = self._road_changing(self.prev)
            self.candidates[s] = {r: was.get(r, 0) + per_road.get(r, 0) for r in set(was) | set(per_road)}
        self.prev = lanes

    def check(self, state):
        """state: _state(twin) at a compared step: the vehicles _road_changing() counts are the real ones on a lane whose
        lc_flags carry CFX_LC_CHANGING."""
        real = (state["lc_flags"] & CFX_LC_SHADOW) == 0
        on_lane = state["drivable"] < self.n_lanes
        sel = real & on_lane & ((state["lc_flags"] & CFX_LC_CHANGING) != 0)
        roads, n = np.unique(self.lane_road[state["drivable"][sel]], return_counts=True)
        assert {self.road_ids[int(r)]: int(k) for r, k in zip(roads, n)} == self._road_changing(self.prev)

    # ---- the conditions
    def shadows_on_wide_roads(self):
        return sum(1 for _, road, _, _, _ in self.shadows if self.road_lanes[road] > STAGE_LANES)

    def shadows_while_staged(self, road, slots):
        """new shadows on `road` while its vehicles plus its lanes (one spare slot each) were at most `slots`"""
        k = self.road_lanes[road]
        return sum(1 for _, r, _, b, a in self.shadows if r == road and max(a, b) + k <= slots)

    def shadows_on_full_roads(self, vehicles):
        """per road of at most 8 lanes: new shadows while it held at least `vehicles` vehicles"""
        out = {}
        for _, r, _, b, a in self.shadows:
            if self.road_lanes[r] <= STAGE_LANES and min(a, b) >= vehicles:
                out[r] = out.get(r, 0) + 1
        return out

    def steps_with_more_candidates_than(self, n, lanes_over=None, lanes_up_to=None):
        """checked steps in whose walk one road (of more than / at most so many lanes) had more than n candidates"""
        def counts(road):
            k = self.road_lanes[road]
            return (lanes_over is None or k > lanes_over) and (lanes_up_to is None or k <= lanes_up_to)
        return sum(1 for c in self.candidates.values() if any(v > n and counts(r) for r, v in c.items()))


def run_against_twin(tw, engines, steps, where, each_step=None):
    """`engines` (none: the twin alone) step beside the twin and equal it at every check; -> Reach"""
    reach = Reach(tw)
    for s in range(steps):
        tw.next_step()
        for e in engines:
            e.next_step()
        reach.step(s, tw.get_lane_vehicles())
        if checked(s):
            b = _state(tw)
            reach.check(b)
            for i, e in enumerate(engines):
                assert_equals_twin(e, tw, b, "%s, engine %d, step %d" % (where, i, s))
        if each_step:
            each_step(s, reach)
    want = tw.get_lane_vehicles()
    for i, e in enumerate(engines):
        assert e.get_lane_vehicles() == want, "%s, engine %d: lane lists at the end" % (where, i)
    return reach


# ------------------------------------------------------------------------------------------------ the tests' bodies
# (each with the engines under test, or with none: the reach test below)
def unstaged_by_lanes(mod, workdir, make):
    cfg = lc_config(workdir, "star3")
    tw = twin(mod, cfg)
    reach = run_against_twin(tw, make(cfg), 500, "star3")
    assert max(reach.road_lanes.values()) == 18
    n = reach.shadows_on_wide_roads()
    assert n >= 50, "only %d new shadows on roads of more than 8 lanes" % n


def segment_count(cfg, road):
    """A lower bound of Lane::segments.size(): ceil(polyline / 75) (the engine's interval is 70 m, Road::buildSegmentationByInterval;
    _flat_net() does not expose lane_n_segments)."""
    with open(os.path.join(os.path.dirname(cfg), "roadnet.json")) as f:
        net = json.load(f)
    pts = next(r["points"] for r in net["roads"] if r["id"] == road)
    return math.ceil(sum(math.hypot(b["x"] - a["x"], b["y"] - a["y"]) for a, b in zip(pts, pts[1:])) / 75)


def segments_off_then_unstaged_by_slots(mod, workdir, make):
    cfg = lc_config(workdir, "long5")
    assert segment_count(cfg, "in_0") > STAGE_SEGS
    tw = twin(mod, cfg)
    reach = run_against_twin(tw, make(cfg), 900, "long5")
    assert reach.road_lanes["in_0"] == 5
    n = reach.shadows_while_staged("in_0", 380)
    assert n >= 20, "only %d new shadows on in_0 while it held at most 380 slots" % n
    full = reach.shadows_on_full_roads(400)
    assert max(full.values(), default=0) >= 20, "new shadows on roads of at least 400 vehicles: %r" % full


def shadows_into_one_lane(mod, workdir, make):
    cfg = lc_config(workdir, "wide3")
    tw = twin(mod, cfg)
    engines = make(cfg)

    def lane_order(s, reach):  # the lanes that got two shadows or more in this step: the order of the ids, now
        if s in reach.double_steps:
            for e in engines:
                got = e.get_lane_vehicles()
                for lane in reach.double_steps[s]:
                    assert got[lane] == reach.prev[lane], "wide3, step %d: the order of the vehicles on %s" % (s, lane)

    reach = run_against_twin(tw, engines, 500, "wide3", each_step=lane_order)
    assert len(reach.double_steps) >= 30, "only %d steps in which a lane got 2 new shadows" % len(reach.double_steps)
    assert reach.adjacent_steps >= 20, "only %d steps with adjacent new shadows" % reach.adjacent_steps


def too_many_candidates(mod, workdir, make):
    """wide3 and long5: more than 4 candidates on the 9-lane road (with the walk from global memory), on the 2000 m road of
    wide3 (staged) and on in_3 of long5 (5 lanes, more than 384 slots by then)."""
    total = 0
    for name, steps in (("wide3", 500), ("long5", 600)):
        cfg = lc_config(workdir, name)
        reach = run_against_twin(twin(mod, cfg), make(cfg), steps, name)
        n = reach.steps_with_more_candidates_than(4)
        assert n >= 1, "%s: no checked step with more than 4 candidates on one road" % name
        total += n
        if name == "wide3":
            assert reach.steps_with_more_candidates_than(4, lanes_over=STAGE_LANES) >= 1, "never on the 9-lane road"
            assert reach.steps_with_more_candidates_than(4, lanes_up_to=STAGE_LANES) >= 1, "never on a road of at most 8 lanes"
    assert total >= 30, "only %d checked steps with more than 4 candidates on one road" % total


def vector_wide3(mod, workdir, make_vec, steps=300):
    """Three environments of wide3 against the standalone twins with the seeds 0, 1, 2 (tests/test_vector_engine.py `_check`)."""
    envs = 3
    vec = make_vec(lc_config(workdir, "wide3"), envs) if make_vec else None
    singles = [twin(mod, lc_config(workdir, "wide3", seed=e)) for e in range(envs)]
    assert vec is None or vec.lane_ids() == singles[0].lane_ids()
    reaches = [Reach(e) for e in singles]
    differ = 0
    for s in range(steps):
        if vec is not None:
            vec.next_step()
        for e in range(envs):
            singles[e].next_step()
            reaches[e].step(s, singles[e].get_lane_vehicles())
        if not checked(s):
            continue
        want = [e.get_lane_vehicle_count_array() for e in singles]
        differ += int(all(not np.array_equal(want[a], want[b]) for a in range(envs) for b in range(a)))
        for e in range(envs):
            reaches[e].check(_state(singles[e]))
        if vec is None:
            continue
        counts, waits = vec.get_lane_vehicle_count_array(), vec.get_lane_waiting_vehicle_count_array()
        assert counts.shape == (envs, len(vec.lane_ids()))
        for e in range(envs):
            assert np.array_equal(counts[e], want[e]), (s, e)
            assert np.array_equal(waits[e], singles[e].get_lane_waiting_vehicle_count_array()), (s, e)
            assert vec.get_vehicle_speed(e) == singles[e].get_vehicle_speed(), (s, e)
    if vec is not None:
        assert vec.get_vehicle_count() == sum(e.get_vehicle_count() for e in singles)
    assert differ > 0, "the three environments never held different lane counts at a check"
    n = sum(r.steps_with_more_candidates_than(4) for r in reaches)
    assert n >= 10, "only %d checked steps with more than 4 candidates on one road of one environment" % n


def capacity_step(mod, workdir):
    """-> the first step of wide3 in which one road gets more than 2 new shadows (the twin's run)"""
    tw = twin(mod, lc_config(workdir, "wide3"))
    reach = Reach(tw)
    for s in range(300):
        tw.next_step()
        reach.step(s, tw.get_lane_vehicles())
        if 2 in reach.first_over:
            return s
    raise AssertionError("no road of wide3 got more than 2 new shadows in one step within 300 steps")


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("name, horizons", [("star3", (150, 400)), ("wide3", (150, 400)), ("long5", (300, 900))])
def test_reference_vs_twin(workdir, name, horizons):
    if not os.path.exists(os.path.join(REF_DIR, "libmonotonic_new.so")):
        pytest.skip("oracle/_ref reference build not present")
    cfg = lc_config(workdir, name)
    shadows = 0
    for h in horizons:
        r, t = lcp.run("ref", cfg, h), lcp.run("twin", cfg, h)
        assert lcp.compare(r, t) == [], (name, h)
        shadows += r["count"] - len(r["speed"])
    assert shadows > 0, "no shadow alive at a checkpoint"


def test_twin_runs_reach_every_path(mod, workdir):
    """The conditions of the gpu tests below, on the twin alone."""
    none = lambda cfg: []  # noqa: E731
    unstaged_by_lanes(mod, workdir, none)
    segments_off_then_unstaged_by_slots(mod, workdir, none)
    shadows_into_one_lane(mod, workdir, none)
    too_many_candidates(mod, workdir, none)
    vector_wide3(mod, workdir, None)
    assert capacity_step(mod, workdir) < 300


# ---------------------------------------------------------------------------------------------------------------- GPU
def one_hip(mod):
    # (with lane change the automatic layout is the dense one)
    return lambda cfg: [hip_engine(mod, cfg, "dense")]


@pytest.mark.gpu
def test_unstaged_by_lanes(mod, workdir):
    """star3: shadows on the 18-lane roads — slotVid, slotDrv, slotDisOf, slotSeg, slotLen, laneStart, laneCount from global
    memory."""
    unstaged_by_lanes(mod, workdir, one_hip(mod))


@pytest.mark.gpu
def test_segment_table_off_then_unstaged_by_slots(mod, workdir):
    """long5: in_0 (28 segments) while it fits the stage — `sRunsOff`, buildSegment() per segment over LDS — and then in_0 and
    in_3 with more than 384 slots: the same searches over global memory."""
    segments_off_then_unstaged_by_slots(mod, workdir, one_hip(mod))


@pytest.mark.gpu
def test_shadows_into_a_lane_that_already_got_one(mod, workdir):
    """wide3: `runs` false, the walk's earlier shadows merged into the segment, `followerRec >= 0` and the `seq` rules;
    k_lc_insert with several shadows before one anchor.  The lane's order is compared in the very step."""
    shadows_into_one_lane(mod, workdir, one_hip(mod))


@pytest.mark.gpu
def test_too_many_candidates(mod, workdir):
    """The library built with room for 4 candidates per road: the `tooMany` walk (positions for every vehicle of the road, the
    next candidate by a scan per turn) equals the twin, and so does the default library beside it."""
    lib = variant_lib("cand4")
    too_many_candidates(mod, workdir, lambda cfg: [mod.Engine._with_backend(cfg, 1, lib), hip_engine(mod, cfg, "dense")])


@pytest.mark.gpu
@pytest.mark.parametrize("lib", ["default", "cand4"])
def test_vector_engine_wide3(mod, workdir, lib):
    """Batched environments (the `env >= 0` branch of lcWalkPosition) on the fallbacks: three environments of wide3 equal the
    standalone twins with their seeds."""
    if lib == "default":
        make_vec = lambda cfg, n: mod.VectorEngine(cfg, n, 1)  # noqa: E731
    else:
        path = variant_lib(lib)
        make_vec = lambda cfg, n: mod.VectorEngine._with_backend(cfg, n, 1, path)  # noqa: E731
    vector_wide3(mod, workdir, make_vec)


@pytest.mark.gpu
def test_capacity_error_is_not_silent(mod, workdir):
    """The library built with room for 2 new shadows per road: the step in which a road gets a third one ends in
    CFX_ERR_CAPACITY (overflow code 6; the poll of a step is settled by the next call), never in a silent cut."""
    lib = variant_lib("ins2")
    s = capacity_step(mod, workdir)
    assert s < 300
    cfg = lc_config(workdir, "wide3")
    eng, tw = mod.Engine._with_backend(cfg, 1, lib), twin(mod, cfg)
    assert eng.backend_name() == "hip-gfx950"
    for k in range(s):
        eng.next_step()
        tw.next_step()
        assert_equals_twin(eng, tw, _state(tw), "wide3 on ins2, step %d" % k)
    with pytest.raises(RuntimeError, match=r"lane change.*(more shadows on one road|shadows per road)"):
        eng.next_step()
        eng.get_vehicle_count()
        eng.next_step()
    del eng  # (nothing runs on it again)
