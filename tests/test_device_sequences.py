"""Random call sequences on the device: the trackers, the observation tensors, the signal plan, routes, pushes and archives in
arbitrary order, on the ring layout (block and list form), the dense layout and VectorEngine.

Every feature that keeps state on the device has a test of its own, and every one of them is a fixed script.  Here one seeded
stream of operations drives the HIP engine and the CPU twin in lockstep (the scheme of tests/test_deferred_commit.py: rounds of
1-8 operations from np.random.default_rng(seed)); every random choice comes from the generator and from the TWIN's return
values, so the stream is the same on a machine without a GPU, where the unmarked tests below run the same bodies with a
second twin in the HIP engine's place and so hold the harness, the models and the end-of-sequence conditions.

What the HIP engine is held against — never against itself:
  state             assert_same_state(hip, twin) at the end of every round; every getter's value call by call
  lane flow,        the Python models of test_lane_flow.py / test_movement_flow.py, keyed by vehicle id strings and fed after every
  movement flow     step from the twin's get_lane_vehicles / get_vehicle_speed / get_vehicle_info; reset, load, load_from_file
                    and turning a tracker on are a baseline of its model at the engine's step count
  trip statistics   the twin's observe_trips_array (held against the trip model in test_trip_stats.py), and the engine's own
                    totals (check_reference_totals) while tracking has been on since the last reset
  observations      the twin's array calls; the front tracker columns also against the lane model
  signal plan       the twin in rlTrafficLight mode, its phases set before every step from a restatement of
                    TrafficLight::passTime (test_tl_plan.pass_time) on the durations the test has set so far: the lights against
                    that model at every read, the vehicles against the driven twin at every round's end
                    (test_the_plan_comparators_premise: such a twin equals a fixed-time twin bit for bit)
Each sequence ends by asserting that it was not a quiet one (`Tally.enough`).

The two VectorEngine drivers (run_vector_sequence, and run_vector_plan_sequence with one plan, one pass_time model and one
driven twin per environment) take the network and the number of environments from their caller: grid_6x6 x 3 here,
example_1x1 x 67 in tests/test_vector_many_envs.py."""
import collections
import os
import time

import numpy as np
import pytest

import star_networks
from conftest import SHADOW_GPU, TWIN_LIB, assert_hip_backend, assert_same_state, full_state

torch = pytest.importorskip("torch")

import test_lane_flow as lane_flow  # noqa: E402
import test_movement_flow as movement_flow  # noqa: E402
import test_trip_stats as trip_stats  # noqa: E402
from test_api_sequences import _config  # noqa: E402
from test_device_tensors import tensor_device, twin  # noqa: E402
from test_tl_plan import NAN, Plan, derive, dev, on_device, pass_time  # noqa: E402

FRONT_K = 3
TRACKERS = ("lane", "move", "trip")
TORCH_OF = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64, np.dtype(np.float64): torch.float64}


# ----------------------------------------------------------------------------------------------------------------- helpers
def config(scen, workdir, net, layout, rl=False, compact=0, interval=1.0):
    """grid_6x6 under the dense demand of test_api_sequences._config, or star5; layout "ring" (block form), "list" (the ring
    layout's list form) or "dense"."""
    base = _config(scen, workdir, rl) if net == "grid_6x6" else star_networks.make(workdir, net)
    cfx = {"layout": "dense"} if layout == "dense" else {"layout": "ring", "ringLanesPerWave": 30000 if layout == "list" else 0}
    if compact:
        cfx["compactVehicles"] = compact
    tag = "seq_%s_%s_%d_%s" % (layout, "rl" if rl else "fixed", compact, interval)
    return derive(base, tag, cfx=cfx, rlTrafficLight=bool(rl), interval=interval)


def hip_engine(mod, cfg, layout):
    eng = mod.Engine(cfg, 1)
    assert_hip_backend(eng)
    assert eng._layout() == ("dense" if layout == "dense" else "ring")
    return eng


def filled(eng, shape, dtype):
    """A tensor of a value no output takes: every element must be written."""
    return torch.full(tuple(shape), -7, dtype=TORCH_OF[np.dtype(dtype)], device=tensor_device(eng))


def same(got, want, where):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (where, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), "%s differs" % where


def neighbour(road, arms, rng):
    """A road next to `road` (the anchor of test_api_sequences.py): usually a valid reroute, a U-turn now and then."""
    if road.startswith("road_"):
        x, y, dirn = (int(t) for t in road.split("_")[1:])
        return "road_%d_%d_%d" % (x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn], int(rng.integers(0, 4)))
    if road.startswith("in_"):
        return "out_%d" % int(rng.integers(0, arms))
    return "in_0" if road == "far_in" else "far_out" if road == "out_0" else "in_%d" % int(rng.integers(0, arms))


def pushed_route(roads, arms, rng):
    if arms:
        i = int(rng.integers(0, arms))
        return ["in_%d" % i, "out_%d" % ((i + 1 + int(rng.integers(0, arms - 1))) % arms)]
    start = roads[int(rng.integers(0, len(roads)))]
    x, y, dirn = (int(t) for t in start.split("_")[1:])
    nxt = "road_%d_%d_%d" % (x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn], dirn)
    return [start, nxt] if nxt in roads else [start]


def draw(rng, table):
    names, weights = zip(*table)
    w = np.array(weights, dtype=np.float64)
    return names[int(rng.choice(len(names), p=w / w.sum()))]


class Tally:
    """What a sequence did, and what it must have done (the issue's conditions: they stop a quiet stream from passing)."""

    def __init__(self):
        self.ops = collections.Counter()
        self.steps = 0            # the engine's step count (a load sets it back, a reset to 0)
        self.clock = 0            # next_step calls so far
        self.run = 0              # ... since the last call that was not a step
        self.long_runs_read = 0   # runs of 9 or more steps that a read followed directly
        self.merged = 0           # steps whose predecessor's commit must have ridden with their admission (see run_sequence)
        self.drains = collections.defaultdict(set)
        self.ever_on = set()
        self.off_at = {}
        self.on_again = 0
        self.loads_back_tracked = 0
        self.resets = 0
        self.verdicts = set()
        self.totals_checked = 0
        self.commit_launches = 0
        self.flow = collections.Counter()  # per flow tracker: vehicles that left plus waiting steps, over the model's drains
        self.flow_checked = ()    # the trackers whose drains go through a model (run_sequence)
        self.exact_totals = False

    def read(self):
        if self.run >= 9:
            self.long_runs_read += 1
        self.run = 0

    def enough(self, kinds, where, reroutes=True, loads=True, merged=True):
        few = sorted(k for k in kinds if self.ops[k] < 2)
        assert not few, "%s: operation kinds that ran less than twice: %s" % (where, few)
        for t in self.ever_on & {"lane", "move"}:
            assert self.drains[t] == {True, False}, "%s: the %s tracker was drained with reset in %s only" % (where, t, sorted(self.drains[t]))
        for t in self.ever_on:
            assert self.drains[t], "%s: the %s tracker was never read" % (where, t)
        assert self.resets >= 1, where + ": no reset"
        assert self.long_runs_read >= 2, "%s: %d runs of 9 or more steps were followed directly by a read" % (where, self.long_runs_read)
        if loads:
            assert self.loads_back_tracked >= 1, where + ": no load went back to an earlier step while a tracker was on"
        if self.ever_on:
            assert self.on_again >= 1, where + ": no tracker was switched off and on again with steps in between"
        if reroutes:
            assert self.verdicts == {True, False}, "%s: reroute verdicts %s" % (where, sorted(self.verdicts))
        for t in self.ever_on & set(self.flow_checked):
            assert self.flow[t] > 0, "%s: the %s tracker's drains never held a vehicle that left or waited" % (where, t)
        if self.exact_totals and "trip" in self.ever_on:
            assert self.totals_checked >= 1, where + ": the trip tracker's totals were never held against the engine's own"
        if merged:
            assert self.merged >= 1, where + ": no run of ten steps with every tracker off: no commit rode with the next admission"


def profile_begin(hip, ring):
    on = ring and not SHADOW_GPU and hip._device_buffers()
    if on:
        hip.sync()
        hip._profile_enable(True)
    return on


def profile_round(hip, tally):
    # (reading launchNamed: profiling changes how a kernel is launched — with a pair of events — never which kernels a step launches)
    tally.commit_launches += hip._profile_read()["k_commit"][1]


def profile_end(hip, tally, where):
    hip._profile_enable(False)
    assert 0 < tally.commit_launches < tally.clock, \
        "%s: %d k_commit launches over %d steps: deferred and standalone commits did not alternate" % (where, tally.commit_launches, tally.clock)


# ------------------------------------------------------------------------------------------- control + trackers + observations
OPS = (("steps", 9.0), ("count_array", 1.0), ("count_tensor", 1.0), ("phases", 1.0), ("phases_tensor", 1.0), ("speed", 1.0),
       ("speed_buffered", 1.0), ("getters", 1.0), ("snapshot", 1.2), ("load", 1.4), ("dump", 1.0), ("load_file", 1.2),
       ("reset", 0.45), ("reseed_reset", 0.45), ("reroute", 2.0), ("push", 1.0), ("track", 2.5), ("all_off", 0.6), ("drain", 3.0),
       ("observe_lanes", 1.2), ("observe_intersections", 1.0))
RL_ONLY = ("phases", "phases_tensor")


def run_sequence(hip, tw, seed, rounds, rl, tmp_path, where, ring=False, compact=False):
    rng = np.random.default_rng(seed)
    t = Tally()
    t.flow_checked, t.exact_totals = ("lane", "move"), True
    lanes = list(tw.lane_ids())
    assert list(hip.lane_ids()) == lanes and hip.intersection_ids() == tw.intersection_ids()
    L, n_inter = len(lanes), len(tw.intersection_ids())
    roads = sorted({lane.rsplit("_", 1)[0] for lane in lanes})
    arms = sum(r.startswith("in_") for r in roads)
    phase_counts = tw._phase_counts()
    edges = tw.lane_lengths()[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, np.inf])
    feed = movement_flow.reference_feed(tw, tw)
    models = {"lane": lane_flow.Model(lanes), "move": movement_flow.Model(tw._flat_net(), n_inter)}
    on = dict.fromkeys(TRACKERS, False)
    archives = files = None
    n_files = 0
    fresh = True        # no step and no load since the engine was made or reset
    trip_exact = False  # the trip tracker has been on since then: its totals are the engine's own
    pushed = False      # a vehicle was pushed since the last step (the reference counts it at once, the tracker with the next step)
    profiling = profile_begin(hip, ring)
    table = [(k, w) for k, w in OPS if rl or k not in RL_ONLY]
    kinds = [k for k, _ in table]

    def at():
        return "%s seed %d, step %d (call %d)" % (where, seed, t.steps, sum(t.ops.values()))

    def baseline(which):
        if which == "lane":
            models["lane"].baseline(tw.get_lane_vehicles(), t.steps)
        elif which == "move":
            models["move"].baseline(feed()[0], t.steps)

    def set_tracker(which, state):
        for e in (hip, tw):
            getattr(e, {"lane": "track_lane_flow", "move": "track_movement_flow", "trip": "track_trips"}[which])(state)
        on[which] = state

    def phases():
        ph = np.array([int(rng.integers(0, c)) if c > 0 else 0 for c in phase_counts], dtype=np.int32)
        return ph

    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 9))):
            op = draw(rng, table)
            if op == "steps":
                # A run with every tracker off and no read: the lane counts' publishing (`observing` / `devObserving`, cfx_hip.hip)
                # expires with the 9th step, which defers its commit; the 10th step's admission then carries that commit.
                for _ in range(int(rng.integers(1, 15))):
                    hip.next_step()
                    tw.next_step()
                    t.steps, t.clock, t.run = t.steps + 1, t.clock + 1, t.run + 1
                    t.merged += t.run >= 10 and not any(on.values())
                    if on["lane"]:
                        models["lane"].tick(tw.get_lane_vehicles(), tw.get_vehicle_speed(), t.steps)
                    if on["move"]:
                        models["move"].tick(*feed(), t.steps)
                fresh = pushed = False
                t.ops[op] += 1
                continue
            if op in ("count_array", "count_tensor", "getters", "drain", "observe_lanes", "observe_intersections"):
                t.read()
            t.run = 0
            if op == "count_array":
                same(hip.get_lane_vehicle_count_array(), tw.get_lane_vehicle_count_array(), at() + ": lane counts")
            elif op == "count_tensor":
                same(hip.get_lane_vehicle_count_tensor(out=filled(hip, (L,), np.int32)), tw.get_lane_vehicle_count_array(), at() + ": lane count tensor")
                same(hip.get_lane_waiting_vehicle_count_tensor(), tw.get_lane_waiting_vehicle_count_array(), at() + ": waiting count tensor")
            elif op == "phases":
                ph = phases()
                hip.set_tl_phases(ph)
                tw.set_tl_phases(ph)
            elif op == "phases_tensor":  # -1 keeps a signal's phase: the twin is given the phase it has
                ph = np.where(rng.random(n_inter) < 0.3, -1, phases()).astype(np.int32)
                hip.set_tl_phases_tensor(dev(hip, ph))
                tw.set_tl_phases(np.where(ph == -1, np.asarray(tw._tl_state()[0]), ph).astype(np.int32))
            elif op == "speed":
                speeds = tw.get_vehicle_speed()
                assert hip.get_vehicle_speed() == speeds, at()
                if not speeds:
                    continue
                vid = sorted(speeds)[int(rng.integers(0, len(speeds)))]
                v = float(rng.uniform(0.0, 12.0))
                hip.set_vehicle_speed(vid, v)
                tw.set_vehicle_speed(vid, v)
                assert hip.get_vehicle_info(vid) == tw.get_vehicle_info(vid), at()
            elif op == "speed_buffered":  # a vehicle that still waits in its lane's buffer: the speed takes effect in its first step
                everybody, running = tw.get_vehicles(True), set(tw.get_vehicles())
                assert sorted(hip.get_vehicles(True)) == sorted(everybody) and set(hip.get_vehicles()) == running, at()
                first = {}  # per flow (and among the pushed ones) the oldest: the next its lane admits
                for v in everybody:
                    if v not in running:
                        flow, n = v.rsplit("_", 1)
                        first[flow] = min(first.get(flow, int(n)), int(n))
                if not first:
                    continue
                flow = sorted(first)[int(rng.integers(0, len(first)))]
                vid = "%s_%d" % (flow, first[flow])
                v = float(rng.uniform(0.0, 9.0))
                hip.set_vehicle_speed(vid, v)
                tw.set_vehicle_speed(vid, v)
                assert hip.get_vehicle_info(vid) == tw.get_vehicle_info(vid), at()
            elif op == "getters":
                assert hip.get_vehicle_count() == tw.get_vehicle_count(), at()
                assert hip.get_lane_waiting_vehicle_count() == tw.get_lane_waiting_vehicle_count(), at()
                assert hip.get_lane_vehicles() == tw.get_lane_vehicles(), at()
                assert hip.get_vehicle_distance() == tw.get_vehicle_distance(), at()
                assert hip.get_current_time() == tw.get_current_time(), at()
                assert hip.get_average_travel_time() == tw.get_average_travel_time(), at()
            elif op == "snapshot":
                archives = (hip.snapshot(), tw.snapshot(), t.steps)
            elif op in ("load", "load_file"):
                if (archives if op == "load" else files) is None:
                    continue
                if op == "load":
                    hip.load(archives[0])
                    tw.load(archives[1])
                    back_to = archives[2]
                else:  # both load the file the HIP engine wrote
                    hip.load_from_file(files[0])
                    tw.load_from_file(files[0])
                    back_to = files[1]
                t.loads_back_tracked += back_to < t.steps and any(on.values())
                t.steps = back_to
                fresh = trip_exact = pushed = False
                for which in TRACKERS:
                    if on[which]:
                        baseline(which)
            elif op == "dump":
                n_files += 1
                files = (os.path.join(str(tmp_path), "seq%d.json" % n_files), t.steps)
                hip.snapshot().dump(files[0])
            elif op in ("reset", "reseed_reset"):
                if op == "reseed_reset":
                    # (one step first: the reference's reset frees the vehicles but leaves those pushed since the last step in
                    # their road's planRouteBuffer — tests/test_api_sequences.py)
                    hip.next_step()
                    tw.next_step()
                    t.clock += 1
                    new_seed = int(rng.integers(0, 1000))
                    hip.set_random_seed(new_seed)
                    tw.set_random_seed(new_seed)
                hip.reset(op == "reseed_reset")
                tw.reset(op == "reseed_reset")
                archives = files = None
                t.steps, t.resets = 0, t.resets + 1
                fresh, trip_exact, pushed = True, on["trip"], False
                for which in TRACKERS:
                    if on[which]:
                        baseline(which)
            elif op == "reroute":
                ids = sorted(tw.get_vehicles())
                if not ids:
                    continue
                vid = ids[int(rng.integers(0, len(ids)))]
                info = tw.get_vehicle_info(vid)
                assert hip.get_vehicle_info(vid) == info, at()
                anchor = neighbour(info["road"], arms, rng) if info.get("road") else None
                if anchor not in roads:
                    continue
                a, b = hip.set_vehicle_route(vid, [anchor]), tw.set_vehicle_route(vid, [anchor])
                assert a == b, "%s: set_vehicle_route(%s, %s) says %s, the twin %s" % (at(), vid, anchor, a, b)
                assert hip.get_vehicle_info(vid) == tw.get_vehicle_info(vid), at()
                t.verdicts.add(b)
            elif op == "push":
                info = {"length": float(rng.uniform(3.0, 8.0)), "maxSpeed": float(rng.uniform(8.0, 16.0)), "minGap": 2.5}
                route = pushed_route(roads, arms, rng)
                hip.push_vehicle(info, route)
                tw.push_vehicle(info, route)
                pushed = True
                assert sorted(hip.get_vehicles(True)) == sorted(tw.get_vehicles(True)), at()
            elif op == "track":
                which = TRACKERS[int(rng.integers(0, len(TRACKERS)))]
                set_tracker(which, not on[which])
                if on[which]:
                    t.ever_on.add(which)
                    t.on_again += which in t.off_at and t.clock > t.off_at[which]
                    baseline(which)
                    if which == "trip":
                        trip_exact = fresh
                else:
                    t.off_at[which] = t.clock
            elif op == "all_off":
                if not any(on.values()):
                    continue
                for which in TRACKERS:
                    if on[which]:
                        set_tracker(which, False)
                        t.off_at[which] = t.clock
            elif op == "drain":
                live = [k for k in TRACKERS if on[k]]
                if not live:
                    continue
                which = live[int(rng.integers(0, len(live)))]
                reset = bool(rng.integers(0, 2))
                if which == "trip":  # (its accumulators are never reset)
                    want = tw.observe_trips_array()
                    out = {k: filled(hip, (), trip_stats.DTYPES[k]) for k in trip_stats.NAMES}
                    hip.observe_trips_tensor(**out)
                    got = {k: out[k].cpu().numpy() for k in trip_stats.NAMES}
                    for k in trip_stats.NAMES:
                        same(got[k], want[k], "%s: trips %s" % (at(), k))
                    if trip_exact and not pushed:
                        trip_stats.check_reference_totals(hip, got, at())
                        t.totals_checked += 1
                    t.drains[which].add(False)
                else:
                    m = lane_flow if which == "lane" else movement_flow
                    peek, want = models[which].outputs(), models[which].drain(reset)
                    theirs = (tw.observe_lane_flow_array if which == "lane" else tw.observe_movement_flow_array)(reset=reset)
                    for k in m.NAMES:  # (the twin's tracker against the model: the harness itself)
                        same(theirs[k], peek[k], "%s: the twin's %s %s" % (at(), which, k))
                    m.check_drain(hip, peek, want, reset, "%s %s" % (at(), which))
                    t.drains[which].add(reset)
                    t.flow[which] += int(want["left"].sum()) + int(want["waiting_steps"].sum())
            elif op == "observe_lanes":
                out = {"counts": filled(hip, (L,), np.int32), "waiting": filled(hip, (L,), np.int32), "speed_sum": filled(hip, (L,), np.float64),
                       "bins": filled(hip, (L, 3), np.int32), "front_distance": filled(hip, (L, FRONT_K), np.float64),
                       "front_speed": filled(hip, (L, FRONT_K), np.float64)}
                if on["lane"]:
                    out["front_lane_steps"] = filled(hip, (L, FRONT_K), np.int32)
                    out["front_waiting_steps"] = filled(hip, (L, FRONT_K), np.int32)
                hip.observe_lanes_tensor(edges=dev(hip, edges), **out)
                want = dict(tw.get_lane_front_vehicles_array(FRONT_K), counts=tw.get_lane_vehicle_count_array(),
                            waiting=tw.get_lane_waiting_vehicle_count_array(), speed_sum=tw.get_lane_speed_sum_array(),
                            bins=tw.get_lane_vehicle_bins_array(edges))
                assert sorted(want) == sorted(out), at()
                for k in out:
                    same(out[k], want[k], "%s: observe_lanes_tensor %s" % (at(), k))
                if on["lane"]:  # the tracker columns against the model too
                    lv = tw.get_lane_vehicles()
                    since, wait = np.zeros((L, FRONT_K), dtype=np.int32), np.zeros((L, FRONT_K), dtype=np.int32)
                    for l, lane in enumerate(lanes):
                        for k, v in enumerate(lv[lane][:FRONT_K]):
                            since[l, k], wait[l, k] = t.steps - models["lane"].on[l][v][0], models["lane"].on[l][v][1]
                    same(out["front_lane_steps"], since, at() + ": front_lane_steps against the model")
                    same(out["front_waiting_steps"], wait, at() + ": front_waiting_steps against the model")
            elif op == "observe_intersections":
                want = tw.observe_intersections_array()
                out = {k: filled(hip, a.shape, a.dtype) for k, a in want.items()}
                hip.observe_intersections_tensor(**out)
                for k in out:
                    same(out[k], want[k], "%s: observe_intersections_tensor %s" % (at(), k))
            t.ops[op] += 1
        t.read()
        assert_same_state(hip, tw, "%s, round %d" % (at(), round_))
        if profiling:
            profile_round(hip, t)
    assert hip.get_average_travel_time() == tw.get_average_travel_time()
    t.enough(kinds, where)
    if compact:
        assert tw._vehicle_table()[1] > 0 and hip._vehicle_table() == tw._vehicle_table(), (hip._vehicle_table(), tw._vehicle_table())
    if profiling:
        profile_end(hip, t, where)
    return t


# (net, rl, compactVehicles) -> seed: chosen by running the driver twin against twin (the unmarked test below), so that
# Tally.enough holds; the stream does not depend on the layout
ROUNDS = 70
SEEDS = {("grid_6x6", True, 0): 301, ("grid_6x6", False, 0): 100, ("grid_6x6", True, 40): 401, ("grid_6x6", False, 40): 200,
         ("star5", False, 0): 501, ("star5", True, 0): 603}
GPU_CASES = [("grid_6x6", layout, rl, 0) for layout in ("ring", "list", "dense") for rl in (True, False)] + \
            [("grid_6x6", "ring", True, 40), ("grid_6x6", "dense", False, 40), ("star5", "ring", False, 0), ("star5", "dense", True, 0)]


@pytest.mark.parametrize("net,rl,compact", sorted(SEEDS))
def test_sequences_twin_against_twin(mod, scen, workdir, tmp_path, net, rl, compact):
    cfg = config(scen, workdir, net, "ring", rl, compact)
    run_sequence(twin(mod, cfg), twin(mod, cfg), SEEDS[net, rl, compact], ROUNDS, rl, tmp_path, "%s twin" % net, compact=bool(compact))


@pytest.mark.gpu
@pytest.mark.parametrize("net,layout,rl,compact", GPU_CASES)
def test_sequences_equal_twin_and_models(mod, scen, workdir, tmp_path, net, layout, rl, compact):
    cfg = config(scen, workdir, net, layout, rl, compact)
    t0 = time.perf_counter()
    run_sequence(hip_engine(mod, cfg, layout), twin(mod, cfg), SEEDS[net, rl, compact], ROUNDS, rl, tmp_path,
                 "%s %s" % (net, layout), ring=layout != "dense", compact=bool(compact))
    print("%s %s rl %s compact %d: %.1f s" % (net, layout, rl, compact, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------------------- the signal plan
PLAN_OPS = (("steps", 8.0), ("speed", 1.5), ("push", 1.0), ("reset", 0.6), ("durations", 1.0), ("durations_sparse", 1.0), ("phase", 1.0),
            ("phase_remain", 1.0), ("restore", 0.8), ("get_durations", 1.0), ("lights", 1.5), ("observe_intersections", 1.0),
            ("count_array", 1.0))


def same_vehicles(a, b, where):
    """assert_same_state without the lights: the driven twin's remaining times do not advance in rl mode."""
    sa, sb = full_state(a), full_state(b)
    for k in ("vid", "drivable", "prev_drivable", "dis", "speed", "leader", "blocker", "enter_ll_time", "route_pos"):
        assert sa[k].shape == sb[k].shape, "%s: %s count differs (%s vs %s)" % (where, k, sa[k].shape, sb[k].shape)
        assert np.array_equal(sa[k], sb[k]), "%s: %s differs" % (where, k)
    has = sa["leader"] >= 0
    assert np.array_equal(sa["gap"][has], sb["gap"][has]), "%s: gap differs" % where
    assert np.array_equal(a.get_lane_vehicle_count_array(), b.get_lane_vehicle_count_array()), where + ": lane counts"
    ca, cb = a._scalars(), b._scalars()
    for k in ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time"):
        assert ca[k] == cb[k], "%s: scalar %s differs (%r vs %r)" % (where, k, ca[k], cb[k])


def quarter(rng, low, high, size=None):
    """Multiples of 0.25 in [low, high): the same doubles in a tensor, in a sum and in the model."""
    return 0.25 * rng.integers(int(low * 4), int(high * 4), size=size)


def run_plan_sequence(hip, tw, cfg, seed, rounds, interval, where, ring=False):
    """`tw`: the twin with rlTrafficLight, driven by the model.  `hip` None: the operation stream and the driven twin alone (what
    a machine without a GPU can run of this sequence: the twin keeps no plan)."""
    rng = np.random.default_rng(seed)
    t = Tally()
    plan = Plan(tw, cfg)
    real, count = plan.real, plan.count
    T = plan.file()
    phase, remain = np.zeros(plan.I, dtype=np.int64), np.array(T[:, 0])
    lanes = list(tw.lane_ids())
    roads = sorted({lane.rsplit("_", 1)[0] for lane in lanes})
    arms = sum(r.startswith("in_") for r in roads)
    profiling = hip is not None and profile_begin(hip, ring)
    kinds = [k for k, _ in PLAN_OPS]

    def at():
        return "%s seed %d, step %d (call %d)" % (where, seed, t.steps, sum(t.ops.values()))

    def lights():
        if hip is not None:
            got_phase, got_remain = (np.asarray(a) for a in hip._tl_state())
            assert np.array_equal(got_phase[real], phase[real]), at() + ": phases differ from pass_time's"
            assert np.array_equal(got_remain[real], remain[real]), at() + ": remaining times differ from pass_time's"

    def some():
        return [i for i in real if rng.random() < 0.35]

    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 9))):
            op = draw(rng, PLAN_OPS)
            if op == "steps":
                for _ in range(int(rng.integers(1, 15))):
                    tw.set_tl_phases(phase.astype(np.int32))
                    tw.next_step()
                    if hip is not None:
                        hip.next_step()
                    pass_time(phase, remain, T, count, interval)
                    t.steps, t.clock, t.run = t.steps + 1, t.clock + 1, t.run + 1
                    t.merged += t.run >= 10
                t.ops[op] += 1
                continue
            if op in ("get_durations", "lights", "observe_intersections", "count_array"):
                t.read()
            t.run = 0
            if op == "speed":
                speeds = tw.get_vehicle_speed()
                if not speeds:
                    continue
                vid = sorted(speeds)[int(rng.integers(0, len(speeds)))]
                v = float(rng.uniform(0.0, 12.0))
                tw.set_vehicle_speed(vid, v)
                if hip is not None:
                    assert hip.get_vehicle_speed() == speeds, at()
                    hip.set_vehicle_speed(vid, v)
            elif op == "push":
                info = {"length": float(rng.uniform(3.0, 8.0)), "maxSpeed": float(rng.uniform(8.0, 16.0)), "minGap": 2.5}
                route = pushed_route(roads, arms, rng)
                tw.push_vehicle(info, route)
                if hip is not None:
                    hip.push_vehicle(info, route)
            elif op == "reset":  # keeps the durations, restarts phase and remaining time from them
                tw.next_step()  # (one step first, as in run_sequence: vehicles pushed since the last step)
                if hip is not None:
                    hip.next_step()
                    hip.reset(False)
                tw.reset(False)
                t.clock += 1
                phase[:], remain[:] = 0, T[:, 0]
                t.steps, t.resets = 0, t.resets + 1
            elif op == "durations":  # every entry; some phases of no length, the last one of a second at least
                new = np.zeros_like(T)
                for i in real:
                    new[i, :count[i]] = quarter(rng, 0.0, 8.0, count[i]) * (rng.random(count[i]) < 0.8)
                    new[i, count[i] - 1] = quarter(rng, 1.0, 8.0)
                T = new
                if hip is not None:
                    hip.set_tl_plan_tensor(durations=dev(hip, plan.dirty(T)))
            elif op == "durations_sparse":  # NaN keeps an entry
                change = np.full_like(T, NAN)
                for i in some():
                    p = int(rng.integers(0, count[i]))
                    change[i, p] = T[i, p] = quarter(rng, 1.0, 8.0)
                if hip is not None:
                    hip.set_tl_plan_tensor(durations=dev(hip, change))
            elif op == "phase":  # -1 keeps it; the remaining time is not touched
                only = np.full(plan.I, -1, dtype=np.int32)
                for i in some():
                    only[i] = phase[i] = int(rng.integers(0, count[i]))
                if hip is not None:
                    hip.set_tl_plan_tensor(phase=dev(hip, only))
            elif op == "phase_remain":
                only = np.full(plan.I, NAN)
                for i in some():
                    only[i] = remain[i] = quarter(rng, 0.0, 10.0)
                if hip is not None:
                    hip.set_tl_plan_tensor(phase_remain=dev(hip, only))
            elif op == "restore":
                T = plan.file()
                if hip is not None:
                    hip.restore_tl_plan()
            elif op == "get_durations":
                if hip is not None:
                    same(hip.get_tl_phase_durations_tensor(out=filled(hip, T.shape, np.float64)), T, at() + ": durations in force")
            elif op == "lights":
                lights()
            elif op == "observe_intersections":
                if hip is not None:
                    want = tw.observe_intersections_array()
                    out = {k: filled(hip, a.shape, a.dtype) for k, a in want.items()}
                    hip.observe_intersections_tensor(**out)
                    for k in out:
                        if k == "phase":  # (the driven twin holds the phase its last step began with)
                            assert np.array_equal(out[k].cpu().numpy()[real], phase[real]), at() + ": phase tensor"
                        elif k == "phase_remain":
                            assert np.array_equal(out[k].cpu().numpy()[real], remain[real]), at() + ": phase_remain tensor"
                        else:
                            same(out[k], want[k], "%s: observe_intersections_tensor %s" % (at(), k))
            elif op == "count_array":
                if hip is not None:
                    same(hip.get_lane_vehicle_count_array(), tw.get_lane_vehicle_count_array(), at() + ": lane counts")
            t.ops[op] += 1
        t.read()
        lights()
        if hip is not None:
            same_vehicles(hip, tw, "%s, round %d" % (at(), round_))
        if profiling:
            profile_round(hip, t)
    t.enough(kinds, where, reroutes=False, loads=False)
    assert tw.get_vehicle_count() > 0
    if profiling:
        profile_end(hip, t, where)
    return t


PLAN_ROUNDS = 80
PLAN_CASES = [("star5", 1.0, 11), ("star5", 0.5, 12), ("grid_6x6", 1.0, 13)]


def plan_config(scen, workdir, net, layout, interval, rl):
    return config(scen, workdir, net, layout, rl=rl, interval=interval)


@pytest.mark.parametrize("net,interval,seed", PLAN_CASES)
def test_plan_sequence_stream_on_the_driven_twin(mod, scen, workdir, net, interval, seed):
    cfg = plan_config(scen, workdir, net, "ring", interval, True)
    run_plan_sequence(None, twin(mod, cfg), cfg, seed, PLAN_ROUNDS, interval, "%s %s s" % (net, interval))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ring", "dense"])
@pytest.mark.parametrize("net,interval,seed", PLAN_CASES)
def test_plan_sequence_equals_pass_time_and_the_driven_twin(mod, scen, workdir, net, interval, seed, layout):
    hip = on_device(hip_engine(mod, plan_config(scen, workdir, net, layout, interval, False), layout))
    cfg = plan_config(scen, workdir, net, layout, interval, True)
    t0 = time.perf_counter()
    run_plan_sequence(hip, twin(mod, cfg), cfg, seed, PLAN_ROUNDS, interval, "%s %s %s s" % (net, layout, interval), ring=layout == "ring")
    print("plan %s %s %s s: %.1f s" % (net, layout, interval, time.perf_counter() - t0))


@pytest.mark.parametrize("net", ["grid_6x6", "star5", "example_1x1"])
def test_the_plan_comparators_premise(mod, scen, workdir, net):
    """A twin in rlTrafficLight mode whose phases are set before every step from pass_time's model equals a fixed-time twin:
    every vehicle array, and the fixed-time twin's lights equal the model — 400 steps of 0.5 s with a few custom speeds."""
    if net == "example_1x1":
        fixed_cfg, rl_cfg = (scen.materialize(net, workdir, interval=0.5, rlTrafficLight=rl) for rl in (False, True))
    else:
        fixed_cfg, rl_cfg = (plan_config(scen, workdir, net, "ring", 0.5, rl) for rl in (False, True))
    fixed, driven = twin(mod, fixed_cfg), twin(mod, rl_cfg)
    plan = Plan(fixed, fixed_cfg)
    T = plan.file()
    phase, remain = np.zeros(plan.I, dtype=np.int64), np.array(T[:, 0])
    rng = np.random.default_rng(7)
    changed = False
    for s in range(400):
        got_phase, got_remain = (np.asarray(a) for a in fixed._tl_state())
        assert np.array_equal(got_phase[plan.real], phase[plan.real]) and np.array_equal(got_remain[plan.real], remain[plan.real]), s
        changed = changed or phase.any()
        if s % 40 == 39:
            speeds = fixed.get_vehicle_speed()
            assert speeds == driven.get_vehicle_speed()
            vid = sorted(speeds)[int(rng.integers(0, len(speeds)))]
            v = float(rng.uniform(0.0, 12.0))
            fixed.set_vehicle_speed(vid, v)
            driven.set_vehicle_speed(vid, v)
        driven.set_tl_phases(phase.astype(np.int32))
        fixed.next_step()
        driven.next_step()
        pass_time(phase, remain, T, plan.count, 0.5)
        if s % 20 == 19:
            same_vehicles(fixed, driven, "%s, step %d" % (net, s))
    assert changed and fixed.get_vehicle_count() > 0


# ---------------------------------------------------------------------------------------------------------------- VectorEngine
VECTOR_OPS = (("steps", 8.0), ("count_array", 1.0), ("count_tensor", 1.0), ("phases", 1.0), ("phases_tensor", 1.0), ("reset", 0.6),
              ("speeds", 1.0), ("track", 2.5), ("all_off", 0.6), ("drain", 3.0), ("observe_lanes", 1.2), ("observe_intersections", 1.0))


HIGH_ENV = 64  # k_trip_tick's kTripLdsEnvs: environments from here on take its road straight to memory


def run_vector_sequence(vec, singles, seed, rounds, where):
    """`singles`: standalone twins seeded like the environments; every [R, ...] output row by row.  With environments beyond
    HIGH_ENV the sequence must also have had all three trackers on, read the trip tracker while one of those environments had a
    finished vehicle, observed the lanes with per-lane edges and reset while a tracker was on."""
    rng = np.random.default_rng(seed)
    t = Tally()
    R = len(singles)
    t.resets_tracked = t.trips_read_high = t.edges_observed = 0
    lanes = list(singles[0].lane_ids())
    assert list(vec.lane_ids()) == lanes and vec.num_envs == R
    L, n_inter = len(lanes), len(singles[0].intersection_ids())
    phase_counts = singles[0]._phase_counts()
    # (a row of edges per lane, and neighbouring lanes' rows differ: a kernel that took another lane's row would show)
    edges = singles[0].lane_lengths()[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, np.inf]) * (0.7 + 0.1 * (np.arange(L) % 4))[:, None]
    assert len({tuple(row) for row in edges[:4].tolist()}) == 4
    on = dict.fromkeys(TRACKERS, False)
    track ={"lane": "track_lane_flow", "move": "track_movement_flow", "trip": "track_trips"}
    kinds = [k for k, _ in VECTOR_OPS]

    def at():
        return "%s seed %d, step %d (call %d)" % (where, seed, t.steps, sum(t.ops.values()))

    def rows(call):
        return np.stack([call(e) for e in singles])

    def set_tracker(which, state):
        for e in [vec] + singles:
            getattr(e, track[which])(state)
        on[which] = state

    def phases():
        return np.array([[int(rng.integers(0, c)) if c > 0 else 0 for c in phase_counts] for _ in range(R)], dtype=np.int32)

    def give(ph):
        for r, e in enumerate(singles):
            e.set_tl_phases(ph[r])

    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 9))):
            op = draw(rng, VECTOR_OPS)
            if op == "steps":
                for _ in range(int(rng.integers(1, 15))):
                    vec.next_step()
                    for e in singles:
                        e.next_step()
                    t.steps, t.clock, t.run = t.steps + 1, t.clock + 1, t.run + 1
                t.ops[op] += 1
                continue
            if op in ("count_array", "count_tensor", "speeds", "drain", "observe_lanes", "observe_intersections"):
                t.read()
            t.run = 0
            if op == "count_array":
                same(vec.get_lane_vehicle_count_array(), rows(lambda e: e.get_lane_vehicle_count_array()), at() + ": lane counts")
                same(vec.get_lane_waiting_vehicle_count_array(), rows(lambda e: e.get_lane_waiting_vehicle_count_array()), at() + ": waiting counts")
            elif op == "count_tensor":
                same(vec.get_lane_vehicle_count_tensor(out=filled(vec, (R, L), np.int32)), rows(lambda e: e.get_lane_vehicle_count_array()),
                     at() + ": lane count tensor")
            elif op == "phases":
                ph = phases()
                vec.set_tl_phases(ph)
                give(ph)
            elif op == "phases_tensor":
                ph = np.where(rng.random((R, n_inter)) < 0.3, -1, phases()).astype(np.int32)
                vec.set_tl_phases_tensor(dev(vec, ph))
                give(np.where(ph == -1, rows(lambda e: np.asarray(e._tl_state()[0])), ph).astype(np.int32))
            elif op == "reset":
                vec.reset(False)
                for e in singles:
                    e.reset(False)
                t.steps, t.resets = 0, t.resets + 1
                t.resets_tracked += any(on.values())
            elif op == "speeds":
                for r, e in enumerate(singles):
                    assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "%s: env %d" % (at(), r)
            elif op == "track":
                which = TRACKERS[int(rng.integers(0, len(TRACKERS)))]
                set_tracker(which, not on[which])
                if on[which]:
                    t.ever_on.add(which)
                    t.on_again += which in t.off_at and t.clock > t.off_at[which]
                else:
                    t.off_at[which] = t.clock
            elif op == "all_off":
                if not any(on.values()):
                    continue
                for which in TRACKERS:
                    if on[which]:
                        set_tracker(which, False)
                        t.off_at[which] = t.clock
            elif op == "drain":
                live = [k for k in TRACKERS if on[k]]
                if not live:
                    continue
                which = live[int(rng.integers(0, len(live)))]
                reset = bool(rng.integers(0, 2)) and which != "trip"
                if which == "trip":
                    per_env = [e.observe_trips_array() for e in singles]
                    out = {k: filled(vec, (R,), trip_stats.DTYPES[k]) for k in trip_stats.NAMES}
                    vec.observe_trips_tensor(**out)
                    names = trip_stats.NAMES
                    t.trips_read_high += any(p["finished"] > 0 for p in per_env[HIGH_ENV:])
                elif which == "lane":
                    per_env = [e.observe_lane_flow_array(reset=reset) for e in singles]
                    out = lane_flow.empty_outputs(vec, lead=(R,))
                    vec.observe_lane_flow_tensor(reset=reset, **out)
                    names = lane_flow.NAMES
                else:
                    per_env = [e.observe_movement_flow_array(reset=reset) for e in singles]
                    out = movement_flow.empty_outputs(vec, lead=(R,))
                    vec.observe_movement_flow_tensor(reset=reset, **out)
                    names = movement_flow.NAMES
                for k in names:
                    same(out[k], np.stack([p[k] for p in per_env]), "%s: %s %s" % (at(), which, k))
                t.drains[which].add(reset)
            elif op == "observe_lanes":
                out = {"counts": filled(vec, (R, L), np.int32), "waiting": filled(vec, (R, L), np.int32),
                       "speed_sum": filled(vec, (R, L), np.float64), "bins": filled(vec, (R, L, 3), np.int32),
                       "front_distance": filled(vec, (R, L, FRONT_K), np.float64), "front_speed": filled(vec, (R, L, FRONT_K), np.float64)}
                if on["lane"]:
                    out["front_lane_steps"] = filled(vec, (R, L, FRONT_K), np.int32)
                    out["front_waiting_steps"] = filled(vec, (R, L, FRONT_K), np.int32)
                vec.observe_lanes_tensor(edges=dev(vec, edges), **out)
                per_env = [dict(e.get_lane_front_vehicles_array(FRONT_K), counts=e.get_lane_vehicle_count_array(),
                                waiting=e.get_lane_waiting_vehicle_count_array(), speed_sum=e.get_lane_speed_sum_array(),
                                bins=e.get_lane_vehicle_bins_array(edges)) for e in singles]
                for k in out:
                    same(out[k], np.stack([p[k] for p in per_env]), "%s: observe_lanes_tensor %s" % (at(), k))
                t.edges_observed += 1
            elif op == "observe_intersections":
                per_env = [e.observe_intersections_array() for e in singles]
                want = {k: np.stack([p[k] for p in per_env]) for k in per_env[0]}
                out = {k: filled(vec, a.shape, a.dtype) for k, a in want.items()}
                vec.observe_intersections_tensor(**out)
                for k in out:
                    same(out[k], want[k], "%s: observe_intersections_tensor %s" % (at(), k))
            t.ops[op] += 1
        t.read()
        where_ = "%s, round %d" % (at(), round_)
        same(vec.get_lane_vehicle_count_array(), rows(lambda e: e.get_lane_vehicle_count_array()), where_ + ": lane counts")
        same(vec.get_lane_waiting_vehicle_count_array(), rows(lambda e: e.get_lane_waiting_vehicle_count_array()), where_ + ": waiting counts")
        ph, rem = vec._tl_state()
        same(ph, rows(lambda e: np.asarray(e._tl_state()[0])), where_ + ": phases")
        same(rem, rows(lambda e: np.asarray(e._tl_state()[1])), where_ + ": remaining times")
        for r, e in enumerate(singles):
            assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "%s: env %d vehicle speeds" % (where_, r)
        sc, each = vec._scalars(), [e._scalars() for e in singles]
        for k in ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time"):
            assert sc[k] == sum(x[k] for x in each), "%s: scalar %s" % (where_, k)
    t.enough(kinds, where, reroutes=False, loads=False, merged=False)
    assert vec.get_vehicle_count() > 0
    if R > HIGH_ENV:
        assert t.ever_on == set(TRACKERS), "%s: trackers that were never on: %s" % (where, sorted(set(TRACKERS) - t.ever_on))
        assert t.trips_read_high >= 1, "%s: the trip tracker was never read while an environment from %d on had a finished vehicle" % (where, HIGH_ENV)
        assert t.edges_observed >= 1, where + ": no observe_lanes call with per-lane edges"
        assert t.resets_tracked >= 1, where + ": no reset while a tracker was on"
    return t


# (net, R) -> seed, chosen like SEEDS: twin against twins until Tally.enough and, at 67 environments, the conditions above hold
# (tests/test_vector_many_envs.py runs the 67 case)
VECTOR_ROUNDS = 70
VECTOR_SEEDS = {("grid_6x6", 3): 31, ("example_1x1", 67): 30}
VECTOR_SEED = VECTOR_SEEDS["grid_6x6", 3]


def vector_engines(scen, workdir, make_vec, net="grid_6x6", R=3):
    cfg = scen.materialize(net, workdir, rlTrafficLight=True)
    return make_vec(cfg, R), [scen.materialize(net, workdir, rlTrafficLight=True, seed=r) for r in range(R)]


def test_vector_sequence_twin_against_twins(mod, scen, workdir):
    vec, cfgs = vector_engines(scen, workdir, lambda cfg, R: mod.VectorEngine._with_backend(cfg, R, 1, TWIN_LIB))
    run_vector_sequence(vec, [twin(mod, c) for c in cfgs], VECTOR_SEED, VECTOR_ROUNDS, "vector twin")


@pytest.mark.gpu
def test_vector_sequence_equals_standalone_twins(mod, scen, workdir):
    vec, cfgs = vector_engines(scen, workdir, lambda cfg, R: mod.VectorEngine(cfg, R))
    t0 = time.perf_counter()
    run_vector_sequence(vec, [twin(mod, c) for c in cfgs], VECTOR_SEED, VECTOR_ROUNDS, "vector")
    print("vector grid_6x6 x3: %.1f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------- VectorEngine: one plan per environment
VECTOR_PLAN_OPS = (("steps", 8.0), ("reset", 0.6), ("durations", 1.0), ("durations_sparse", 1.0), ("phase", 1.0), ("phase_remain", 1.0),
                   ("restore", 0.8), ("get_durations", 1.0), ("lights", 1.5), ("observe_intersections", 1.0), ("count_array", 1.0))


def run_vector_plan_sequence(vec, singles, cfg, seed, rounds, interval, where):
    """run_plan_sequence for batched environments.  `vec`: a fixed-time VectorEngine on the device; `singles`: one twin per
    environment in rlTrafficLight mode, seeded like the environment, each driven before every step from ITS pass_time model
    (phase[r], remain[r], T[r]).  `vec` None: the operation stream, the models and the driven twins alone.  `cfg`: a config of
    the network (for the roadnet file's plan)."""
    rng = np.random.default_rng(seed)
    t = Tally()
    R = len(singles)
    plan = Plan(singles[0], cfg)
    real, count, I = plan.real, plan.count, plan.I
    T = np.stack([plan.file()] * R)
    phase, remain = np.zeros((R, I), dtype=np.int64), np.array(T[:, :, 0])
    kinds = [k for k, _ in VECTOR_PLAN_OPS]
    high_differed = 0  # reads at which two environments from HIGH_ENV on showed lights unlike each other's and environment 0's
    durations_differed = 0  # reads of the durations in force at which no two environments had the same
    if vec is not None:
        assert vec.num_envs == R and vec.intersection_ids() == singles[0].intersection_ids()

    def at():
        return "%s seed %d, step %d (call %d)" % (where, seed, t.steps, sum(t.ops.values()))

    def rows(call):
        return np.stack([call(e) for e in singles])

    def lights():
        nonlocal high_differed
        if vec is not None:
            got_phase, got_remain = (np.asarray(a) for a in vec._tl_state())
            assert got_phase.shape == (R, I) and got_remain.shape == (R, I), at()
            assert np.array_equal(got_phase[:, real], phase[:, real]), at() + ": phases differ from pass_time's"
            assert np.array_equal(got_remain[:, real], remain[:, real]), at() + ": remaining times differ from pass_time's"
        light = [(phase[r, real].tolist(), remain[r, real].tolist()) for r in range(R)]
        unlike = [r for r in range(HIGH_ENV, R) if light[r] != light[0]]
        high_differed += any(light[a] != light[b] for a in unlike for b in unlike)

    def some_envs():
        return [r for r in range(R) if rng.random() < 0.35]

    def some():
        return [i for i in real if rng.random() < 0.5]

    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 9))):
            op = draw(rng, VECTOR_PLAN_OPS)
            if op == "steps":
                for _ in range(int(rng.integers(1, 15))):
                    for r, e in enumerate(singles):
                        e.set_tl_phases(phase[r].astype(np.int32))
                        e.next_step()
                        pass_time(phase[r], remain[r], T[r], count, interval)
                    if vec is not None:
                        vec.next_step()
                    t.steps, t.clock, t.run = t.steps + 1, t.clock + 1, t.run + 1
                    t.merged += t.run >= 10
                t.ops[op] += 1
                continue
            if op in ("get_durations", "lights", "observe_intersections", "count_array"):
                t.read()
            t.run = 0
            if op == "reset":  # keeps the durations, restarts phase and remaining time from them
                if vec is not None:
                    vec.reset(False)
                for e in singles:
                    e.reset(False)
                phase[:], remain[:] = 0, T[:, :, 0]
                t.steps, t.resets = 0, t.resets + 1
            elif op == "durations":  # every entry of every environment; some phases of no length, the last one of a second at least
                new = np.zeros_like(T)
                for r in range(R):
                    for i in real:
                        new[r, i, :count[i]] = quarter(rng, 0.0, 8.0, count[i]) * (rng.random(count[i]) < 0.8)
                        new[r, i, count[i] - 1] = quarter(rng, 1.0, 8.0)
                T = new
                if vec is not None:
                    vec.set_tl_plan_tensor(durations=dev(vec, np.stack([plan.dirty(T[r]) for r in range(R)])))
            elif op == "durations_sparse":  # NaN keeps an entry; only some environments change
                change = np.full_like(T, NAN)
                for r in some_envs():
                    for i in some():
                        p = int(rng.integers(0, count[i]))
                        change[r, i, p] = T[r, i, p] = quarter(rng, 1.0, 8.0)
                if vec is not None:
                    vec.set_tl_plan_tensor(durations=dev(vec, change))
            elif op == "phase":  # -1 keeps it; the remaining time is not touched
                only = np.full((R, I), -1, dtype=np.int32)
                for r in some_envs():
                    for i in some():
                        only[r, i] = phase[r, i] = int(rng.integers(0, count[i]))
                if vec is not None:
                    vec.set_tl_plan_tensor(phase=dev(vec, only))
            elif op == "phase_remain":
                only = np.full((R, I), NAN)
                for r in some_envs():
                    for i in some():
                        only[r, i] = remain[r, i] = quarter(rng, 0.0, 10.0)
                if vec is not None:
                    vec.set_tl_plan_tensor(phase_remain=dev(vec, only))
            elif op == "restore":
                T = np.stack([plan.file()] * R)
                if vec is not None:
                    vec.restore_tl_plan()
            elif op == "get_durations":
                if vec is not None:
                    same(vec.get_tl_phase_durations_tensor(out=filled(vec, T.shape, np.float64)), T, at() + ": durations in force")
                durations_differed += len({T[r].tobytes() for r in range(R)}) == R
            elif op == "lights":
                lights()
            elif op == "observe_intersections":
                if vec is not None:
                    per_env =[e.observe_intersections_array() for e in singles]
                    want = {k: np.stack([p[k] for p in per_env]) for k in per_env[0]}
                    out = {k: filled(vec, a.shape, a.dtype) for k, a in want.items()}
                    vec.observe_intersections_tensor(**out)
                    for k in out:
                        if k == "phase":  # (a driven twin holds the phase its last step began with)
                            assert np.array_equal(out[k].cpu().numpy()[:, real], phase[:, real]), at() + ": phase tensor"
                        elif k == "phase_remain":
                            assert np.array_equal(out[k].cpu().numpy()[:, real], remain[:, real]), at() + ": phase_remain tensor"
                        else:
                            same(out[k], want[k], "%s: observe_intersections_tensor %s" % (at(), k))
            elif op == "count_array":
                if vec is not None:
                    same(vec.get_lane_vehicle_count_array(), rows(lambda e: e.get_lane_vehicle_count_array()), at() + ": lane counts")
            t.ops[op] += 1
        t.read()
        lights()
        if vec is not None:
            where_ = "%s, round %d" % (at(), round_)
            same(vec.get_lane_vehicle_count_array(), rows(lambda e: e.get_lane_vehicle_count_array()), where_ + ": lane counts")
            for r, e in enumerate(singles):
                assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "%s: env %d vehicle speeds" % (where_, r)
    t.enough(kinds, where, reroutes=False, loads=False)
    assert sum(e.get_vehicle_count() for e in singles) > 0
    assert durations_differed >= 1, where + ": the durations in force were never read while every environment had a plan of its own"
    if R > HIGH_ENV:
        assert high_differed >= 1, "%s: at no read did two environments from %d on differ from each other and from environment 0" % (where, HIGH_ENV)
    return t


# (net, R, interval) -> seed, chosen on the driven twins alone (tests/test_vector_many_envs.py runs them)
VECTOR_PLAN_ROUNDS = 80
VECTOR_PLAN_SEEDS = {("example_1x1", 67, 1.0): 21, ("grid_6x6", 3, 0.5): 20}


def vector_plan_engines(mod, scen, workdir, net, R, interval, make_vec):
    """(the fixed-time batched engine or None, the driven twins, a config for Plan)"""
    vec = make_vec(scen.materialize(net, workdir, interval=interval), R) if make_vec else None
    cfgs = [scen.materialize(net, workdir, interval=interval, rlTrafficLight=True, seed=r) for r in range(R)]
    return vec, [twin(mod, c) for c in cfgs], cfgs[0]
