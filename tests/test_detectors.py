"""Virtual loop detectors: track_detectors / observe_detectors_tensor / observe_detectors_array on Engine and VectorEngine
(cityflow_amd/torch_io.py; kr_detectors / kd_detectors / k_detectors_drain on the device, the host tracker of
csrc/host/detectors.cpp on the twin).

Detector d = (l, start, end) sees the FRONT position of the vehicles get_lane_vehicles() lists on lane l, front to back; "in
the zone" is start <= dis(v) < end.  After every step:
  passed                 +1 for every v on l with dis(v) >= start that was not on l after the previous step or had dis'(v) < start,
                         +1 for every v that was on l with dis'(v) < start and is on l no longer
  occupied_steps         +1 if a vehicle is in the zone
  vehicle_steps          + the vehicles in the zone
  waiting_vehicle_steps  + those of them with speed < 0.1
  speed_sum              acc = acc + t, t = the zone's speeds added front to back in one running float
  count                  the vehicles in the zone now (not accumulated)
A baseline (defining the detectors, reset, load, rollback) counts nothing, zeroes the five accumulators and remembers every
vehicle then on a lane with its current distance.

The oracle is the small model of this table below, fed only by getters that existed before the feature (get_lane_vehicles,
get_vehicle_distance, get_vehicle_speed) — never by the feature's own arrays.  It adds speed_sum in the stated order with
Python floats, so every check, speed_sum included, is array_equal."""
import time

import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB, assert_same_state

torch = pytest.importorskip("torch")

import star_networks  # noqa: E402
from test_device_tensors import tensor_device  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_lane_flow import drain_plan, hip_engine, layout_config  # noqa: E402

NAMES = ("passed", "occupied_steps", "vehicle_steps", "waiting_vehicle_steps", "speed_sum", "count")
ACCUMULATED = NAMES[:5]
DTYPES = {"passed": np.int32, "occupied_steps": np.int32, "vehicle_steps": np.int64, "waiting_vehicle_steps": np.int64,
          "speed_sum": np.float64, "count": np.int32}
INF = float("inf")


def detector_set(eng):
    """The set of the issue, from lane_lengths(): per lane (0, inf), a stop-bar zone (len - 1, inf) that gets jumped,
    (len / 2, len / 2 + 30), a second, overlapping zone on every third lane, nothing on every fifth lane, and one detector
    entirely beyond its lane's end."""
    lane, start, end = [], [], []
    for l, length in enumerate(eng.lane_lengths().tolist()):
        if l % 5 == 4:
            continue
        zones = [(0.0, INF), (max(length - 1.0, 0.0), INF), (length / 2, length / 2 + 30)]
        if l % 3 == 0:
            zones.append((length / 2 + 10, length / 2 + 60))
        if l == 1:
            zones.append((length + 5.0, length + 50.0))
        for a, b in zones:
            lane.append(l)
            start.append(a)
            end.append(b)
    return np.array(lane, dtype=np.int32), np.array(start), np.array(end)


def lanes_of(source, lane_ids):
    """Per lane, front to back: [(vehicle, distance, speed)], from the three older getters."""
    on, dis, speed = source.get_lane_vehicles(), source.get_vehicle_distance(), source.get_vehicle_speed()
    return [[(v, dis[v], speed[v]) for v in on[lane]] for lane in lane_ids]


# ------------------------------------------------------------------------------------------------------------------ oracle
class Model:
    """The table of the module docstring over lanes_of()."""

    def __init__(self, lane, start, end):
        self.dets = list(zip([int(l) for l in lane], [float(a) for a in start], [float(b) for b in end]))
        self.acc = {k: np.zeros(len(self.dets), dtype=DTYPES[k]) for k in ACCUMULATED}
        self.count = np.zeros(len(self.dets), dtype=np.int32)
        self.prev = {}  # lane -> {vehicle: distance} after the previous step
        # what a run must have looked at
        self.kinds = {"crossed": 0, "entered_beyond": 0, "entered_beyond_a_start_above_zero": 0, "jumped": 0}
        self.most_in_a_zone = self.longest_walk = self.ticks = 0
        self.occupied_total = np.zeros(len(self.dets), dtype=np.int64)
        self.waiting_total = 0

    def _remember(self, lanes):
        self.prev = {l: {v: d for v, d, _ in lanes[l]} for l in {l for l, _, _ in self.dets}}

    def _counts(self, lanes):
        for i, (l, a, b) in enumerate(self.dets):
            self.count[i] = sum(1 for _, d, _ in lanes[l] if a <= d < b)

    def baseline(self, lanes):
        for x in self.acc.values():
            x[:] = 0
        self._counts(lanes)
        self._remember(lanes)

    def tick(self, lanes):
        self.ticks += 1
        for i, (l, a, b) in enumerate(self.dets):
            prev, now = self.prev[l], lanes[l]
            self.longest_walk = max(self.longest_walk, len(now))
            here = set()
            for v, d, _ in now:
                here.add(v)
                if d >= a and (v not in prev or prev[v] < a):
                    self.acc["passed"][i] += 1
                    if v in prev:
                        self.kinds["crossed"] += 1
                    else:
                        self.kinds["entered_beyond"] += 1
                        self.kinds["entered_beyond_a_start_above_zero"] += a > 0
            for v, d in prev.items():
                if v not in here and d < a:
                    self.acc["passed"][i] += 1
                    self.kinds["jumped"] += 1
            zone = [s for _, d, s in now if a <= d < b]
            waiting = sum(1 for s in zone if s < 0.1)
            t = 0.0
            for s in zone:  # (front to back: the order is part of the definition)
                t = t + s
            self.acc["occupied_steps"][i] += 1 if zone else 0
            self.acc["vehicle_steps"][i] += len(zone)
            self.acc["waiting_vehicle_steps"][i] += waiting
            self.acc["speed_sum"][i] = float(self.acc["speed_sum"][i]) + t
            self.count[i] = len(zone)
            self.most_in_a_zone = max(self.most_in_a_zone, len(zone))
            self.occupied_total[i] += 1 if zone else 0
            self.waiting_total += waiting
        self._remember(lanes)

    def outputs(self):
        o = {k: a.copy() for k, a in self.acc.items()}
        o["count"] = self.count.copy()
        return o

    def drain(self, reset):
        o = self.outputs()
        if reset:
            for a in self.acc.values():
                a[:] = 0
        return o


def empty_outputs(eng, n, lead=()):
    # (filled with a value no output takes: every element must be written)
    return {k: torch.full(lead + (n,), -7, dtype=getattr(torch, np.dtype(DTYPES[k]).name), device=tensor_device(eng)) for k in NAMES}


def check_drain(eng, want_peek, want, reset, where):
    """The array call without a reset, then the tensor call with `reset`; both against the model.  Returns what the engine gave."""
    got = eng.observe_detectors_array()
    assert sorted(got) == sorted(NAMES)
    for k in NAMES:
        assert got[k].dtype == DTYPES[k] and got[k].shape == want_peek[k].shape, "%s: %s is %s %s" % (where, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want_peek[k]), "%s: %s differs (array call)" % (where, k)
    t = empty_outputs(eng, want["passed"].shape[-1], lead=want["passed"].shape[:-1])
    eng.observe_detectors_tensor(reset=reset, **t)
    for k in NAMES:
        assert np.array_equal(t[k].cpu().numpy(), want[k]), "%s: %s differs (tensor call, reset=%s)" % (where, k, reset)
    return {k: t[k].cpu().numpy() for k in NAMES}


def assert_looked_at_something(model, kinds, after_reset, where):
    for kind in ("crossed", "entered_beyond", "jumped"):
        assert model.kinds[kind] > 0, "%s: no vehicle passed a detector as '%s' (%s)" % (where, kind, model.kinds)
    assert model.most_in_a_zone >= 2, "%s: no zone ever held two vehicles" % where
    assert model.longest_walk > 16, "%s: no detector lane was walked with more than 16 vehicles (most: %d)" % (where, model.longest_walk)
    assert ((model.occupied_total > 0) & (model.occupied_total < model.ticks)).any(), "%s: no detector was occupied part of the time" % where
    assert model.waiting_total > 0, "%s: no vehicle waited in a zone" % where
    assert after_reset > 0, "%s: no drain after a reset=True drain was non-zero" % where
    assert kinds == {True, False}, "%s: drains of both kinds are needed: %s" % (where, kinds)


def run_against_model(eng, source, steps, where):
    """`source`: the engine whose older getters feed the model (the reference in lockstep, or `eng` itself)."""
    lane, start, end = detector_set(eng)
    ids = eng.lane_ids()
    assert not eng.detector_tracking()
    eng.track_detectors(lane, start, end)
    assert eng.detector_tracking()
    layout = eng.detector_layout()
    assert layout["lane"].dtype == np.int32 and layout["start"].dtype == np.float64 and layout["end"].dtype == np.float64
    assert np.array_equal(layout["lane"], lane) and np.array_equal(layout["start"], start) and np.array_equal(layout["end"], end)
    model = Model(lane, start, end)
    model.baseline(lanes_of(source, ids))
    plan, kinds = drain_plan(steps), set()
    was_reset, after_reset = False, 0
    beyond = lane.tolist().index(1) + (4 if 1 % 3 == 0 else 3)  # the detector entirely beyond lane 1's end
    assert start[beyond] > eng.lane_lengths()[1]
    for s in range(steps):
        eng.next_step()
        if source is not eng:
            source.next_step()
        model.tick(lanes_of(source, ids))
        if s in plan:
            at = "%s, step %d" % (where, s)
            peek = model.outputs()
            out = check_drain(eng, peek, model.drain(plan[s]), plan[s], at)
            # (nothing is ever IN a zone beyond the lane's end; by the second rule of `passed` every vehicle that leaves the lane
            # was upstream of it and is counted, which the comparison with the model has just checked)
            assert not any(out[k][beyond] for k in NAMES[1:]), at + ": the detector beyond the lane's end saw something"
            kinds.add(plan[s])
            after_reset += was_reset and any(out[k].any() for k in ACCUMULATED)
            was_reset = plan[s]
    assert_looked_at_something(model, kinds, after_reset, where)
    return model


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
@pytest.mark.parametrize("name", ["grid_6x6", "example_1x1"])
def test_equals_the_model_fed_by_the_reference(mod, ref_module, scen, workdir, name):
    cfg = scen.materialize(name, workdir)
    ref = ref_module.Engine(cfg, 1)
    run_against_model(twin(mod, cfg), ref, 400, name)
    time.sleep(0.2)  # reference destructor race
    del ref


def star7_body(eng, where):
    model = run_against_model(eng, eng, 400, where)
    assert model.longest_walk > 64, "%s: no detector lane held more than 64 vehicles (most: %d)" % (where, model.longest_walk)
    assert model.kinds["entered_beyond_a_start_above_zero"] > 0, where + ": no entrant was already beyond a start > 0"
    assert {25.0, 800.0} <= set(eng.lane_lengths().tolist())


def test_equals_the_model_on_star7(mod, workdir):
    star7_body(twin(mod, star_networks.make(workdir, "star7")), "star7")


def accumulators_are_zero(eng, model, where):
    got = eng.observe_detectors_array()
    for k in ACCUMULATED:
        assert not got[k].any(), "%s: %s is not zero after a baseline" % (where, k)
    assert np.array_equal(got["count"], model.count), where + ": count is not as of now"
    assert eng.detector_tracking(), where


def follow(eng, model, steps, where):
    ids = eng.lane_ids()
    for s in range(steps):
        eng.next_step()
        model.tick(lanes_of(eng, ids))
    want, got = model.outputs(), eng.observe_detectors_array()
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (where, k)
    return want


def baseline_rules_body(make, cfg, tmp_path):
    eng = make(cfg)
    ids = eng.lane_ids()
    lane, start, end = detector_set(eng)
    assert not eng.detector_tracking()
    for s in range(120):
        eng.next_step()
    assert eng.get_lane_vehicle_count_array().sum() > 50
    # turned on mid-run: the vehicles already there have passed nothing, and are known with their distances
    eng.track_detectors(lane, start, end)
    model = Model(lane, start, end)
    model.baseline(lanes_of(eng, ids))
    accumulators_are_zero(eng, model, "turned on at step 120")
    assert model.count.sum() > 50
    want = follow(eng, model, 40, "after turning on at step 120")
    assert want["passed"].sum() > 0 and want["waiting_vehicle_steps"].sum() > 0 and model.kinds["crossed"] > 0
    archive = eng.snapshot()
    path = str(tmp_path / "detectors_archive.json")
    archive.dump(path)
    follow(eng, model, 30, "after the snapshot")
    eng.load(archive)
    model.baseline(lanes_of(eng, ids))
    accumulators_are_zero(eng, model, "load")
    follow(eng, model, 30, "after load")
    eng.load_from_file(path)
    model.baseline(lanes_of(eng, ids))
    accumulators_are_zero(eng, model, "load_from_file")
    follow(eng, model, 30, "after load_from_file")
    if not eng._checkpoint_unsupported():  # (the ring layout of the HIP engine only)
        ck = eng.checkpoint()
        follow(eng, model, 25, "after the checkpoint")
        eng.rollback(ck)
        model.baseline(lanes_of(eng, ids))
        accumulators_are_zero(eng, model, "rollback")
        follow(eng, model, 25, "after rollback")
    eng.reset()
    model.baseline(lanes_of(eng, ids))
    accumulators_are_zero(eng, model, "reset")
    want = follow(eng, model, 60, "after reset")
    assert want["passed"].sum() > 0
    # redefinition while on: another set, a new baseline
    keep = np.arange(len(lane)) % 2 == 0
    lane2, start2, end2 = lane[keep][::-1].copy(), (start[keep] + 3.0)[::-1].copy(), end[keep][::-1].copy()
    eng.track_detectors(lane2.tolist(), start2.tolist(), end2.tolist())
    assert np.array_equal(eng.detector_layout()["lane"], lane2) and np.array_equal(eng.detector_layout()["start"], start2)
    model = Model(lane2, start2, end2)
    model.baseline(lanes_of(eng, ids))
    accumulators_are_zero(eng, model, "defined again")
    want = follow(eng, model, 40, "after defining again")
    assert want["passed"].sum() > 0
    # off and on again: a new baseline; off: the observe calls raise and the layout is gone
    eng.track_detectors(on=False)
    assert not eng.detector_tracking()
    with pytest.raises(RuntimeError):
        eng.observe_detectors_array()
    with pytest.raises(RuntimeError):
        eng.detector_layout()
    with pytest.raises(ValueError):
        eng.track_detectors()  # (nothing to turn on)
    eng.next_step()
    eng.track_detectors(lane, start, end)
    model = Model(lane, start, end)
    model.baseline(lanes_of(eng, ids))
    accumulators_are_zero(eng, model, "turned on again")
    follow(eng, model, 20, "after turning on again")
    return eng


def test_baseline_rules(mod, scen, workdir, tmp_path):
    baseline_rules_body(lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir), tmp_path)


def compaction_body(make, scen, workdir, steps=300):
    a = make(scen.materialize("grid_6x6", workdir, cfx={"compactVehicles": 40}))
    b = make(scen.materialize("grid_6x6", workdir, cfx={"compactVehicles": 0}))
    lane, start, end = detector_set(a)
    a.track_detectors(lane, start, end)
    b.track_detectors(lane, start, end)
    plan = drain_plan(steps)
    passed = 0
    for s in range(steps):
        a.next_step()
        b.next_step()
        if s in plan:
            ga, gb = a.observe_detectors_array(reset=plan[s]), b.observe_detectors_array(reset=plan[s])
            for k in NAMES:
                assert np.array_equal(ga[k], gb[k]), "step %d: %s differs from the engine that never compacts" % (s, k)
            passed += int(gb["passed"].sum())
    assert a._vehicle_table()[1] >= 2 and b._vehicle_table()[1] == 0, (a._vehicle_table(), b._vehicle_table())
    assert passed > 0 and gb["speed_sum"].sum() > 0


def test_compaction_is_invisible(mod, scen, workdir):
    compaction_body(lambda cfg: twin(mod, cfg), scen, workdir)


def vector_body(vec, singles, steps, every):
    """A VectorEngine against standalone engines of the environments' seeds.  Returns whether rollback(ck, envs=) was checked
    (engines with checkpoints in device memory only)."""
    R = len(singles)
    lane, start, end = detector_set(singles[0])
    N = len(lane)
    vec.track_detectors(lane, start, end)
    for e in singles:
        e.track_detectors(lane, start, end)
    assert np.array_equal(vec.detector_layout()["lane"], lane)

    def run(steps, sources, where):
        seen, differ = 0, 0
        for s in range(steps):
            vec.next_step()
            for e in set(sources):
                e.next_step()
            if s % every != every - 1:
                continue
            reset = (s // every) % 2 == 0
            peek = {id(e): e.observe_detectors_array() for e in set(sources)}
            got = vec.observe_detectors_array()
            t = empty_outputs(singles[0], N, lead=(R,))
            vec.observe_detectors_tensor(reset=reset, **t)
            if reset:
                for e in set(sources):
                    e.observe_detectors_array(reset=True)
            for k in NAMES:
                w = np.stack([peek[id(e)][k] for e in sources])
                assert got[k].shape == (R, N) and got[k].dtype == DTYPES[k], k
                assert np.array_equal(got[k], w), "%s, step %d: %s (array)" % (where, s, k)
                assert np.array_equal(t[k].cpu().numpy(), w), "%s, step %d: %s (tensor)" % (where, s, k)
            seen += int(got["passed"].sum())
            differ += not (np.array_equal(got["passed"][0], got["passed"][1]) and np.array_equal(got["passed"][0], got["passed"][2]))
        assert seen > 0, where
        return differ

    assert run(steps, singles, "three seeds") > 0, "the environments never differed"
    if vec._checkpoint_unsupported():
        return False
    # rollback(ck, envs=): a baseline, and slot r goes on as envs[r] does from its own checkpoint
    ck, cks = vec.checkpoint(), [e.checkpoint() for e in singles]
    run(every, singles, "past the checkpoint")
    envs = [1, 1, 0]
    vec.rollback(ck, envs=envs)
    for e, c in zip(singles, cks):
        e.rollback(c)
    got = vec.observe_detectors_array()
    for k in ACCUMULATED:
        assert not got[k].any(), "rollback(envs=): %s is not zero" % k
    assert np.array_equal(got["count"], np.stack([singles[s].observe_detectors_array()["count"] for s in envs]))
    run(2 * every, [singles[s] for s in envs], "after rollback(envs=[1, 1, 0])")
    return True


def test_vector_engine_equals_standalone_twins(mod, workdir):
    # (star5: on the grid scenarios the seed changes nothing, here every lane of the first road is a candidate)
    vec = mod.VectorEngine._with_backend(star_networks.make(workdir, "star5"), 3, 1, TWIN_LIB)
    singles = [twin(mod, star_networks.make(workdir, "star5", seed=e)) for e in range(3)]
    assert not vector_body(vec, singles, 150, 15)  # (the twin has no checkpoints in device memory)
    with pytest.raises(NotImplementedError):
        vec.checkpoint()


def test_all_four_trackers_at_once(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    alone, together, flow_only = twin(mod, cfg), twin(mod, cfg), twin(mod, cfg)
    lane, start, end = detector_set(alone)
    whole = np.flatnonzero((start == 0.0) & np.isinf(end))
    alone.track_detectors(lane, start, end)
    together.track_lane_flow(True)
    together.track_movement_flow(True)
    together.track_trips(True)
    together.track_detectors(lane, start, end)
    flow_only.track_lane_flow(True)
    plan, entered = drain_plan(250), 0
    for s in range(250):
        for e in (alone, together, flow_only):
            e.next_step()
        if s not in plan:
            continue
        a, b = alone.observe_detectors_array(reset=plan[s]), together.observe_detectors_array(reset=plan[s])
        for k in NAMES:
            assert np.array_equal(a[k], b[k]), "step %d: %s changes with the other trackers on" % (s, k)
        f, g = together.observe_lane_flow_array(reset=plan[s]), flow_only.observe_lane_flow_array(reset=plan[s])
        for k in f:
            assert np.array_equal(f[k], g[k]), "step %d: lane-flow %s changes with the detectors on" % (s, k)
        assert np.array_equal(b["passed"][whole], f["entered"][lane[whole]]), "step %d: (l, 0, inf).passed != entered" % s
        assert np.array_equal(b["count"][whole], together.get_lane_vehicle_count_array()[lane[whole]]), "step %d: count" % s
        entered += int(f["entered"].sum())
    assert entered > 0
    assert together.observe_movement_flow_array()["entered"].sum() > 0 and together.observe_trips_array()["entered"] > 0
    assert_same_state(together, alone, "four trackers against one")


def test_argument_errors(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = twin(mod, cfg)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    L = len(eng.lane_ids())
    for e in (eng, vec):  # tracking is off
        with pytest.raises(RuntimeError):
            e.observe_detectors_array()
        with pytest.raises(RuntimeError):
            e.observe_detectors_tensor(passed=torch.zeros(3, dtype=torch.int32))
        with pytest.raises(RuntimeError):
            e.detector_layout()
    good = ([0, 1, 1], [0.0, 5.0, 250.0], [INF, 50.0, 1e9])
    eng.track_detectors(*good)
    vec.track_detectors(np.array(good[0]), np.array(good[1], dtype=np.float32), good[2])
    for s in range(30):
        eng.next_step()
    before = eng.observe_detectors_array()
    assert before["vehicle_steps"].sum() > 0

    def rejected(exc, *args):
        for e in (eng, vec):
            with pytest.raises(exc):
                e.track_detectors(*args)
            assert np.array_equal(e.detector_layout()["lane"], good[0]) and np.array_equal(e.detector_layout()["end"], good[2])
        now = eng.observe_detectors_array()
        for k in NAMES:
            assert np.array_equal(now[k], before[k]), "a rejected call changed " + k

    # 1. types first: a bool or a float in lane, whatever else is wrong with the call
    rejected(TypeError, [0, True], [0.0], [-1.0, 2.0, 3.0])
    rejected(TypeError, [0, 1.0], [0.0, 0.0], [1.0, 1.0])
    rejected(TypeError, np.array([0.0, 1.0]), [0.0], [1.0])
    rejected(TypeError, np.array([True, False]), [0.0, 0.0], [1.0, 1.0])
    rejected(TypeError, 3, [0.0], [1.0])
    rejected(TypeError, [0], ["a"], [1.0])
    # 2. then equal lengths and N >= 1, whatever the values are
    rejected(ValueError, [0, L + 7], [0.0], [1.0, 2.0])
    rejected(ValueError, [0], [0.0, 1.0], [1.0])
    rejected(ValueError, [], [], [])
    rejected(ValueError, [0], None, [1.0])
    # 3. then the values, naming the position
    for args, position in ((([0, 1, L], [0.0] * 3, [1.0] * 3), 2), (([0, -1], [0.0] * 2, [1.0] * 2), 1),
                           (([0, 1], [0.0, -0.5], [1.0, 1.0]), 1), (([0, 1], [0.0, INF], [1.0, INF]), 1),
                           (([0, 1], [float("nan"), 0.0], [1.0, 1.0]), 0), (([0, 1, 2], [0.0, 1.0, 2.0], [1.0, 2.0, 2.0]), 2),
                           (([0, 1], [0.0, 1.0], [1.0, float("nan")]), 1), (([0, 1], [5.0, 1.0], [4.0, 2.0]), 0)):
        for e in (eng, vec):
            with pytest.raises(ValueError, match="position %d" % position):
                e.track_detectors(*args)
        rejected(ValueError, *args)
    with pytest.raises(ValueError):
        vec.track_detectors([L], [0.0], [1.0])  # (the set is one environment's: lane < L)
    # the observe call: at least one output; every buffer before anything is enqueued
    N = 3
    with pytest.raises(ValueError):
        eng.observe_detectors_tensor()
    with pytest.raises(ValueError):
        eng.observe_detectors_tensor(reset=True)
    with pytest.raises(TypeError):
        eng.observe_detectors_tensor(passed=torch.zeros(N, dtype=torch.int64))
    with pytest.raises(TypeError):
        eng.observe_detectors_tensor(vehicle_steps=torch.zeros(N, dtype=torch.int32))
    with pytest.raises(TypeError):
        eng.observe_detectors_tensor(speed_sum=torch.zeros(N, dtype=torch.float32))
    with pytest.raises(TypeError):
        eng.observe_detectors_tensor(count=np.zeros(N, dtype=np.int32))
    with pytest.raises(TypeError):
        eng.observe_detectors_tensor(count=torch.zeros(N, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError):
        eng.observe_detectors_tensor(count=torch.zeros(N + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        eng.observe_detectors_tensor(count=torch.zeros(2 * N, dtype=torch.int32)[::2])  # not contiguous
    with pytest.raises(ValueError):
        vec.observe_detectors_tensor(count=torch.zeros(N, dtype=torch.int32))  # [R, N] wanted
    # nothing is written, and nothing is reset, when a later argument is wrong
    kept = torch.full((N,), -7, dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.observe_detectors_tensor(passed=kept, count=torch.zeros(N + 2, dtype=torch.int32), reset=True)
    assert bool((kept == -7).all())
    assert np.array_equal(eng.observe_detectors_array()["vehicle_steps"], before["vehicle_steps"])
    # reset zeroes all five accumulators, asked for or not, and leaves count
    count = torch.zeros(N, dtype=torch.int32)
    eng.observe_detectors_tensor(count=count, reset=True)
    after = eng.observe_detectors_array()
    assert not any(after[k].any() for k in ACCUMULATED)
    assert np.array_equal(after["count"], before["count"]) and np.array_equal(count.numpy(), before["count"])
    # the VectorEngine's outputs are [R, N]
    assert vec.observe_detectors_array()["passed"].shape == (2, N)


def test_lane_change_is_not_implemented(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    eng = twin(mod, cfg)
    with pytest.raises(NotImplementedError):
        eng.track_detectors([0], [0.0], [INF])
    assert not eng.detector_tracking()
    eng.track_detectors(on=False)  # (turning it off is no error)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    with pytest.raises(NotImplementedError):
        vec.track_detectors([0], [0.0], [INF])


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    code = ("import sys, cityflow_amd; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert hasattr(cityflow_amd.Engine, 'observe_detectors_tensor'); "
            "assert hasattr(cityflow_amd.VectorEngine, 'track_detectors'); "
            "assert not hasattr(cityflow_amd.TiledEngine, 'track_detectors')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def tracking_changes_no_result_body(make, cfg, steps=300):
    tracked, plain = make(cfg), make(cfg)
    tracked.track_detectors(*detector_set(tracked))
    for s in range(steps):
        tracked.next_step()
        plain.next_step()
    assert_same_state(tracked, plain, "tracked against untracked after %d steps" % steps)
    assert tracked.get_average_travel_time() == plain.get_average_travel_time()
    assert tracked.observe_detectors_array()["passed"].sum() > 0


def test_tracking_changes_no_result(mod, scen, workdir):
    tracking_changes_no_result_body(lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir))


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("name", ["grid_6x6", "example_1x1"])
def test_equals_the_model(mod, scen, workdir, name, layout):
    eng = hip_engine(mod, layout_config(scen, workdir, name, layout), layout)
    run_against_model(eng, eng, 400, "%s %s" % (name, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_equals_the_model_on_star7_on_the_device(mod, workdir, layout):
    star7_body(hip_engine(mod, star_networks.make(workdir, "star7", layout=layout), layout), "star7 " + layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_hip_equals_twin(mod, scen, workdir, layout):
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    eng, tw = hip_engine(mod, cfg, layout), twin(mod, cfg)
    lane, start, end = detector_set(tw)
    eng.track_detectors(lane, start, end)
    tw.track_detectors(lane, start, end)
    plan = drain_plan(300)
    for s in range(300):
        eng.next_step()
        tw.next_step()
        if s in plan:
            peek = tw.observe_detectors_array()
            check_drain(eng, peek, peek, plan[s], "step %d" % s)
            tw.observe_detectors_array(reset=plan[s])
    assert peek["passed"].sum() > 0 and peek["speed_sum"].sum() > 0 and peek["waiting_vehicle_steps"].sum() > 0


@pytest.mark.gpu
def test_baseline_rules_on_the_device(mod, scen, workdir, tmp_path):
    eng = baseline_rules_body(lambda cfg: mod.Engine(cfg, 1), scen.materialize("grid_6x6", workdir), tmp_path)
    assert SHADOW_GPU or not eng._checkpoint_unsupported(), "checkpoint / rollback was not checked: " + eng._checkpoint_unsupported()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_compaction_is_invisible_on_the_device(mod, scen, workdir, layout):
    class S:  # (scen with the layout added to every config)
        @staticmethod
        def materialize(name, wd, cfx):
            return layout_config(scen, wd, name, layout, **cfx)
    compaction_body(lambda cfg: hip_engine(mod, cfg, layout), S, workdir)


@pytest.mark.gpu
def test_vector_engine_equals_standalone(mod, workdir):
    vec = mod.VectorEngine(star_networks.make(workdir, "star5"), 3)
    singles = [mod.Engine(star_networks.make(workdir, "star5", seed=e), 1) for e in range(3)]
    assert vector_body(vec, singles, 150, 30) or SHADOW_GPU, "rollback(ck, envs=) was not checked"


@pytest.mark.gpu
def test_tables_and_rings_grow_while_tracking(mod, scen, workdir):
    import os
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense.json"), 400, seed=7, interval=2.0,
                            base_flow=os.path.join(d, "flow.json"))
    small = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring", "ringCapacityPercent": 30}), 1)
    large = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring"}), 1)
    lane, start, end = detector_set(small)
    small.track_detectors(lane, start, end)
    large.track_detectors(lane, start, end)
    plan = drain_plan(300)
    for s in range(300):
        small.next_step()
        large.next_step()
        if s in plan:
            a, b = small.observe_detectors_array(reset=plan[s]), large.observe_detectors_array(reset=plan[s])
            for k in NAMES:
                assert np.array_equal(a[k], b[k]), "step %d: %s differs from the engine that starts large" % (s, k)
    assert b["waiting_vehicle_steps"].sum() > 0 and b["passed"].sum() > 0
    if small._device_buffers():
        assert small._ring_info()[1] >= 2, small._ring_info()
        assert small._vehicle_table()[0] > 4096  # (the start-small knob starts the vehicle tables at 4096 numbers)
        assert small._host_stats(False)["table_grows_total"] > large._host_stats(False)["table_grows_total"]


@pytest.mark.gpu
def test_detectors_on_a_side_stream_without_a_host_wait(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    ids = ref.lane_ids()
    for s in range(100):  # warm: rings built, tables uploaded, traffic on the lanes
        eng.next_step()
        ref.next_step()
    lane, start, end = detector_set(eng)
    eng.track_detectors(lane, start, end)
    model = Model(lane, start, end)
    model.baseline(lanes_of(ref, ids))
    t = empty_outputs(eng, len(lane))
    eng.observe_detectors_tensor(**t)
    eng.sync()
    device = tensor_device(eng)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device=device)
    records = []
    eng._device_spin(200000)  # 200 ms of device work in front of everything below
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for s in range(8):
            eng.next_step()
            eng.observe_detectors_tensor(reset=True, **t)
            records.append({k: v.clone() for k, v in t.items()})  # consumed on `side`, then the outputs are reused
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the loop waited for the device (%.1f ms for 8 iterations behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    passed = 0
    for s in range(8):
        ref.next_step()
        model.tick(lanes_of(ref, ids))
        want = model.drain(True)
        passed += int(want["passed"].sum())
        for k in NAMES:
            assert np.array_equal(records[s][k].cpu().numpy(), want[k]), "step %d: %s" % (s, k)
    assert passed > 0
    assert_same_state(eng, ref, "after the unsynchronised loop")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_tracking_changes_no_result_free_running(mod, scen, workdir, layout):
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    tracking_changes_no_result_body(lambda c: hip_engine(mod, c, layout), cfg)
