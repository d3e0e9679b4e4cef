"""Per-lane flow and waiting-time statistics across steps: track_lane_flow / observe_lane_flow_tensor / observe_lane_flow_array
on Engine and VectorEngine (cityflow_amd/torch_io.py; kr_lane_flow / kd_lane_flow / k_lane_flow_drain on the device, the host
tracker of csrc/host/lane_flow.cpp on the twin).

After every step, with s = steps taken and P(l) = the vehicles get_lane_vehicles() lists on lane l:
  1. v new on l:          entered[l] += 1, since(v) = s, wait(v) = 0
  2. v no longer on l:    left[l] += 1, left_steps[l] += s - since(v), left_waiting_steps[l] += wait(v)
  3. v on l, speed < 0.1: wait(v) += 1
waiting_steps / max_waiting_steps are the sum / the maximum of wait over P(l).  A baseline (tracking turned on, reset, load)
starts every vehicle then on a lane at since = s, wait = 0 without counting it as entered, with all accumulators zero.

Everything is an integer: every check is array_equal.  The oracle is the small model of these three rules below, fed only by
getters that existed before the feature (get_lane_vehicles + get_vehicle_speed; at bench scale _vehicle_state()'s vid,
drivable and speed) — never by the feature's own arrays."""
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_hip_backend, assert_same_state

torch = pytest.importorskip("torch")

from test_device_tensors import tensor_device  # noqa: E402
from test_lane_features import twin  # noqa: E402

NAMES = ("entered", "left", "left_steps", "left_waiting_steps", "waiting_steps", "max_waiting_steps")
ACCUMULATED = NAMES[:4]
DTYPES = {"entered": np.int32, "left": np.int32, "left_steps": np.int64, "left_waiting_steps": np.int64,
          "waiting_steps": np.int64, "max_waiting_steps": np.int32}


# ------------------------------------------------------------------------------------------------------------------ oracle
class Model:
    """The three rules over {lane id: [vehicle ids]} and {vehicle id: speed}."""

    def __init__(self, lane_ids):
        self.lanes = list(lane_ids)
        self.on = [dict() for _ in self.lanes]  # per lane: vehicle -> [since, wait]
        self.acc = {k: np.zeros(len(self.lanes), dtype=DTYPES[k]) for k in ACCUMULATED}
        # what a run must have looked at
        self.refills = 0
        self._filled = [0] * len(self.lanes)  # 0 never had a vehicle, 1 has some, 2 had some and is empty
        self.total_left = 0
        self.max_wait = 0

    def baseline(self, lane_vehicles, s):
        self.on = [{v: [s, 0] for v in lane_vehicles[lane]} for lane in self.lanes]
        for a in self.acc.values():
            a[:] = 0

    def tick(self, lane_vehicles, speed, s):
        for l, lane in enumerate(self.lanes):
            prev, now = self.on[l], lane_vehicles[lane]
            here = set(now)
            for v in [v for v in prev if v not in here]:
                since, wait = prev.pop(v)
                self.acc["left"][l] += 1
                self.acc["left_steps"][l] += s - since
                self.acc["left_waiting_steps"][l] += wait
                self.total_left += 1
            for v in now:
                if v not in prev:
                    prev[v] = [s, 0]
                    self.acc["entered"][l] += 1
                if speed[v] < 0.1:
                    prev[v][1] += 1
                    self.max_wait = max(self.max_wait, prev[v][1])
            if prev:
                self.refills += self._filled[l] == 2
                self._filled[l] = 1
            elif self._filled[l] == 1:
                self._filled[l] = 2

    def outputs(self):
        o = {k: a.copy() for k, a in self.acc.items()}
        o["waiting_steps"] = np.array([sum(r[1] for r in d.values()) for d in self.on], dtype=np.int64)
        o["max_waiting_steps"] = np.array([max([r[1] for r in d.values()] + [0]) for d in self.on], dtype=np.int32)
        return o

    def drain(self, reset):
        o = self.outputs()
        if reset:
            for a in self.acc.values():
                a[:] = 0
        return o


class ArrayModel:
    """The same rules, vectorised over _vehicle_state()'s vid / drivable / speed (no vehicle compaction during its life)."""

    def __init__(self, n_lanes):
        self.L = n_lanes
        self.lane = np.full(0, -1, dtype=np.int64)  # by vid: the lane at the last tick, -1 = on none
        self.since = np.zeros(0, dtype=np.int64)
        self.wait = np.zeros(0, dtype=np.int64)
        self.acc = {k: np.zeros(n_lanes, dtype=np.int64) for k in ACCUMULATED}

    def _now(self, state):
        vid, drv = state["vid"].astype(np.int64), state["drivable"].astype(np.int64)
        n = max(int(vid.max()) + 1 if vid.size else 0, self.lane.size)
        grow = n - self.lane.size
        self.lane = np.concatenate([self.lane, np.full(grow, -1, dtype=np.int64)])
        self.since = np.concatenate([self.since, np.zeros(grow, dtype=np.int64)])
        self.wait = np.concatenate([self.wait, np.zeros(grow, dtype=np.int64)])
        now = np.full(n, -1, dtype=np.int64)
        on = drv < self.L
        now[vid[on]] = drv[on]
        slow = np.zeros(n, dtype=bool)
        slow[vid[on]] = state["speed"][on] < 0.1
        return now, slow

    def baseline(self, state, s):
        self.lane, _ = self._now(state)
        self.since[:] = s
        self.wait[:] = 0
        for a in self.acc.values():
            a[:] = 0

    def tick(self, state, s):
        now, slow = self._now(state)
        stay = (now == self.lane) & (now >= 0)
        gone, new = (self.lane >= 0) & ~stay, (now >= 0) & ~stay
        np.add.at(self.acc["left"], self.lane[gone], 1)
        np.add.at(self.acc["left_steps"], self.lane[gone], s - self.since[gone])
        np.add.at(self.acc["left_waiting_steps"], self.lane[gone], self.wait[gone])
        np.add.at(self.acc["entered"], now[new], 1)
        self.since[new] = s
        self.wait[new] = 0
        self.wait[slow] += 1
        self.lane = now

    def drain(self, reset):
        o = {k: a.astype(DTYPES[k]) for k, a in self.acc.items()}
        on = self.lane >= 0
        w = np.zeros(self.L, dtype=np.int64)
        np.add.at(w, self.lane[on], self.wait[on])
        m = np.zeros(self.L, dtype=np.int64)
        np.maximum.at(m, self.lane[on], self.wait[on])
        o["waiting_steps"], o["max_waiting_steps"] = w, m.astype(np.int32)
        if reset:
            for a in self.acc.values():
                a[:] = 0
        return o


def empty_outputs(eng, lead=()):
    shape = lead + (len(eng.lane_ids()),)
    # (filled with a value no output takes: every element must be written)
    return {k: torch.full(shape, -7, dtype=torch.int64 if DTYPES[k] is np.int64 else torch.int32, device=tensor_device(eng)) for k in NAMES}


def check_drain(eng, want_peek, want, reset, where):
    """The array call without a reset, then the tensor call with `reset`; both against the model.  Returns what the engine gave."""
    got = eng.observe_lane_flow_array()
    assert sorted(got) == sorted(NAMES)
    for k in NAMES:
        assert got[k].dtype == DTYPES[k] and got[k].shape == want_peek[k].shape, "%s: %s is %s %s" % (where, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want_peek[k]), "%s: %s differs (array call)" % (where, k)
    t = empty_outputs(eng)
    eng.observe_lane_flow_tensor(reset=reset, **t)
    for k in NAMES:
        assert np.array_equal(t[k].cpu().numpy(), want[k]), "%s: %s differs (tensor call, reset=%s)" % (where, k, reset)
    return {k: t[k].cpu().numpy() for k in NAMES}  # (the engine's own values: the identities are checked on them)


class Identities:
    """Per lane, at every drain: sum entered - sum left == count now - count at the baseline, and
    waiting_steps + sum left_waiting_steps == sum over the ticks of the waiting counts (a pre-existing getter)."""

    def __init__(self, eng):
        self.count0 = eng.get_lane_vehicle_count_array().astype(np.int64).reshape(-1)
        self.waiting_ticks = np.zeros_like(self.count0)
        self.tot = {k: np.zeros_like(self.count0) for k in ACCUMULATED}

    def tick(self, eng):
        self.waiting_ticks += eng.get_lane_waiting_vehicle_count_array().reshape(-1)

    def drained(self, eng, out, reset, where):
        cum = {k: self.tot[k] + out[k] for k in ACCUMULATED}
        now = eng.get_lane_vehicle_count_array().astype(np.int64).reshape(-1)
        assert np.array_equal(cum["entered"] - cum["left"], now - self.count0), where + ": entered - left != change of the counts"
        assert np.array_equal(out["waiting_steps"] + cum["left_waiting_steps"], self.waiting_ticks), where + ": waiting steps are not the ticks' waiting counts"
        if reset:
            self.tot = cum


def drain_plan(steps):
    """Irregular drain points: {step: reset}."""
    plan, s, i = {}, 0, 0
    gaps = (1, 7, 3, 19, 2, 31, 11, 5, 43)
    while True:
        s += gaps[i % len(gaps)]
        if s >= steps:
            break
        plan[s] = i % 3 != 1
        i += 1
    plan[steps - 1] = False
    return plan


def assert_looked_at_something(model, kinds, finished, drained, refills):
    assert finished > 0, "no vehicle finished"
    assert model.total_left > 0, "no vehicle left a lane"
    assert drained["left_waiting_steps"] > 0, "no lane ever reported left_waiting_steps > 0"
    assert model.max_wait >= 10, "no vehicle waited ten steps (max %d)" % model.max_wait
    assert drained["max_waiting_steps"] >= 10, "max_waiting_steps never reached 10 at a drain"
    if refills:
        assert model.refills > 0, "no lane emptied and refilled"
    assert kinds == {True, False}, "drains of both kinds are needed: %s" % kinds


def run_against_model(eng, source, steps, where, refills=False):
    """`source`: the engine whose pre-existing getters feed the model (the reference in lockstep, or `eng` itself)."""
    eng.track_lane_flow(True)
    assert eng.lane_flow_tracking()
    model = Model(eng.lane_ids())
    model.baseline(source.get_lane_vehicles(), 0)
    ident = Identities(eng)
    plan, kinds = drain_plan(steps), set()
    ever, drained = set(), {"left_waiting_steps": 0, "max_waiting_steps": 0}
    for s in range(steps):
        eng.next_step()
        if source is not eng:
            source.next_step()
        speed = source.get_vehicle_speed()
        ever |= set(speed)
        model.tick(source.get_lane_vehicles(), speed, s + 1)
        ident.tick(eng)
        if s in plan:
            at = "%s, step %d" % (where, s)
            peek = model.outputs()
            out = check_drain(eng, peek, model.drain(plan[s]), plan[s], at)
            ident.drained(eng, out, plan[s], at)
            kinds.add(plan[s])
            drained["left_waiting_steps"] += int((out["left_waiting_steps"] > 0).sum())
            drained["max_waiting_steps"] = max(drained["max_waiting_steps"], int(out["max_waiting_steps"].max()))
    assert_looked_at_something(model, kinds, len(ever - set(source.get_vehicle_speed())), drained, refills)


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
@pytest.mark.parametrize("name", ["grid_6x6", "example_1x1"])
def test_equals_the_model_fed_by_the_reference(mod, ref_module, scen, workdir, name):
    cfg = scen.materialize(name, workdir)
    run_against_model(twin(mod, cfg), ref_module.Engine(cfg, 1), 400, name, refills=name == "example_1x1")


def accumulators_are_zero(eng, where):
    got = eng.observe_lane_flow_array()
    for k in NAMES:
        assert not got[k].any(), "%s: %s is not zero after a baseline" % (where, k)
    assert eng.lane_flow_tracking(), where


def follow(eng, model, steps, where, first_step):
    for s in range(steps):
        eng.next_step()
        model.tick(eng.get_lane_vehicles(), eng.get_vehicle_speed(), first_step + s + 1)
    want = model.outputs()
    got = eng.observe_lane_flow_array()
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (where, k)
    return want


def baseline_rules_body(make, cfg, tmp_path):
    eng = make(cfg)
    assert not eng.lane_flow_tracking()
    for s in range(120):
        eng.next_step()
    assert eng.get_lane_vehicle_count_array().sum() > 50
    # turned on mid-run: the vehicles already there are not counted as entered and have not waited
    eng.track_lane_flow(True)
    accumulators_are_zero(eng, "turned on at step 120")
    model = Model(eng.lane_ids())
    model.baseline(eng.get_lane_vehicles(), 120)
    want = follow(eng, model, 40, "after turning on at step 120", 120)
    assert want["left"].sum() > 0 and want["waiting_steps"].sum() > 0
    archive = eng.snapshot()
    path = str(tmp_path / "lane_flow_archive.json")
    archive.dump(path)
    follow(eng, model, 30, "after the snapshot", 160)
    # load: a baseline on the archive's state, at the archive's step
    eng.load(archive)
    accumulators_are_zero(eng, "load")
    model.baseline(eng.get_lane_vehicles(), 160)
    follow(eng, model, 30, "after load", 160)
    eng.load_from_file(path)
    accumulators_are_zero(eng, "load_from_file")
    model.baseline(eng.get_lane_vehicles(), 160)
    follow(eng, model, 30, "after load_from_file", 160)
    eng.reset()
    accumulators_are_zero(eng, "reset")
    model.baseline(eng.get_lane_vehicles(), 0)
    want = follow(eng, model, 60, "after reset", 0)
    assert want["entered"].sum() > 0
    # off and on again: a new baseline; off: the observe calls raise
    eng.track_lane_flow(False)
    assert not eng.lane_flow_tracking()
    with pytest.raises(RuntimeError):
        eng.observe_lane_flow_array()
    eng.next_step()
    eng.track_lane_flow(True)
    accumulators_are_zero(eng, "turned on again")
    model.baseline(eng.get_lane_vehicles(), 61)
    follow(eng, model, 20, "after turning on again", 61)


def test_baseline_rules(mod, scen, workdir, tmp_path):
    baseline_rules_body(lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir), tmp_path)


def compaction_body(make, scen, workdir, steps=300):
    a = make(scen.materialize("grid_6x6", workdir, cfx={"compactVehicles": 40}))
    b = make(scen.materialize("grid_6x6", workdir, cfx={"compactVehicles": 0}))
    a.track_lane_flow(True)
    b.track_lane_flow(True)
    plan = drain_plan(steps)
    for s in range(steps):
        a.next_step()
        b.next_step()
        if s in plan:
            ga, gb = a.observe_lane_flow_array(reset=plan[s]), b.observe_lane_flow_array(reset=plan[s])
            for k in NAMES:
                assert np.array_equal(ga[k], gb[k]), "step %d: %s differs from the engine that never compacts" % (s, k)
    assert a._vehicle_table()[1] >= 2 and b._vehicle_table()[1] == 0, (a._vehicle_table(), b._vehicle_table())
    assert gb["left"].sum() + gb["waiting_steps"].sum() > 0


def test_compaction_is_invisible(mod, scen, workdir):
    compaction_body(lambda cfg: twin(mod, cfg), scen, workdir)


def vector_body(vec, singles, steps, every):
    R = len(singles)
    vec.track_lane_flow(True)
    for e in singles:
        e.track_lane_flow(True)
    seen = 0
    for s in range(steps):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % every != every - 1:
            continue
        reset = (s // every) % 2 == 0
        peek = [e.observe_lane_flow_array() for e in singles]
        got = vec.observe_lane_flow_array()
        t = empty_outputs(singles[0], lead=(R,))
        vec.observe_lane_flow_tensor(reset=reset, **t)
        if reset:
            for e in singles:
                e.observe_lane_flow_array(reset=True)
        for k in NAMES:
            w = np.stack([x[k] for x in peek])
            assert got[k].shape == w.shape and got[k].dtype == w.dtype, k
            assert np.array_equal(got[k], w), "step %d: %s (array)" % (s, k)
            assert np.array_equal(t[k].cpu().numpy(), w), "step %d: %s (tensor)" % (s, k)
        seen += int(np.stack([x["left"] for x in peek]).sum())
    assert seen > 0


def test_vector_engine_equals_standalone_twins(mod, scen, workdir):
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 3, 1, TWIN_LIB)
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=e)) for e in range(3)]
    vector_body(vec, singles, 90, 15)


def test_argument_errors_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = twin(mod, cfg)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    L = len(eng.lane_ids())
    with pytest.raises(RuntimeError):  # tracking is off
        eng.observe_lane_flow_tensor(entered=torch.zeros(L, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        eng.observe_lane_flow_array()
    with pytest.raises(RuntimeError):
        vec.observe_lane_flow_array()
    eng.track_lane_flow()
    vec.track_lane_flow(True)
    for s in range(5):
        eng.next_step()
    with pytest.raises(ValueError):
        eng.observe_lane_flow_tensor()
    with pytest.raises(ValueError):
        eng.observe_lane_flow_tensor(reset=True)
    with pytest.raises(TypeError):
        eng.observe_lane_flow_tensor(entered=torch.zeros(L, dtype=torch.int64))
    with pytest.raises(TypeError):
        eng.observe_lane_flow_tensor(left_steps=torch.zeros(L, dtype=torch.int32))
    with pytest.raises(TypeError):
        eng.observe_lane_flow_tensor(waiting_steps=torch.zeros(L, dtype=torch.float64))
    with pytest.raises(TypeError):
        eng.observe_lane_flow_tensor(left=np.zeros(L, dtype=np.int32))
    if torch.cuda.is_available():
        with pytest.raises(TypeError):  # (the twin's tensors live on the CPU)
            eng.observe_lane_flow_tensor(left=torch.zeros(L, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        eng.observe_lane_flow_tensor(left=torch.zeros(L, dtype=torch.int32, device="meta"))
    with pytest.raises(ValueError):
        eng.observe_lane_flow_tensor(max_waiting_steps=torch.zeros(L + 1, dtype=torch.int32))
    with pytest.raises(ValueError):
        eng.observe_lane_flow_tensor(entered=torch.zeros(2 * L, dtype=torch.int32)[::2])  # not contiguous
    with pytest.raises(ValueError):
        vec.observe_lane_flow_tensor(entered=torch.zeros(L, dtype=torch.int32))  # [R, L] wanted
    # nothing is written, and nothing is reset, when a later argument is wrong
    before = eng.observe_lane_flow_array()
    assert before["entered"].sum() > 0
    good = torch.full((L,), -7, dtype=torch.int32)
    with pytest.raises(ValueError):
        eng.observe_lane_flow_tensor(entered=good, max_waiting_steps=torch.zeros(L + 2, dtype=torch.int32), reset=True)
    assert bool((good == -7).all())
    assert np.array_equal(eng.observe_lane_flow_array()["entered"], before["entered"])
    # reset zeroes all four accumulators, asked for or not
    eng.observe_lane_flow_tensor(waiting_steps=torch.zeros(L, dtype=torch.int64), reset=True)
    after = eng.observe_lane_flow_array()
    assert not any(after[k].any() for k in ACCUMULATED)


def test_lane_change_is_not_implemented(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    eng = twin(mod, cfg)
    with pytest.raises(NotImplementedError):
        eng.track_lane_flow(True)
    assert not eng.lane_flow_tracking()
    eng.track_lane_flow(False)  # (turning it off is no error)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    with pytest.raises(NotImplementedError):
        vec.track_lane_flow(True)


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    code = ("import sys, cityflow_amd; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert hasattr(cityflow_amd.Engine, 'observe_lane_flow_tensor'); "
            "assert hasattr(cityflow_amd.VectorEngine, 'track_lane_flow'); "
            "assert not hasattr(cityflow_amd.TiledEngine, 'track_lane_flow')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def tracking_changes_no_result_body(make, cfg, steps=300):
    tracked, plain = make(cfg), make(cfg)
    tracked.track_lane_flow(True)
    for s in range(steps):
        tracked.next_step()
        plain.next_step()
    assert_same_state(tracked, plain, "tracked against untracked after %d steps" % steps)
    assert tracked.get_average_travel_time() == plain.get_average_travel_time()
    assert tracked.observe_lane_flow_array()["left"].sum() > 0


def test_tracking_changes_no_result(mod, scen, workdir):
    tracking_changes_no_result_body(lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir))


# ---------------------------------------------------------------------------------------------------------------- GPU
def layout_config(scen, workdir, name, layout, **cfx):
    if layout == "dense":
        cfx["layout"] = "dense"
    return scen.materialize(name, workdir, **({"cfx": cfx} if cfx else {}))


def hip_engine(mod, cfg, layout):
    eng = mod.Engine(cfg, 1)
    assert_hip_backend(eng)
    if eng._device_buffers():
        assert eng._layout() == ("dense" if layout == "dense" else "ring")
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("name", ["grid_6x6", "example_1x1"])
def test_equals_the_model(mod, scen, workdir, name, layout):
    eng = hip_engine(mod, layout_config(scen, workdir, name, layout), layout)
    run_against_model(eng, eng, 400, "%s %s" % (name, layout), refills=name == "example_1x1")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_hip_equals_twin(mod, scen, workdir, layout):
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    eng, tw = hip_engine(mod, cfg, layout), twin(mod, cfg)
    eng.track_lane_flow(True)
    tw.track_lane_flow(True)
    plan = drain_plan(300)
    for s in range(300):
        eng.next_step()
        tw.next_step()
        if s in plan:
            peek = tw.observe_lane_flow_array()
            check_drain(eng, peek, peek, plan[s], "step %d" % s)
            tw.observe_lane_flow_array(reset=plan[s])
    assert peek["left"].sum() + peek["waiting_steps"].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ring", "dense"])
def test_equals_the_model_on_the_bench_workload(mod, workdir, layout):
    import bench
    extra = {} if layout == "ring" else {"cfx": {"layout": "dense"}}
    cfg = bench.with_config(bench.build_workload(workdir, 0), "lane_flow_" + layout, **extra)
    eng = hip_engine(mod, cfg, layout)
    L = len(eng.lane_ids())
    for s in range(60):  # demand builds up first: the baseline is taken on a loaded network
        eng.next_step()
    assert eng.get_vehicle_count() > 10000
    eng.track_lane_flow(True)
    model = ArrayModel(L)
    model.baseline(eng._vehicle_state(), 60)
    ident = Identities(eng)
    for s in range(60):
        eng.next_step()
        model.tick(eng._vehicle_state(), 61 + s)
        ident.tick(eng)
        if s in (0, 17, 38, 59):
            reset = s in (17, 38)
            want = model.drain(False)
            out = check_drain(eng, want, want, reset, "bench %s, step %d" % (layout, s))
            model.drain(reset)
            ident.drained(eng, out, reset, "bench %s, step %d" % (layout, s))
    assert out["left"].sum() > 0 and out["waiting_steps"].sum() > 0 and out["max_waiting_steps"].max() >= 10


@pytest.mark.gpu
def test_tables_and_rings_grow_while_tracking(mod, scen, workdir):
    import os
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense.json"), 400, seed=7, interval=2.0,
                            base_flow=os.path.join(d, "flow.json"))
    small = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring", "ringCapacityPercent": 30}), 1)
    large = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring"}), 1)
    small.track_lane_flow(True)
    large.track_lane_flow(True)
    plan = drain_plan(300)
    for s in range(300):
        small.next_step()
        large.next_step()
        if s in plan:
            a, b = small.observe_lane_flow_array(reset=plan[s]), large.observe_lane_flow_array(reset=plan[s])
            for k in NAMES:
                assert np.array_equal(a[k], b[k]), "step %d: %s differs from the engine that starts large" % (s, k)
    assert b["waiting_steps"].sum() > 0
    if small._device_buffers():
        assert small._ring_info()[1] >= 2, small._ring_info()
        assert small._vehicle_table()[0] > 4096  # (the start-small knob starts the vehicle tables at 4096 numbers)
        assert small._host_stats(False)["table_grows_total"] > large._host_stats(False)["table_grows_total"]


@pytest.mark.gpu
def test_baseline_rules_on_the_device(mod, scen, workdir, tmp_path):
    baseline_rules_body(lambda cfg: mod.Engine(cfg, 1), scen.materialize("grid_6x6", workdir), tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_compaction_is_invisible_on_the_device(mod, scen, workdir, layout):
    class S:  # (scen with the layout added to every config)
        @staticmethod
        def materialize(name, wd, cfx):
            return layout_config(scen, wd, name, layout, **cfx)
    compaction_body(lambda cfg: hip_engine(mod, cfg, layout), S, workdir)


@pytest.mark.gpu
def test_vector_engine_equals_standalone(mod, scen, workdir):
    vec = mod.VectorEngine(scen.materialize("grid_6x6", workdir), 4)
    singles = [mod.Engine(scen.materialize("grid_6x6", workdir, seed=e), 1) for e in range(4)]
    vector_body(vec, singles, 150, 30)


@pytest.mark.gpu
def test_lane_flow_on_a_side_stream_without_a_host_wait(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    for s in range(100):  # warm: rings built, tables uploaded, traffic on the lanes
        eng.next_step()
        ref.next_step()
    eng.track_lane_flow(True)
    model = Model(ref.lane_ids())
    model.baseline(ref.get_lane_vehicles(), 100)
    t = empty_outputs(eng)
    eng.observe_lane_flow_tensor(**t)
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
            eng.observe_lane_flow_tensor(reset=True, **t)
            records.append({k: v.clone() for k, v in t.items()})  # consumed on `side`, then the outputs are reused
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the loop waited for the device (%.1f ms for 8 iterations behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    left = 0
    for s in range(8):
        ref.next_step()
        model.tick(ref.get_lane_vehicles(), ref.get_vehicle_speed(), 101 + s)
        want = model.drain(True)
        left += int(want["left"].sum())
        for k in NAMES:
            assert np.array_equal(records[s][k].cpu().numpy(), want[k]), "step %d: %s" % (s, k)
    assert left > 0
    assert_same_state(eng, ref, "after the unsynchronised loop")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_tracking_changes_no_result_free_running(mod, scen, workdir, layout):
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    tracking_changes_no_result_body(lambda c: hip_engine(mod, c, layout), cfg)
