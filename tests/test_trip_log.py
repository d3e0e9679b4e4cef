"""The trip log: one row per finished vehicle, kept by the trip tracker and drained into tensors — track_trips(log=N) /
trip_log_capacity / observe_trip_log_tensor / observe_trip_log_array / road_ids on Engine and VectorEngine
(cityflow_amd/torch_io.py; the append in k_trip_tick and k_trip_log_drain on the device, the host log of
csrc/host/trip_stats.cpp on the twin).

At the tick that ends step s every vehicle finished now and not at the previous tick is one row {env, vehicle, origin_road,
destination_road, enter_step, finish_step = s, travel_steps = (s - 1) - e(v)}; a baseline empties the log; a row that does not
fit is dropped and counted.

The oracle uses only calls that existed before the feature: after every step the ids get_vehicles(True) no longer lists have
finished at that step, e(v) = (step of first sight) - 1, and origin / destination of `flow_<i>_<n>` are the first and last road
of flow i in the scenario's flow.json, looked up in road_ids().  Rows are compared as sorted tuples (env, finish_step,
enter_step, origin_road, destination_road, travel_steps); on an Engine that never compacts `vehicle` is checked through the
ids of the vehicle numbers as well."""
import json
import os

import numpy as np
import pytest

from conftest import TWIN_LIB

torch = pytest.importorskip("torch")

from test_trip_stats import hip_engine, tensor_device, twin  # noqa: E402

COLUMNS = ("env", "vehicle", "origin_road", "destination_road", "enter_step", "finish_step", "travel_steps")
OUTPUTS = ("count", "dropped") + COLUMNS
KEY = ("env", "finish_step", "enter_step", "origin_road", "destination_road", "travel_steps")


# ------------------------------------------------------------------------------------------------------------------ oracle
def scenario_files(cfg):
    with open(cfg) as f:
        c = json.load(f)
    return os.path.join(c["dir"], c["roadnetFile"]), os.path.join(c["dir"], c["flowFile"])


class Oracle:
    """Who finished when, from get_vehicles(True) after every step.  Fed from the engine's first step on, so it knows every
    vehicle's enter step when a baseline is taken later; `rows` holds (finish_step, id) since the last clear()."""

    def __init__(self, cfg, road_ids, env=0):
        with open(scenario_files(cfg)[1]) as f:
            flows = json.load(f)
        index = {r: i for i, r in enumerate(road_ids)}
        self.flow_od = [(index[fl["route"][0]], index[fl["route"][-1]]) for fl in flows]
        self.od = {}      # ids that are no flow's (pushed vehicles), and vehicles whose route was replaced
        self.env = env
        self.enter = {}
        self.alive = set()
        self.rows = []
        self.finished_now = set()

    def tick(self, eng, s):
        alive = set(eng.get_vehicles(True))
        for v in alive - self.enter.keys():
            self.enter[v] = s - 1
        self.finished_now = self.alive - alive
        self.rows += [(s, v) for v in sorted(self.finished_now)]
        self.alive = alive

    def clear(self):
        self.rows = []

    def od_of(self, v):
        return self.od[v] if v in self.od else self.flow_od[int(v.split("_")[1])]

    def key(self, s, v):
        e = self.enter[v]
        o, d = self.od_of(v)
        return (self.env, s, e, o, d, (s - 1) - e)

    def keys(self, rows=None):
        return sorted(self.key(s, v) for s, v in (self.rows if rows is None else rows))


def keys_of(log):
    return sorted(zip(*[log[k].tolist() for k in KEY]))


def drain(eng, where, reset=False, tensor_reset=False):
    """The tensor call into buffers filled with -7, then the array call: they must agree after sorting.  Behind `count` every
    column is -1 and nothing keeps its -7.  `tensor_reset`: the tensor call empties the log, the array call then finds it
    empty.  Returns the array form (of the tensor call's rows)."""
    dev, cap = tensor_device(eng), eng.trip_log_capacity()
    t = {k: torch.full(() if k in ("count", "dropped") else (cap,), -7, dtype=torch.int32, device=dev) for k in OUTPUTS}
    ret = eng.observe_trip_log_tensor(reset=tensor_reset, **t)
    assert sorted(ret) == sorted(OUTPUTS) and all(ret[k] is t[k] for k in OUTPUTS), where
    t = {k: v.cpu().numpy() for k, v in t.items()}
    n = int(t["count"])
    assert 0 <= n <= cap and int(t["dropped"]) >= 0, where
    for k in COLUMNS:
        assert (t[k][n:] == -1).all(), "%s: %s is not -1 behind count" % (where, k)
        assert not (t[k] == -7).any(), "%s: %s has elements nobody wrote" % (where, k)
    assert (np.diff(t["finish_step"][:n]) >= 0).all(), "%s: the rows are not in ascending finish_step" % where
    order = np.lexsort((t["vehicle"][:n], t["env"][:n], t["finish_step"][:n]))
    mine = {k: t[k][:n][order] for k in COLUMNS}
    mine["dropped"] = int(t["dropped"])
    got = eng.observe_trip_log_array(reset=reset)
    assert sorted(got) == sorted(COLUMNS + ("dropped",)), where
    if tensor_reset:
        assert all(got[k].shape == (0,) for k in COLUMNS) and got["dropped"] == 0, "%s: reset=True left rows behind" % where
        return mine
    for k in COLUMNS:
        assert got[k].dtype == np.int32 and got[k].shape == (n,), where
        assert np.array_equal(got[k], mine[k]), "%s: %s differs between the tensor and the array call" % (where, k)
    assert got["dropped"] == mine["dropped"], where
    return got


def check_ids(eng, log, oracle_rows, where):
    """(Engine that never compacts) each row's vehicle number is the id the oracle saw finish at that step."""
    ids = eng._vehicle_ids(np.ascontiguousarray(log["vehicle"]))
    assert sorted(zip(log["finish_step"].tolist(), ids)) == sorted(oracle_rows), where


def concat(logs):
    return {k: np.concatenate([l[k] for l in logs]) for k in COLUMNS}


# ------------------------------------------------------------------------------------------------------------- the bodies
def example_body(make, scen, workdir, layout, with_twin=None):
    """Case 1.  Returns the final log."""
    cfg = scen.materialize("example_1x1", workdir, **({"cfx": {"layout": "dense"}} if layout == "dense" else {}))
    eng = make(cfg)
    other = with_twin(cfg) if with_twin else None
    assert eng.trip_log_capacity() == 0
    eng.track_trips(True, log=1024)
    assert eng.trip_tracking() and eng.trip_log_capacity() == 1024
    if other is not None:
        other.track_trips(True, log=1024)
    orc = Oracle(cfg, eng.road_ids())
    first = None
    for s in range(1, 201):
        eng.next_step()
        orc.tick(eng, s)
        at = "example_1x1 %s, step %d" % (layout, s)
        log = drain(eng, at)
        assert keys_of(log) == orc.keys(), at
        check_ids(eng, log, orc.rows, at)
        assert log["dropped"] == 0
        if first is None and len(log["env"]):
            first = s
        if other is not None:
            other.next_step()
            theirs = other.observe_trip_log_array()
            for k in COLUMNS + ("dropped",):
                assert np.array_equal(log[k], theirs[k]), "%s: %s differs from the twin's host log" % (at, k)
    trips = eng.observe_trips_array()
    assert first == 41 and len(log["env"]) == 292 == int(trips["finished"])
    assert int(log["travel_steps"].sum()) == 17915 == int(trips["finished_travel_steps"])
    assert len(set(log["vehicle"].tolist())) == 292
    assert len(set(zip(log["origin_road"].tolist(), log["destination_road"].tolist()))) > 1
    return log


def draining_body(make, scen, workdir):
    """Case 2: reset=True every 25 steps, alternately through the tensor call and the array call."""
    cfg = scen.materialize("example_1x1", workdir)
    eng = make(cfg)
    eng.track_trips(True, log=1024)
    orc = Oracle(cfg, eng.road_ids())
    whole = Oracle(cfg, eng.road_ids())
    drains, finished = [], 0
    for s in range(1, 201):
        eng.next_step()
        orc.tick(eng, s)
        whole.tick(eng, s)
        if s % 25 == 0:
            at = "drain at step %d" % s
            by_tensor = (s // 25) % 2 == 1
            log = drain(eng, at, reset=not by_tensor, tensor_reset=by_tensor)
            now = int(eng.observe_trips_array()["finished"])
            assert len(log["env"]) == now - finished, at
            finished = now
            assert keys_of(log) == orc.keys(), at
            check_ids(eng, log, orc.rows, at)
            orc.clear()
            drains.append(log)
            assert len(eng.observe_trip_log_array()["env"]) == 0, at
    assert finished == 292 and sum(len(d["env"]) > 0 for d in drains) > 2
    assert keys_of(concat(drains)) == whole.keys()
    assert np.array_equal(concat(drains)["finish_step"], np.sort(concat(drains)["finish_step"]))


def overflow_body(make, scen, workdir):
    """Case 3."""
    cfg = scen.materialize("example_1x1", workdir)
    eng = make(cfg)
    eng.track_trips(True, log=64)
    orc = Oracle(cfg, eng.road_ids())
    for s in range(1, 201):
        eng.next_step()
        orc.tick(eng, s)
    log = drain(eng, "overflow")
    assert len(log["env"]) == 64 and log["dropped"] == 228
    assert int(eng.observe_trips_array()["finished"]) == 292
    # the first 64 of the canonical order up to ties within a step: the complete steps as a multiset, membership for the last
    last = int(log["finish_step"].max())
    complete = [r for r in orc.rows if r[0] < last]
    assert len(complete) <= 64 <= len(complete) + sum(1 for r in orc.rows if r[0] == last)
    mine = keys_of(log)
    assert [k for k in mine if k[1] < last] == orc.keys(complete)
    assert set(k for k in mine if k[1] == last) <= set(orc.keys([r for r in orc.rows if r[0] == last]))
    ids = eng._vehicle_ids(np.ascontiguousarray(log["vehicle"]))
    assert set(zip(log["finish_step"].tolist(), ids)) <= set(orc.rows) and len(set(ids)) == 64
    drain(eng, "overflow, emptied", tensor_reset=True)
    orc.clear()
    for s in range(201, 221):
        eng.next_step()
        orc.tick(eng, s)
    log = drain(eng, "20 steps after the overflow")
    assert log["dropped"] == 0 and 0 < len(log["env"]) <= 64
    assert keys_of(log) == orc.keys()


def follow(eng, orc, first, steps, where):
    for s in range(first + 1, first + steps + 1):
        eng.next_step()
        orc.tick(eng, s)
    log = drain(eng, where)
    assert keys_of(log) == orc.keys(), where
    check_ids(eng, log, orc.rows, where)
    assert log["dropped"] == 0
    return log


def baselines_body(make, scen, workdir, tmp_path):
    """Case 4."""
    cfg = scen.materialize("example_1x1", workdir)
    eng = make(cfg)
    orc = Oracle(cfg, eng.road_ids())
    for s in range(1, 61):
        eng.next_step()
        orc.tick(eng, s)
    assert orc.rows  # vehicles have finished before tracking is on: they are no rows
    orc.clear()
    with pytest.raises(RuntimeError):
        eng.observe_trip_log_array()
    eng.track_trips(True, log=256)
    assert len(drain(eng, "turned on at step 60")["env"]) == 0
    log = follow(eng, orc, 60, 40, "40 steps after turning on at step 60")
    assert len(log["env"]) > 0 and (log["enter_step"] < 60).any()
    # changing the log while tracking is on: an empty log, the accumulators as they were
    before = eng.observe_trips_array()
    eng.track_trips(True, log=512)
    assert eng.trip_log_capacity() == 512 and len(drain(eng, "log replaced")["env"]) == 0
    after = eng.observe_trips_array()
    assert all(np.array_equal(before[k], after[k]) for k in before) and int(after["finished"]) > 0
    eng.track_trips(True)  # (log=None leaves it)
    assert eng.trip_log_capacity() == 512
    orc.clear()
    log = follow(eng, orc, 100, 10, "after replacing the log")
    archive = eng.snapshot()
    path = str(tmp_path / "trip_log_archive.json")
    archive.dump(path)
    kept_alive, kept_enter = set(orc.alive), dict(orc.enter)
    ck = eng.checkpoint() if eng._checkpoint_calls() else None
    follow(eng, orc, 110, 15, "after the snapshot")
    assert orc.rows
    loads = [("load", lambda: eng.load(archive)), ("load_from_file", lambda: eng.load_from_file(path))]
    if ck is not None:
        loads.append(("rollback", lambda: eng.rollback(ck)))
    for how, call in loads:
        call()
        assert eng.trip_tracking() and eng.trip_log_capacity() == 512
        orc.alive, orc.enter = set(kept_alive), dict(kept_enter)
        orc.clear()
        assert len(drain(eng, how)["env"]) == 0, how
        assert len(follow(eng, orc, 110, 15, "after " + how)["env"]) > 0
    eng.reset()
    orc = Oracle(cfg, eng.road_ids())
    assert eng.trip_log_capacity() == 512 and len(drain(eng, "reset")["env"]) == 0
    assert len(follow(eng, orc, 0, 60, "after reset")["env"]) > 0
    # log=0 drops it; tracking stays on
    eng.track_trips(True, log=0)
    assert eng.trip_tracking() and eng.trip_log_capacity() == 0
    with pytest.raises(RuntimeError):
        eng.observe_trip_log_array()
    with pytest.raises(RuntimeError):
        eng.observe_trip_log_tensor(count=torch.zeros((), dtype=torch.int32, device=tensor_device(eng)))
    assert int(eng.observe_trips_array()["finished"]) > 0
    # tracking off drops the log as well
    eng.track_trips(True, log=8)
    eng.track_trips(False)
    assert eng.trip_log_capacity() == 0
    eng.track_trips(True)
    assert eng.trip_log_capacity() == 0


def compaction_body(make, scen, workdir, layout="auto"):
    """Case 5."""
    extra = {"layout": "dense"} if layout == "dense" else {}
    a = make(scen.materialize("example_1x1", workdir, cfx=dict(extra, compactVehicles=100)))
    b = make(scen.materialize("example_1x1", workdir, cfx=dict(extra, compactVehicles=0)))
    a.track_trips(True, log=1024)
    b.track_trips(True, log=1024)
    for s in range(1, 201):
        a.next_step()
        b.next_step()
    assert a._vehicle_table()[1] > 0 and b._vehicle_table()[1] == 0, (a._vehicle_table(), b._vehicle_table())
    la, lb = drain(a, "compacting"), drain(b, "never compacting")
    assert len(lb["env"]) == 292 and la["dropped"] == lb["dropped"] == 0
    assert keys_of(la) == keys_of(lb)
    assert not np.array_equal(np.sort(la["vehicle"]), np.sort(lb["vehicle"]))  # (numbers were reused)


def vector_body(make_vec, make_single, scen, workdir, R, seeds, capacity, other=None):
    """Cases 6 and 7: every environment's rows against the oracle of a standalone engine with that environment's seed."""
    cfg = scen.materialize("example_1x1", workdir)
    vec = make_vec(cfg, R, seeds)
    vec.track_trips(True, log=capacity)
    assert vec.trip_log_capacity() == capacity
    distinct = sorted(set(seeds))
    singles = {sd: make_single(scen.materialize("example_1x1", workdir, seed=sd)) for sd in distinct}
    oracles = {sd: Oracle(cfg, vec.road_ids()) for sd in distinct}
    assert vec.road_ids() == singles[distinct[0]].road_ids()
    for s in range(1, 201):
        vec.next_step()
        for sd in distinct:
            singles[sd].next_step()
            oracles[sd].tick(singles[sd], s)
        if s % 50 == 0:
            at = "x%d, step %d" % (R, s)
            log = drain(vec, at)
            mine = keys_of(log)
            for r in range(R):
                want = [(r,) + k[1:] for k in oracles[seeds[r]].keys()]
                assert [k for k in mine if k[0] == r] == want, "%s: environment %d" % (at, r)
    assert log["dropped"] == 0 and len(log["env"]) == sum(len(oracles[sd].rows) for sd in seeds)
    assert len(set(log["vehicle"].tolist())) == len(log["vehicle"])
    assert np.array_equal(np.bincount(log["env"], minlength=R), vec.observe_trips_array()["finished"])
    return log


def set_route_body(make, scen, workdir):
    """Case 8, on grid_6x6: a junction of example_1x1 has one lane per turn, so no running vehicle can take another route there."""
    cfg = scen.materialize("grid_6x6", workdir)
    eng = make(cfg)
    eng.track_trips(True, log=1024)
    roads = eng.road_ids()
    orc = Oracle(cfg, roads)
    follow(eng, orc, 0, 30, "before set_vehicle_route")
    changed = None
    for vid in sorted(eng.get_vehicles()):
        old = eng.get_vehicle_info(vid)["route"].split()
        for anchor in roads:
            if anchor not in old and eng.set_vehicle_route(vid, [anchor]):
                route = eng.get_vehicle_info(vid)["route"].split()
                assert route[-1] == anchor and roads.index(anchor) != orc.od_of(vid)[1]
                changed = (vid, roads.index(anchor), set(roads.index(r) for r in route))
                break
        if changed:
            break
    assert changed, "no running vehicle took a new route"
    for s in range(31, 201):
        eng.next_step()
        orc.tick(eng, s)
    log = drain(eng, "after set_vehicle_route")
    ids = eng._vehicle_ids(np.ascontiguousarray(log["vehicle"]))
    assert changed[0] in ids, "the vehicle with the new route has not finished"
    i = ids.index(changed[0])
    assert int(log["destination_road"][i]) == changed[1]
    assert int(log["origin_road"][i]) in changed[2]  # (the first road of the NEW route, which starts where the vehicle was)
    orc.od[changed[0]] = (int(log["origin_road"][i]), changed[1])
    assert keys_of(log) == orc.keys()
    check_ids(eng, log, orc.rows, "after set_vehicle_route")


def push_vehicle_body(make, scen, workdir):
    """Case 9."""
    cfg = scen.materialize("example_1x1", workdir)
    eng = make(cfg)
    eng.track_trips(True, log=1024)
    roads = eng.road_ids()
    orc = Oracle(cfg, roads)
    follow(eng, orc, 0, 20, "before the push")
    with open(scenario_files(cfg)[1]) as f:
        route = json.load(f)[0]["route"]
    before = set(eng.get_vehicles(True))
    eng.push_vehicle({"length": 5.0, "maxSpeed": 11.0}, [route[0], route[-1]])
    (pushed,) = set(eng.get_vehicles(True)) - before
    orc.od[pushed] = (roads.index(route[0]), roads.index(route[-1]))
    log = follow(eng, orc, 20, 180, "after the push")
    ids = eng._vehicle_ids(np.ascontiguousarray(log["vehicle"]))
    assert pushed in ids, "the pushed vehicle has not finished"
    i = ids.index(pushed)
    assert (int(log["origin_road"][i]), int(log["destination_road"][i])) == orc.od[pushed]


def argument_errors_body(eng, vec):
    """Case 10."""
    dev = tensor_device(eng)

    def buf(n=16, dtype=torch.int32, device=dev):
        return torch.full((n,) if n is not None else (), -7, dtype=dtype, device=device)

    for bad in (-1, (1 << 26) + 1, 2.5, "8", True):
        with pytest.raises(ValueError):
            eng.track_trips(True, log=bad)
        assert not eng.trip_tracking()  # (checked before anything is changed)
    with pytest.raises(ValueError):
        eng.track_trips(False, log=8)
    with pytest.raises(RuntimeError):  # tracking is off
        eng.observe_trip_log_array()
    eng.track_trips(True)
    with pytest.raises(RuntimeError):  # tracking is on, but there is no log
        eng.observe_trip_log_tensor(env=buf())
    with pytest.raises(RuntimeError):
        vec.observe_trip_log_array()
    eng.track_trips(True, log=16)
    vec.track_trips(True, log=np.int64(16))
    for s in range(50):
        eng.next_step()
    with pytest.raises(ValueError):  # no output given
        eng.observe_trip_log_tensor()
    with pytest.raises(ValueError):
        eng.observe_trip_log_tensor(reset=True)
    with pytest.raises(TypeError):   # wrong dtypes
        eng.observe_trip_log_tensor(env=buf(dtype=torch.int64))
    with pytest.raises(TypeError):
        eng.observe_trip_log_tensor(count=buf(None, dtype=torch.int64))
    with pytest.raises(TypeError):
        eng.observe_trip_log_tensor(travel_steps=np.zeros(16, dtype=np.int32))
    with pytest.raises(TypeError):   # wrong device
        eng.observe_trip_log_tensor(vehicle=buf(device="meta"))
    if dev.type == "cuda":
        with pytest.raises(TypeError):
            eng.observe_trip_log_tensor(vehicle=buf(device="cpu"))
    with pytest.raises(ValueError):  # wrong shapes
        eng.observe_trip_log_tensor(env=buf(15))
    with pytest.raises(ValueError):
        eng.observe_trip_log_tensor(count=buf(1))
    with pytest.raises(ValueError):
        vec.observe_trip_log_tensor(env=torch.zeros((2, 16), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):  # not contiguous
        eng.observe_trip_log_tensor(env=buf(32)[::2])
    # nothing is written, and nothing is reset, when a later argument is wrong
    good = buf()
    with pytest.raises(ValueError):
        eng.observe_trip_log_tensor(env=good, travel_steps=buf(3), reset=True)
    assert bool((good == -7).all())
    finished = int(eng.observe_trips_array()["finished"])
    assert finished > 0
    n = min(finished, 16)
    count = buf(None)
    ret = eng.observe_trip_log_tensor(env=good, count=count)
    assert list(ret) == ["count", "env"] and int(count) == n
    assert bool((good[:n] == 0).all()) and bool((good[n:] == -1).all())


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
def twin_vec(mod):
    return lambda cfg, n, seeds: mod.VectorEngine._with_backend(cfg, n, 1, TWIN_LIB, seeds=seeds)


@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_example_equals_the_oracle(mod, scen, workdir, layout):
    example_body(lambda cfg: twin(mod, cfg), scen, workdir, layout)


def test_draining(mod, scen, workdir):
    draining_body(lambda cfg: twin(mod, cfg), scen, workdir)


def test_overflow(mod, scen, workdir):
    overflow_body(lambda cfg: twin(mod, cfg), scen, workdir)


def test_baselines(mod, scen, workdir, tmp_path):
    baselines_body(lambda cfg: twin(mod, cfg), scen, workdir, tmp_path)


def test_compaction_is_invisible(mod, scen, workdir):
    compaction_body(lambda cfg: twin(mod, cfg), scen, workdir)


def test_vector_engine(mod, scen, workdir):
    log = vector_body(twin_vec(mod), lambda cfg: twin(mod, cfg), scen, workdir, 3, [0, 1, 2], 4096)
    per_env = [sorted(k[1:] for k in keys_of(log) if k[0] == r) for r in range(3)]
    assert per_env[0] != per_env[1] or per_env[1] != per_env[2], "the environments' rows were equal"


def test_vector_engine_beyond_64_environments(mod, scen, workdir):
    log = vector_body(twin_vec(mod), lambda cfg: twin(mod, cfg), scen, workdir, 67, [3] * 67, 32768)
    # (289 vehicles finish in an engine with seed 3, which vector_body has checked row by row; the 292 of the other tests is seed 0's)
    assert len(log["env"]) == 67 * 289 and (log["env"] >= 64).any()


def test_set_vehicle_route(mod, scen, workdir):
    set_route_body(lambda cfg: twin(mod, cfg), scen, workdir)


def test_push_vehicle(mod, scen, workdir):
    push_vehicle_body(lambda cfg: twin(mod, cfg), scen, workdir)


def test_argument_errors(mod, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir)
    argument_errors_body(twin(mod, cfg), mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB))


def test_lane_change_is_not_implemented(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    eng = twin(mod, cfg)
    with pytest.raises(NotImplementedError):
        eng.track_trips(True, log=64)
    assert not eng.trip_tracking() and eng.trip_log_capacity() == 0
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    with pytest.raises(NotImplementedError):
        vec.track_trips(True, log=64)


def test_tiled_engine_has_no_trip_log(mod):
    for name in ("trip_log_capacity", "observe_trip_log_tensor", "observe_trip_log_array", "road_ids"):
        assert hasattr(mod.Engine, name) and hasattr(mod.VectorEngine, name), name
        assert not hasattr(mod.TiledEngine, name), name


# ---------------------------------------------------------------------------------------------------------------- GPU
def hip_vec(mod):
    # (the library the default constructor loads, named so that the seeds can be given)
    return lambda cfg, n, seeds: mod.VectorEngine._with_backend(cfg, n, 1, mod._default_backend_path(), seeds=seeds)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_example_equals_the_oracle_and_the_twin_on_the_device(mod, scen, workdir, layout):
    example_body(lambda cfg: hip_engine(mod, cfg), scen, workdir, layout, with_twin=lambda cfg: twin(mod, cfg))


@pytest.mark.gpu
def test_draining_on_the_device(mod, scen, workdir):
    draining_body(lambda cfg: hip_engine(mod, cfg), scen, workdir)


@pytest.mark.gpu
def test_overflow_on_the_device(mod, scen, workdir):
    overflow_body(lambda cfg: hip_engine(mod, cfg), scen, workdir)


@pytest.mark.gpu
def test_baselines_on_the_device(mod, scen, workdir, tmp_path):
    baselines_body(lambda cfg: hip_engine(mod, cfg), scen, workdir, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_compaction_is_invisible_on_the_device(mod, scen, workdir, layout):
    compaction_body(lambda cfg: hip_engine(mod, cfg), scen, workdir, layout)


@pytest.mark.gpu
def test_vector_engine_on_the_device(mod, scen, workdir):
    vector_body(hip_vec(mod), lambda cfg: twin(mod, cfg), scen, workdir, 3, [0, 1, 2], 4096)


@pytest.mark.gpu
def test_vector_engine_beyond_64_environments_on_the_device(mod, scen, workdir):
    log = vector_body(hip_vec(mod), lambda cfg: twin(mod, cfg), scen, workdir, 67, [3] * 67, 32768)
    # (289 vehicles finish in an engine with seed 3, which vector_body has checked row by row; the 292 of the other tests is seed 0's)
    assert len(log["env"]) == 67 * 289 and (log["env"] >= 64).any()


@pytest.mark.gpu
def test_set_vehicle_route_on_the_device(mod, scen, workdir):
    set_route_body(lambda cfg: hip_engine(mod, cfg), scen, workdir)


@pytest.mark.gpu
def test_push_vehicle_on_the_device(mod, scen, workdir):
    push_vehicle_body(lambda cfg: hip_engine(mod, cfg), scen, workdir)


@pytest.mark.gpu
def test_argument_errors_on_the_device(mod, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir)
    argument_errors_body(hip_engine(mod, cfg), mod.VectorEngine(cfg, 2))


@pytest.mark.gpu
def test_lane_change_is_not_implemented_on_the_device(mod, scen, workdir):
    eng = mod.Engine(scen.materialize("grid_6x6", workdir, laneChange=True), 1)
    with pytest.raises(NotImplementedError):
        eng.track_trips(True, log=64)
    assert not eng.trip_tracking() and eng.trip_log_capacity() == 0
