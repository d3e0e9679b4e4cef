"""Checkpoints in device memory: Engine.checkpoint() / rollback() and the same pair on VectorEngine (cityflow_amd/torch_io.py,
cfx_checkpoint_* of include/cityflow_amd.h).  rollback(ck) leaves the engine as load(snapshot()) would, except that the vehicles
keep their place in their routes — so an engine that checkpoints, does anything at all and rolls back must go on bit for bit
like one that never left the checkpointed state.  Every comparison here is exact.

The GPU tests skip themselves on a backend without the entry points (the twin standing in for the device under
CFX_SHADOW_GPU).  The durations set by set_tl_plan belong to the engine, not to the checkpoint: an engine that tried another
plan after the checkpoint puts the plan it wants back itself (restore_tl_plan() here), which is the "roll back, try the next
plan" loop the call exists for."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

try:  # (before the first engine loads the HIP library: torch and the engine then share one HIP runtime in this process)
    import torch
except ImportError:
    torch = None

from conftest import ROOT, TWIN_LIB, assert_hip_backend, assert_same_state, full_state

STATE_KEYS = ("vid", "drivable", "prev_drivable", "dis", "speed", "leader", "blocker", "enter_ll_time", "route_pos")


def _cfx(path, tag, top=None, **cfx):
    with open(path) as f:
        c = json.load(f)
    c.update(top or {})
    if cfx:
        c["cfx"] = dict(c.get("cfx", {}), **cfx)
    out = path.replace(".json", "_ck_%s.json" % tag)
    with open(out, "w") as f:
        json.dump(c, f)
    return out


def _hip(mod, cfg):
    eng = mod.Engine(cfg, 1)
    assert_hip_backend(eng)
    if not eng._checkpoint_calls():
        pytest.skip("the backend %s has no checkpoints in device memory" % eng.backend_name())
    return eng


def _roads(cfg):
    with open(cfg) as f:
        c = json.load(f)
    with open(os.path.join(c["dir"], c["roadnetFile"])) as f:
        return [r["id"] for r in json.load(f)["roads"]]


def _other_plan(eng):
    d = eng.get_tl_phase_durations_array()
    return np.where(d > 0, d + 7.0, d)


def _diverge(b, roads, steps, plan=True):
    """Leave the checkpointed state for good: another signal plan, a custom speed, a pushed vehicle, a new route."""
    for s in range(steps):
        if s == 0 and plan:
            b.set_tl_plan(durations=_other_plan(b))
        ids = sorted(b.get_vehicles(False))
        if s == 1 and ids:
            b.set_vehicle_speed(ids[0], 1.25)
        if s == 2:
            b.push_vehicle({"length": 4.5, "maxSpeed": 9.0}, [roads[len(roads) // 2]])
        if s in (3, 9) and ids:
            b.set_vehicle_route(ids[-1], [roads[(7 * s) % len(roads)]])
        b.next_step()


def _record(e):
    return (full_state(e), e.get_vehicles(include_waiting=True), e.get_lane_vehicle_count_array(), e._tl_state(), e._scalars())


def _assert_recorded(e, rec, where):
    s, vehicles, lanes, tl, sc = _record(e)
    for k in STATE_KEYS + ("gap",):
        assert np.array_equal(s[k], rec[0][k], equal_nan=True), "%s: %s differs" % (where, k)
    assert vehicles == rec[1], where + ": vehicles"
    assert np.array_equal(lanes, rec[2]), where + ": lane counts"
    assert np.array_equal(tl[0], rec[3][0]) and np.array_equal(tl[1], rec[3][1]), where + ": lights"
    for k in ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time"):
        assert sc[k] == rec[4][k], "%s: scalar %s" % (where, k)


def _step_together(a, b, steps, where, record=None):
    for s in range(steps):
        a.next_step()
        b.next_step()
        assert_same_state(a, b, "%s, step %d after the rollback" % (where, s + 1))
        assert a.get_vehicles(include_waiting=True) == b.get_vehicles(include_waiting=True), (where, s)
        if record is not None:
            record.append(_record(b))


def _assert_same_end(a, b, tmp_path, where):
    for v in a.get_vehicles(include_waiting=True):
        assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (where, v)
    assert a.get_average_travel_time() == b.get_average_travel_time(), where
    assert a._keeps_lane_history() and b._keeps_lane_history()
    pa, pb = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    a.snapshot().dump(pa)
    b.snapshot().dump(pb)
    with open(pa, "rb") as fa, open(pb, "rb") as fb:
        assert fa.read() == fb.read(), where + ": Archive files differ (Lane::history included)"


def _as_an_uninterrupted_run(mod, base, cfg, tmp_path, where, before=60, away=40, after=40, between=None):
    """A and B step `before` times; B checkpoints, leaves for `away` steps, rolls back; both step `after` times, equal after every
    step; a second rollback gives B the same steps again; the end state equals A's and an uninterrupted twin's."""
    a, b = _hip(mod, cfg), _hip(mod, cfg)
    tw = mod.Engine._with_backend(base, 1, TWIN_LIB)
    roads = _roads(base)
    for _ in range(before):
        a.next_step()
        b.next_step()
        tw.next_step()
    ck = b.checkpoint()
    assert not ck.released and ck.step == before and ck.device_bytes > 0
    assert ck.num_running == b.get_vehicle_count() and ck.num_vehicle_numbers == b._vehicle_table()[0]
    info = between(b) if between else None
    _diverge(b, roads, away)
    if between:
        between(b, info)
    b.rollback(ck)
    b.restore_tl_plan()
    assert b.get_current_time() == a.get_current_time()
    assert_same_state(a, b, where + ", right after the rollback")
    first = []
    _step_together(a, b, after, where, record=first)
    _diverge(b, roads, 7)
    b.rollback(ck)
    b.restore_tl_plan()
    for s in range(after):
        b.next_step()
        _assert_recorded(b, first[s], "%s, second rollback, step %d" % (where, s + 1))
    _assert_same_end(a, b, tmp_path, where)
    for _ in range(after):
        tw.next_step()
    assert_same_state(b, tw, where + ": against the uninterrupted twin")
    ck.release()
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("form", [20000, 30000])
@pytest.mark.parametrize("name", ["example_1x1", "grid_6x6"])
def test_rollback_continues_as_an_uninterrupted_run(mod, scen, workdir, tmp_path, name, form):
    base = scen.materialize(name, workdir)
    cfg = _cfx(base, "form%d" % form, ringLanesPerWave=form)
    _as_an_uninterrupted_run(mod, base, cfg, tmp_path, "%s form %d" % (name, form))


@pytest.mark.gpu
def test_checkpoint_at_step_0(mod, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir)
    a, b = _hip(mod, cfg), _hip(mod, cfg)
    ck = b.checkpoint()
    assert (ck.step, ck.num_running, ck.num_vehicle_numbers) == (0, 0, 0)
    _diverge(b, _roads(cfg), 30)
    b.rollback(ck)
    b.restore_tl_plan()
    assert b.get_current_time() == 0.0 and b.get_vehicles(include_waiting=True) == []
    _step_together(a, b, 40, "checkpoint at step 0")


@pytest.mark.gpu
def test_checkpoint_with_the_commit_still_pending(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    a, b = _hip(mod, cfg), _hip(mod, cfg)
    for _ in range(60):
        a.next_step()
        b.next_step()
    ck = b.checkpoint()  # (nothing was read since next_step(): the step's commit and Lane::history record are still pending)
    for _ in range(10):
        b.next_step()
    b.rollback(ck)
    assert_same_state(a, b, "pending commit, right after the rollback")
    _step_together(a, b, 30, "pending commit")
    ha, hb = a._lane_history(), b._lane_history()
    for k in ha:
        assert np.array_equal(ha[k], hb[k]), ("lane history", k)


def _congested(scen, workdir):
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense_ck.json"), 400, seed=7, interval=2.0,
                            base_flow=os.path.join(d, "flow.json"))
    return scen.materialize("grid_6x6", workdir, flow_file=flow)


@pytest.mark.gpu
def test_checkpoint_of_a_congested_state(mod, scen, workdir):
    cfg = _congested(scen, workdir)
    a, b = _hip(mod, cfg), _hip(mod, cfg)
    for _ in range(150):
        a.next_step()
        b.next_step()
    ck = b.checkpoint()
    lanes = b._waiting()[1]
    assert lanes.size and np.bincount(lanes).max() >= 2, "no entry buffer holds two vehicles"
    assert (full_state(b)["blocker"] >= 0).any(), "no vehicle has a blocker"
    assert ck.num_running == b.get_vehicle_count() > 1000
    _diverge(b, _roads(cfg), 20)
    b.rollback(ck)
    b.restore_tl_plan()
    assert_same_state(a, b, "congested, right after the rollback")
    assert [np.array_equal(x, y) for x, y in zip(a._waiting(), b._waiting())] == [True, True]
    _step_together(a, b, 30, "congested")


@pytest.mark.gpu
def test_ring_growth_after_the_checkpoint(mod, scen, workdir, tmp_path):
    base = _congested(scen, workdir)
    cfg = _cfx(base, "ring30", layout="ring", ringCapacityPercent=30)
    scales = []

    def between(b, before=None):
        scales.append(b._ring_info()[1])
        return None

    _as_an_uninterrupted_run(mod, base, cfg, tmp_path, "ring growth", before=30, away=120, after=40, between=between)
    assert scales[1] > scales[0], "the rings did not grow between checkpoint and rollback: %r" % (scales,)


@pytest.mark.gpu
def test_compaction_after_and_before_the_checkpoint(mod, scen, workdir):
    from test_compaction import compacting, unsaturated_grid, visible
    base = unsaturated_grid(scen, workdir)
    a, b = _hip(mod, compacting(base, 0)), _hip(mod, compacting(base, 40))
    n = len(a.intersection_ids())
    rng = np.random.default_rng(5)

    def step(engines, k):
        for _ in range(k):
            ph = rng.integers(0, 4, n).astype(np.int32)
            for e in engines:
                e.set_tl_phases(ph)
                e.next_step()

    def same(where):
        va, vb = visible(a), visible(b)
        for k in va:
            assert va[k] == vb[k], (where, k)
        for v in va["vehicles"]:
            assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (where, v)

    step((a, b), 60)
    # a compaction between checkpoint and rollback: the checkpoint holds the numbers of before
    ck = b.checkpoint()
    done = b._vehicle_table()[1]
    step((b,), 80)
    assert b._vehicle_table()[1] > done, "no compaction between checkpoint and rollback"
    b.rollback(ck)
    same("compaction after the checkpoint, right after the rollback")
    for s in range(8):
        step((a, b), 10)
        same("compaction after the checkpoint, step %d" % (10 * s + 10))
    # a checkpoint taken after a compaction, rolled back before the next one
    assert b._vehicle_table()[1] > done
    b._compact_vehicles()
    done = b._vehicle_table()[1]
    ck = b.checkpoint(into=ck)
    step((b,), 3)
    assert b._vehicle_table()[1] == done, "a compaction ran between checkpoint and rollback"
    b.rollback(ck)
    same("checkpoint after a compaction, right after the rollback")
    for s in range(4):
        step((a, b), 10)
        same("checkpoint after a compaction, step %d" % (10 * s + 10))
    assert a._vehicle_table()[1] == 0


def _drains(e):
    out = {}
    for name, got in (("lane", e.observe_lane_flow_array(reset=True)), ("movement", e.observe_movement_flow_array(reset=True)),
                      ("trips", e.observe_trips_array())):
        for k, v in got.items():
            out[name + "." + k] = v
    return out


@pytest.mark.gpu
def test_trackers_take_a_new_baseline_as_after_a_load(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    a, b = _hip(mod, cfg), _hip(mod, cfg)
    for e in (a, b):
        e.track_lane_flow(True)
        e.track_movement_flow(True)
        e.track_trips(True)
    for _ in range(50):
        a.next_step()
        b.next_step()
    archive, ck = a.snapshot(), b.checkpoint()
    for _ in range(15):
        a.next_step()
        b.next_step()
    a.load(archive)
    b.rollback(ck)
    for n in (1, 12):
        for _ in range(n):
            a.next_step()
            b.next_step()
        da, db = _drains(a), _drains(b)
        assert sorted(da) == sorted(db)
        for k in da:
            assert np.array_equal(da[k], db[k], equal_nan=True), (n, k)
    assert b.lane_flow_tracking() and b.movement_flow_tracking() and b.trip_tracking()
    assert da["lane.entered"].sum() > 0 and da["trips.in_system"].sum() > 0


@pytest.mark.gpu
def test_the_plan_stays_the_engines(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    e = _hip(mod, cfg)
    for _ in range(20):
        e.next_step()
    x = _other_plan(e)
    e.set_tl_plan(durations=x)
    for _ in range(5):
        e.next_step()
    phase, remain = [v.copy() for v in e._tl_state()]
    ck = e.checkpoint()
    y = np.where(x > 0, x + 11.0, x)
    e.set_tl_plan(durations=y, phase=np.where(np.asarray(e._phase_counts()) > 1, 1, -1).astype(np.int32))
    for _ in range(25):
        e.next_step()
    assert not np.array_equal(e._tl_state()[1], remain)
    e.rollback(ck)
    assert np.array_equal(e.get_tl_phase_durations_array(), y)
    assert np.array_equal(e._tl_state()[0], phase) and np.array_equal(e._tl_state()[1], remain)


@pytest.mark.gpu
def test_stream_order_from_a_side_stream(mod, scen, workdir):
    if torch is None:
        pytest.skip("needs torch")
    cfg = _cfx(scen.materialize("grid_6x6", workdir), "rl", top={"rlTrafficLight": True})
    e = _hip(mod, cfg)
    device = torch.device("cuda", e._stream_handle()[1])
    side = torch.cuda.Stream(device)
    M, P = e._intersection_dims()
    n = len(e.intersection_ids())

    def loop(steps, keep):
        for _ in range(steps):
            phase = torch.empty(n, dtype=torch.int32, device=device)
            inside = torch.empty((n, M), dtype=torch.int32, device=device)
            pressure = torch.empty((n, P), dtype=torch.int32, device=device)
            e.observe_intersections_tensor(phase=phase, movement_inside=inside, phase_pressure=pressure)
            e.set_tl_phases_tensor(torch.argmax(pressure, dim=1).to(torch.int32))
            e.next_step()
            if keep is not None:
                keep.append((phase, inside, pressure))

    with torch.cuda.stream(side):
        loop(40, None)
        ck = e.checkpoint()
        first, second = [], []
        loop(10, first)
        e.rollback(ck)
        loop(10, second)
        same = [torch.equal(x, y) for f, s in zip(first, second) for x, y in zip(f, s)]
    side.synchronize()
    assert len(same) == 30 and all(same), same
    assert int(sum(int(f[1].sum()) for f in first)) > 0


def _vector_record(v):
    out = {"lanes": v.get_lane_vehicle_count_array(), "waiting": v.get_lane_waiting_vehicle_count_array(), "tl": v._tl_state(),
           "scalars": v._scalars()}
    for r in range(v.num_envs):
        out["speed%d" % r] = v.get_vehicle_speed(r)
        out["count%d" % r] = v.get_lane_vehicle_count(r)
    return out


def _assert_vector_same(a, b, where):
    ra, rb = _vector_record(a), _vector_record(b)
    for k in ra:
        if k == "tl":
            assert np.array_equal(ra[k][0], rb[k][0]) and np.array_equal(ra[k][1], rb[k][1]), (where, k)
        elif isinstance(ra[k], np.ndarray):
            assert np.array_equal(ra[k], rb[k]), (where, k)
        else:
            assert ra[k] == rb[k], (where, k)


@pytest.mark.gpu
@pytest.mark.parametrize("envs", [3, 33])
def test_vector_engine_rollback(mod, scen, workdir, envs):
    base = scen.materialize("example_1x1", workdir)
    a, b = mod.VectorEngine(base, envs, 1), mod.VectorEngine(base, envs, 1)  # (environment r runs on seed + r)
    if not a._checkpoint_calls():
        pytest.skip("the backend %s has no checkpoints in device memory" % a.backend_name())
    with open(base) as f:
        seed1 = json.load(f)["seed"] + 1
    single = _hip(mod, _cfx(base, "seed%d" % seed1, top={"seed": seed1}))
    file_plan = a.get_tl_phase_durations_array()
    x = file_plan.copy()
    for r in range(envs):  # one plan per environment
        x[r] = np.where(file_plan[r] > 0, file_plan[r] + 1.0 + (r % 5), file_plan[r])
    for v in (a, b):
        v.set_tl_plan(durations=x)
    single.set_tl_plan(durations=x[1])
    for _ in range(60):
        a.next_step()
        b.next_step()
        single.next_step()
    ck = b.checkpoint()
    assert ck.step == 60 and ck.num_running == b.get_vehicle_count() and ck.device_bytes > 0
    first = []
    for attempt in range(2):
        b.set_tl_plan(durations=np.where(x > 0, x + 9.0, x))
        for _ in range(40 if attempt == 0 else 5):
            b.next_step()
        b.rollback(ck)
        b.set_tl_plan(durations=x)
        assert b._scalars()["step"] == 60
        for s in range(40):
            b.next_step()
            if attempt == 0:
                a.next_step()
                single.next_step()
                _assert_vector_same(a, b, "VectorEngine %d envs, step %d after the rollback" % (envs, s + 1))
                first.append(_vector_record(b))
            else:
                again = _vector_record(b)
                for k in ("lanes", "waiting"):
                    assert np.array_equal(again[k], first[s][k]), (s, k)
                assert again["speed1"] == first[s]["speed1"] and again["scalars"] == first[s]["scalars"], s
    assert b.get_vehicle_speed(1) == single.get_vehicle_speed() and b.get_lane_vehicle_count(1) == single.get_lane_vehicle_count()
    assert len(single.get_vehicle_speed()) > 0


@pytest.mark.gpu
def test_into_release_and_lifetime(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    e, other = _hip(mod, cfg), _hip(mod, cfg)
    for _ in range(30):
        e.next_step()
    ck = e.checkpoint()
    step, running = ck.step, ck.num_running
    for _ in range(30):
        e.next_step()
    same = e.checkpoint(into=ck)
    assert same is ck and ck.step == step + 30 and ck.num_running == e.get_vehicle_count() != running
    with pytest.raises(ValueError):
        other.rollback(ck)
    with pytest.raises(ValueError):
        other.checkpoint(into=ck)
    ck.release()
    assert ck.released and ck.device_bytes == 0
    with pytest.raises(ValueError):
        e.rollback(ck)
    with pytest.raises(ValueError):
        e.checkpoint(into=ck)
    ck.release()  # (twice is harmless)
    # the checkpoint keeps its engine alive: dropping the engine first is harmless
    late = other.checkpoint()
    del other
    gc.collect()
    assert late.device_bytes > 0
    late.release()
    del late
    # memory: what a checkpoint takes it gives back
    e.checkpoint().release()
    e.sync()
    free_after_first = e._device_memory()[0]
    for _ in range(20):
        e.checkpoint().release()
    e.sync()
    assert e._device_memory()[0] == free_after_first


@pytest.mark.gpu
def test_only_on_the_ring_layout(mod, scen, workdir):
    base = scen.materialize("example_1x1", workdir)
    probe = _hip(mod, base)  # (skips on a backend without the calls)
    assert probe._layout() == "ring" and probe._checkpoint_unsupported() == ""
    dense = mod.Engine(_cfx(base, "dense", layout="dense"), 1)
    with pytest.raises(NotImplementedError, match="dense"):
        dense.checkpoint()
    lc = mod.Engine(scen.materialize("example_1x1", workdir, laneChange=True), 1)
    with pytest.raises(NotImplementedError, match="laneChange"):
        lc.checkpoint()
    with pytest.raises(NotImplementedError, match="laneChange"):
        lc.rollback(None)


def test_no_device_checkpoints_on_the_twin(mod, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir)
    tw = mod.Engine._with_backend(cfg, 1, TWIN_LIB)
    assert not tw._checkpoint_calls()
    with pytest.raises(NotImplementedError, match=tw.backend_name()):
        tw.checkpoint()
    with pytest.raises(NotImplementedError):
        tw.rollback(None)
    lc = mod.Engine._with_backend(scen.materialize("example_1x1", workdir, laneChange=True), 1, TWIN_LIB)
    with pytest.raises(NotImplementedError):
        lc.checkpoint()
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    with pytest.raises(NotImplementedError, match=vec.backend_name()):
        vec.checkpoint()
    from cityflow_amd import _cityflow
    assert not hasattr(_cityflow.TiledEngine, "checkpoint") and not hasattr(_cityflow.TiledEngine, "rollback")
    assert hasattr(_cityflow.Engine, "checkpoint") and hasattr(_cityflow.VectorEngine, "rollback")


def test_importing_the_package_still_does_not_import_torch():
    code = "import sys; import cityflow_amd; assert cityflow_amd.Engine.checkpoint and 'torch' not in sys.modules"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)
