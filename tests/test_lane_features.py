"""Per-lane speed and position features: lane_lengths, get_lane_speed_sum_array / _tensor, get_lane_vehicle_bins_array /
_tensor and observe_lanes_tensor on Engine and VectorEngine (cityflow_amd/torch_io.py, cfx_observe_lanes_device /
cfx_get_lane_features).

Every value is exact: the speed sum is added front to back like the reference's curSpeedSum, and the bins are integer
counts, so each check below is array_equal against an oracle built from the dict getters (or, with lane change, from the
vehicle view grouped by drivable).  CPU tests pin the semantics on the twin (the host computes the arrays from
cfx_get_vehicles there); gpu tests run kr_lane_features / kd_lane_features."""
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_same_state

torch = pytest.importorskip("torch")

from test_device_tensors import host_apply, policy_rule, tensor_device  # noqa: E402


def twin(mod, cfg):
    return mod.Engine._with_backend(cfg, 1, TWIN_LIB)


def edge_sets(lengths):
    """(name, float64 edges) pairs: per-lane [L, B+1] and shared [B+1] schemes, including the corner cases of the rule."""
    L = lengths.shape[0]
    inf = np.inf
    return [
        ("thirds", lengths[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, inf])),
        ("last 50 m", np.stack([lengths - 50.0, np.full(L, inf)], axis=1)),
        ("inverted and NaN", np.array([-inf, 0.0, 20.0, 10.0, inf, np.nan, 5.0])),
        ("B = 32 per lane", lengths[:, None] * np.linspace(0.0, 1.0, 33)),
        ("B = 32 shared", np.concatenate([[-inf], np.linspace(0.0, 300.0, 31), [inf]])),
        # (the shared row is written for 300 m lanes; the same scheme scaled to each lane's own length)
        ("B = 32 per lane, open ends", np.concatenate([np.full((L, 1), -inf), lengths[:, None] * np.linspace(0.0, 1.0, 31),
                                                        np.full((L, 1), inf)], axis=1)),
        ("one bin", np.array([0.0, 100.0])),
    ]


def dict_oracle(eng, edges):
    """speed sum [L] and bins [L, B] from get_lane_vehicles / get_vehicle_speed / get_vehicle_distance (no lane change)."""
    lanes, speed, dist = eng.get_lane_vehicles(), eng.get_vehicle_speed(), eng.get_vehicle_distance()
    ids = eng.lane_ids()
    L, B = len(ids), edges.shape[-1] - 1
    rows = edges if edges.ndim == 2 else np.broadcast_to(edges, (L, B + 1))
    ssum = np.zeros(L)
    bins = np.zeros((L, B), dtype=np.int32)
    for l, lid in enumerate(ids):
        s = 0.0
        for v in lanes[lid]:
            s += speed[v]
            d = dist[v]
            bins[l] += (rows[l, :-1] <= d) & (d < rows[l, 1:])  # (every bin at once: lo <= d < hi)
        ssum[l] = s
    return ssum, bins


def view_oracle(eng, edges):
    """The same from _vehicle_state() grouped by drivable (front to back inside one): lane-change shadows included."""
    st = eng._vehicle_state()
    L, B = len(eng.lane_ids()), edges.shape[-1] - 1
    rows = edges if edges.ndim == 2 else np.broadcast_to(edges, (L, B + 1))
    ssum = np.zeros(L)
    bins = np.zeros((L, B), dtype=np.int32)
    counts = np.zeros(L, dtype=np.int64)
    for d, x, v in zip(st["drivable"], st["dis"], st["speed"]):
        if d >= L:
            continue
        counts[d] += 1
        ssum[d] = ssum[d] + v
        bins[d] += (rows[d, :-1] <= x) & (x < rows[d, 1:])  # (every bin at once: lo <= x < hi)
    return ssum, bins, counts


def check_features(eng, oracle, where, with_tensors=True):
    lengths = eng.lane_lengths()
    for name, edges in edge_sets(lengths):
        want_sum, want_bins = oracle(eng, edges)[:2]
        got_sum = eng.get_lane_speed_sum_array()
        got_bins = eng.get_lane_vehicle_bins_array(edges)
        assert got_sum.dtype == np.float64 and got_bins.dtype == np.int32
        assert np.array_equal(got_sum, want_sum), "%s: speed sums differ" % where
        assert np.array_equal(got_bins, want_bins), "%s, %s: bins differ" % (where, name)
        if not with_tensors:
            continue
        device = tensor_device(eng)
        te = torch.from_numpy(np.ascontiguousarray(edges)).to(device)
        tb = eng.get_lane_vehicle_bins_tensor(te)
        ts = eng.get_lane_speed_sum_tensor()
        assert tb.dtype == torch.int32 and ts.dtype == torch.float64 and tb.device == device
        assert np.array_equal(tb.cpu().numpy(), want_bins), "%s, %s: bins tensor differs" % (where, name)
        assert np.array_equal(ts.cpu().numpy(), want_sum), "%s: speed sum tensor differs" % where
        L, B = want_bins.shape
        c = torch.empty(L, dtype=torch.int32, device=device)
        w = torch.empty(L, dtype=torch.int32, device=device)
        s = torch.empty(L, dtype=torch.float64, device=device)
        b = torch.empty((L, B), dtype=torch.int32, device=device)
        eng.observe_lanes_tensor(counts=c, waiting=w, speed_sum=s, bins=b, edges=te.float())  # (float32 edges: converted)
        want_bins32 = oracle(eng, te.float().double().cpu().numpy())[1]
        assert np.array_equal(c.cpu().numpy(), eng.get_lane_vehicle_count_array()), where
        assert np.array_equal(w.cpu().numpy(), eng.get_lane_waiting_vehicle_count_array()), where
        assert np.array_equal(s.cpu().numpy(), want_sum), where
        assert np.array_equal(b.cpu().numpy(), want_bins32), "%s, %s (float32 edges)" % (where, name)


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
def test_features_equal_the_dict_oracle_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir))
    busy = 0
    for s in range(60):
        eng.next_step()
        if s % 10 == 9:
            check_features(eng, dict_oracle, "step %d" % s)
            busy += int((eng.get_lane_speed_sum_array() > 0).sum())
    assert busy > 0


def test_vector_engine_equals_standalone_twins(mod, scen, workdir):
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 3, 1, TWIN_LIB)
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=e)) for e in range(3)]
    lengths = vec.lane_lengths()
    assert np.array_equal(lengths, singles[0].lane_lengths())
    L = lengths.shape[0]
    for s in range(60):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % 10 != 9:
            continue
        got = vec.get_lane_speed_sum_array()
        assert got.shape == (3, L)
        assert np.array_equal(got, np.stack([e.get_lane_speed_sum_array() for e in singles])), "step %d" % s
        for name, edges in edge_sets(lengths):
            got = vec.get_lane_vehicle_bins_array(edges)
            assert got.shape == (3, L, edges.shape[-1] - 1)
            want = np.stack([e.get_lane_vehicle_bins_array(edges) for e in singles])
            assert np.array_equal(got, want), "step %d, %s" % (s, name)
            tb = vec.get_lane_vehicle_bins_tensor(torch.from_numpy(np.ascontiguousarray(edges)))
            assert np.array_equal(tb.numpy(), want), "step %d, %s (tensor)" % (s, name)
        ts = torch.empty((3, L), dtype=torch.float64)
        assert vec.get_lane_speed_sum_tensor(out=ts) is ts
        assert np.array_equal(ts.numpy(), vec.get_lane_speed_sum_array())


def test_lane_lengths_equal_the_roadnet_probe(mod, scen, workdir):
    import os
    cfg = scen.materialize("grid_6x6", workdir)
    probe = mod._roadnet_probe(os.path.join(os.path.dirname(cfg), "roadnet.json")).decode().splitlines()
    lines = [ln for ln in probe if ln.startswith("L ")]
    eng = twin(mod, cfg)
    lengths = eng.lane_lengths()
    assert lengths.dtype == np.float64 and lengths.shape == (len(eng.lane_ids()),) == (len(lines),)
    for lid, x, ln in zip(eng.lane_ids(), lengths, lines):
        assert ln.split()[1:3] == [lid, "%.17g" % x]


def test_argument_errors_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir))
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 2, 1, TWIN_LIB)
    L = len(eng.lane_ids())
    for e in (eng, vec):
        with pytest.raises(ValueError):  # B = 0
            e.get_lane_vehicle_bins_array(np.array([1.0]))
        with pytest.raises(ValueError):  # B = 33
            e.get_lane_vehicle_bins_array(np.arange(34.0))
        with pytest.raises(ValueError):  # per-lane edges with the wrong number of rows
            e.get_lane_vehicle_bins_array(np.zeros((L + 1, 3)))
        with pytest.raises(ValueError):
            e.get_lane_vehicle_bins_array(np.zeros((L, 3, 1)))
        with pytest.raises(ValueError):
            e.get_lane_vehicle_bins_tensor(torch.zeros(1, dtype=torch.float64))
        with pytest.raises(ValueError):
            e.get_lane_vehicle_bins_tensor(torch.zeros(34, dtype=torch.float64))
        with pytest.raises(ValueError):
            e.get_lane_vehicle_bins_tensor(torch.zeros((L - 1, 4), dtype=torch.float64))
        with pytest.raises(TypeError):
            e.get_lane_vehicle_bins_tensor(torch.zeros(4, dtype=torch.int64))
        with pytest.raises(TypeError):
            e.get_lane_vehicle_bins_tensor(np.zeros(4))
    shape = (L,)
    with pytest.raises(TypeError):
        eng.get_lane_speed_sum_tensor(out=torch.zeros(shape, dtype=torch.float32))
    with pytest.raises(ValueError):
        eng.get_lane_speed_sum_tensor(out=torch.zeros(L + 1, dtype=torch.float64))
    with pytest.raises(TypeError):
        eng.get_lane_vehicle_bins_tensor(torch.zeros(4), out=torch.zeros((L, 3), dtype=torch.int64))
    with pytest.raises(ValueError):
        eng.get_lane_vehicle_bins_tensor(torch.zeros(4), out=torch.zeros((L, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        vec.get_lane_speed_sum_tensor(out=torch.zeros(L, dtype=torch.float64))  # [R, L] wanted
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor()
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor(bins=torch.zeros((L, 3), dtype=torch.int32))
    with pytest.raises(TypeError):
        eng.observe_lanes_tensor(counts=torch.zeros(L, dtype=torch.float64))
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor(waiting=torch.zeros((L, 1), dtype=torch.int32))


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    code = ("import sys, cityflow_amd; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert hasattr(cityflow_amd.Engine, 'observe_lanes_tensor')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_features_equal_the_dict_oracle_grid_6x6(mod, scen, workdir, layout):
    extra = {} if layout == "auto" else {"cfx": {"layout": "dense"}}
    eng = mod.Engine(scen.materialize("grid_6x6", workdir, **extra), 1)
    if eng._device_buffers():
        assert eng._layout() == ("ring" if layout == "auto" else "dense")
    for s in range(300):
        eng.next_step()
        if s % 25 == 24:
            check_features(eng, dict_oracle, "%s, step %d" % (layout, s))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ring", "dense"])
def test_features_on_the_bench_workload(mod, workdir, layout):
    import bench
    extra = {} if layout == "ring" else {"cfx": {"layout": "dense"}}
    cfg = bench.with_config(bench.build_workload(workdir, 0), "features_" + layout, **extra)
    eng = mod.Engine(cfg, 1)
    if eng._device_buffers():
        assert eng._layout() == layout
    for s in range(100):
        eng.next_step()
        if s % 50 == 49:
            check_features(eng, dict_oracle, "%s, step %d" % (layout, s), with_tensors=(s == 99))
    assert eng.get_vehicle_count() > 10000


@pytest.mark.gpu
def test_features_with_lane_change_dense(mod, scen, workdir):
    eng = mod.Engine(scen.materialize("grid_6x6", workdir, laneChange=True), 1)
    if eng._device_buffers():
        assert eng._layout() == "dense"
    for s in range(200):
        eng.next_step()
        if s % 20 != 19:
            continue
        check_features(eng, view_oracle, "lane change, step %d" % s)
        counts = view_oracle(eng, np.array([0.0, 1.0]))[2]
        assert np.array_equal(counts, eng.get_lane_vehicle_count_array()), "step %d: lane populations" % s
    assert eng.get_vehicle_count() > 0


@pytest.mark.gpu
def test_observe_lanes_closed_loop(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    dev, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    device = tensor_device(dev)
    n_np = dev._phase_counts()
    n_phases = torch.from_numpy(n_np).to(device).long()
    L = len(dev.lane_ids())
    edges_np = dev.lane_lengths()[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, np.inf])
    edges = torch.from_numpy(edges_np).to(device)
    c = torch.empty(L, dtype=torch.int32, device=device)
    w = torch.empty(L, dtype=torch.int32, device=device)
    sp = torch.empty(L, dtype=torch.float64, device=device)
    b = torch.empty((L, 3), dtype=torch.int32, device=device)
    for s in range(200):
        dev.observe_lanes_tensor(counts=c, waiting=w, speed_sum=sp, bins=b, edges=edges)
        near = b[:, 2].long()  # (the policy reads a bin, so a wrong one changes the trajectory)
        dev.set_tl_phases_tensor(policy_rule(c.long() + near, w.long(), s, n_phases, torch))
        hc, hw = ref.get_lane_vehicle_count_array(), ref.get_lane_waiting_vehicle_count_array()
        hb = ref.get_lane_vehicle_bins_array(edges_np)
        assert np.array_equal(c.cpu().numpy(), hc), "counts differ at step %d" % s
        assert np.array_equal(w.cpu().numpy(), hw), "waiting counts differ at step %d" % s
        assert np.array_equal(sp.cpu().numpy(), ref.get_lane_speed_sum_array()), "speed sums differ at step %d" % s
        assert np.array_equal(b.cpu().numpy(), hb), "bins differ at step %d" % s
        host_apply(ref, policy_rule(hc.astype(np.int64) + hb[:, 2], hw.astype(np.int64), s, n_np.astype(np.int64), np))
        dev.next_step()
        ref.next_step()
    assert_same_state(dev, ref, "after the closed loop")


@pytest.mark.gpu
def test_vector_engine_tensors_equal_standalone(mod, scen, workdir):
    vec = mod.VectorEngine(scen.materialize("grid_6x6", workdir), 4)
    singles = [mod.Engine(scen.materialize("grid_6x6", workdir, seed=e), 1) for e in range(4)]
    device = tensor_device(vec)
    lengths = vec.lane_lengths()
    L = lengths.shape[0]
    for s in range(150):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % 30 != 29:
            continue
        for name, edges in edge_sets(lengths):
            te = torch.from_numpy(np.ascontiguousarray(edges)).to(device)
            B = edges.shape[-1] - 1
            c = torch.empty((4, L), dtype=torch.int32, device=device)
            sp = torch.empty((4, L), dtype=torch.float64, device=device)
            b = torch.empty((4, L, B), dtype=torch.int32, device=device)
            vec.observe_lanes_tensor(counts=c, speed_sum=sp, bins=b, edges=te)
            want_b = np.stack([e.get_lane_vehicle_bins_array(edges) for e in singles])
            want_s = np.stack([dict_oracle(e, edges)[0] for e in singles])
            assert np.array_equal(b.cpu().numpy(), want_b), "step %d, %s" % (s, name)
            assert np.array_equal(sp.cpu().numpy(), want_s), "step %d" % s
            assert np.array_equal(c.cpu().numpy(), np.stack([e.get_lane_vehicle_count_array() for e in singles]))
            assert np.array_equal(vec.get_lane_vehicle_bins_array(edges), want_b), "step %d, %s (array)" % (s, name)
            assert np.array_equal(vec.get_lane_speed_sum_tensor().cpu().numpy(), want_s)


@pytest.mark.gpu
def test_hip_features_equal_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, tw = mod.Engine(cfg, 1), twin(mod, cfg)
    for s in range(240):
        eng.next_step()
        tw.next_step()
        if s % 30 != 29:
            continue
        assert np.array_equal(eng.get_lane_speed_sum_array(), tw.get_lane_speed_sum_array()), "step %d" % s
        assert np.array_equal(eng.get_lane_speed_sum_tensor().cpu().numpy(), tw.get_lane_speed_sum_array()), "step %d" % s
        for name, edges in edge_sets(eng.lane_lengths()):
            want = tw.get_lane_vehicle_bins_array(edges)
            assert np.array_equal(eng.get_lane_vehicle_bins_array(edges), want), "step %d, %s" % (s, name)
            te = torch.from_numpy(np.ascontiguousarray(edges)).to(tensor_device(eng))
            assert np.array_equal(eng.get_lane_vehicle_bins_tensor(te).cpu().numpy(), want), "step %d, %s" % (s, name)


@pytest.mark.gpu
def test_features_on_a_side_stream_without_a_host_wait(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    device = tensor_device(eng)
    L = len(eng.lane_ids())
    edges_np = np.stack([eng.lane_lengths() - 100.0, np.full(L, np.inf)], axis=1)
    edges = torch.from_numpy(edges_np).to(device)
    for s in range(20):  # warm: rings built, tables uploaded, the first observation taken
        eng.next_step()
        ref.next_step()
    c = torch.empty(L, dtype=torch.int32, device=device)
    sp = torch.empty(L, dtype=torch.float64, device=device)
    b = torch.empty((L, 1), dtype=torch.int32, device=device)
    eng.observe_lanes_tensor(counts=c, speed_sum=sp, bins=b, edges=edges)
    eng.sync()
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device=device)
    records = []
    eng._device_spin(200000)  # 200 ms of device work in front of everything below
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for s in range(8):
            eng.next_step()
            eng.observe_lanes_tensor(counts=c, speed_sum=sp, bins=b, edges=edges)
            records.append((c.clone(), sp.clone(), b.clone()))  # consumed on `side`, then the outputs are reused
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the feature loop waited for the device (%.1f ms for 8 iterations behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    for s in range(8):
        ref.next_step()
        got_c, got_s, got_b = (t.cpu().numpy() for t in records[s])
        assert np.array_equal(got_c, ref.get_lane_vehicle_count_array()), "step %d" % s
        assert np.array_equal(got_s, ref.get_lane_speed_sum_array()), "step %d" % s
        assert np.array_equal(got_b, ref.get_lane_vehicle_bins_array(edges_np)), "step %d" % s
    assert_same_state(eng, ref, "after the unsynchronised loop")
