"""Lane observations and signal control as torch tensors (cityflow_amd/torch_io.py): get_lane_vehicle_count_tensor,
get_lane_waiting_vehicle_count_tensor, set_tl_phases_tensor on Engine and VectorEngine.

CPU tests pin the semantics on the twin (CPU tensors over the array calls); gpu tests run the device path (kd_lane_features /
kr_lane_features, k_set_phases_dense) against HIP engines driven through the numpy calls, and against the twin."""
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_same_state

torch = pytest.importorskip("torch")


def twin(mod, cfg):
    return mod.Engine._with_backend(cfg, 1, TWIN_LIB)


def tensor_device(eng):
    """Where this engine's tensors live: its GPU, or the CPU for a backend without device buffers (the twin)."""
    return torch.device("cuda", eng._stream_handle()[1]) if eng._device_buffers() else torch.device("cpu")


def virtual_mask(eng):
    return eng._phase_counts() < 0


def policy_rule(counts, waiting, step, n_phases, xp):
    """Any rule whose output depends on the observation: a stale or early read changes the trajectory.  Works on numpy
    arrays and torch tensors alike (`xp` = the module); -1 (keep) where the chosen lane's count is a multiple of 5."""
    flat_c = counts.reshape(-1)
    flat_w = waiting.reshape(-1)
    L = flat_c.shape[0]
    I = n_phases.shape[0]
    ar = xp.arange(I, device=counts.device) if xp is torch else xp.arange(I)
    a = flat_c[(ar * 7 + step) % L]
    b = flat_w[(ar * 3 + 1) % L]
    npos = xp.where(n_phases > 0, n_phases, xp.ones_like(n_phases))
    p = (a + b + ar + step) % npos
    p = xp.where(a % 5 == 0, -xp.ones_like(p), p)
    return xp.where(n_phases > 0, p, -xp.ones_like(p))


def host_apply(eng, want):
    """The numpy path with -1 = keep: what set_tl_phases_tensor must equal."""
    cur = np.asarray(eng._tl_state()[0]).reshape(want.shape)
    eng.set_tl_phases(np.where(want == -1, cur, want).astype(np.int32))


def assert_tl_equal(a, b, where):
    pa, pb = a._tl_state(), b._tl_state()
    assert np.array_equal(pa[0], pb[0]), where + ": phases differ"
    assert np.array_equal(pa[1], pb[1]), where + ": remaining times differ"


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
def test_getters_equal_arrays_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir))
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 3, 1, TWIN_LIB)
    L = len(eng.lane_ids())
    out_c = torch.zeros(L, dtype=torch.int32)
    out_w = torch.zeros(L, dtype=torch.int32)
    vout = torch.zeros((3, L), dtype=torch.int32)
    for s in range(60):
        eng.next_step()
        vec.next_step()
        if s % 10:
            continue
        c, w = eng.get_lane_vehicle_count_tensor(), eng.get_lane_waiting_vehicle_count_tensor()
        assert c.dtype == torch.int32 and w.dtype == torch.int32 and tuple(c.shape) == (L,) == tuple(w.shape)
        assert np.array_equal(c.numpy(), eng.get_lane_vehicle_count_array())
        assert np.array_equal(w.numpy(), eng.get_lane_waiting_vehicle_count_array())
        assert eng.get_lane_vehicle_count_tensor(out=out_c) is out_c
        assert eng.get_lane_waiting_vehicle_count_tensor(out=out_w) is out_w
        assert torch.equal(out_c, c) and torch.equal(out_w, w)
        vc = vec.get_lane_vehicle_count_tensor()
        assert tuple(vc.shape) == (3, L) and vc.dtype == torch.int32
        assert np.array_equal(vc.numpy(), vec.get_lane_vehicle_count_array())
        assert vec.get_lane_waiting_vehicle_count_tensor(out=vout) is vout
        assert np.array_equal(vout.numpy(), vec.get_lane_waiting_vehicle_count_array())
    assert int(c.sum()) > 0


def test_set_tensor_equals_numpy_200_steps_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    a, b = twin(mod, cfg), twin(mod, cfg)
    n_phases = a._phase_counts()
    rng = np.random.default_rng(7)
    for s in range(200):
        if s % 3 == 0:
            p = (rng.integers(0, 1 << 20, size=n_phases.shape[0]) % np.maximum(n_phases, 1)).astype(np.int32)
            a.set_tl_phases_tensor(torch.from_numpy(p.astype(np.int64)))
            b.set_tl_phases(p)
        a.next_step()
        b.next_step()
        assert_tl_equal(a, b, "step %d" % s)
        assert np.array_equal(a.get_lane_vehicle_count_array(), b.get_lane_vehicle_count_array()), "step %d" % s
    assert_same_state(a, b, "after 200 steps")


def test_minus_one_keeps_and_virtual_ignored_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir, rlTrafficLight=True))
    n_phases = eng._phase_counts()
    virt = virtual_mask(eng)
    assert virt.any() and (~virt).any()
    base = np.where(virt, 0, 1).astype(np.int32)
    eng.set_tl_phases(base)
    want = np.where(virt, 12345, -1).astype(np.int64)  # keep every real signal; garbage where the entry is ignored
    real = np.nonzero(~virt)[0]
    want[real[::2]] = (n_phases[real[::2]] - 1)
    eng.set_tl_phases_tensor(torch.from_numpy(want))
    got = eng._tl_state()[0]
    expect = base.copy()
    expect[real[::2]] = n_phases[real[::2]] - 1
    assert np.array_equal(got[~virt], expect[~virt])


def test_invalid_phase_rejects_whole_call_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng, ref = twin(mod, cfg), twin(mod, cfg)
    ids = eng.intersection_ids()
    virt = virtual_mask(eng)
    real = np.nonzero(~virt)[0]
    for _ in range(20):
        eng.next_step()
        ref.next_step()
    bad = np.ones(len(ids), dtype=np.int32)
    bad[real[3]] = eng._phase_counts()[real[3]]  # one past the last phase
    before = eng._tl_state()[0].copy()
    with pytest.raises(IndexError, match=ids[real[3]]):
        eng.set_tl_phases_tensor(torch.from_numpy(bad))
        eng.sync()
    assert np.array_equal(eng._tl_state()[0], before), "a rejected call changed a signal"
    for s in range(40):
        eng.next_step()
        ref.next_step()
    assert_same_state(eng, ref, "after the rejected call")


def test_numpy_tensor_numpy_ends_at_numpy_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir, rlTrafficLight=True))
    n_phases = eng._phase_counts()
    p = np.where(n_phases > 0, 1, 0).astype(np.int32)
    q = np.where(n_phases > 0, 2, 0).astype(np.int32)
    eng.set_tl_phases(p)
    eng.next_step()
    eng.set_tl_phases_tensor(torch.from_numpy(q))
    eng.next_step()
    eng.set_tl_phases(p)
    eng.next_step()
    real = n_phases > 0
    assert np.array_equal(eng._tl_state()[0][real], p[real])


def test_without_rl_traffic_light_changes_nothing_twin(mod, scen, workdir, capfd):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, ref = twin(mod, cfg), twin(mod, cfg)
    n = len(eng.intersection_ids())
    for s in range(30):
        eng.set_tl_phases_tensor(torch.full((n,), 1, dtype=torch.int32))
        eng.next_step()
        ref.next_step()
    assert "please set rlTrafficLight to true" in capfd.readouterr().err
    assert_same_state(eng, ref, "rlTrafficLight false")


def test_vector_engine_tensor_control_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    vec = mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB)
    ref = mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB)
    n_phases = vec._phase_counts()
    for s in range(80):
        c, w = vec.get_lane_vehicle_count_tensor(), vec.get_lane_waiting_vehicle_count_tensor()
        want = torch.stack([policy_rule(c[r], w[r], s + r, torch.from_numpy(n_phases), torch) for r in range(3)])
        vec.set_tl_phases_tensor(want)
        host_apply(ref, want.numpy())
        vec.next_step()
        ref.next_step()
        assert np.array_equal(vec._tl_state()[0], ref._tl_state()[0]), "step %d" % s
        assert np.array_equal(vec.get_lane_vehicle_count_array(), ref.get_lane_vehicle_count_array()), "step %d" % s
    bad = want.clone()
    real = np.nonzero(n_phases >= 0)[0]
    bad[2, int(real[0])] = -2
    with pytest.raises(IndexError, match="env 2"):
        vec.set_tl_phases_tensor(bad)
        vec.sync()


def test_argument_errors_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir, rlTrafficLight=True))
    L, I = len(eng.lane_ids()), len(eng.intersection_ids())
    with pytest.raises(TypeError):
        eng.get_lane_vehicle_count_tensor(out=torch.zeros(L, dtype=torch.int64))
    with pytest.raises(ValueError):
        eng.get_lane_vehicle_count_tensor(out=torch.zeros(L + 1, dtype=torch.int32))
    with pytest.raises(TypeError):
        eng.set_tl_phases_tensor(torch.zeros(I, dtype=torch.float32))
    with pytest.raises(ValueError):
        eng.set_tl_phases_tensor(torch.zeros(I - 1, dtype=torch.int32))
    with pytest.raises(TypeError):
        eng.set_tl_phases_tensor(np.zeros(I, dtype=np.int32))


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    code = "import sys; import cityflow_amd, cityflow; assert 'torch' not in sys.modules, 'torch imported'"
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---------------------------------------------------------------------------------------------------------------- GPU
def closed_loop(dev_eng, ref_eng, steps, speeds_every=50, twin_eng=None):
    """dev_eng: the policy on the engine's device through the tensor calls; ref_eng: the same rule on the host over the
    numpy getters (twin_eng, optional: a third engine driven like ref_eng, compared at the end)."""
    device = tensor_device(dev_eng)
    n_phases_np = dev_eng._phase_counts()
    n_phases = torch.from_numpy(n_phases_np).to(device)
    shape = tuple(dev_eng._tensor_shapes()[0])
    out_c = torch.empty(shape, dtype=torch.int32, device=device)
    out_w = torch.empty(shape, dtype=torch.int32, device=device)
    envs = shape[0] if len(shape) == 2 else 0

    def rule(c, w, s, xp, npf):
        if not envs:
            return policy_rule(c, w, s, npf, xp)
        rows = [policy_rule(c[r], w[r], s + r, npf, xp) for r in range(envs)]
        return xp.stack(rows)

    for s in range(steps):
        c = dev_eng.get_lane_vehicle_count_tensor(out=out_c)
        w = dev_eng.get_lane_waiting_vehicle_count_tensor(out=out_w)
        dev_eng.set_tl_phases_tensor(rule(c.long(), w.long(), s, torch, n_phases.long()))
        for e in [ref_eng] + ([twin_eng] if twin_eng is not None else []):
            hc, hw = e.get_lane_vehicle_count_array(), e.get_lane_waiting_vehicle_count_array()
            host_apply(e, rule(hc.astype(np.int64), hw.astype(np.int64), s, np, n_phases_np.astype(np.int64)))
        dev_eng.next_step()
        for e in [ref_eng] + ([twin_eng] if twin_eng is not None else []):
            e.next_step()
        got_c = dev_eng.get_lane_vehicle_count_tensor().cpu().numpy()
        got_w = dev_eng.get_lane_waiting_vehicle_count_tensor().cpu().numpy()
        assert np.array_equal(got_c, ref_eng.get_lane_vehicle_count_array()), "lane counts differ at step %d" % s
        assert np.array_equal(got_w, ref_eng.get_lane_waiting_vehicle_count_array()), "waiting counts differ at step %d" % s
        assert np.array_equal(dev_eng._tl_state()[0], ref_eng._tl_state()[0]), "signals differ at step %d" % s
        if speeds_every and s % speeds_every == speeds_every - 1 and not envs:
            assert_same_state(dev_eng, ref_eng, "step %d" % s)
    if twin_eng is not None:
        assert_same_state(dev_eng, twin_eng, "against the twin")
    assert int(got_c.sum()) > 0


@pytest.mark.gpu
def test_closed_loop_grid_6x6(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    closed_loop(mod.Engine(cfg, 1), mod.Engine(cfg, 1), 300, twin_eng=twin(mod, cfg))


@pytest.mark.gpu
def test_closed_loop_bench_workload_ring(mod, workdir):
    import bench
    cfg = bench.with_config(bench.build_workload(workdir, 0), "rl", rlTrafficLight=True)
    dev = mod.Engine(cfg, 1)
    assert dev._layout() == "ring"
    closed_loop(dev, mod.Engine(cfg, 1), 100)


@pytest.mark.gpu
def test_closed_loop_lane_change_dense(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True, laneChange=True)
    dev = mod.Engine(cfg, 1)
    assert dev._layout() == "dense" or not dev._device_buffers()  # (lane change runs on the dense layout; the twin has none)
    closed_loop(dev, mod.Engine(cfg, 1), 150)


@pytest.mark.gpu
def test_closed_loop_vector_engine_vs_standalone(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    vec = mod.VectorEngine(cfg, 4)
    singles = [mod.Engine(scen.materialize("grid_6x6", workdir, rlTrafficLight=True, seed=e), 1) for e in range(4)]

    class Stacked:  # the four standalone engines seen as one [4, ...] engine through the numpy calls
        def get_lane_vehicle_count_array(self):
            return np.stack([e.get_lane_vehicle_count_array() for e in singles])

        def get_lane_waiting_vehicle_count_array(self):
            return np.stack([e.get_lane_waiting_vehicle_count_array() for e in singles])

        def _tl_state(self):
            st = [e._tl_state() for e in singles]
            return np.stack([s[0] for s in st]), np.stack([s[1] for s in st])

        def set_tl_phases(self, p):
            for e, row in zip(singles, p):
                e.set_tl_phases(row)

        def next_step(self):
            for e in singles:
                e.next_step()

    closed_loop(vec, Stacked(), 200, speeds_every=0)
    for r, e in enumerate(singles):
        assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "env %d speeds" % r


@pytest.mark.gpu
def test_observe_on_a_side_stream(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    device = tensor_device(eng)
    side = torch.cuda.Stream(device=device)
    out = torch.empty(len(eng.lane_ids()), dtype=torch.int32, device=device)
    clones, want = [], []
    for s in range(120):
        eng.next_step()
        ref.next_step()
        with torch.cuda.stream(side):
            c = eng.get_lane_vehicle_count_tensor(out=out)
            clones.append((c * 1).clone())  # consumed on `side`, then `out` is reused by the next observation
        want.append(ref.get_lane_vehicle_count_array())
    side.synchronize()
    for s, (got, w) in enumerate(zip(clones, want)):
        assert np.array_equal(got.cpu().numpy(), w), "step %d" % s


@pytest.mark.gpu
def test_tensor_loop_does_not_wait_for_the_device(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: the twin's calls are synchronous by nature")
    device = tensor_device(eng)
    n_phases = torch.from_numpy(eng._phase_counts()).to(device).long()
    L = len(eng.lane_ids())
    for s in range(20):  # warm: rings built, tables uploaded, the first observation taken
        eng.next_step()
        ref.next_step()
    c = eng.get_lane_vehicle_count_tensor()
    w = eng.get_lane_waiting_vehicle_count_tensor()
    eng.sync()
    torch.cuda.synchronize(device)
    records = []
    eng._device_spin(200000)  # 200 ms of device work in front of everything below
    t0 = time.perf_counter()
    for s in range(8):
        eng.set_tl_phases_tensor(policy_rule(c.long(), w.long(), s, n_phases, torch))
        eng.next_step()
        c = eng.get_lane_vehicle_count_tensor()
        w = eng.get_lane_waiting_vehicle_count_tensor()
        records.append((c, w))
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the tensor loop waited for the device (%.1f ms for 8 iterations behind a 200 ms spin)" % (elapsed * 1e3)
    eng.sync()
    torch.cuda.synchronize(device)
    for s in range(8):
        prev_c = ref.get_lane_vehicle_count_array().astype(np.int64)
        prev_w = ref.get_lane_waiting_vehicle_count_array().astype(np.int64)
        host_apply(ref, policy_rule(prev_c, prev_w, s, eng._phase_counts().astype(np.int64), np))
        ref.next_step()
        assert np.array_equal(records[s][0].cpu().numpy(), ref.get_lane_vehicle_count_array()), "step %d" % s
        assert np.array_equal(records[s][1].cpu().numpy(), ref.get_lane_waiting_vehicle_count_array()), "step %d" % s
    assert_same_state(eng, ref, "after the unsynchronised loop")


@pytest.mark.gpu
def test_invalid_phase_on_the_device(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    device = tensor_device(eng)
    ids = eng.intersection_ids()
    n_phases = eng._phase_counts()
    real = np.nonzero(n_phases >= 0)[0]
    for _ in range(30):
        eng.next_step()
        ref.next_step()
    good = torch.from_numpy(np.where(n_phases > 0, 1, 0).astype(np.int32)).to(device)
    bad = good.clone()
    bad[int(real[5])] = int(n_phases[real[5]]) + 3
    bad[int(real[9])] = -7  # the first offender is the one named
    before = eng._tl_state()[0].copy()
    with pytest.raises(IndexError, match=ids[real[5]]):
        eng.set_tl_phases_tensor(bad)
        eng.sync()
    assert np.array_equal(eng._tl_state()[0], before), "a rejected call changed a signal"
    for s in range(50):
        eng.next_step()
        ref.next_step()
    eng.set_tl_phases_tensor(good)
    ref.set_tl_phases(good.cpu().numpy())
    for s in range(50):
        eng.next_step()
        ref.next_step()
    assert_same_state(eng, ref, "after the rejected call")


@pytest.mark.gpu
def test_tensor_arguments_are_checked_up_front(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng = mod.Engine(cfg, 1)
    device = tensor_device(eng)
    L, I = len(eng.lane_ids()), len(eng.intersection_ids())
    with pytest.raises(TypeError):
        eng.get_lane_vehicle_count_tensor(out=torch.zeros(L, dtype=torch.int64, device=device))
    with pytest.raises(ValueError):
        eng.get_lane_waiting_vehicle_count_tensor(out=torch.zeros((L, 1), dtype=torch.int32, device=device))
    with pytest.raises(TypeError):
        eng.set_tl_phases_tensor(torch.zeros(I, dtype=torch.float64, device=device))
    with pytest.raises(ValueError):
        eng.set_tl_phases_tensor(torch.zeros(I + 1, dtype=torch.int32, device=device))
    if eng._device_buffers():
        with pytest.raises(TypeError):  # the HIP engine never falls back to host tensors
            eng.get_lane_vehicle_count_tensor(out=torch.zeros(L, dtype=torch.int32))
        with pytest.raises(TypeError):
            eng.set_tl_phases_tensor(torch.zeros(I, dtype=torch.int32))
        if torch.cuda.device_count() > 1:
            other = torch.device("cuda", (device.index + 1) % torch.cuda.device_count())
            with pytest.raises(TypeError):
                eng.set_tl_phases_tensor(torch.zeros(I, dtype=torch.int32, device=other))
    eng.next_step()
    eng.sync()  # nothing above was enqueued
