"""Per-lane front-K vehicle observations: the front_* outputs of observe_lanes_tensor, get_lane_front_vehicles_tensor and
get_lane_front_vehicles_array on Engine and VectorEngine (cityflow_amd/torch_io.py; cfx_observe_lane_obs_device / cfx_get_lane_obs,
kr_lane_features / kd_lane_features on the device; the vehicle view and the host tracker on the twin).

For lane l with n vehicles, slot k < n holds its k-th vehicle from the front, in get_lane_vehicles()'s order: its distance and
speed (copies of what get_vehicle_distance / get_vehicle_speed give) and, while track_lane_flow is on, s - since and wait of
the lane-flow tracker.  Slots k >= n hold -1.0 / 0.0 / 0 / 0.  Everything is a copy or an integer: every check is array_equal.

The oracle is built only from getters that predate the feature: get_lane_vehicles()[lane][:K] with get_vehicle_distance() /
get_vehicle_speed(); with lane change _vehicle_state() grouped by drivable; for the tracker columns test_lane_flow.Model.

K in {1, 15, 16, 17, 32, 33, 64}: one chunk of the lane walk's sixteen threads, the chunk boundary at either side, two chunks, one
slot more, and more slots than any lane holds.  Every value test asserts that what it looked at held, for every K <= 33, a lane
with more than K vehicles, an empty lane and (K >= 2: a lane cannot hold between 0 and 1 vehicles) a lane with 0 < n < K."""
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_same_state

torch = pytest.importorskip("torch")

from test_device_tensors import tensor_device  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_lane_flow import Model, hip_engine, layout_config  # noqa: E402

KS = (1, 15, 16, 17, 32, 33, 64)
FRONT = ("front_distance", "front_speed")
TRACKER = ("front_lane_steps", "front_waiting_steps")
DTYPES = {"front_distance": np.float64, "front_speed": np.float64, "front_lane_steps": np.int32, "front_waiting_steps": np.int32}
PAD = {"front_distance": -1.0, "front_speed": 0.0, "front_lane_steps": 0, "front_waiting_steps": 0}


# ------------------------------------------------------------------------------------------------------------------ oracle
def dict_lanes(eng, model=None, s=0):
    """Per lane, front to back: [(distance, speed, lane steps, waiting steps)] from the dict getters (and the model)."""
    lanes, speed, dist = eng.get_lane_vehicles(), eng.get_vehicle_speed(), eng.get_vehicle_distance()
    out = []
    for l, lid in enumerate(eng.lane_ids()):
        rec = model.on[l] if model is not None else None
        out.append([(dist[v], speed[v]) + ((s - rec[v][0], rec[v][1]) if rec is not None else (0, 0)) for v in lanes[lid]])
    return out


def view_lanes(eng):
    """The same from _vehicle_state() grouped by drivable (front to back inside one): lane-change shadows included."""
    st = eng._vehicle_state()
    out = [[] for _ in eng.lane_ids()]
    for d, x, v in zip(st["drivable"], st["dis"], st["speed"]):
        if d < len(out):
            out[d].append((x, v, 0, 0))
    return out


def want_fronts(lanes, k):
    want = {name: np.full((len(lanes), k), PAD[name], dtype=DTYPES[name]) for name in FRONT + TRACKER}
    for l, vehicles in enumerate(lanes):
        for j, rec in enumerate(vehicles[:k]):
            for name, x in zip(FRONT + TRACKER, rec):
                want[name][l, j] = x
    return want


class Looked:
    """What the checked states contained, per K.  `beyond_64`: the three kinds of lane are asked for at K = 64 too (a network
    whose lanes hold more than 64 vehicles)."""

    def __init__(self, beyond_64=False):
        self.beyond_64 = beyond_64
        self.seen = {k: set() for k in KS}
        self.moving = self.steps = self.waits = 0

    def at(self, lanes_per_env):
        for lanes in lanes_per_env:
            n = np.array([len(v) for v in lanes])
            for k in KS:
                self.seen[k] |= {name for name, hit in (("n > K", n > k), ("0 < n < K", (n > 0) & (n < k)), ("n = 0", n == 0)) if hit.any()}
            self.moving += sum(r[1] > 0 for v in lanes for r in v)
            self.steps += sum(r[2] > 0 for v in lanes for r in v)
            self.waits += sum(r[3] > 0 for v in lanes for r in v)

    def enough(self, tracker=False):
        for k in KS:
            if k <= 33 or self.beyond_64:
                need = {"n > K", "n = 0"} | ({"0 < n < K"} if k >= 2 else set())
                assert need <= self.seen[k], "K = %d: the checked states never had %s" % (k, sorted(need - self.seen[k]))
        assert self.moving > 0, "no vehicle with a speed in the checked states"
        if tracker:
            assert self.steps > 0 and self.waits > 0, "the tracker columns were zero throughout (%d, %d)" % (self.steps, self.waits)


def filled(eng, names, k, lead=()):
    """Tensors of a value no output takes: every element must be written."""
    shape = lead + (len(eng.lane_ids()), k)
    return {name: torch.full(shape, -7, dtype=torch.float64 if name in FRONT else torch.int32, device=tensor_device(eng)) for name in names}


def check_fronts(eng, lanes_per_env, where, tracker, ks=KS):
    """Array call, getter and observe_lanes_tensor for every K against the oracle.  `lanes_per_env`: one oracle per environment
    (a VectorEngine: a leading [R]) or a single one."""
    vector = hasattr(eng, "num_envs")
    names = FRONT + (TRACKER if tracker else ())
    for k in ks:
        per_env = [want_fronts(lanes, k) for lanes in lanes_per_env]
        want = {name: np.stack([w[name] for w in per_env]) if vector else per_env[0][name] for name in names}
        got = eng.get_lane_front_vehicles_array(k)
        assert sorted(got) == sorted(names), "%s: the array call gives %s" % (where, sorted(got))
        for name in names:
            assert got[name].dtype == DTYPES[name] and got[name].shape == want[name].shape, (where, name, got[name].dtype, got[name].shape)
            assert np.array_equal(got[name], want[name]), "%s, K = %d: %s differs (array call)" % (where, k, name)
        d, sp = eng.get_lane_front_vehicles_tensor(k)
        assert d.dtype == sp.dtype == torch.float64 and d.device == tensor_device(eng)
        assert np.array_equal(d.cpu().numpy(), want["front_distance"]), "%s, K = %d: distance getter" % (where, k)
        assert np.array_equal(sp.cpu().numpy(), want["front_speed"]), "%s, K = %d: speed getter" % (where, k)
        t = filled(eng, names, k, lead=(len(lanes_per_env),) if vector else ())
        eng.observe_lanes_tensor(**t)
        for name in names:
            assert np.array_equal(t[name].cpu().numpy(), want[name]), "%s, K = %d: %s differs (tensor call)" % (where, k, name)
        one = filled(eng, names[-1:], k, lead=(len(lanes_per_env),) if vector else ())  # (a single output on its own)
        eng.observe_lanes_tensor(**one)
        assert np.array_equal(one[names[-1]].cpu().numpy(), want[names[-1]]), "%s, K = %d: %s alone" % (where, k, names[-1])


def run_against_dict_oracle(eng, steps, every, where, tracker, fused=False, looked=None):
    """`tracker`: tracking on from the start, the tracker columns against Model.  `fused`: at every check one launch that fills all
    eight lane outputs, against the four getters that were there before.  `looked`: a Looked to fill and check instead of a fresh one."""
    model = None
    if tracker:
        eng.track_lane_flow(True)
        model = Model(eng.lane_ids())
        model.baseline(eng.get_lane_vehicles(), 0)
    looked = Looked() if looked is None else looked
    for s in range(steps):
        eng.next_step()
        if model is not None:
            model.tick(eng.get_lane_vehicles(), eng.get_vehicle_speed(), s + 1)
        if s % every != every - 1:
            continue
        lanes = dict_lanes(eng, model, s + 1)
        looked.at([lanes])
        check_fronts(eng, [lanes], "%s, step %d" % (where, s), tracker)
        if fused:
            check_all_eight(eng, lanes, "%s, step %d" % (where, s))
    looked.enough(tracker)


def check_all_eight(eng, lanes, where, k=17):
    device, L = tensor_device(eng), len(lanes)
    edges = eng.lane_lengths()[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, np.inf])
    t = filled(eng, FRONT + TRACKER, k)
    c = torch.full((L,), -7, dtype=torch.int32, device=device)
    w = torch.full((L,), -7, dtype=torch.int32, device=device)
    sp = torch.full((L,), -7.0, dtype=torch.float64, device=device)
    b = torch.full((L, 3), -7, dtype=torch.int32, device=device)
    eng.observe_lanes_tensor(counts=c, waiting=w, speed_sum=sp, bins=b, edges=torch.from_numpy(edges).to(device), **t)
    want = want_fronts(lanes, k)
    for name in FRONT + TRACKER:
        assert np.array_equal(t[name].cpu().numpy(), want[name]), "%s: %s differs in the fused launch" % (where, name)
    assert np.array_equal(c.cpu().numpy(), eng.get_lane_vehicle_count_array()), where
    assert np.array_equal(w.cpu().numpy(), eng.get_lane_waiting_vehicle_count_array()), where
    assert np.array_equal(sp.cpu().numpy(), eng.get_lane_speed_sum_array()), where
    assert np.array_equal(b.cpu().numpy(), eng.get_lane_vehicle_bins_array(edges)), where
    # a slot is real exactly if k < counts[l]
    real = np.arange(k)[None, :] < c.cpu().numpy()[:, None]
    assert np.array_equal(t["front_distance"].cpu().numpy() >= 0, real), where + ": the padding is not where counts says"


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
def test_fronts_equal_the_dict_oracle_twin(mod, scen, workdir):
    run_against_dict_oracle(twin(mod, scen.materialize("grid_6x6", workdir)), 400, 25, "twin", tracker=False)


def test_tracker_columns_equal_the_model_twin(mod, scen, workdir):
    run_against_dict_oracle(twin(mod, scen.materialize("grid_6x6", workdir)), 400, 25, "twin, tracking", tracker=True, fused=True)


def vector_body(vec, singles, steps, every, looked=None):
    looked = Looked() if looked is None else looked
    for s in range(steps):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % every != every - 1:
            continue
        lanes = [dict_lanes(e) for e in singles]
        looked.at(lanes)
        check_fronts(vec, lanes, "vector, step %d" % s, tracker=False)
    looked.enough()


def test_vector_engine_equals_standalone_twins(mod, scen, workdir):
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 3, 1, TWIN_LIB)
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=e)) for e in range(3)]
    vector_body(vec, singles, 400, 25)


def vector_tracker_body(vec, singles, steps, every, looked=None):
    """The tracker columns of a VectorEngine against standalone engines that track too (those against Model: the tests above).
    `looked`: a Looked to fill with what the standalone engines held at every check (the caller asks it what it needs)."""
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
        if looked is not None:
            looked.at([dict_lanes(e) for e in singles])
        for k in (16, 33):
            got, want = vec.get_lane_front_vehicles_array(k), [e.get_lane_front_vehicles_array(k) for e in singles]
            for name in FRONT + TRACKER:
                assert np.array_equal(got[name], np.stack([w[name] for w in want])), "step %d, K = %d: %s" % (s, k, name)
            seen += int(got["front_waiting_steps"].sum())
    assert seen > 0


def test_vector_engine_tracker_columns_twin(mod, scen, workdir):
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 3, 1, TWIN_LIB)
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=e)) for e in range(3)]
    vector_tracker_body(vec, singles, 120, 30)


def follow(eng, model, steps, first_step, looked, where):
    """`steps` steps with the model ticked after each, then the tracker columns (and the others) against it."""
    for s in range(steps):
        eng.next_step()
        model.tick(eng.get_lane_vehicles(), eng.get_vehicle_speed(), first_step + s + 1)
    check_now(eng, model, first_step + steps, looked, where)


def check_now(eng, model, s, looked, where):
    lanes = dict_lanes(eng, model, s)
    looked.at([lanes])
    flow = eng.observe_lane_flow_array()
    check_fronts(eng, [lanes], where, tracker=True, ks=(1, 16, 33, 64))
    after = eng.observe_lane_flow_array()
    for name in flow:  # reading is not draining
        assert np.array_equal(flow[name], after[name]), "%s: reading the fronts changed %s" % (where, name)


def baselines_body(make, cfg):
    """Enable mid-run, snapshot / load, reset: each a baseline, read right behind it and again after more steps."""
    eng = make(cfg)
    looked = Looked()
    for s in range(220):
        eng.next_step()
    with pytest.raises(RuntimeError):  # tracking is off
        eng.observe_lanes_tensor(**filled(eng, TRACKER, 4))
    assert sorted(eng.get_lane_front_vehicles_array(4)) == sorted(FRONT)
    eng.track_lane_flow(True)
    model = Model(eng.lane_ids())
    model.baseline(eng.get_lane_vehicles(), 220)
    check_now(eng, model, 220, looked, "turned on at step 220")
    follow(eng, model, 30, 220, looked, "30 steps after turning on")
    archive = eng.snapshot()
    follow(eng, model, 20, 250, looked, "after the snapshot")
    eng.load(archive)
    model.baseline(eng.get_lane_vehicles(), 250)
    check_now(eng, model, 250, looked, "right after load")
    follow(eng, model, 30, 250, looked, "30 steps after load")
    eng.reset()
    model.baseline(eng.get_lane_vehicles(), 0)
    check_now(eng, model, 0, looked, "right after reset")
    follow(eng, model, 60, 0, looked, "60 steps after reset")
    eng.track_lane_flow(False)
    assert sorted(eng.get_lane_front_vehicles_array(4)) == sorted(FRONT)
    looked.enough(tracker=True)


def test_tracker_columns_across_baselines_twin(mod, scen, workdir):
    baselines_body(lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir))


def compaction_body(make, materialize, steps=300, every=25):
    eng = make(materialize(cfx={"compactVehicles": 40}))
    eng.track_lane_flow(True)
    model = Model(eng.lane_ids())
    model.baseline(eng.get_lane_vehicles(), 0)
    looked, compactions = Looked(), set()
    for s in range(steps):
        eng.next_step()
        model.tick(eng.get_lane_vehicles(), eng.get_vehicle_speed(), s + 1)
        if s % every == every - 1:
            check_now(eng, model, s + 1, looked, "compacting engine, step %d" % s)
            compactions.add(eng._vehicle_table()[1])
    assert len(compactions) >= 3 and max(compactions) >= 2, "the checks did not straddle compactions: %s" % sorted(compactions)
    looked.enough(tracker=True)


def test_tracker_columns_survive_compaction_twin(mod, scen, workdir):
    compaction_body(lambda cfg: twin(mod, cfg), lambda **kw: scen.materialize("grid_6x6", workdir, **kw))


def lane_change_body(eng, steps=400, every=25):
    looked = Looked()
    for s in range(steps):
        eng.next_step()
        if s % every != every - 1:
            continue
        lanes = view_lanes(eng)
        assert np.array_equal([len(v) for v in lanes], eng.get_lane_vehicle_count_array()), "step %d: lane populations" % s
        looked.at([lanes])
        check_fronts(eng, [lanes], "lane change, step %d" % s, tracker=False)
    with pytest.raises(RuntimeError):  # tracking cannot be on with lane change
        eng.observe_lanes_tensor(**filled(eng, TRACKER, 4))
    looked.enough()


def test_lane_change_twin(mod, scen, workdir):
    lane_change_body(twin(mod, scen.materialize("grid_6x6", workdir, laneChange=True)))


def test_argument_errors_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = twin(mod, cfg)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    L = len(eng.lane_ids())
    for s in range(30):
        eng.next_step()
    f64 = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64)  # noqa: E731
    i32 = lambda *shape: torch.full(shape, -7, dtype=torch.int32)  # noqa: E731
    for e in (eng, vec):
        for k in (0, 65, -1):
            with pytest.raises(ValueError):
                e.get_lane_front_vehicles_array(k)
            with pytest.raises(ValueError):
                e.get_lane_front_vehicles_tensor(k)
        with pytest.raises(TypeError):
            e.get_lane_front_vehicles_tensor(4.0)
    with pytest.raises(ValueError):  # K = 0 / 65 as a tensor's last dimension
        eng.observe_lanes_tensor(front_distance=f64(L, 0))
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor(front_speed=f64(L, 65))
    with pytest.raises(ValueError):  # disagreeing K
        eng.observe_lanes_tensor(front_distance=f64(L, 8), front_speed=f64(L, 9))
    with pytest.raises(ValueError):
        eng.get_lane_front_vehicles_tensor(8, distance=f64(L, 9))
    with pytest.raises(ValueError):
        eng.get_lane_front_vehicles_tensor(8, speed=f64(L, 9))
    with pytest.raises(TypeError):  # dtype
        eng.observe_lanes_tensor(front_distance=torch.zeros((L, 8), dtype=torch.float32))
    with pytest.raises(TypeError):
        eng.observe_lanes_tensor(front_speed=i32(L, 8))
    with pytest.raises(TypeError):
        eng.observe_lanes_tensor(front_distance=np.zeros((L, 8)))
    with pytest.raises(ValueError):  # shape
        eng.observe_lanes_tensor(front_distance=f64(L + 1, 8))
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor(front_distance=f64(L))
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor(front_distance=torch.tensor(0.0, dtype=torch.float64))
    with pytest.raises(ValueError):
        vec.observe_lanes_tensor(front_distance=f64(L, 8))  # [R, L, K] wanted
    with pytest.raises(TypeError):  # device (the twin's tensors live on the CPU)
        eng.observe_lanes_tensor(front_distance=torch.zeros((L, 8), dtype=torch.float64, device="meta"))
    if torch.cuda.is_available():
        with pytest.raises(TypeError):
            eng.observe_lanes_tensor(front_distance=torch.zeros((L, 8), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):  # not contiguous
        eng.observe_lanes_tensor(front_distance=f64(L, 16)[:, ::2])
    with pytest.raises(ValueError):  # nothing given
        eng.observe_lanes_tensor()
    with pytest.raises(RuntimeError):  # tracker columns while tracking is off
        eng.observe_lanes_tensor(front_lane_steps=i32(L, 8))
    with pytest.raises(RuntimeError):
        vec.observe_lanes_tensor(front_waiting_steps=i32(2, L, 8))
    with pytest.raises(TypeError):  # (the dtype is checked before the tracker is asked)
        eng.observe_lanes_tensor(front_lane_steps=f64(L, 8))
    # a call that fails its checks enqueues nothing: the outputs given before the wrong one keep their marker
    good, counts = f64(L, 8), i32(L)
    with pytest.raises(ValueError):
        eng.observe_lanes_tensor(counts=counts, front_distance=good, front_speed=f64(L, 9))
    with pytest.raises(RuntimeError):
        eng.observe_lanes_tensor(counts=counts, front_distance=good, front_waiting_steps=i32(L, 8))
    assert bool((good == -7).all()) and bool((counts == -7).all())
    eng.observe_lanes_tensor(counts=counts, front_distance=good)
    assert not bool((good == -7).any()) and int(counts.sum()) > 0
    eng.track_lane_flow(True)
    steps = i32(L, 8)
    eng.observe_lanes_tensor(front_lane_steps=steps)
    assert not bool((steps == -7).any())
    assert sorted(eng.get_lane_front_vehicles_array(8)) == sorted(FRONT + TRACKER)


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    code = ("import sys, cityflow_amd; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert hasattr(cityflow_amd.Engine, 'get_lane_front_vehicles_tensor'); "
            "assert hasattr(cityflow_amd.VectorEngine, 'get_lane_front_vehicles_array')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_fronts_equal_the_dict_oracle(mod, scen, workdir, layout):
    eng = hip_engine(mod, layout_config(scen, workdir, "grid_6x6", layout), layout)
    run_against_dict_oracle(eng, 400, 25, layout, tracker=True, fused=True)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_fronts_without_tracking(mod, scen, workdir, layout):
    eng = hip_engine(mod, layout_config(scen, workdir, "grid_6x6", layout), layout)
    run_against_dict_oracle(eng, 400, 25, layout, tracker=False)


@pytest.mark.gpu
def test_hip_fronts_equal_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, tw = mod.Engine(cfg, 1), twin(mod, cfg)
    eng.track_lane_flow(True)
    tw.track_lane_flow(True)
    looked = Looked()
    for s in range(240):
        eng.next_step()
        tw.next_step()
        if s % 30 != 29:
            continue
        for k in KS:
            got, want = eng.get_lane_front_vehicles_array(k), tw.get_lane_front_vehicles_array(k)
            t = filled(eng, FRONT + TRACKER, k)
            eng.observe_lanes_tensor(**t)
            for name in FRONT + TRACKER:
                assert np.array_equal(got[name], want[name]), "step %d, K = %d: %s (array)" % (s, k, name)
                assert np.array_equal(t[name].cpu().numpy(), want[name]), "step %d, K = %d: %s (tensor)" % (s, k, name)
        w = tw.get_lane_front_vehicles_array(64)
        n = tw.get_lane_vehicle_count_array()
        looked.at([[list(zip(*(w[name][l, :n[l]] for name in FRONT + TRACKER))) for l in range(len(n))]])
    looked.enough(tracker=True)


@pytest.mark.gpu
def test_lane_change_dense(mod, scen, workdir):
    eng = mod.Engine(scen.materialize("grid_6x6", workdir, laneChange=True), 1)
    if eng._device_buffers():
        assert eng._layout() == "dense"
    lane_change_body(eng)


@pytest.mark.gpu
def test_vector_engine_equals_standalone(mod, scen, workdir):
    vec = mod.VectorEngine(scen.materialize("grid_6x6", workdir), 4)
    singles = [mod.Engine(scen.materialize("grid_6x6", workdir, seed=e), 1) for e in range(4)]
    vector_body(vec, singles, 400, 50)


@pytest.mark.gpu
def test_vector_engine_tracker_columns(mod, scen, workdir):
    vec = mod.VectorEngine(scen.materialize("grid_6x6", workdir), 4)
    singles = [mod.Engine(scen.materialize("grid_6x6", workdir, seed=e), 1) for e in range(4)]
    vector_tracker_body(vec, singles, 120, 30)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_tracker_columns_survive_compaction(mod, scen, workdir, layout):
    compaction_body(lambda cfg: hip_engine(mod, cfg, layout), lambda cfx: layout_config(scen, workdir, "grid_6x6", layout, **cfx))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_tracker_columns_across_baselines(mod, scen, workdir, layout):
    baselines_body(lambda cfg: hip_engine(mod, cfg, layout), layout_config(scen, workdir, "grid_6x6", layout))


@pytest.mark.gpu
def test_fronts_on_a_side_stream_without_a_host_wait(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, ref = mod.Engine(cfg, 1), mod.Engine(cfg, 1)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    for s in range(250):  # warm: rings built, tables uploaded, lanes longer than K
        eng.next_step()
        ref.next_step()
    eng.track_lane_flow(True)
    model = Model(ref.lane_ids())
    model.baseline(ref.get_lane_vehicles(), 250)
    k = 17
    t = filled(eng, FRONT + TRACKER, k)
    eng.observe_lanes_tensor(**t)
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
            eng.observe_lanes_tensor(**t)
            records.append({name: v.clone() for name, v in t.items()})  # consumed on `side`, then the outputs are reused
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the loop waited for the device (%.1f ms for 8 iterations behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    looked = Looked()
    for s in range(8):
        ref.next_step()
        model.tick(ref.get_lane_vehicles(), ref.get_vehicle_speed(), 251 + s)
        lanes = dict_lanes(ref, model, 251 + s)
        looked.at([lanes])
        want = want_fronts(lanes, k)
        for name in FRONT + TRACKER:
            assert np.array_equal(records[s][name].cpu().numpy(), want[name]), "step %d: %s" % (s, name)
    assert {"n > K", "0 < n < K", "n = 0"} <= looked.seen[k] and looked.waits > 0
    assert_same_state(eng, ref, "after the unsynchronised loop")
