"""observe_vehicles_tensor / observe_vehicles_array on Engine and VectorEngine (cityflow_amd/torch_io.py; cfx_observe_vehicles_device:
k_vehicle_tile_sums + kr_vehicle_rows / kd_vehicle_rows): every running vehicle as a row, rows grouped by drivable (CSR).

Oracles use only getters older than the call.  Engine: _vehicle_state() gives the rows (gap masked to 0.0 where there is no
leader, start from its drivable column), cross-checked against get_vehicle_speed() / get_vehicle_distance() through _vehicle_id.
VectorEngine: R standalone twins with seeds base + r, compared environment by environment; the vehicle numbers through one
bijection (env, standalone number) <-> vector number that must stay consistent over a whole run.  Everything is a copy or an
integer: all comparisons are array_equal.

The unmarked tests run on the CPU twin and pin the semantics; the step counts of the gpu tests were chosen there so that the
reference run alone satisfies the Looked record."""
import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB, assert_hip_backend

torch = pytest.importorskip("torch")

import star_networks  # noqa: E402
from cityflow_amd.torch_io import VEHICLE_ROW_TILE  # noqa: E402
from test_device_tensors import tensor_device, twin  # noqa: E402
from test_lane_flow import hip_engine, layout_config  # noqa: E402

ROWS = ("vehicle", "drivable", "env", "distance", "speed", "leader", "gap")
DTYPES = {"start": np.int32, "count": np.int32, "vehicle": np.int32, "drivable": np.int32, "env": np.int32, "distance": np.float64,
          "speed": np.float64, "leader": np.int32, "gap": np.float64}
PAD = {"vehicle": -1, "drivable": -1, "env": -1, "distance": -1.0, "speed": 0.0, "leader": -1, "gap": 0.0}
FILL = -7  # a value no output takes: every element must be written
TORCH_OF = {np.int32: torch.int32, np.float64: torch.float64}


def drivables(eng):
    lanes, links = eng._drivable_counts()
    return lanes, lanes + links


def state_rows(eng):
    """The oracle of one engine from _vehicle_state(): the array form's dict."""
    s = eng._vehicle_state()
    _, D = drivables(eng)
    assert (np.diff(s["drivable"]) >= 0).all()
    start = np.concatenate([[0], np.cumsum(np.bincount(s["drivable"], minlength=D))]).astype(np.int32)
    return {"start": start, "count": np.array(len(s["vid"]), dtype=np.int32), "vehicle": s["vid"].astype(np.int32),
            "drivable": s["drivable"].astype(np.int32), "env": np.zeros(len(s["vid"]), dtype=np.int32), "distance": s["dis"],
            "speed": s["speed"], "leader": s["leader"].astype(np.int32), "gap": np.where(s["leader"] >= 0, s["gap"], 0.0)}


def cross_check_ids(eng, want, where):
    speed, dis = eng.get_vehicle_speed(), eng.get_vehicle_distance()
    assert len(speed) == int(want["count"]), where
    for i, v in enumerate(want["vehicle"]):
        vid = eng._vehicle_id(int(v))
        assert speed[vid] == want["speed"][i] and dis[vid] == want["distance"][i], "%s: row %d (%s)" % (where, i, vid)


def at_length(want, n_rows):
    """The row outputs as a tensor of n_rows rows holds them: cut or padded."""
    keep = min(int(want["count"]), n_rows)
    return {k: np.concatenate([want[k][:keep], np.full(n_rows - keep, PAD[k], dtype=DTYPES[k])]) for k in ROWS}


def tensors(eng, n_rows, names=ROWS + ("start", "count")):
    device = tensor_device(eng)
    lead = tuple(eng._tensor_shapes()[0])[:-1]
    _, D = drivables(eng)
    shapes = dict({k: (n_rows,) for k in ROWS}, start=lead + (D + 1,), count=())
    return {k: torch.full(shapes[k], FILL, dtype=TORCH_OF[DTYPES[k]], device=device) for k in names}


def same(got, want, where):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (where, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), "%s differs" % where


def check_tensors(eng, want, where, lengths=None):
    count = int(want["count"])
    for n_rows in (count + 7,) if lengths is None else lengths:
        t = tensors(eng, n_rows)
        eng.observe_vehicles_tensor(**t)
        rows = at_length(want, n_rows)
        for k in ROWS:
            same(t[k], rows[k], "%s, N = %d: %s" % (where, n_rows, k))
        same(t["start"], want["start"], "%s, N = %d: start" % (where, n_rows))
        same(t["count"], want["count"], "%s, N = %d: count" % (where, n_rows))


def check_array(eng, want, where):
    got = eng.observe_vehicles_array()
    assert sorted(got) == sorted(want)
    for k in want:
        same(got[k], want[k], "%s: array form, %s" % (where, k))


class Looked:
    """What the compared states contained."""
    NEED = ("n = 0", "n = 1", "n = 15", "n = 16", "n = 17", "n > 32", "on a laneLink", "head with a leader elsewhere", "no leader", "moving")

    def __init__(self):
        self.seen = set()

    def at(self, want, n_lanes):
        start = want["start"].reshape(-1, want["start"].shape[-1])
        n = np.diff(start, axis=1)
        heads = start[:, :-1][n > 0]  # (the first row of every drivable that holds a vehicle)
        hits = {"n = 0": (n == 0).any(), "n = 1": (n == 1).any(), "n = 15": (n == 15).any(), "n = 16": (n == 16).any(),
                "n = 17": (n == 17).any(), "n > 32": (n > 32).any(), "on a laneLink": (want["drivable"] >= n_lanes).any(),
                "head with a leader elsewhere": (want["leader"][heads] >= 0).any(), "no leader": (want["leader"] < 0).any(),
                "moving": (want["speed"] > 0).any()}
        self.seen |= {k for k, hit in hits.items() if hit}

    def enough(self):
        assert set(self.NEED) <= self.seen, "the compared states never had: %s" % sorted(set(self.NEED) - self.seen)


# (network, steps): on the twin the three runs together satisfy Looked — star5 alone from step 105 on, grid_6x6 has n > 32 from
# step 112 on, example_1x1 has n = 15, 16, 17 by step 252
NETWORKS = (("example_1x1", 259), ("grid_6x6", 119), ("star5", 112))


def network_config(scen, workdir, name, layout, **cfx):
    if name.startswith("star"):
        assert not cfx
        return star_networks.make(workdir, name, layout="dense" if layout == "dense" else "auto")
    return layout_config(scen, workdir, name, layout, **cfx)


def engine_body(make, config, looked, every=7):
    for name, steps in NETWORKS:
        eng = make(config(name))
        n_lanes, _ = drivables(eng)
        archive = None
        for s in range(1, steps + 1):
            eng.next_step()
            if s == steps // 2:
                archive = eng.snapshot()
            if s % every:
                continue
            where = "%s step %d" % (name, s)
            want = state_rows(eng)
            looked.at(want, n_lanes)
            check_tensors(eng, want, where)
            if s % (5 * every) == 0:
                check_array(eng, want, where)
                cross_check_ids(eng, want, where)
        eng.load(archive)  # (nothing stepped since: every vehicle reports the state's gap)
        want = state_rows(eng)
        assert (want["leader"] >= 0).any()
        check_tensors(eng, want, name + " right after load")
        check_array(eng, want, name + " right after load")
        eng.next_step()
        check_tensors(eng, state_rows(eng), name + " a step after load")


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
def test_rows_equal_the_state_oracle_twin(mod, scen, workdir):
    looked = Looked()
    engine_body(lambda cfg: twin(mod, cfg), lambda name: network_config(scen, workdir, name, "auto"), looked)
    looked.enough()


def truncation_body(eng, steps=60):
    for _ in range(steps):
        eng.next_step()
    want = state_rows(eng)
    count = int(want["count"])
    assert count > 8
    check_tensors(eng, want, "truncation", lengths=(0, 1, count - 1, count, count + 7))
    for names in (("start",), ("count",), ("start", "count")):
        t = tensors(eng, 0, names)
        eng.observe_vehicles_tensor(**t)
        for k in names:
            same(t[k], want[k], "%s alone: %s" % (names, k))
    return want


def test_truncation_and_start_count_alone_twin(mod, scen, workdir):
    truncation_body(twin(mod, scen.materialize("grid_6x6", workdir)))


def one_at_a_time_body(eng, steps=60):
    for _ in range(steps):
        eng.next_step()
    want = state_rows(eng)
    n_rows = int(want["count"]) + 3
    rows = at_length(want, n_rows)
    for k in ROWS:  # (leader without gap and gap without leader among them; distance alone: no leader is looked for)
        t = tensors(eng, n_rows, (k,))
        eng.observe_vehicles_tensor(**t)
        same(t[k], rows[k], "%s alone" % k)
    t = tensors(eng, n_rows, ("leader", "count"))
    eng.observe_vehicles_tensor(**t)
    same(t["leader"], rows["leader"], "leader and count")
    same(t["count"], want["count"], "leader and count")


def test_one_output_at_a_time_twin(mod, scen, workdir):
    one_at_a_time_body(twin(mod, scen.materialize("grid_6x6", workdir)))


def vector_body(vec, singles, steps, every, where, looked=None, extra=None):
    """The batched engine against standalone engines, environment by environment; returns the last compared rows.
    extra(vec, got, total, at), if given, is called with every compared state once it has been held against the singles."""
    R = len(singles)
    n_lanes, D = drivables(singles[0])
    assert vec._drivable_counts() == singles[0]._drivable_counts()
    to_vec, to_single = {}, {}  # (env, standalone number) <-> vector number, over the whole run
    got = None
    for s in range(1, steps + 1):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % every:
            continue
        wants = [state_rows(e) for e in singles]
        total = sum(int(w["count"]) for w in wants)
        t = tensors(vec, total + 5)
        vec.observe_vehicles_tensor(**t)
        got = {k: v.cpu().numpy() for k, v in t.items()}
        at = "%s step %d" % (where, s)
        assert got["start"].shape == (R, D + 1) and int(got["count"]) == total, at
        live = got["vehicle"][:total]
        assert len(np.unique(live)) == total and (live >= 0).all(), at + ": vehicle numbers are not unique"
        for k in ROWS:
            same(got[k][total:], np.full(5, PAD[k], dtype=DTYPES[k]), at + ": padding of " + k)
        arr = vec.observe_vehicles_array()
        for k in ROWS:
            same(arr[k], got[k][:total], at + ": array form, " + k)
        same(arr["start"], got["start"], at + ": array form, start")
        same(arr["count"], got["count"], at + ": array form, count")
        for r, want in enumerate(wants):
            lo, hi = int(got["start"][r, 0]), int(got["start"][r, D])
            assert lo == (0 if r == 0 else int(got["start"][r - 1, D])) and hi - lo == int(want["count"]), "%s: env %d's run of rows" % (at, r)
            same(got["start"][r] - lo, want["start"], "%s: env %d start" % (at, r))
            same(got["env"][lo:hi], np.full(hi - lo, r, dtype=np.int32), "%s: env %d env" % (at, r))
            for k in ("drivable", "distance", "speed", "gap"):
                same(got[k][lo:hi], want[k], "%s: env %d %s" % (at, r, k))
            for mine, theirs in zip(want["vehicle"].tolist(), got["vehicle"][lo:hi].tolist()):
                assert to_vec.setdefault((r, mine), theirs) == theirs and to_single.setdefault(theirs, (r, mine)) == (r, mine), \
                    "%s: env %d vehicle %d is %d now" % (at, r, mine, theirs)
            mapped = np.array([to_vec[r, v] if v >= 0 else -1 for v in want["leader"].tolist()], dtype=np.int32)
            same(got["leader"][lo:hi], mapped, "%s: env %d leader" % (at, r))
        if looked is not None:
            looked.at(dict(got, drivable=got["drivable"][:total], leader=got["leader"][:total], speed=got["speed"][:total]), n_lanes)
        if extra is not None:
            extra(vec, got, total, at)
    return got


def test_vector_engine_is_environment_major_twin(mod, scen, workdir):
    R = 3
    vec = mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), R, 1, TWIN_LIB)
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=r)) for r in range(R)]
    got = vector_body(vec, singles, 84, 21, "grid_6x6 x3")
    total = int(got["count"])
    n_lanes, D = drivables(singles[0])
    key = got["env"][:total].astype(np.int64) * D + got["drivable"][:total]
    assert (np.diff(key) >= 0).all() and (got["drivable"][:total] >= n_lanes).any() and set(got["env"][:total].tolist()) == set(range(R))


def test_array_form_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("grid_6x6", workdir))
    for _ in range(40):
        eng.next_step()
    got = eng.observe_vehicles_array()
    assert sorted(got) == sorted(DTYPES)
    _, D = drivables(eng)
    assert got["start"].shape == (D + 1,) and got["count"].shape == () and int(got["count"]) == eng.get_vehicle_count() > 0
    for k, a in got.items():
        assert a.dtype == DTYPES[k], k
        if k in ROWS:
            assert a.shape == (int(got["count"]),), k
    check_array(eng, state_rows(eng), "step 40")
    vec = mod.VectorEngine._with_backend(scen.materialize("example_1x1", workdir), 2, 1, TWIN_LIB)
    got = vec.observe_vehicles_array()  # before the first step: no vehicle
    assert got["start"].shape == (2, drivables(vec)[1] + 1) and not got["start"].any() and int(got["count"]) == 0
    assert all(got[k].shape == (0,) and got[k].dtype == DTYPES[k] for k in ROWS)


def test_argument_errors_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("example_1x1", workdir))
    eng.next_step()
    _, D = drivables(eng)
    with pytest.raises(ValueError, match="at least one"):
        eng.observe_vehicles_tensor()
    for k in ROWS + ("start", "count"):
        good = tensors(eng, 6, (k,))[k]
        with pytest.raises(TypeError, match="torch.Tensor"):
            eng.observe_vehicles_tensor(**{k: good.numpy()})
        with pytest.raises(TypeError, match="must be torch"):
            eng.observe_vehicles_tensor(**{k: good.to(torch.float32 if DTYPES[k] == np.float64 else torch.int64)})
    with pytest.raises(ValueError, match="shape"):
        eng.observe_vehicles_tensor(start=torch.zeros(D, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        eng.observe_vehicles_tensor(count=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):
        eng.observe_vehicles_tensor(vehicle=torch.zeros((3, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="shape"):  # one N for all row outputs
        eng.observe_vehicles_tensor(vehicle=torch.zeros(6, dtype=torch.int32), speed=torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        eng.observe_vehicles_tensor(speed=torch.zeros(12, dtype=torch.float64)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        eng.observe_vehicles_tensor(start=torch.zeros(2 * (D + 1), dtype=torch.int32)[::2])
    if torch.cuda.is_available():  # (a tensor on another device than the engine's)
        with pytest.raises(TypeError, match="live on"):
            eng.observe_vehicles_tensor(vehicle=torch.zeros(6, dtype=torch.int32, device="cuda"))
    else:
        with pytest.raises(TypeError, match="live on"):
            eng.observe_vehicles_tensor(vehicle=torch.zeros(6, dtype=torch.int32, device="meta"))
    # nothing was written by a rejected call
    t = tensors(eng, 6, ("vehicle", "speed"))
    with pytest.raises(TypeError):
        eng.observe_vehicles_tensor(vehicle=t["vehicle"], speed=t["speed"], gap=torch.zeros(6, dtype=torch.float32))
    assert (t["vehicle"] == FILL).all() and (t["speed"] == FILL).all()
    vec = mod.VectorEngine._with_backend(scen.materialize("example_1x1", workdir), 2, 1, TWIN_LIB)
    with pytest.raises(ValueError, match="shape"):
        vec.observe_vehicles_tensor(start=torch.zeros(2 * (D + 1), dtype=torch.int32))
    assert not hasattr(mod.TiledEngine, "observe_vehicles_tensor")


def lane_change_body(eng):
    eng.next_step()
    with pytest.raises(RuntimeError, match="laneChange"):
        eng.observe_vehicles_tensor(**tensors(eng, 4, ("vehicle", "count")))
    with pytest.raises(RuntimeError, match="laneChange"):
        eng.observe_vehicles_array()


def test_lane_change_raises_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    lane_change_body(twin(mod, cfg))
    lane_change_body(mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB))


def stability_body(make, materialize, ring_growth):
    """Rows equal the oracle immediately after reset(), load(snapshot()), rollback(checkpoint) and a vehicle compaction (and, on
    the ring layout, ring growth)."""
    eng = make(materialize(compactVehicles=40))
    for _ in range(50):
        eng.next_step()
    archive = eng.snapshot()
    ck = eng.checkpoint() if eng._checkpoint_calls() and not eng._checkpoint_unsupported() else None
    check_tensors(eng, state_rows(eng), "step 50")
    compactions = set()
    for s in range(51, 141):
        before = eng._vehicle_table()[1]
        eng.next_step()
        if eng._vehicle_table()[1] != before:  # the numbers were reassigned by this step
            compactions.add(eng._vehicle_table()[1])
            want = state_rows(eng)
            check_tensors(eng, want, "right after compaction %d (step %d)" % (eng._vehicle_table()[1], s))
            cross_check_ids(eng, want, "right after a compaction")
    assert len(compactions) >= 2, compactions
    eng.load(archive)
    check_tensors(eng, state_rows(eng), "right after load")
    eng.next_step()
    check_tensors(eng, state_rows(eng), "a step after load")
    if ck is not None:
        eng.rollback(ck)
        want = state_rows(eng)
        assert int(want["count"]) > 0
        check_tensors(eng, want, "right after rollback")
        eng.next_step()
        check_tensors(eng, state_rows(eng), "a step after rollback")
    eng.reset()
    want = state_rows(eng)
    assert int(want["count"]) == 0
    check_tensors(eng, want, "right after reset")
    for _ in range(20):
        eng.next_step()
    check_tensors(eng, state_rows(eng), "20 steps after reset")
    if ring_growth:
        small = make(materialize(ringCapacityPercent=30))
        scale = small._ring_info()[1] if small._device_buffers() else None
        for s in range(1, 201):
            small.next_step()
            if s % 20 == 0:
                check_tensors(small, state_rows(small), "small rings, step %d" % s)
        if scale is not None:
            assert small._ring_info()[1] > scale, "the rings never grew"


def test_stability_twin(mod, scen, workdir):
    stability_body(lambda cfg: twin(mod, cfg), lambda **cfx: scen.materialize("grid_6x6", workdir, cfx=cfx), ring_growth=False)


# ---------------------------------------------------------------------------------------------------------------- GPU
def hip_network_engine(mod, cfg, layout):
    eng = mod.Engine(cfg, 1)
    assert_hip_backend(eng)
    if eng._device_buffers():
        assert eng._layout() == ("dense" if layout == "dense" else "ring") and eng._vehicle_rows_device()
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_rows_equal_the_state_oracle(mod, scen, workdir, layout):
    looked = Looked()
    engine_body(lambda cfg: hip_network_engine(mod, cfg, layout), lambda name: network_config(scen, workdir, name, layout), looked)
    looked.enough()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_one_scan_tile(mod, scen, workdir, layout):
    eng = hip_engine(mod, layout_config(scen, workdir, "example_1x1", layout), layout)
    assert drivables(eng)[1] < VEHICLE_ROW_TILE
    truncation_body(eng, steps=40)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_vector_engine_across_scan_tiles(mod, scen, workdir, layout):
    R = 3
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    vec = mod.VectorEngine(cfg, R)
    assert SHADOW_GPU or vec.backend_name() == "hip-gfx950"
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=r)) for r in range(R)]
    positions = R * drivables(singles[0])[1]
    assert positions > 2 * VEHICLE_ROW_TILE and positions % VEHICLE_ROW_TILE != 0, positions
    looked = Looked()
    vector_body(vec, singles, 126, 21, "grid_6x6 x%d %s" % (R, layout), looked)
    assert {"n = 0", "n = 1", "n > 32", "on a laneLink", "head with a leader elsewhere", "no leader", "moving"} <= looked.seen, looked.seen


@pytest.mark.gpu
def test_vector_engine_environments_inside_a_tile(mod, scen, workdir):
    R = 3
    vec = mod.VectorEngine(scen.materialize("example_1x1", workdir), R)
    singles = [twin(mod, scen.materialize("example_1x1", workdir, seed=r)) for r in range(R)]
    assert drivables(singles[0])[1] < VEHICLE_ROW_TILE < R * drivables(singles[0])[1]  # (an environment begins inside a tile)
    vector_body(vec, singles, 60, 12, "example_1x1 x%d" % R)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_truncation_on_the_device(mod, scen, workdir, layout):
    eng = hip_engine(mod, layout_config(scen, workdir, "grid_6x6", layout), layout)
    for _ in range(60):
        eng.next_step()
    want = state_rows(eng)
    count, (_, D) = int(want["count"]), drivables(eng)
    device = tensor_device(eng)
    guard = 5  # (odd: the float64 views start at an address that is a multiple of 8 and of nothing more)
    for n_rows in (count - 1, count + 7):
        rows = at_length(want, n_rows)
        ints = ("start", "count", "vehicle", "drivable", "env", "leader")
        sizes = {k: (D + 1 if k == "start" else 1 if k == "count" else n_rows) for k in ints + ("distance", "speed", "gap")}
        views, buffers = {}, []
        for dtype, names in ((torch.int32, ints), (torch.float64, ("distance", "speed", "gap"))):
            buf = torch.full((sum(sizes[k] + guard for k in names) + guard,), FILL, dtype=dtype, device=device)
            off, taken = guard, torch.zeros(buf.shape, dtype=torch.bool, device=device)
            for k in names:
                views[k] = buf[off:off + sizes[k]].reshape(()) if k == "count" else buf[off:off + sizes[k]]
                taken[off:off + sizes[k]] = True
                off += sizes[k] + guard
            buffers.append((buf, taken))
        eng.observe_vehicles_tensor(**views)
        for k in ROWS:
            same(views[k], rows[k], "N = %d: %s" % (n_rows, k))
        same(views["start"], want["start"], "N = %d: start" % n_rows)
        same(views["count"], want["count"], "N = %d: count" % n_rows)
        for buf, taken in buffers:
            assert (buf[~taken] == FILL).all(), "N = %d: a guard element of the %s buffer was written" % (n_rows, buf.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_one_output_at_a_time(mod, scen, workdir, layout):
    one_at_a_time_body(hip_engine(mod, layout_config(scen, workdir, "grid_6x6", layout), layout))


@pytest.mark.gpu
def test_rows_on_a_side_stream_without_a_host_wait(mod, scen, workdir):
    import time
    cfg = scen.materialize("grid_6x6", workdir)
    eng, ref = mod.Engine(cfg, 1), twin(mod, cfg)
    if not eng._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    for _ in range(60):
        eng.next_step()
        ref.next_step()
    n_rows = eng.get_vehicle_count() + 256  # (head room for the eight steps below: some ten vehicles enter per step)
    t = tensors(eng, n_rows)
    eng.observe_vehicles_tensor(**t)  # warm: rings built, scratch allocated
    eng.sync()
    device = tensor_device(eng)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device=device)
    records = []
    eng._device_spin(200000)  # 200 ms of device work in front of everything below
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for _ in range(8):
            eng.next_step()
            eng.observe_vehicles_tensor(**t)
            records.append({k: v.clone() for k, v in t.items()})  # consumed on `side`, then the outputs are reused
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the loop waited for the device (%.1f ms for 8 iterations behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    for s in range(8):
        ref.next_step()
        want = state_rows(ref)
        assert int(want["count"]) <= n_rows
        rows = at_length(want, n_rows)
        for k in ROWS:
            same(records[s][k], rows[k], "step %d: %s" % (s, k))
        same(records[s]["start"], want["start"], "step %d: start" % s)
        same(records[s]["count"], want["count"], "step %d: count" % s)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_stability(mod, scen, workdir, layout):
    stability_body(lambda cfg: hip_engine(mod, cfg, layout), lambda **cfx: layout_config(scen, workdir, "grid_6x6", layout, **cfx),
                   ring_growth=layout == "auto")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_hip_equals_twin(mod, scen, workdir, layout):
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    eng, tw = hip_engine(mod, cfg, layout), twin(mod, cfg)
    for s in range(1, 301):
        eng.next_step()
        tw.next_step()
        if s % 25:
            continue
        got, want = eng.observe_vehicles_array(), tw.observe_vehicles_array()
        for k in want:
            same(got[k], want[k], "step %d: %s" % (s, k))
