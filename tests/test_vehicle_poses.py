"""The pose outputs of observe_vehicles_tensor / observe_vehicles_array(poses=True) and drivable_geometry() on Engine and
VectorEngine (cityflow_amd/torch_io.py; cfx_set_drivable_geometry, kr_vehicle_poses / kd_vehicle_poses): x, y, dir_x, dir_y from
the two walks of the replay writer over the drivable's polyline, length and width from the vehicle's template.

Three oracles, every comparison exact (array_equal, equal_nan for the float columns):
  * the unmodified reference engine's replay file — x, y, the angle as math.atan2(dir_y, dir_x), length, width — against the
    array form on the CPU twin;
  * a plain-numpy restatement of the two walks over drivable_geometry(), with the distance and drivable columns as input;
  * on the GPU, the array form (computed on the host from cfx_get_vehicles) against the tensors the kernels fill.

The step counts of the gpu tests were chosen on the twin, where the host form alone satisfies the Looked record (the dense
layout steps alike).  Where each condition first occurs among the compared states (every 7th step):
  irregular_11 (56 steps)             first segment of a lane, moving: step 7; a later segment of a bent lane: step 14; first
                                      segment of a laneLink, segment >= 5 of a laneLink: step 21; a drivable with >= 17
                                      vehicles: step 49
  star5 (56 steps)                    a laneLink's first segment and its segment >= 5: step 28; >= 17 vehicles: step 49
  example_1x1 (35 steps)              a laneLink's first segment and its segment >= 5: step 28
  irregular_11_long_roads (35 steps)  a polyline longer than the kernel's staging bound of 16 points: step 7 (its straight
                                      roads are redrawn with 19 points; the generated curves have 11, so no stock network
                                      reaches the walk in global memory)
  grid_2x2_mid15, _mid16 (28 steps)   a vehicle on a polyline of exactly the staging bound, and on one of one point more, the
                                      shortest that is walked in global memory: step 21 (2 x 2 grids whose laneLinks are drawn
                                      with 16 and 17 points)"""
import ctypes as C
import json
import math
import os
import time

import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB, assert_hip_backend, assert_same_state

torch = pytest.importorskip("torch")

import star_networks  # noqa: E402
from test_abi_bare import Corridor  # noqa: E402
from test_device_tensors import tensor_device, twin  # noqa: E402
from test_irregular import irregular  # noqa: E402
from test_lane_flow import layout_config  # noqa: E402
from test_replay import _parse_line  # noqa: E402
from test_vehicle_rows import DTYPES as ROW_DTYPES, FILL, PAD as ROW_PAD, ROWS, drivables, hip_network_engine  # noqa: E402

POSES = ("x", "y", "dir_x", "dir_y", "length", "width")
GEOMETRY = POSES[:4]
ALL = ROWS + POSES
DTYPES = dict(ROW_DTYPES, **{k: np.float64 for k in POSES})
PAD = dict(ROW_PAD, x=np.nan, y=np.nan, dir_x=0.0, dir_y=0.0, length=0.0, width=0.0)
TORCH_OF = {np.int32: torch.int32, np.float64: torch.float64}
STAGE_POINTS = 16  # kGeoStage of cfx_kernels.h: a longer polyline is walked in global memory


def same(got, want, where):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s against %s %s" % (where, got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want, equal_nan=got.dtype == np.float64), "%s differs" % where


def tensors(eng, n_rows, names):
    device = tensor_device(eng)
    lead = tuple(eng._tensor_shapes()[0])[:-1]
    _, D = drivables(eng)
    shapes = dict({k: (n_rows,) for k in ALL}, start=lead + (D + 1,), count=())
    return {k: torch.full(shapes[k], FILL, dtype=TORCH_OF[DTYPES[k]], device=device) for k in names}


def at_length(want, n_rows, names=ALL):
    keep = min(int(want["count"]), n_rows)
    return {k: np.concatenate([want[k][:keep], np.full(n_rows - keep, PAD[k], dtype=DTYPES[k])]) for k in names}


def check_tensors(eng, want, where, lengths):
    """Every given tensor element is written: all thirteen row outputs with start and count, then the six alone."""
    for n_rows in lengths:
        for names in (ALL + ("start", "count"), POSES):
            t = tensors(eng, n_rows, names)
            eng.observe_vehicles_tensor(**t)
            rows = at_length(want, n_rows)
            for k in names:
                same(t[k], rows[k] if k in rows else want[k], "%s, N = %d, %d outputs: %s" % (where, n_rows, len(names), k))


# ------------------------------------------------------------------------------------------------- the numpy oracle
def polylines(geometry):
    start, pts = geometry["point_start"], geometry["points"]
    return [pts[start[d]:start[d + 1]] for d in range(len(start) - 1)]


def segment_lengths(pts):
    d = pts[1:] - pts[:-1]
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def walk(pts, dis):
    """(x, y, dir_x, dir_y, segment of the direction) at `dis` along the polyline: getPointByDistance and
    Drivable::getDirectionByDistance of the reference, in numpy float64 scalars."""
    dis = np.float64(dis)
    seg = segment_lengths(pts)
    total = np.float64(0.0)
    for l in seg:
        total = total + l
    lo = dis if dis > 0 else np.float64(0.0)
    rest = lo if lo < total else total
    point = pts[-1]
    if rest <= 0.0:
        point = pts[0]
    else:
        for i in range(1, len(pts)):
            l = seg[i - 1]
            if rest > l:
                rest = rest - l
            else:
                point = pts[i - 1] + (pts[i] - pts[i - 1]) * (rest / l)
                break
    remain, at = dis, len(pts) - 2
    for i in range(len(pts) - 1):
        if remain < seg[i]:
            at = i
            break
        remain = remain - seg[i]
    d = pts[at + 1] - pts[at]
    l = np.sqrt(d[0] * d[0] + d[1] * d[1])
    return point[0], point[1], d[0] / l, d[1] / l, at


def numpy_poses(geometry, rows):
    lines = polylines(geometry)
    out = np.empty((int(rows["count"]), 5))
    with np.errstate(all="ignore"):
        for i, (d, dis) in enumerate(zip(rows["drivable"].tolist(), rows["distance"].tolist())):
            out[i] = walk(lines[d], dis)
    return dict(zip(GEOMETRY, out[:, :4].T.copy()), segment=out[:, 4].astype(np.int64))


class Looked:
    """What the compared states contained."""
    NEED = ("first segment of a lane", "later segment of a bent lane", "first segment of a laneLink", "segment >= 5 of a laneLink",
            "a drivable with >= 17 vehicles", "a polyline beyond the staging bound", "a polyline of exactly the staging bound",
            "one point beyond it", "moving")

    def __init__(self):
        self.seen, self.first = set(), {}

    def at(self, geometry, want, n_lanes, where):
        n_points = np.diff(geometry["point_start"])[want["drivable"]]
        lane, seg = want["drivable"] < n_lanes, numpy_poses(geometry, want)["segment"]
        hits = {"first segment of a lane": (lane & (seg == 0)).any(),
                "later segment of a bent lane": (lane & (n_points >= 3) & (seg >= 1)).any(),
                "first segment of a laneLink": (~lane & (seg == 0)).any(), "segment >= 5 of a laneLink": (~lane & (seg >= 5)).any(),
                "a drivable with >= 17 vehicles": (np.diff(want["start"].reshape(-1)) >= 17).any(),
                "a polyline beyond the staging bound": (n_points > STAGE_POINTS).any(),
                "a polyline of exactly the staging bound": (n_points == STAGE_POINTS).any(),
                "one point beyond it": (n_points == STAGE_POINTS + 1).any(), "moving": (want["speed"] > 0).any()}
        for k, hit in hits.items():
            if hit:
                self.seen.add(k)
                self.first.setdefault(k, where)

    def enough(self):
        assert set(self.NEED) <= self.seen, "the compared states never had: %s" % sorted(set(self.NEED) - self.seen)


# ------------------------------------------------------------------------------------------------- networks
def derived_config(cfg, tag, **changes):
    """The config at `cfg` with `changes`, written beside it (a "cfx" dict is merged)."""
    c = json.load(open(cfg))
    cfx = dict(c.get("cfx", {}), **changes.pop("cfx", {}))
    c.update(changes)
    if cfx:
        c["cfx"] = cfx
    path = os.path.join(os.path.dirname(cfg), "config_%s.json" % tag)
    with open(path, "w") as f:
        json.dump(c, f)
    return path


def long_roads(scen, workdir, points=19):
    """irregular(seed=11) with every straight road redrawn as a polyline of `points` points: both ends stay as long as the
    intersections need, the middle two fifths zigzag by three metres.  Its lanes have `points` points too."""
    base = irregular(scen, workdir, 11)
    net = json.load(open(os.path.join(os.path.dirname(base), "roadnet.json")))
    for r in net["roads"]:
        if len(r["points"]) != 2:
            continue
        (ax, ay), (bx, by) = [(p["x"], p["y"]) for p in r["points"]]
        length = math.hypot(bx - ax, by - ay)
        nx, ny = -(by - ay) / length, (bx - ax) / length
        inner = []
        for j in range(points - 2):
            t, side = 0.3 + 0.4 * j / (points - 3), 3.0 * (-1) ** j
            inner.append({"x": ax + (bx - ax) * t + nx * side, "y": ay + (by - ay) * t + ny * side})
        r["points"] = [r["points"][0]] + inner + [r["points"][1]]
    d = os.path.join(workdir, "irregular_11_long_roads")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "roadnet.json"), "w") as f:
        json.dump(net, f)
    with open(os.path.join(d, "flow.json"), "w") as f:
        json.dump(json.load(open(os.path.join(os.path.dirname(base), "flow.json"))), f)
    cfg = dict(json.load(open(base)), dir=d + "/")
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    return os.path.join(d, "config.json")


def curved_grid(scen, workdir, mid_points):
    """A 2 x 2 grid whose laneLinks are drawn with mid_points + 1 points (the stock generator's 10 give 11): 15 fills the
    kernel's stage exactly, 16 is the shortest polyline that is walked in global memory.  Its lanes have 2 points."""
    d = os.path.join(workdir, "grid_2x2_mid%d" % mid_points)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "roadnet.json"), "w") as f:
        json.dump(scen.grid_roadnet(2, 2, mid_points=mid_points), f)
    with open(os.path.join(d, "flow.json"), "w") as f:
        json.dump(scen.grid_flows(2, 2), f)
    cfg = {"interval": 1.0, "seed": 0, "dir": d + "/", "roadnetFile": "roadnet.json", "flowFile": "flow.json",
           "rlTrafficLight": False, "laneChange": False, "saveReplay": False}
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    return os.path.join(d, "config.json")


# (the two curved grids: vehicles stand on their 16- and 17-point laneLinks at step 21)
CURVED = {"grid_2x2_mid15": STAGE_POINTS, "grid_2x2_mid16": STAGE_POINTS + 1}  # name -> points of a laneLink
NETWORKS = (("irregular_11", 56), ("star5", 56), ("example_1x1", 35), ("irregular_11_long_roads", 35), ("grid_2x2_mid15", 28),
            ("grid_2x2_mid16", 28))


def network_config(scen, workdir, name, layout):
    if name.startswith("star"):
        return star_networks.make(workdir, name, layout="dense" if layout == "dense" else "auto")
    if name in CURVED:
        cfg = curved_grid(scen, workdir, CURVED[name] - 1)
        return derived_config(cfg, "dense", cfx={"layout": "dense"}) if layout == "dense" else cfg
    if name.startswith("irregular"):
        cfg = long_roads(scen, workdir) if name.endswith("long_roads") else irregular(scen, workdir, 11)
        return derived_config(cfg, "dense", cfx={"layout": "dense"}) if layout == "dense" else cfg
    return layout_config(scen, workdir, name, layout)


def engine_body(make, config, looked, every=7):
    for name, steps in NETWORKS:
        eng = make(config(name))
        n_lanes, _ = drivables(eng)
        geometry = eng.drivable_geometry()
        archive = None
        for s in range(1, steps + 1):
            eng.next_step()
            if s == steps // 2:
                archive = eng.snapshot()
            if s % every:
                continue
            where = "%s step %d" % (name, s)
            want = eng.observe_vehicles_array(poses=True)
            count = int(want["count"])
            assert count > 3, where
            looked.at(geometry, want, n_lanes, where)
            check_tensors(eng, want, where, (count + 7, count - 3, 0))
        eng.load(archive)
        want = eng.observe_vehicles_array(poses=True)
        assert int(want["count"]) > 0
        check_tensors(eng, want, name + " right after load", (int(want["count"]) + 7,))
        eng.reset()
        want = eng.observe_vehicles_array(poses=True)
        assert int(want["count"]) == 0
        check_tensors(eng, want, name + " right after reset", (7,))
        eng.next_step()
        eng.next_step()
        want = eng.observe_vehicles_array(poses=True)
        check_tensors(eng, want, name + " two steps after reset", (int(want["count"]) + 7,))


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
def replay_config(cfg, tag):
    c = json.load(open(cfg))
    path = derived_config(cfg, "poses_replay_%s" % tag, saveReplay=True, roadnetLogFile="roadnet_log_poses_%s.json" % tag,
                          replayLogFile="replay_poses_%s.txt" % tag)
    return path, c["dir"] + "replay_poses_%s.txt" % tag


@pytest.mark.parametrize("name,steps", [("example_1x1", 150), ("irregular_11", 120)])
def test_poses_equal_the_reference_replay(mod, scen, workdir, ref_module, name, steps):
    cfg = irregular(scen, workdir, 11) if name == "irregular_11" else scen.materialize(name, workdir)
    cfg_ref, log = replay_config(cfg, "ref")
    ref, tw = ref_module.Engine(cfg_ref, 1), twin(mod, cfg)
    taken = {}
    for s in range(1, steps + 1):
        ref.next_step()
        tw.next_step()
        if s % 7 == 0:
            rows = tw.observe_vehicles_array(poses=True)
            taken[s] = (rows, [tw._vehicle_id(int(v)) for v in rows["vehicle"]])
    time.sleep(0.2)  # reference destructor race
    del ref          # closes the log
    lines = open(log).read().splitlines()
    assert len(lines) == steps
    compared = turned = 0
    for s, (rows, ids) in taken.items():
        logged = {v[3]: v for v in _parse_line(lines[s - 1])[0]}
        assert sorted(logged) == sorted(ids), "step %d: the vehicles differ" % s
        for i, vid in enumerate(ids):
            x, y, angle, _, _, length, width = logged[vid]
            got = tuple(float(rows[k][i]) for k in POSES)
            assert got[:2] == (x, y), "step %d, %s: point %r against %r" % (s, vid, got[:2], (x, y))
            assert math.atan2(got[3], got[2]) == angle, "step %d, %s: direction %r against the angle %r" % (s, vid, got[2:4], angle)
            assert got[4:] == (length, width), "step %d, %s: length and width" % (s, vid)
            compared += 1
            turned += got[2] != 0.0 and got[3] != 0.0
    assert compared > 100 and turned > 10, (compared, turned)


@pytest.mark.parametrize("name", ["irregular_11", "irregular_11_long_roads", "star5", "example_1x1"] + sorted(CURVED))
def test_poses_equal_the_numpy_walks_over_the_geometry(mod, scen, workdir, name):
    eng = twin(mod, network_config(scen, workdir, name, "auto"))
    n_lanes, D = drivables(eng)
    geometry = eng.drivable_geometry()
    if name in CURVED:  # every laneLink has exactly that many points, every lane two
        n_points = np.diff(geometry["point_start"])
        assert (n_points[n_lanes:] == CURVED[name]).all() and (n_points[:n_lanes] == 2).all(), sorted(set(n_points.tolist()))
    assert sorted(geometry) == ["point_start", "points"]
    start, points = geometry["point_start"], geometry["points"]
    assert start.dtype == np.int32 and start.shape == (D + 1,) and points.dtype == np.float64 and points.shape == (int(start[-1]), 2)
    assert start[0] == 0 and (np.diff(start) >= 2).all()
    with np.errstate(all="ignore"):
        lengths = []
        for line in polylines(geometry)[:n_lanes]:
            total = np.float64(0.0)
            for l in segment_lengths(line):
                total = total + l
            lengths.append(total)
    same(np.array(lengths), eng.lane_lengths(), "the lanes' summed segment lengths")
    looked = Looked()
    for s in range(1, 71):
        eng.next_step()
        if s % 7:
            continue
        rows = eng.observe_vehicles_array(poses=True)
        assert sorted(rows) == sorted(DTYPES) and int(rows["count"]) > 0
        for k in POSES:
            assert rows[k].dtype == np.float64 and rows[k].shape == (int(rows["count"]),), k
        want = numpy_poses(geometry, rows)
        for k in GEOMETRY:
            same(rows[k], want[k], "%s step %d: %s" % (name, s, k))
        assert (rows["length"] > 0).all() and (rows["width"] > 0).all()
        looked.at(geometry, rows, n_lanes, "step %d" % s)
    assert {"first segment of a lane", "segment >= 5 of a laneLink", "moving"} <= looked.seen, looked.seen
    # (a curved grid's eight flows run in step, and none of their vehicles is met on the short first segment of its spline)
    assert "first segment of a laneLink" in looked.seen or name in CURVED, looked.seen
    if name.startswith("irregular"):
        assert "later segment of a bent lane" in looked.seen
    assert ("a polyline beyond the staging bound" in looked.seen) == (name.endswith("long_roads") or CURVED.get(name, 0) > STAGE_POINTS)
    assert ("a polyline of exactly the staging bound" in looked.seen) == (CURVED.get(name) == STAGE_POINTS)  # (a vehicle stood on one)
    assert ("one point beyond it" in looked.seen) == (CURVED.get(name) == STAGE_POINTS + 1)


def test_a_last_segment_of_length_zero_gives_nan():
    pts = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0]])
    with np.errstate(all="ignore"):
        assert walk(pts, 2.5)[:4] == (1.5, 2.0, 0.6, 0.8)
        assert all(math.isnan(v) for v in walk(pts, 5.0)[2:4]) and all(math.isnan(v) for v in walk(pts, 7.0)[2:4])


def test_engine_body_on_the_twin(mod, scen, workdir):
    looked = Looked()
    engine_body(lambda cfg: twin(mod, cfg), lambda name: network_config(scen, workdir, name, "auto"), looked)
    looked.enough()


def test_only_x_and_the_fallback_padding_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("example_1x1", workdir))
    for _ in range(40):
        eng.next_step()
    want = eng.observe_vehicles_array(poses=True)
    count = int(want["count"])
    assert count > 3
    t = tensors(eng, count + 2, ("x",))
    eng.observe_vehicles_tensor(**t)
    same(t["x"], at_length(want, count + 2, ("x",))["x"], "x alone")
    assert np.isnan(t["x"][count:].numpy()).all()
    assert sorted(eng.observe_vehicles_array()) == sorted(ROW_DTYPES)  # (without poses: the keys it always had)
    assert sorted(eng.observe_vehicles_array(poses=False)) == sorted(ROW_DTYPES)


def test_argument_errors_twin(mod, scen, workdir):
    eng = twin(mod, scen.materialize("example_1x1", workdir))
    eng.next_step()
    for k in POSES:
        good = tensors(eng, 6, (k,))[k]
        with pytest.raises(TypeError, match="torch.Tensor"):
            eng.observe_vehicles_tensor(**{k: good.numpy()})
        with pytest.raises(TypeError, match="must be torch"):
            eng.observe_vehicles_tensor(**{k: good.to(torch.float32)})
        with pytest.raises(ValueError, match="shape"):
            eng.observe_vehicles_tensor(**{k: torch.zeros((3, 2), dtype=torch.float64)})
        with pytest.raises(ValueError, match="shape"):  # one N for all row outputs
            eng.observe_vehicles_tensor(vehicle=torch.zeros(6, dtype=torch.int32), **{k: torch.zeros(7, dtype=torch.float64)})
        with pytest.raises(ValueError, match="contiguous"):
            eng.observe_vehicles_tensor(**{k: torch.zeros(12, dtype=torch.float64)[::2]})
        with pytest.raises(TypeError, match="live on"):
            eng.observe_vehicles_tensor(**{k: torch.zeros(6, dtype=torch.float64, device="cuda" if torch.cuda.is_available() else "meta")})
    t = tensors(eng, 6, ("x", "dir_y", "speed"))  # nothing was written by a rejected call
    with pytest.raises(TypeError):
        eng.observe_vehicles_tensor(width=torch.zeros(6, dtype=torch.float32), **t)
    with pytest.raises(ValueError):
        eng.observe_vehicles_tensor(length=torch.zeros(5, dtype=torch.float64), **t)
    assert all((v == FILL).all() for v in t.values())
    with pytest.raises(ValueError, match="at least one"):
        eng.observe_vehicles_tensor()


def test_lane_change_raises_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    for eng in (twin(mod, cfg), mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)):
        eng.next_step()
        t = tensors(eng, 4, ("x", "width"))
        with pytest.raises(RuntimeError, match="laneChange"):
            eng.observe_vehicles_tensor(**t)
        assert all((v == FILL).all() for v in t.values())
        with pytest.raises(RuntimeError, match="laneChange"):
            eng.observe_vehicles_array(poses=True)


def vector_body(vec, singles, steps, every, where, extra=None):
    """Each environment's run of rows equals the array form of the standalone engine with that seed.
    extra(vec, got, total, at), if given, is called with every compared state once it has been held against the singles."""
    R = len(singles)
    _, D = drivables(singles[0])
    geometry = vec.drivable_geometry()
    for k, a in singles[0].drivable_geometry().items():
        same(geometry[k], a, where + ": drivable_geometry " + k)
    for s in range(1, steps + 1):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % every:
            continue
        wants = [e.observe_vehicles_array(poses=True) for e in singles]
        total = sum(int(w["count"]) for w in wants)
        assert total > R
        names = ("drivable", "env", "distance", "speed") + POSES
        t = tensors(vec, total + 5, names + ("start", "count"))
        vec.observe_vehicles_tensor(**t)
        got = {k: v.cpu().numpy() for k, v in t.items()}
        at = "%s step %d" % (where, s)
        assert int(got["count"]) == total, at
        for k in names:
            same(got[k][total:], np.full(5, PAD[k], dtype=DTYPES[k]), at + ": padding of " + k)
        arr = vec.observe_vehicles_array(poses=True)
        for k in names:
            same(arr[k], got[k][:total], at + ": array form, " + k)
        for r, want in enumerate(wants):
            lo, hi = int(got["start"][r, 0]), int(got["start"][r, D])
            assert hi - lo == int(want["count"]), "%s: env %d's run of rows" % (at, r)
            same(got["env"][lo:hi], np.full(hi - lo, r, dtype=np.int32), "%s: env %d env" % (at, r))
            for k in ("drivable", "distance", "speed") + POSES:
                same(got[k][lo:hi], want[k], "%s: env %d %s" % (at, r, k))
        if extra is not None:
            extra(vec, got, total, at)


def test_vector_engine_twin(mod, scen, workdir):
    cfg = irregular(scen, workdir, 11)
    vec = mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB)
    vector_body(vec, [twin(mod, derived_config(cfg, "seed%d" % (11 + r), seed=11 + r)) for r in range(3)], 42, 21, "irregular_11 x3")


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_poses_equal_the_host_form(mod, scen, workdir, layout):
    looked = Looked()

    def make(cfg):
        eng = hip_network_engine(mod, cfg, layout)
        assert SHADOW_GPU or eng._vehicle_poses_device()
        return eng

    engine_body(make, lambda name: network_config(scen, workdir, name, layout), looked)
    looked.enough()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("name", ["irregular_11", "example_1x1"])
def test_vector_engine(mod, scen, workdir, name, layout):
    R = 3
    base = network_config(scen, workdir, name, layout)
    seed = json.load(open(base))["seed"]
    vec = mod.VectorEngine(base, R)
    assert SHADOW_GPU or (vec.backend_name() == "hip-gfx950" and vec._vehicle_poses_device())
    singles = [twin(mod, derived_config(base, "%s_seed%d" % (layout, seed + r), seed=seed + r)) for r in range(R)]
    vector_body(vec, singles, 63, 21, "%s x%d %s" % (name, R, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_observing_poses_leaves_the_state_alone(mod, scen, workdir, layout):
    cfg = network_config(scen, workdir, "irregular_11", layout)
    watched, free = hip_network_engine(mod, cfg, layout), hip_network_engine(mod, cfg, layout)
    t = tensors(watched, 2048, POSES + ("count",))
    for s in range(60):
        watched.next_step()
        free.next_step()
        watched.observe_vehicles_tensor(**t)
    assert 0 < int(t["count"]) <= 2048 and not np.isnan(t["x"][:int(t["count"])].cpu().numpy()).any()
    assert_same_state(watched, free, "60 steps, poses observed every step")


class CfxVehicleRows(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_rows", C.c_int32)] + [(n, C.c_void_p) for n in (
        "start", "count", "vehicle", "drivable", "env", "distance", "speed", "leader", "gap") + POSES]


class CfxDrivableGeometry(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_drivables", C.c_int32), ("n_points", C.c_int32), ("point_start", C.c_void_p),
                ("xy", C.c_void_p)]


@pytest.mark.gpu
def test_bare_abi_on_the_hip_library(mod):
    """cfx_set_drivable_geometry and the pose members of cfx_vehicle_rows with nothing but ctypes, on test_abi_bare's corridor:
    a pose pointer before any geometry is CFX_ERR_STATE, a table that is none CFX_ERR_INVALID, a caller whose struct_size ends
    before the pose members is served as ever, and the outputs equal the numpy walks — over polylines the roadnet loader
    would never make: a bent laneLink, and a lane whose polyline ends in a segment of length zero halfway along it, so that
    the direction beyond it is NaN."""
    if SHADOW_GPU:
        pytest.skip("the twin has no such entry point")
    e = Corridor(mod._default_backend_path())
    try:
        observe, set_geometry = e.dll.cfx_observe_vehicles_device, e.dll.cfx_set_drivable_geometry
        observe.argtypes = [C.c_void_p, C.POINTER(CfxVehicleRows), C.c_void_p]
        set_geometry.argtypes = [C.c_void_p, C.POINTER(CfxDrivableGeometry)]
        for s in range(4):
            e.step(spawn_priority=1000 + s if s in (0, 3) else None, time=float(s))
        n_rows = 8
        t = {k: torch.full((n_rows,), FILL, dtype=TORCH_OF[DTYPES[k]], device="cuda:0") for k in ("drivable", "distance") + POSES}
        count = torch.full((), FILL, dtype=torch.int32, device="cuda:0")
        rows = CfxVehicleRows(struct_size=C.sizeof(CfxVehicleRows), n_rows=n_rows, count=count.data_ptr(), **{k: v.data_ptr() for k, v in t.items()})
        assert observe(e.h, C.byref(rows), None) == -4 and b"cfx_set_drivable_geometry" in e.dll.cfx_last_error(e.h)  # CFX_ERR_STATE
        torch.cuda.synchronize()
        assert all((v == FILL).all() for v in t.values())
        older = CfxVehicleRows(struct_size=CfxVehicleRows.x.offset, n_rows=n_rows, count=count.data_ptr(), x=t["x"].data_ptr())
        e.ok(observe(e.h, C.byref(older), None))  # (the pose members lie behind its struct_size: not read)
        torch.cuda.synchronize()
        assert int(count) == 2 and (t["x"] == FILL).all()
        start = np.array([0, 2, 5, 8], dtype=np.int32)
        xy = np.array([[0, 0], [100, 0], [110, 10], [110, 60], [110, 60], [100, 0], [110, 0], [110, 10]], dtype=np.float64)
        table = lambda st, n_drv=3: CfxDrivableGeometry(  # noqa: E731
            struct_size=C.sizeof(CfxDrivableGeometry), n_drivables=n_drv, n_points=len(xy), point_start=st.ctypes.data, xy=xy.ctypes.data)
        for bad in (table(start, 2), table(np.array([0, 2, 3, 8], dtype=np.int32)), table(np.array([1, 2, 5, 8], dtype=np.int32)),
                    table(np.array([0, 2, 5, 7], dtype=np.int32)), table(np.array([0, 5, 2, 8], dtype=np.int32))):
            assert set_geometry(e.h, C.byref(bad)) == -1 and e.dll.cfx_last_error(e.h)  # CFX_ERR_INVALID
        assert observe(e.h, C.byref(rows), None) == -4
        e.ok(set_geometry(e.h, C.byref(table(start))))
        geometry = {"point_start": start, "points": xy}
        seen = set()
        for s in range(4, 40):
            e.step(spawn_priority=1000 + s if s == 6 else None, time=float(s))
            if s == 20:
                e.ok(e.dll.cfx_reset(e.h))  # (the geometry is the engine's as the network is: a reset leaves it alone)
                e.spawned, e.last_on_lane0 = 0, -1
                e.step(spawn_priority=2000, time=0.0)
            e.ok(observe(e.h, C.byref(rows), None))
            torch.cuda.synchronize()
            v = e.vehicles()
            n = len(v["vid"])
            assert int(count) == n
            got = {k: x.cpu().numpy() for k, x in t.items()}
            same(got["drivable"][:n], v["drivable"], "step %d: drivable" % s)
            same(got["distance"][:n], v["dis"], "step %d: distance" % s)
            want = numpy_poses(geometry, {"count": n, "drivable": v["drivable"], "distance": v["dis"]})
            for k in GEOMETRY:
                same(got[k], np.concatenate([want[k], np.full(n_rows - n, PAD[k])]), "step %d: %s" % (s, k))
            same(got["length"], np.concatenate([np.full(n, 5.0), np.zeros(n_rows - n)]), "step %d: length" % s)
            same(got["width"], np.concatenate([np.full(n, 2.0), np.zeros(n_rows - n)]), "step %d: width" % s)
            seen |= {(int(d), bool(np.isnan(u))) for d, u in zip(v["drivable"], want["dir_x"])}
        assert seen == {(0, False), (1, False), (1, True), (2, False)}, seen
    finally:
        e.close()
