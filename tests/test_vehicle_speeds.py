"""set_vehicle_speeds_tensor / set_vehicle_speeds on Engine and VectorEngine (cityflow_amd/torch_io.py; cfx_set_vehicle_speeds_device:
k_speeds_claim + k_speeds_apply, and k_speeds_flag_dense on the dense layout): set_vehicle_speed() for many vehicles at once, by the
vehicle numbers of observe_vehicles_tensor.

The oracle is the per-vehicle call.  Two engines are built from one config and seed: A takes the batched call, B takes
set_vehicle_speed(_vehicle_id(v), s) for the rows that should take effect, in row order.  After every step _vehicle_state() of A
and B must be equal in every column (`gap` where the vehicle has a leader: without one the column holds no state, and
conftest.assert_same_state leaves it out for the same reason), at the end get_vehicle_speed() and get_vehicle_distance() too.
Nothing is approximate: all comparisons are array_equal.  The unmarked tests run A on the CPU twin and pin the semantics; in the
gpu tests A is the HIP engine and B the twin, which is also the HIP-equals-twin pin.

The step counts of CONTROL_RUNS were chosen on the twin so that the reference run alone satisfies the Looked record: on the twin
grid_6x6 alone has all five by its 10th call (step 30) and star5 alone by its 19th (step 57); example_1x1 has four by its 11th
(step 33) and never commands a vehicle in an entry buffer."""
import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB

torch = pytest.importorskip("torch")

from test_device_tensors import tensor_device, twin  # noqa: E402
from test_lane_flow import hip_engine, layout_config  # noqa: E402
from test_vehicle_rows import hip_network_engine, network_config  # noqa: E402

NAN = float("nan")
LENGTHS = (0, 1, 63, 64, 65, 257, None)  # rows of a call, in turn (None: count + 7): the edges of a wavefront and of a block
CONTROL_RUNS = (("example_1x1", 90), ("star5", 63), ("grid_6x6", 63))


# ----------------------------------------------------------------------------------------------------------------- helpers
def dev(eng, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tensor_device(eng))


def same_state(a, b, where, skip=()):
    sa, sb = a._vehicle_state(), b._vehicle_state()
    assert sorted(sa) == sorted(sb), where
    has = sa["leader"] >= 0
    for k in sorted(set(sa) - set(skip)):
        x, y = sa[k], sb[k]
        assert x.shape == y.shape, "%s: %s holds %s rows against %s" % (where, k, x.shape, y.shape)
        if k == "gap":
            x, y = x[has], y[has]
        assert np.array_equal(x, y), "%s: %s differs" % (where, k)


def same_dicts(a, b, where):
    assert a.get_vehicle_speed() == b.get_vehicle_speed(), where + ": get_vehicle_speed()"
    assert a.get_vehicle_distance() == b.get_vehicle_distance(), where + ": get_vehicle_distance()"


def issued(eng):
    return int(eng._scalars()["spawned_vehicle_count"])


def command(a, b, vehicle, speed, effective, want_ignored=0, form="tensor", where=""):
    """The batched call on A, the per-vehicle calls for the rows `effective` [(number, speed)] on B."""
    vehicle, speed = np.asarray(vehicle, dtype=np.int32), np.asarray(speed, dtype=np.float64)
    if form == "tensor":
        ignored = torch.full((), -7, dtype=torch.int32, device=tensor_device(a))
        a.set_vehicle_speeds_tensor(dev(a, vehicle), dev(a, speed), ignored)
        got = int(ignored.item())
    else:
        got = a.set_vehicle_speeds(vehicle, speed)
    assert got == want_ignored, "%s: %d rows ignored, not %d" % (where, got, want_ignored)
    for v, s in effective:
        b.set_vehicle_speed(b._vehicle_id(int(v)), float(s))


def random_rows(rng, live, length, share=0.6):
    """`length` rows: a random subset of `live` (no vehicle twice) with speeds from [0, 12) at random rows, the other rows half
    padding (-1, any speed) and half masked (a live number, NaN).  -> vehicle, speed, the rows in force [(number, speed)]"""
    vehicle = np.full(length, -1, dtype=np.int32)
    speed = rng.uniform(0.0, 12.0, length)
    k = min(len(live), int(np.ceil(share * length)))
    if k == 0:
        return vehicle, speed, []
    chosen = rng.choice(np.asarray(live), k, replace=False)
    at = np.sort(rng.choice(length, k, replace=False))
    vehicle[at] = chosen
    rest = np.setdiff1d(np.arange(length), at)
    masked = rest[rng.random(len(rest)) < 0.5]
    vehicle[masked] = rng.choice(np.asarray(live), len(masked))
    speed[masked] = NAN
    return vehicle, speed, [(int(vehicle[i]), float(speed[i])) for i in at]


def after_one_step(mod, cfg, archive, commands):
    """{id: distance} one step after `archive`, on a fresh twin that took `commands` [(number, speed)] first."""
    eng = twin(mod, cfg)
    eng.load(archive)
    ids = {}
    for v, s in commands:
        ids[int(v)] = eng._vehicle_id(int(v))
        eng.set_vehicle_speed(ids[int(v)], float(s))
    eng.next_step()
    return eng.get_vehicle_distance(), ids


class Looked:
    """What the compared runs commanded (read on B, the reference run)."""
    NEED = ("on a laneLink", "in an entry buffer", "lane head without a leader", "follower held below its command",
            "changed the next position")

    def __init__(self):
        self.seen = set()
        self.pending = None

    def before(self, mod, cfg, b, effective):
        rows, waiting = b.observe_vehicles_array(), set(b._waiting()[0].tolist())
        n_lanes = b._drivable_counts()[0]
        row_of = {int(v): i for i, v in enumerate(rows["vehicle"])}
        followers = []
        for v, s in effective:
            if v in waiting:
                self.seen.add("in an entry buffer")
                continue
            i = row_of[v]
            d = int(rows["drivable"][i])
            if d >= n_lanes:
                self.seen.add("on a laneLink")
            if rows["leader"][i] < 0 and d < n_lanes and i == int(rows["start"][d]):
                self.seen.add("lane head without a leader")
            if rows["leader"][i] >= 0:
                followers.append((v, s))
        self.pending = followers
        if "changed the next position" not in self.seen and effective:
            archive = b.snapshot()
            running = [(v, s) for v, s in effective if v in row_of]
            free, _ = after_one_step(mod, cfg, archive, [])
            held, ids = after_one_step(mod, cfg, archive, running)
            if any(ids[v] in free and ids[v] in held and free[ids[v]] != held[ids[v]] for v, _ in running):
                self.seen.add("changed the next position")

    def after(self, b):
        rows = b.observe_vehicles_array()
        speed_of = dict(zip(rows["vehicle"].tolist(), rows["speed"].tolist()))
        if any(v in speed_of and speed_of[v] < s for v, s in self.pending or ()):  # (min(custom, car following) took the latter)
            self.seen.add("follower held below its command")
        self.pending = None

    def enough(self):
        assert set(self.NEED) <= self.seen, "the compared runs never commanded: %s" % sorted(set(self.NEED) - self.seen)


def live_numbers(b):
    return np.concatenate([b.observe_vehicles_array()["vehicle"], b._waiting()[0].astype(np.int32)])


# ------------------------------------------------------------------------------------------------------- 1. random control
def control_body(mod, make_a, config, looked, runs=CONTROL_RUNS, form="tensor", seed=5):
    rng = np.random.default_rng(seed)
    for name, steps in runs:
        cfg = config(name)
        a, b = make_a(cfg), twin(mod, cfg)
        calls = 0
        for s in range(1, steps + 1):
            where = "%s step %d" % (name, s)
            commanded = s % 3 == 0
            if commanded:
                live = live_numbers(b)
                length = LENGTHS[calls % len(LENGTHS)]
                length = int(b.observe_vehicles_array()["count"]) + 7 if length is None else length
                calls += 1
                vehicle, speed, effective = random_rows(rng, live, length)
                if looked is not None:
                    looked.before(mod, cfg, b, effective)
                command(a, b, vehicle, speed, effective, 0, form, where)
            a.next_step()
            b.next_step()
            same_state(a, b, where)
            if commanded and looked is not None:
                looked.after(b)
        assert calls >= len(LENGTHS), name
        same_dicts(a, b, name)


def test_random_control_twin(mod, scen, workdir):
    looked = Looked()
    control_body(mod, lambda cfg: twin(mod, cfg), lambda name: network_config(scen, workdir, name, "auto"), looked)
    looked.enough()


def test_random_control_array_form_twin(mod, scen, workdir):
    control_body(mod, lambda cfg: twin(mod, cfg), lambda name: network_config(scen, workdir, name, "auto"), None,
                 runs=(("grid_6x6", 45),), form="array")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_random_control(mod, scen, workdir, layout):
    looked = Looked()
    control_body(mod, lambda cfg: hip_network_engine(mod, cfg, layout), lambda name: network_config(scen, workdir, name, layout), looked)
    looked.enough()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_random_control_array_form(mod, scen, workdir, layout):
    control_body(mod, lambda cfg: hip_network_engine(mod, cfg, layout), lambda name: network_config(scen, workdir, name, layout), None,
                 runs=(("grid_6x6", 45),), form="array")


# ------------------------------------------------------------------------------------------------------------ 2. duplicates
def pick_discriminating(mod, cfg, b, speeds):
    """A running vehicle of B whose next position is another one under each of `speeds` (looked for on fresh twins)."""
    rows, archive = b.observe_vehicles_array(), b.snapshot()
    order = np.argsort(np.abs(rows["speed"] - 4.0), kind="stable")  # (slow enough to reach every one of them in one step)
    for i in order[:40].tolist():
        v = int(rows["vehicle"][i])
        ends = set()
        for s in speeds:
            dist, ids = after_one_step(mod, cfg, archive, [(v, s)])
            ends.add(dist.get(ids[v]))
        if len(ends) == len(speeds) and None not in ends:
            return v
    raise AssertionError("no running vehicle tells the speeds %s apart" % (speeds,))


def duplicates_body(mod, make_a, cfg):
    a, b = make_a(cfg), twin(mod, cfg)
    for _ in range(40):
        a.next_step()
        b.next_step()
    speeds = (0.5, 1.0, 1.5)

    def rows_of(v, last):
        vehicle = np.full(301, -1, dtype=np.int32)
        speed = np.full(301, 9.0)
        vehicle[[2, 70, 300]] = v  # two wavefronts of the first block, and the second block
        speed[[2, 70]] = speeds[:2]
        speed[300] = last
        return vehicle, speed

    def step(where):
        for _ in range(2):  # (the command's step, and one more: it held for one step only)
            a.next_step()
            b.next_step()
            same_state(a, b, where)

    v = pick_discriminating(mod, cfg, b, speeds)
    command(a, b, *rows_of(v, speeds[2]), [(v, speeds[2])], where="the highest row wins")
    step("the highest row wins")
    v = pick_discriminating(mod, cfg, b, speeds)
    command(a, b, *rows_of(v, NAN), [(v, speeds[1])], where="a NaN row does not compete")
    step("a NaN row does not compete")
    v = pick_discriminating(mod, cfg, b, speeds + (0.75,))
    command(a, b, *rows_of(v, speeds[2]), [], where="first call")
    command(a, b, [-1, v], [9.0, 0.75], [(v, 0.75)], where="second call")  # (row 1 < 2: a stamp left standing would win)
    step("the later call wins")
    same_dicts(a, b, "duplicates")


def test_duplicates_twin(mod, scen, workdir):
    duplicates_body(mod, lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_duplicates(mod, scen, workdir, layout):
    duplicates_body(mod, lambda cfg: hip_engine(mod, cfg, layout), layout_config(scen, workdir, "grid_6x6", layout))


# --------------------------------------------------------------------------------------------------------------- 3. ignored
def ignored_body(mod, make_a, cfg):
    a, b = make_a(cfg), twin(mod, cfg)
    seen = set()
    finished = None
    for s in range(1, 261):
        a.next_step()
        b.next_step()
        alive = set(live_numbers(b).tolist())
        gone = seen - alive
        seen |= alive
        if gone and b._scalars()["finished_vehicle_count"] > 0:
            finished = min(gone)
            break
    assert finished is not None, "no vehicle finished in 260 steps"
    same_state(a, b, "before the call")
    rows = b.observe_vehicles_array()["vehicle"]
    live = [int(rows[0]), int(rows[len(rows) // 2])]
    vehicle = [finished, issued(b) + 3, -5, 2 ** 31 - 1, -1, int(rows[1]), live[0], live[1]]
    speed = [1.0, 1.0, 1.0, 1.0, 1.0, NAN, 0.5, 0.25]
    command(a, b, vehicle, speed, [(live[0], 0.5), (live[1], 0.25)], want_ignored=4, where="ignored")
    for s in range(3):
        a.next_step()
        b.next_step()
        same_state(a, b, "%d steps after the call" % (s + 1))
    same_dicts(a, b, "ignored")


def test_ignored_twin(mod, scen, workdir):
    ignored_body(mod, lambda cfg: twin(mod, cfg), scen.materialize("example_1x1", workdir))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_ignored(mod, scen, workdir, layout):
    ignored_body(mod, lambda cfg: hip_engine(mod, cfg, layout), layout_config(scen, workdir, "example_1x1", layout))


# ------------------------------------------------------------------------------------------- 4. one step only, and archives
def archives_body(mod, make_a, cfg, seed=11):
    rng = np.random.default_rng(seed)
    a, b = make_a(cfg), twin(mod, cfg)

    def call(where, share=0.6):
        live = live_numbers(b)
        vehicle, speed, effective = random_rows(rng, live, len(live) + 5, share)
        assert effective, where
        command(a, b, vehicle, speed, effective, where=where)

    def steps(n, where, skip=()):
        for s in range(n):
            a.next_step()
            b.next_step()
            same_state(a, b, "%s, step %d" % (where, s + 1), skip)

    steps(40, "free")
    call("one step only")
    steps(5, "one step only")  # (the vehicles move freely again from the second step on, on both)
    call("before snapshot")
    archives = a.snapshot(), b.snapshot()
    fresh = make_a(cfg), twin(mod, cfg)
    fresh[0].load(archives[0])
    fresh[1].load(archives[1])
    for s in range(3):
        fresh[0].next_step()
        fresh[1].next_step()
        same_state(fresh[0], fresh[1], "loaded into a fresh engine, step %d" % (s + 1))
    del fresh
    steps(3, "after snapshot")
    ck = a.checkpoint() if a._checkpoint_calls() and not a._checkpoint_unsupported() else None
    at_ck = b.snapshot()
    steps(4, "after checkpoint")
    a.load(archives[0])
    b.load(archives[1])
    call("right after load")
    steps(3, "right after load")
    if ck is not None:
        a.rollback(ck)
        b.load(at_ck)
        call("right after rollback")
        # (B has no checkpoints and loads an archive of the same moment; a load restarts every route position at the route's
        # begin, Archive's way, a rollback keeps them: the one column the two may differ in until the reset below)
        steps(3, "right after rollback", skip=("route_pos",))
    a.reset()
    b.reset()
    command(a, b, [0, 1, -1], [1.0, NAN, 2.0], [], want_ignored=1, where="right after reset")  # (no vehicle number is issued)
    steps(12, "after reset")
    call("12 steps after reset")
    steps(3, "12 steps after reset")
    same_dicts(a, b, "archives")


def test_one_step_only_and_archives_twin(mod, scen, workdir):
    archives_body(mod, lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_one_step_only_and_archives(mod, scen, workdir, layout):
    archives_body(mod, lambda cfg: hip_engine(mod, cfg, layout), layout_config(scen, workdir, "grid_6x6", layout))


# ---------------------------------------------------------------------------------------------------------- 5. VectorEngine
def vector_body(mod, scen, workdir, vec, steps=60, seed=3):
    R = 3
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=r)) for r in range(R)]
    rng = np.random.default_rng(seed)
    envs_commanded = set()
    for s in range(1, steps + 1):
        if s % 3 == 0:
            got = vec.observe_vehicles_array()
            wants = [e.observe_vehicles_array() for e in singles]
            D = vec._drivable_counts()[0] + vec._drivable_counts()[1]
            vehicle, per_env = [], []
            for r, want in enumerate(wants):  # row j of environment r is row j of twin r
                lo, hi = int(got["start"][r, 0]), int(got["start"][r, D])
                assert hi - lo == int(want["count"]), "step %d: env %d" % (s, r)
                assert np.array_equal(got["distance"][lo:hi], want["distance"]), "step %d: env %d" % (s, r)
                take = np.flatnonzero(rng.random(hi - lo) < 0.3)
                vehicle.append(got["vehicle"][lo:hi][take])
                per_env.append(want["vehicle"][take])
                envs_commanded |= {r} if len(take) else set()
            vehicle = np.concatenate(vehicle + [np.array([-1, -1], dtype=np.int32)]).astype(np.int32)
            speed = rng.uniform(0.0, 12.0, len(vehicle))
            order = rng.permutation(len(vehicle))  # (the environments' vehicles mixed within the one call)
            ignored = torch.full((), -7, dtype=torch.int32, device=tensor_device(vec))
            vec.set_vehicle_speeds_tensor(dev(vec, vehicle[order]), dev(vec, speed[order]), ignored)
            assert int(ignored.item()) == 0, s
            at = 0
            for e, numbers in zip(singles, per_env):
                for v in numbers.tolist():
                    e.set_vehicle_speed(e._vehicle_id(v), float(speed[at]))
                    at += 1
        vec.next_step()
        for r, e in enumerate(singles):
            e.next_step()
            assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "step %d: env %d" % (s, r)
    assert envs_commanded == set(range(R))


def test_vector_engine_twin(mod, scen, workdir):
    vector_body(mod, scen, workdir, mod.VectorEngine._with_backend(scen.materialize("grid_6x6", workdir), 3, 1, TWIN_LIB))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_vector_engine(mod, scen, workdir, layout):
    vec = mod.VectorEngine(layout_config(scen, workdir, "grid_6x6", layout), 3)
    assert SHADOW_GPU or vec.backend_name() == "hip-gfx950"
    vector_body(mod, scen, workdir, vec)


# ---------------------------------------------------------------------------------------------------- 6. stream order (gpu)
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_inputs_from_a_side_stream(mod, scen, workdir, layout):
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    a, b = hip_engine(mod, cfg, layout), twin(mod, cfg)
    if not a._device_buffers():
        pytest.skip("needs device buffers: torch streams do not exist on the twin")
    for _ in range(50):
        a.next_step()
        b.next_step()
    device = tensor_device(a)
    side = torch.cuda.Stream(device=device)
    for round_ in range(4):
        rows = b.observe_vehicles_array()
        n = int(rows["count"])
        base = np.linspace(0.5, 6.0, n)
        vehicle = dev(a, rows["vehicle"])
        seed = dev(a, base)
        speed = torch.zeros(n, dtype=torch.float64, device=device)
        ignored = torch.full((), -7, dtype=torch.int32, device=device)
        torch.cuda.synchronize(device)
        with torch.cuda.stream(side):
            big = torch.ones((2048, 2048), device=device)  # (work in front of the producer: the engine must wait for `side`)
            for _ in range(8):
                big = big @ big * 1e-4
            speed.copy_(seed * 2.0 + big[0, 0] * 0.0)
            a.set_vehicle_speeds_tensor(vehicle, speed, ignored)
            a.next_step()
            assert int(ignored.item()) == 0  # (read on `side`, with no synchronise of our own before it)
        for v, s in zip(rows["vehicle"].tolist(), (base * 2.0).tolist()):
            b.set_vehicle_speed(b._vehicle_id(v), s)
        b.next_step()
        same_state(a, b, "round %d" % round_)
    same_dicts(a, b, "side stream")


# ---------------------------------------------------------------------------------------------------------------- 7. errors
def test_argument_errors_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    a, b = twin(mod, cfg), twin(mod, cfg)
    for _ in range(30):
        a.next_step()
        b.next_step()
    live = b.observe_vehicles_array()["vehicle"][:6]
    vehicle, speed = torch.from_numpy(live.copy()), torch.full((6,), 0.5, dtype=torch.float64)
    ignored = torch.full((), -7, dtype=torch.int32)
    call = a.set_vehicle_speeds_tensor
    with pytest.raises(TypeError, match="torch.Tensor"):
        call(vehicle.numpy(), speed)
    with pytest.raises(TypeError, match="torch.Tensor"):
        call(vehicle, speed.numpy())
    with pytest.raises(TypeError, match="must be torch"):
        call(vehicle.to(torch.int64), speed)
    with pytest.raises(TypeError, match="must be torch"):
        call(vehicle, speed.to(torch.float32))
    with pytest.raises(TypeError, match="must be torch"):
        call(vehicle, speed, ignored.to(torch.int64))
    with pytest.raises(ValueError, match="shape"):
        call(vehicle.reshape(3, 2), speed)
    with pytest.raises(ValueError, match="shape"):  # one N for both
        call(vehicle, torch.full((7,), 0.5, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        call(vehicle, speed, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="contiguous"):
        call(torch.from_numpy(np.repeat(live, 2))[::2], speed)
    with pytest.raises(ValueError, match="contiguous"):
        call(vehicle, torch.full((12,), 0.5, dtype=torch.float64)[::2])
    other = "cuda" if torch.cuda.is_available() else "meta"  # (a tensor on another device than the engine's)
    with pytest.raises(TypeError, match="live on"):
        call(vehicle.to(other), speed)
    with pytest.raises(TypeError, match="live on"):
        call(vehicle, speed, ignored.to(other))
    for bad in ((live.astype(np.int64), np.full(6, 0.5)), (live, np.full(6, 0.5, dtype=np.float32)), (live.tolist(), np.full(6, 0.5))):
        with pytest.raises(TypeError):
            a.set_vehicle_speeds(*bad)
    for bad in ((live, np.full(7, 0.5)), (live.reshape(3, 2), np.full(6, 0.5)), (np.repeat(live, 2)[::2], np.full(6, 0.5))):
        with pytest.raises(ValueError):
            a.set_vehicle_speeds(*bad)
    assert int(ignored) == -7  # nothing was written by a rejected call ...
    a.next_step()
    b.next_step()
    same_state(a, b, "after the rejected calls")  # ... and nothing commanded
    call(vehicle[:0], speed[:0], ignored)  # N = 0 is a call
    assert int(ignored) == 0 and a.set_vehicle_speeds(live[:0], np.zeros(0)) == 0
    assert not hasattr(mod.TiledEngine, "set_vehicle_speeds_tensor") and not hasattr(mod.TiledEngine, "set_vehicle_speeds")


def lane_change_body(eng):
    eng.next_step()
    with pytest.raises(RuntimeError, match="laneChange"):
        eng.set_vehicle_speeds_tensor(torch.zeros(2, dtype=torch.int32, device=tensor_device(eng)),
                                      torch.zeros(2, dtype=torch.float64, device=tensor_device(eng)))
    with pytest.raises(RuntimeError, match="laneChange"):
        eng.set_vehicle_speeds(np.zeros(2, dtype=np.int32), np.zeros(2))


def test_lane_change_raises_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    lane_change_body(twin(mod, cfg))
    lane_change_body(mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB))


@pytest.mark.gpu
def test_lane_change_raises(mod, scen, workdir):
    lane_change_body(mod.Engine(scen.materialize("grid_6x6", workdir, laneChange=True), 1))
