"""The lanes' speed limits as engine state: set_lane_speed_limits_tensor / get_lane_speed_limits_tensor / set_lane_speed_limits /
get_lane_speed_limits_array / restore_lane_speed_limits on Engine and VectorEngine (cityflow_amd/torch_io.py,
cfx_set_lane_speed_limits_device and its kin).

The oracle is the engine on another input, as in test_tl_plan.py: an engine BUILT from a roadnet file whose lanes' `maxSpeed`
fields were rewritten must equal an engine built from the original file and GIVEN those limits through the new call — every
vehicle, exactly (assert_same_state).  Where a limit changes mid-run the built engine loads the other's snapshot.  The limits
are 3.0 + ((7 i + 5 k) % 9) * 1.25 for lane i of scheme k: short decimals that are exact doubles, so the JSON literals and the
tensors hold the same numbers.

An equality that holds because nothing changed proves nothing, so every equality test first shows on the EXPECTED engine
that the limits bind: some vehicle on a lane drives exactly at that lane's limit, one below the file's 16.67, and the state
differs from that of an engine built from the unchanged file.  (A limit caps the speed a step computes and is no deceleration,
so no test asserts speed <= limit per vehicle.)"""
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_hip_backend, assert_same_state, full_state

torch = pytest.importorskip("torch")

from test_device_tensors import tensor_device  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_tl_plan import derive, dev, network, roadnet_of  # noqa: E402

NAN = float("nan")
FILE_LIMIT = 16.67  # every lane of the stock scenarios and of the star networks


# ----------------------------------------------------------------------------------------------------------------- helpers
class Limits:
    """The lanes' limits of a config's roadnet file in lane_ids() order, from the JSON alone."""

    def __init__(self, eng, cfg):
        self.cfg = cfg
        self.ids = eng.lane_ids()
        by_id = {"%s_%d" % (road["id"], k): float(lane["maxSpeed"]) for road in roadnet_of(cfg)["roads"]
                 for k, lane in enumerate(road["lanes"])}
        self.file = np.array([by_id[i] for i in self.ids])
        self.L = len(self.ids)
        assert self.L > 0 and (self.file == FILE_LIMIT).all()

    def scheme(self, k=0):
        i = np.arange(self.L)
        return 3.0 + ((7 * i + 5 * k) % 9) * 1.25

    def kept(self, k=0):
        """(the input, the limits in force after it over the file's): scheme k with NaN on every third lane."""
        given = self.scheme(k)
        given[(np.arange(self.L) + k) % 3 == 0] = NAN
        return given, np.where(np.isnan(given), self.file, given)

    def built(self, V, tag, **overrides):
        """A config whose roadnet file carries the limits V."""
        net = roadnet_of(self.cfg)
        at = {i: n for n, i in enumerate(self.ids)}
        for road in net["roads"]:
            for k, lane in enumerate(road["lanes"]):
                lane["maxSpeed"] = float(V[at["%s_%d" % (road["id"], k)]])
        return derive(self.cfg, "sl_" + tag, roadnet=net, **overrides)


def on_device(eng):
    """The limits are state only the device library keeps.  Where the CPU twin stands in for it (the shadow run of the GPU
    tests, conftest.py) there is nothing to run; on the HIP library this never skips, with or without the new entry points."""
    if not eng._device_buffers():
        pytest.skip("the lanes' speed limits as engine state need the device library: the twin has no such calls")
    return eng


def limits_of(eng):
    """The getter, three ways, all equal: the array call, a new tensor, a pre-filled `out`."""
    got = eng.get_lane_speed_limits_array()
    t = eng.get_lane_speed_limits_tensor()
    assert t.dtype == torch.float64 and tuple(t.shape) == got.shape and np.array_equal(t.cpu().numpy(), got)
    out = torch.full(got.shape, -7.0, dtype=torch.float64, device=tensor_device(eng))  # (every element must be written)
    assert eng.get_lane_speed_limits_tensor(out=out) is out
    assert np.array_equal(out.cpu().numpy(), got)
    return got


def at_a_limit(eng, V):
    """Vehicles on a lane whose speed is exactly that lane's limit, where the limit is below the file's."""
    s = eng._vehicle_state()
    lane = s["drivable"] < len(V)
    v = V[s["drivable"][lane]]
    return int(((s["speed"][lane] == v) & (v < FILE_LIMIT)).sum())


def differs(a, b):
    sa, sb = full_state(a), full_state(b)
    return sa["vid"].shape != sb["vid"].shape or not (np.array_equal(sa["speed"], sb["speed"]) and np.array_equal(sa["dis"], sb["dis"]))


def run_equal(expected, others, steps, where, V, plain=None, every=25):
    """Step all engines together: the whole state of each of `others` equals `expected`'s every `every` steps and at the end.
    First the precondition, on `expected`: vehicles drive exactly at limits of V, and (`plain`: an engine on the unchanged file
    in the same state at the start, stepped along) the state leaves the unchanged file's."""
    bound, left = 0, plain is None
    for s in range(steps):
        for e in [expected] + list(others) + ([] if plain is None else [plain]):
            e.next_step()
        if s % every == every - 1 or s == steps - 1:
            bound += at_a_limit(expected, V)
            left = left or differs(expected, plain)
            if s == steps - 1:
                assert bound > 0, where + ": no vehicle of the expected engine ever drove at its lane's limit"
                assert left, where + ": the expected engine never left the unchanged file's state"
            for e in others:
                assert_same_state(expected, e, "%s, step %d" % (where, s))
    assert expected.get_vehicle_count() > 0, where + ": no vehicle ran"


def rejected_tensor(eng):
    return torch.full((1,), -7, dtype=torch.int32, device=tensor_device(eng))


LAYOUTS = ["auto", "dense"]
NETS = ["example_1x1", "star3", "star5"]


# ----------------------------------------------------------------------------------------------------------------- GPU
def built_equals_set_at_step_0(mod, cfg, tag, steps=150):
    given, plain = on_device(mod.Engine(cfg, 1)), mod.Engine(cfg, 1)
    assert_hip_backend(given)
    lim = Limits(given, cfg)
    assert np.array_equal(limits_of(given), lim.file)
    values, V = lim.kept(0)
    assert np.isnan(values).sum() >= lim.L // 3 and not np.array_equal(V, lim.file)
    built = mod.Engine(lim.built(V, tag), 1)
    assert built._layout() == given._layout()
    rejected = rejected_tensor(given)
    given.set_lane_speed_limits_tensor(dev(given, values), rejected)
    assert int(rejected.item()) == 0
    assert np.array_equal(limits_of(given), V)
    assert np.array_equal(limits_of(built), V)
    run_equal(built, [given], steps, tag, V, plain)
    assert np.array_equal(limits_of(given), V)
    return given


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("net", NETS)
def test_built_equals_set_at_step_0(mod, scen, workdir, net, layout):
    given = built_equals_set_at_step_0(mod, network(scen, workdir, net, layout), "built0_%s_%s" % (net, layout))
    assert given._layout() == ("ring" if layout == "auto" else "dense")


@pytest.mark.gpu
@pytest.mark.parametrize("form", [20000, 30000, 40000])
def test_built_equals_set_on_the_ring_forms(mod, scen, workdir, form):
    """The ring layout's forced forms: lane walking kr_action, the vehicle list kl_action, and the separate commit."""
    cfg = scen.materialize("grid_6x6", workdir, cfx={"layout": "ring", "ringLanesPerWave": form})
    given = built_equals_set_at_step_0(mod, cfg, "form%d" % form)
    assert given._layout() == "ring"


def set_mid_run(mod, lim, b, k, tag, steps, plain_cfg):
    """Scheme k (with its kept lanes) given to b now; the engine built from the resulting limits loads b's snapshot, and so do
    b and an engine on the unchanged file.  -> the limits in force"""
    values, V = lim.kept(k)
    V = np.where(np.isnan(values), limits_of(b), values)
    arch = b.snapshot()
    a, plain = mod.Engine(lim.built(V, tag), 1), mod.Engine(plain_cfg, 1)
    for e in (a, b, plain):
        e.load(arch)  # (all go on from the archive, so all number their vehicles alike)
    b.set_lane_speed_limits_tensor(dev(b, values))
    assert np.array_equal(limits_of(b), V)
    run_equal(a, [b], steps, tag, V, plain)
    return V


@pytest.mark.gpu
@pytest.mark.parametrize("net,layout", [("example_1x1", "auto"), ("example_1x1", "dense"), ("grid_6x6", "auto"), ("star5", "dense")])
def test_built_equals_set_mid_run(mod, scen, workdir, net, layout):
    cfg = network(scen, workdir, net, layout)
    b = on_device(mod.Engine(cfg, 1))
    lim = Limits(b, cfg)
    for s in range(60):
        b.next_step()
    first = set_mid_run(mod, lim, b, 0, "mid0_%s_%s" % (net, layout), 150, cfg)
    second = set_mid_run(mod, lim, b, 1, "mid1_%s_%s" % (net, layout), 100, cfg)
    assert not np.array_equal(first, second) and (second != FILE_LIMIT).all()  # (every lane was set by one of the two)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_rejected_entries_are_left_out_and_counted(mod, scen, workdir, layout):
    cfg = network(scen, workdir, "example_1x1", layout)
    b = on_device(mod.Engine(cfg, 1))
    lim = Limits(b, cfg)
    assert lim.L >= 12
    base = lim.scheme(2)
    assert b.set_lane_speed_limits(base) == 0
    for form in ("tensor", "array"):
        values = lim.scheme(3)
        bad = {1: -0.5, 4: np.inf, 7: -np.inf, 10: -1e300}
        keep = [2, 5]
        for i, x in bad.items():
            values[i] = x
        values[keep] = NAN
        values[0], values[3] = 0.0, 45.0  # (a closed lane and a limit above 30 are values like any other)
        want = np.array(values)
        for i in list(bad) + keep:
            want[i] = base[i]
        if form == "tensor":
            rejected = rejected_tensor(b)
            b.set_lane_speed_limits_tensor(dev(b, values), rejected)
            assert int(rejected.item()) == len(bad)
            b.set_lane_speed_limits_tensor(dev(b, np.full(lim.L, NAN)), rejected)  # (the count is this call's own)
            assert int(rejected.item()) == 0
        else:
            assert b.set_lane_speed_limits(values) == len(bad)
        assert np.array_equal(limits_of(b), want), form
        assert b.set_lane_speed_limits(base) == 0
    assert b.set_lane_speed_limits(np.full(lim.L, -np.inf)) == lim.L  # (nothing applied)
    assert np.array_equal(limits_of(b), base)
    a = mod.Engine(lim.built(base, "rejected_" + layout), 1)
    run_equal(a, [b], 60, "after the rejected calls " + layout, base, mod.Engine(cfg, 1))


def approach_lane(eng, cfg):
    """The lane with the most vehicles among those that end at a signalised intersection."""
    net = roadnet_of(cfg)
    real = {it["id"] for it in net["intersections"] if not it["virtual"]}
    ids = eng.lane_ids()
    approach = [n for n, i in enumerate(ids) if any(r["id"] == i.rsplit("_", 1)[0] and r["endIntersection"] in real for r in net["roads"])]
    counts = eng.get_lane_vehicle_count_array()
    return max(approach, key=lambda n: counts[n])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_closed_lane_and_its_reopening(mod, scen, workdir, layout):
    cfg = network(scen, workdir, "example_1x1", layout)
    b = on_device(mod.Engine(cfg, 1))
    lim = Limits(b, cfg)
    for s in range(60):
        b.next_step()
    lane = approach_lane(b, cfg)
    assert b.get_lane_vehicle_count_array()[lane] >= 2
    closed = np.array(lim.file)
    closed[lane] = 0.0
    only = np.full(lim.L, NAN)
    only[lane] = 0.0
    arch = b.snapshot()
    a, plain = twin(mod, lim.built(closed, "closed_" + layout)), twin(mod, cfg)
    for e in (a, b, plain):
        e.load(arch)
    b.set_lane_speed_limits_tensor(dev(b, only))
    assert np.array_equal(limits_of(b), closed)
    run_equal(a, [b], 30, "closed lane " + layout, closed, plain, every=10)
    on_lane = a._vehicle_state()
    assert (on_lane["speed"][on_lane["drivable"] == lane] == 0.0).sum() >= 2
    only[lane] = FILE_LIMIT
    arch = b.snapshot()
    a = twin(mod, cfg)  # (the third roadnet file is the first)
    a.load(arch)
    b.load(arch)
    b.set_lane_speed_limits_tensor(dev(b, only))
    assert np.array_equal(limits_of(b), lim.file)
    for s in range(60):
        a.next_step()
        b.next_step()
        if s % 10 == 9:
            assert_same_state(a, b, "reopened lane %s, step %d" % (layout, s))
    on_lane = a._vehicle_state()
    assert (on_lane["speed"][on_lane["drivable"] == lane] > 0.0).any(), "the reopened lane never moved"


# ---- ownership: the limits belong to the engine like the roadnet
def given_engine(mod, cfg, k):
    b = on_device(mod.Engine(cfg, 1))
    lim = Limits(b, cfg)
    values, V = lim.kept(k)
    b.set_lane_speed_limits_tensor(dev(b, values))
    return b, lim, V


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_reset_keeps_the_limits_and_restore_brings_the_files_back(mod, scen, workdir, layout):
    cfg = network(scen, workdir, "example_1x1", layout)
    b, lim, V = given_engine(mod, cfg, 4)
    for s in range(40):
        b.next_step()
    b.reset(True)  # (with the seed: a new engine starts from it)
    assert np.array_equal(limits_of(b), V), "reset() changed the limits in force"
    run_equal(mod.Engine(lim.built(V, "reset_" + layout), 1), [b], 100, "after reset " + layout, V, mod.Engine(cfg, 1))
    b.restore_lane_speed_limits()
    assert np.array_equal(limits_of(b), lim.file)
    b.reset(True)
    fresh = mod.Engine(cfg, 1)
    for s in range(100):
        fresh.next_step()
        b.next_step()
    assert_same_state(fresh, b, "after restore_lane_speed_limits " + layout)
    assert fresh.get_vehicle_count() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("what", ["load", "compact"])
def test_load_and_compaction_leave_the_limits_alone(mod, scen, workdir, layout, what):
    cfg = network(scen, workdir, "example_1x1", layout)
    b, lim, V = given_engine(mod, cfg, 5)
    a, plain = mod.Engine(lim.built(V, "%s_%s" % (what, layout)), 1), mod.Engine(cfg, 1)
    for s in range(60):
        for e in (a, b, plain):
            e.next_step()
    assert_same_state(a, b, "before the " + what)
    if what == "load":
        arch = b.snapshot()
        for e in (a, b):
            e.load(arch)
    else:
        for e in (a, b, plain):
            e._compact_vehicles()
    assert np.array_equal(limits_of(b), V), what + " changed the limits in force"
    run_equal(a, [b], 100, "after the %s %s" % (what, layout), V, plain)


@pytest.mark.gpu
def test_ring_growth_leaves_the_limits_alone(mod, scen, workdir):
    import os
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense.json"), 400, seed=7, interval=2.0,
                            base_flow=os.path.join(d, "flow.json"))
    cfg = scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring", "ringCapacityPercent": 30})
    b, lim, V = given_engine(mod, cfg, 6)
    a = mod.Engine(lim.built(V, "growth", cfx={"layout": "ring"}), 1)  # (starts large)
    plain = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring"}), 1)
    run_equal(a, [b], 300, "growing rings", V, plain, every=50)
    assert b._ring_info()[1] >= 2 and a._ring_info()[1] == 1, (b._ring_info(), a._ring_info())
    assert np.array_equal(limits_of(b), V), "ring growth changed the limits in force"


@pytest.mark.gpu
def test_checkpoint_and_rollback_leave_the_limits_alone(mod, scen, workdir):
    cfg = network(scen, workdir, "example_1x1")
    b, lim, V = given_engine(mod, cfg, 7)
    if not b._checkpoint_calls():
        pytest.skip("the backend %s has no checkpoints in device memory" % b.backend_name())
    for s in range(60):
        b.next_step()
    ck = b.checkpoint()
    assert np.array_equal(limits_of(b), V), "checkpoint() changed the limits in force"
    values, second = lim.kept(8)
    second = np.where(np.isnan(values), V, values)
    b.set_lane_speed_limits_tensor(dev(b, values))
    for s in range(30):
        b.next_step()
    b.rollback(ck)
    assert np.array_equal(limits_of(b), second), "rollback() changed the limits in force"
    arch = b.snapshot()
    a, plain = mod.Engine(lim.built(second, "rollback"), 1), mod.Engine(cfg, 1)
    for e in (a, b, plain):
        e.load(arch)
    run_equal(a, [b], 100, "after the rollback", second, plain)


@pytest.mark.gpu
def test_vector_engine_one_scheme_per_environment(mod, scen, workdir):
    R = 3
    cfg = scen.materialize("example_1x1", workdir)
    vec = on_device(mod.VectorEngine(cfg, R))
    lim = Limits(mod.Engine(cfg, 1), cfg)
    given = [lim.kept(k) for k in range(R)]
    schemes = np.stack([V for _, V in given])
    assert not np.array_equal(schemes[0], schemes[1]) and not np.array_equal(schemes[1], schemes[2])
    singles = [mod.Engine(lim.built(schemes[r], "env%d" % r, seed=r), 1) for r in range(R)]  # (environment r runs on seed + r)
    plain = [mod.Engine(scen.materialize("example_1x1", workdir, seed=r), 1) for r in range(R)]
    assert np.array_equal(limits_of(vec), np.stack([lim.file] * R))
    rejected = rejected_tensor(vec)
    vec.set_lane_speed_limits_tensor(dev(vec, np.stack([v for v, _ in given])), rejected)
    assert int(rejected.item()) == 0
    assert np.array_equal(limits_of(vec), schemes)
    assert vec.lane_ids() == singles[0].lane_ids()
    ck = None
    for s in range(150):
        vec.next_step()
        for e in singles + plain:
            e.next_step()
        if s == 99 and vec._checkpoint_calls():
            ck = vec.checkpoint()
        if s % 10 != 9:
            continue
        counts, waits = vec.get_lane_vehicle_count_array(), vec.get_lane_waiting_vehicle_count_array()
        for r, e in enumerate(singles):
            assert np.array_equal(counts[r], e.get_lane_vehicle_count_array()), (s, r)
            assert np.array_equal(waits[r], e.get_lane_waiting_vehicle_count_array()), (s, r)
            assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), (s, r)
    for r, e in enumerate(singles):
        assert at_a_limit(e, schemes[r]) > 0 and differs(e, plain[r]), "env %d: the limits never bound" % r
    assert vec.get_vehicle_count() == sum(e.get_vehicle_count() for e in singles)
    assert ck is not None
    vec.rollback(ck, envs=[2, 2, 0])
    assert np.array_equal(limits_of(vec), schemes), "rollback(envs=...) moved the limits with the states"
    assert vec.set_lane_speed_limits(np.full((R, lim.L), NAN)) == 0
    assert np.array_equal(vec.get_lane_speed_limits_array(), schemes)
    vec.restore_lane_speed_limits()
    assert np.array_equal(limits_of(vec), np.stack([lim.file] * R))


@pytest.mark.gpu
def test_limits_from_a_side_stream_without_a_host_wait(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = on_device(mod.Engine(cfg, 1))
    lim = Limits(eng, cfg)
    values, V = lim.kept(9)
    ref, plain = mod.Engine(lim.built(V, "side"), 1), mod.Engine(cfg, 1)
    for s in range(20):  # warm: rings built, tables uploaded
        for e in (eng, plain):
            e.next_step()
    arch = eng.snapshot()
    for e in (eng, ref, plain):
        e.load(arch)
    device = tensor_device(eng)
    half = dev(eng, values / 2)
    out = torch.full((lim.L,), -7.0, dtype=torch.float64, device=device)
    rejected = rejected_tensor(eng)
    eng.set_lane_speed_limits_tensor(dev(eng, np.full(lim.L, NAN)), rejected)  # (the kernels' code is loaded: not timed)
    eng.get_lane_speed_limits_tensor(out=out)
    eng.sync()
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):  # (torch loads a kernel's code at its first launch and waits for the device to do so: not timed)
        warm = half + half
        del warm
    side.synchronize()
    eng._device_spin(200000)  # 200 ms of device work in front of everything below
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        made = half + half  # the limits are the output of a torch op on `side`, handed over as they are
        eng.set_lane_speed_limits_tensor(made, rejected)
        del made  # (its memory may be handed out again by work enqueued on `side` from here on)
        scribble = torch.full((lim.L,), -1.0, dtype=torch.float64, device=device)
        eng.next_step()
        eng.get_lane_speed_limits_tensor(out=out)
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the calls waited for the device (%.1f ms behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    assert bool((scribble == -1.0).all())
    assert np.array_equal(out.cpu().numpy(), V) and int(rejected.item()) == 0
    ref.next_step()
    plain.next_step()
    run_equal(ref, [eng], 60, "after the unsynchronised calls", V, plain, every=20)
    # a count that many waves of several blocks add to
    assert lim.L > 256
    bad = np.full(lim.L, NAN)
    bad[::2] = -1.0
    eng.set_lane_speed_limits_tensor(dev(eng, bad), rejected)
    assert int(rejected.item()) == (lim.L + 1) // 2 and eng.set_lane_speed_limits(bad) == (lim.L + 1) // 2
    assert np.array_equal(limits_of(eng), V)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_with_vehicle_speed_commands_in_the_same_loop(mod, scen, workdir, layout):
    from test_vehicle_speeds import command, live_numbers, random_rows
    cfg = network(scen, workdir, "example_1x1", layout)
    a, lim, V = given_engine(mod, cfg, 10)
    b, plain = twin(mod, lim.built(V, "commands_" + layout)), twin(mod, cfg)
    rng = np.random.default_rng(17)
    bound, left = 0, False
    for s in range(1, 91):
        where = "%s step %d" % (layout, s)
        if s % 3 == 0:
            vehicle, speed, effective = random_rows(rng, live_numbers(b), 24)
            command(a, b, vehicle, speed, effective, 0, "tensor", where)
            there = set(plain.get_vehicles(include_waiting=True))  # (vehicles are named alike; the faster side's may have finished)
            for v, x in effective:
                if b._vehicle_id(int(v)) in there:
                    plain.set_vehicle_speed(b._vehicle_id(int(v)), float(x))
        if s == 45:  # a second scheme between two commands, by the numpy form
            values, _ = lim.kept(11)
            V = np.where(np.isnan(values), V, values)
            assert a.set_lane_speed_limits(values) == 0
            arch = a.snapshot()
            b = twin(mod, lim.built(V, "commands2_" + layout))
            for e in (a, b, plain):
                e.load(arch)
        for e in (a, b, plain):
            e.next_step()
        if s % 15 == 0:
            bound += at_a_limit(b, V)
            left = left or differs(b, plain)
            assert_same_state(b, a, where)
    assert bound > 0 and left, "the limits never bound"
    assert a.get_vehicle_speed() == b.get_vehicle_speed() and a.get_vehicle_distance() == b.get_vehicle_distance()


@pytest.mark.gpu
def test_built_equals_set_with_lane_change(mod, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir, laneChange=True)
    given, plain = on_device(mod.Engine(cfg, 1)), mod.Engine(cfg, 1)
    assert given._layout() == "dense"
    lim = Limits(given, cfg)
    values, V = lim.kept(12)
    built = mod.Engine(lim.built(V, "lanechange"), 1)
    given.set_lane_speed_limits_tensor(dev(given, values))
    run_equal(built, [given], 150, "lane change", V, plain)
    assert np.array_equal(limits_of(given), V)


@pytest.mark.gpu
def test_a_random_sequence_of_steps_and_limit_changes(mod, scen, workdir):
    """200 steps with limit changes, a reset, a restore and a rollback at steps drawn with a fixed seed.  At each change the
    twin is rebuilt from the limits then in force and both sides (and a twin on the unchanged file) load the snapshot."""
    cfg = network(scen, workdir, "example_1x1")
    b = on_device(mod.Engine(cfg, 1))
    if not b._checkpoint_calls():
        pytest.skip("the backend %s has no checkpoints in device memory" % b.backend_name())
    lim = Limits(b, cfg)
    rng = np.random.default_rng(23)
    at = sorted(int(x) for x in rng.choice(np.arange(8, 190), 8, replace=False))
    events = dict(zip(at, ["change", "checkpoint", "change", "reset", "change", "rollback", "restore", "change"]))
    V = np.array(lim.file)
    a, plain = twin(mod, cfg), twin(mod, cfg)
    ck, k, bound, left, made = None, 0, 0, False, 0

    def rebuild(tag):
        arch = b.snapshot()
        t = twin(mod, lim.built(V, "seq_%s" % tag) if not np.array_equal(V, lim.file) else cfg)
        for e in (t, b, plain):
            e.load(arch)
        return t

    for s in range(200):
        what = events.get(s)
        where = "step %d (%s)" % (s, what)
        if what is not None:
            assert_same_state(a, b, "before " + where)
        if what == "change":
            values = lim.scheme(20 + k)
            values[rng.random(lim.L) < 0.4] = NAN
            if k == 1:
                values[3] = -2.0  # (a rejected entry among the others)
            rejected = rejected_tensor(b)
            b.set_lane_speed_limits_tensor(dev(b, values), rejected)
            assert int(rejected.item()) == (1 if k == 1 else 0)
            values[values < 0] = NAN
            V = np.where(np.isnan(values), V, values)
            a = rebuild("change%d" % k)
            k += 1
        elif what == "checkpoint":
            ck = b.checkpoint()
        elif what == "reset":
            for e in (a, b, plain):
                e.reset(True)
        elif what == "rollback":
            b.rollback(ck)
            a = rebuild("rollback")
        elif what == "restore":
            b.restore_lane_speed_limits()
            V = np.array(lim.file)
            a = rebuild("restore")
        if what is not None:
            made += 1
            assert np.array_equal(limits_of(b), V), where
        for e in (a, b, plain):
            e.next_step()
        if s % 25 == 24 or s == 199:
            bound += at_a_limit(a, V)
            left = left or differs(a, plain)
            assert_same_state(a, b, "step %d" % s)
    assert made == 8 and bound > 0 and left and not np.array_equal(V, lim.file)


# ----------------------------------------------------------------------------------------------------------------- CPU (twin)
def test_argument_errors_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = twin(mod, cfg)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    L = len(eng.lane_ids())
    good = torch.zeros(L, dtype=torch.float64)
    count = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError):  # not a tensor
        eng.set_lane_speed_limits_tensor(good.numpy())
    with pytest.raises(TypeError):  # wrong device (the twin's tensors live on the CPU)
        eng.set_lane_speed_limits_tensor(good.to("meta"))
    with pytest.raises(TypeError):  # wrong dtype
        eng.set_lane_speed_limits_tensor(good.to(torch.float32))
    with pytest.raises(ValueError):  # wrong shape
        eng.set_lane_speed_limits_tensor(torch.cat([good, good]))
    with pytest.raises(ValueError):  # [R, L] wanted
        vec.set_lane_speed_limits_tensor(good)
    with pytest.raises(ValueError):  # [L] wanted
        eng.set_lane_speed_limits_tensor(torch.zeros((2, L), dtype=torch.float64))
    noncontig = torch.zeros((L, 2), dtype=torch.float64)[:, 0]
    assert tuple(noncontig.shape) == (L,) and not noncontig.is_contiguous()
    with pytest.raises(ValueError):
        eng.set_lane_speed_limits_tensor(noncontig)
    with pytest.raises(TypeError):
        eng.set_lane_speed_limits_tensor(good, rejected=count.numpy())
    with pytest.raises(TypeError):
        eng.set_lane_speed_limits_tensor(good, rejected=count.to("meta"))
    with pytest.raises(TypeError):
        eng.set_lane_speed_limits_tensor(good, rejected=count.to(torch.int64))
    with pytest.raises(ValueError):
        eng.set_lane_speed_limits_tensor(good, rejected=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        eng.set_lane_speed_limits_tensor(good, rejected=torch.zeros((), dtype=torch.int32))
    with pytest.raises(ValueError):  # a later argument that is wrong: still an argument error, not the missing backend call
        vec.set_lane_speed_limits_tensor(torch.zeros((2, L), dtype=torch.float64), rejected=torch.zeros((1, 1), dtype=torch.int32))
    with pytest.raises(TypeError):
        eng.get_lane_speed_limits_tensor(out=torch.zeros(L, dtype=torch.float32))
    with pytest.raises(TypeError):
        eng.get_lane_speed_limits_tensor(out=np.zeros(L))
    with pytest.raises(ValueError):
        eng.get_lane_speed_limits_tensor(out=torch.zeros(L + 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        vec.get_lane_speed_limits_tensor(out=torch.zeros(L, dtype=torch.float64))
    with pytest.raises(ValueError):
        eng.get_lane_speed_limits_tensor(out=noncontig)
    with pytest.raises(TypeError):
        eng.set_lane_speed_limits(np.zeros(L, dtype=np.int32))
    with pytest.raises(TypeError):
        eng.set_lane_speed_limits(None)
    with pytest.raises(ValueError):
        eng.set_lane_speed_limits(np.zeros(L + 1))
    with pytest.raises(ValueError):
        vec.set_lane_speed_limits(np.zeros(L))


def test_a_backend_without_the_calls_says_so_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    L = len(twin(mod, cfg).lane_ids())
    for eng, lead in ((twin(mod, cfg), ()), (mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB), (2,))):
        assert not eng._lane_limit_calls()
        with pytest.raises(NotImplementedError, match=eng.backend_name()):
            eng.set_lane_speed_limits_tensor(torch.ones(lead + (L,), dtype=torch.float64))
        with pytest.raises(NotImplementedError):
            eng.set_lane_speed_limits_tensor(torch.ones(lead + (L,), dtype=torch.float64), rejected=torch.zeros(1, dtype=torch.int32))
        with pytest.raises(NotImplementedError):
            eng.set_lane_speed_limits(np.ones(lead + (L,)))
        with pytest.raises(NotImplementedError):
            eng.get_lane_speed_limits_tensor()
        with pytest.raises(NotImplementedError):
            eng.get_lane_speed_limits_tensor(out=torch.zeros(lead + (L,), dtype=torch.float64))
        with pytest.raises(NotImplementedError):
            eng.get_lane_speed_limits_array()
        with pytest.raises(NotImplementedError):
            eng.restore_lane_speed_limits()
        for s in range(3):  # (and the engine is none the worse for it)
            eng.next_step()


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    names = ("set_lane_speed_limits_tensor", "get_lane_speed_limits_tensor", "set_lane_speed_limits", "get_lane_speed_limits_array",
             "restore_lane_speed_limits")
    code = ("import sys, cityflow_amd; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert all(hasattr(c, n) for c in (cityflow_amd.Engine, cityflow_amd.VectorEngine) for n in %r); "
            "assert not any(hasattr(cityflow_amd.TiledEngine, n) for n in %r)" % (names, names))
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)

