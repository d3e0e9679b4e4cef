"""The fixed-time signal plan as engine state: set_tl_plan_tensor / get_tl_phase_durations_tensor / set_tl_plan /
get_tl_phase_durations_array / restore_tl_plan on Engine and VectorEngine (cityflow_amd/torch_io.py, cfx_set_tl_plan_device and
its kin), and VectorEngine(seeds=...).

The oracle of the behaviour tests is the engine itself on another input: an engine BUILT from a roadnet file whose lightphase
`time` fields were rewritten must equal an engine built from the original file and GIVEN that plan through the new call —
every vehicle (assert_same_state) and, on every step, every light (_tl_state()).  The lights alone are also held against a
restatement of TrafficLight::passTime in Python.  All comparisons are exact: the plan values are small multiples of 0.25, so
the JSON literals, the tensors and the sums are the same doubles everywhere."""
import json
import os
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_hip_backend, assert_same_state

torch = pytest.importorskip("torch")

import star_networks  # noqa: E402
from test_device_tensors import tensor_device  # noqa: E402
from test_lane_features import twin  # noqa: E402

NAN = float("nan")


# ----------------------------------------------------------------------------------------------------------------- helpers
def derive(cfg, tag, roadnet=None, **overrides):
    """A copy of config `cfg` beside it, with `overrides` and, if given, the roadnet dict written to a file of its own."""
    with open(cfg) as f:
        c = json.load(f)
    if roadnet is not None:
        c["roadnetFile"] = "roadnet_%s.json" % tag
        with open(os.path.join(c["dir"], c["roadnetFile"]), "w") as f:
            json.dump(roadnet, f)
    c.update(overrides)
    path = cfg[:-5] + "_" + tag + ".json"
    with open(path, "w") as f:
        json.dump(c, f)
    return path


def roadnet_of(cfg):
    with open(cfg) as f:
        c = json.load(f)
    with open(os.path.join(c["dir"], c["roadnetFile"])) as f:
        return json.load(f)


def network(scen, workdir, name, layout="auto", **config):
    """Config of example_1x1 / grid_6x6 / star3 / star5 on the given layout ("auto" or "dense")."""
    if name.startswith("star"):
        cfg = star_networks.make(workdir, name, layout=layout)
        tag = "tlplan_" + "_".join("%s-%s" % (k, config[k]) for k in sorted(config))
        return derive(cfg, tag, **config) if config else cfg
    if layout == "dense":
        config["cfx"] = {"layout": "dense"}
    return scen.materialize(name, workdir, **config)


class Plan:
    """The signal plan of a config's roadnet file in the engine's intersection order, from the JSON alone."""

    def __init__(self, eng, cfg):
        self.cfg = cfg
        self.ids = eng.intersection_ids()
        by_id = {it["id"]: it for it in roadnet_of(cfg)["intersections"]}
        self.times = [None if by_id[i]["virtual"] else [float(ph["time"]) for ph in by_id[i]["trafficLight"]["lightphases"]]
                      for i in self.ids]
        self.I = len(self.ids)
        self.P = max(len(t) for t in self.times if t is not None)
        self.real = [i for i, t in enumerate(self.times) if t is not None]
        self.count = [0 if t is None else len(t) for t in self.times]
        self.big = max(self.real, key=lambda i: self.count[i])    # the signalised intersections with the most ...
        self.small = min(self.real, key=lambda i: self.count[i])  # ... and the fewest phases

    def file(self):
        """[I, P] as the getter shows the file's plan: 0.0 in the padding and at virtual intersections."""
        T = np.zeros((self.I, self.P))
        for i in self.real:
            T[i, :self.count[i]] = self.times[i]
        return T

    def other(self, k=0):
        """Another plan, [I, P] as the getter would show it: 3 to 15 s in steps of 1.5."""
        T = np.zeros((self.I, self.P))
        for i in self.real:
            for p in range(self.count[i]):
                T[i, p] = 3.0 + ((7 * i + 3 * p + 5 * k) % 9) * 1.5
        return T

    def dirty(self, T):
        """T with values no plan may hold wherever the call must not look: the padding and the virtual rows."""
        D = np.array(T, dtype=np.float64)
        for i in range(self.I):
            if self.count[i] == 0:
                D[i, :] = (-1.0, np.inf, NAN)[i % 3]
            else:
                D[i, self.count[i]:] = -5.0
        return D

    def built(self, T, tag, **overrides):
        """A config whose roadnet file carries plan T."""
        net = roadnet_of(self.cfg)
        by_id = {it["id"]: it for it in net["intersections"]}
        for i in self.real:
            for p, ph in enumerate(by_id[self.ids[i]]["trafficLight"]["lightphases"]):
                ph["time"] = float(T[i, p])
        return derive(self.cfg, tag, roadnet=net, **overrides)


def dev(eng, a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(tensor_device(eng))


def lights(eng):
    ph, rem = eng._tl_state()
    return np.array(ph), np.array(rem)


def same_lights(a, b, where):
    (pa, ra), (pb, rb) = lights(a), lights(b)
    assert np.array_equal(pa, pb), "%s: phases differ" % where
    assert np.array_equal(ra, rb), "%s: remaining times differ" % where


def run_equal(engines, steps, where, every=25):
    """Step all engines together: the lights equal on every step, the whole state every `every` steps and at the end."""
    changed = False
    first = lights(engines[0])[0]
    for s in range(steps):
        for e in engines:
            e.next_step()
        for e in engines[1:]:
            same_lights(engines[0], e, "%s, step %d" % (where, s))
        changed = changed or not np.array_equal(lights(engines[0])[0], first)
        if s % every == every - 1 or s == steps - 1:
            for e in engines[1:]:
                assert_same_state(engines[0], e, "%s, step %d" % (where, s))
    assert changed, where + ": no light ever changed its phase"
    assert engines[0].get_vehicle_count() > 0, where + ": no vehicle ran"


def durations_of(eng):
    """The getter, three ways, all equal: the array call, a new tensor, a pre-filled `out`."""
    got = eng.get_tl_phase_durations_array()
    t = eng.get_tl_phase_durations_tensor()
    assert t.dtype == torch.float64 and np.array_equal(t.cpu().numpy(), got)
    out = torch.full(tuple(got.shape), -7.0, dtype=torch.float64, device=tensor_device(eng))  # (every element must be written)
    assert eng.get_tl_phase_durations_tensor(out=out) is out
    assert np.array_equal(out.cpu().numpy(), got)
    return got


def on_device(eng):
    """The plan is state only the device library keeps.  Where the CPU twin stands in for it (the shadow run of the GPU tests,
    conftest.py) there is nothing to run; on the HIP library this never skips, with or without the new entry points."""
    if not eng._device_buffers():
        pytest.skip("the signal plan as engine state needs the device library: the twin has no such calls")
    return eng


LAYOUTS = ["auto", "dense"]
NETS = ["example_1x1", "star3", "star5"]


# ----------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("net", NETS)
def test_built_equals_set_at_step_0(mod, scen, workdir, net, layout):
    cfg = network(scen, workdir, net, layout)
    by_remain, by_reset = on_device(mod.Engine(cfg, 1)), mod.Engine(cfg, 1)
    plan = Plan(by_remain, cfg)
    T = plan.other()
    assert not np.array_equal(T, plan.file())
    built = mod.Engine(plan.built(T, "built0_" + layout), 1)
    assert_hip_backend(by_remain)
    if built._device_buffers():
        assert built._layout() == ("ring" if layout == "auto" else "dense")
    by_remain.set_tl_plan_tensor(durations=dev(by_remain, plan.dirty(T)), phase_remain=dev(by_remain, plan.dirty(T)[:, 0]))
    by_reset.set_tl_plan_tensor(durations=dev(by_reset, plan.dirty(T)))
    by_reset.reset()
    for e in (by_remain, by_reset):
        e.sync()
        assert np.array_equal(durations_of(e), T)
        same_lights(built, e, "before the first step")
    run_equal([built, by_remain, by_reset], 150, "%s %s" % (net, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("net", NETS)
def test_built_equals_set_mid_run(mod, scen, workdir, net, layout):
    cfg = network(scen, workdir, net, layout)
    b = on_device(mod.Engine(cfg, 1))
    plan = Plan(b, cfg)
    T = plan.other(1)
    a = mod.Engine(plan.built(T, "builtmid_" + layout), 1)
    for s in range(60):
        b.next_step()
    arch = b.snapshot()
    a.load(arch)
    b.load(arch)  # (both go on from the archive, so both number their vehicles alike)
    b.set_tl_plan_tensor(durations=dev(b, plan.dirty(T)))
    same_lights(a, b, "after the load")  # (the running phase keeps the remaining time the file's plan gave it)
    assert np.array_equal(durations_of(b), T)
    run_equal([a, b], 150, "%s %s mid-run" % (net, layout))


def pass_time(phase, remain, T, count, interval):
    """TrafficLight::passTime for every signalised intersection, on numpy rows."""
    for i, n in enumerate(count):
        if n == 0:
            continue
        rem, ph = remain[i] - interval, phase[i]
        while rem <= 0.0:
            ph = (ph + 1) % n
            rem += T[i, ph]
        remain[i], phase[i] = rem, ph


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("interval", [1.0, 0.5])
def test_lights_equal_pass_time_restated(mod, scen, workdir, layout, interval):
    cfg = network(scen, workdir, "star5", layout, interval=interval)
    eng = on_device(mod.Engine(cfg, 1))
    plan = Plan(eng, cfg)
    assert len(set(plan.count[i] for i in plan.real)) >= 2, "the rows are not ragged"
    # zero-length phases (skipped), phases shorter than the interval (several hops in one step), and ordinary ones
    T = plan.file()
    c, small = plan.big, plan.small
    assert plan.count[c] == 10 and plan.count[small] == 2 and len(plan.real) == 2
    T[c, :10] = (0.0, 0.25, 4.0, 0.25, 0.0, 0.0, 2.5, 0.25, 0.25, 7.0)
    T[small, :2] = (0.25, 1.0)
    phase, remain = lights(eng)
    phase, remain = phase.astype(np.int64), remain.astype(np.float64)
    want_phase = np.full(plan.I, -1, dtype=np.int64)
    want_remain = np.full(plan.I, NAN)
    want_phase[c], want_remain[c] = 3, 0.75  # an offset at one intersection; -1 / NaN keep the other's
    eng.set_tl_plan_tensor(durations=dev(eng, T), phase=dev(eng, want_phase), phase_remain=dev(eng, want_remain))
    phase[c], remain[c] = 3, 0.75
    hops = 0
    for s in range(300):
        if s == 100:  # mid-run: some durations kept (NaN), a phase offset alone, a remaining time alone
            change = np.full_like(T, NAN)
            change[c, 2] = 0.5
            T[c, 2] = 0.5
            eng.set_tl_plan_tensor(durations=dev(eng, change))
        if s == 150:
            only = np.full(plan.I, -1, dtype=np.int32)
            only[c] = 6
            eng.set_tl_plan_tensor(phase=dev(eng, only))
            phase[c] = 6
        if s == 200:
            only = np.full(plan.I, NAN)
            only[small] = 0.0
            eng.set_tl_plan_tensor(phase_remain=dev(eng, only))
            remain[small] = 0.0
        before = phase.copy()
        eng.next_step()
        pass_time(phase, remain, T, plan.count, interval)
        hops += int(sum((phase[i] - before[i]) % plan.count[i] > 1 for i in plan.real))
        got_phase, got_remain = lights(eng)
        assert np.array_equal(got_phase[plan.real], phase[plan.real]), "phases differ at step %d" % s
        assert np.array_equal(got_remain[plan.real], remain[plan.real]), "remaining times differ at step %d" % s
    # (the big intersection's cycle is at most 14.5 s and crosses its zero-length phases twice, 3 -> 6 and 9 -> 1: 300 steps of
    # 0.5 s are ten cycles, so twenty such steps at the very least, whatever the small one adds)
    assert hops >= 20, "hardly a step took a light across more than one phase (%d)" % hops
    assert np.array_equal(durations_of(eng), T)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_reset_keeps_the_plan_and_restore_brings_the_files_back(mod, scen, workdir, layout):
    cfg = network(scen, workdir, "star5", layout)
    eng, fresh = on_device(mod.Engine(cfg, 1)), mod.Engine(cfg, 1)
    plan = Plan(eng, cfg)
    T = plan.other(2)
    assert np.array_equal(durations_of(eng), plan.file())
    eng.set_tl_plan(durations=plan.dirty(T))  # (the numpy form)
    for s in range(40):
        eng.next_step()
    eng.reset(True)
    assert np.array_equal(durations_of(eng), T), "reset() changed the durations in force"
    phase, remain = lights(eng)
    assert not phase.any() and np.array_equal(remain[plan.real], T[plan.real, 0])
    for s in range(40):
        eng.next_step()
    before = lights(eng)
    eng.restore_tl_plan()
    assert np.array_equal(durations_of(eng), plan.file())
    after = lights(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "restore_tl_plan() touched the lights"
    eng.reset(True)
    run_equal([fresh, eng], 100, "after restore_tl_plan %s" % layout)


def one_plan_per_environment(vec, singles, plan, plans, steps=120, every_step=None):
    """The batched engine GIVEN plans[r] in environment r at step 0 against singles[r] BUILT with it (vec = an Engine: one
    plan, one single; vec = None: the singles alone, for what the test needs of them).  Lights and lane counts every 10
    steps, every vehicle's speed at the end; every_step(s, singles), if given, is called after every step.  Returns the
    environments' phases at the compared steps, [compared, R, I], from the singles."""
    R = len(singles)
    batched = vec is not None and len(vec._tensor_shapes()[1]) == 2
    rows = (lambda a: np.asarray(a)) if batched else (lambda a: np.asarray(a)[None])
    if vec is not None:
        stacked = np.stack([plan.dirty(T) for T in plans])
        if not batched:
            stacked = stacked[0]
        vec.set_tl_plan_tensor(durations=dev(vec, stacked), phase_remain=dev(vec, stacked[..., 0]))
        assert np.array_equal(rows(durations_of(vec)), np.stack(plans))
    seen = []
    for s in range(steps):
        if vec is not None:
            vec.next_step()
        for e in singles:
            e.next_step()
        if every_step is not None:
            every_step(s, singles)
        if s % 10 != 9:
            continue
        seen.append(np.stack([lights(e)[0] for e in singles]))
        if vec is None:
            continue
        ph, rem = [rows(a) for a in vec._tl_state()]
        counts = rows(vec.get_lane_vehicle_count_array())
        for r, e in enumerate(singles):
            p1, r1 = lights(e)
            assert np.array_equal(ph[r], p1) and np.array_equal(rem[r], r1), "env %d: lights differ at step %d" % (r, s)
            assert np.array_equal(counts[r], e.get_lane_vehicle_count_array()), "env %d: lane counts differ at step %d" % (r, s)
    if vec is not None:
        for r, e in enumerate(singles):
            got = vec.get_vehicle_speed(r) if batched else vec.get_vehicle_speed()
            assert got == e.get_vehicle_speed(), "env %d: vehicle speeds differ" % r
    assert R == 1 or any(not np.array_equal(ph[r], ph[r + 1]) for ph in seen for r in range(R - 1)), "the environments' lights never differed"
    return np.stack(seen)


@pytest.mark.gpu
def test_vector_engine_one_plan_per_environment(mod, scen, workdir):
    R = 3
    cfg = scen.materialize("grid_6x6", workdir)
    vec = on_device(mod.VectorEngine(cfg, R))
    probe = mod.Engine(cfg, 1)
    plan = Plan(probe, cfg)
    plans = [plan.other(k) for k in range(R)]
    assert not np.array_equal(plans[0], plans[1]) and not np.array_equal(plans[1], plans[2])
    singles = [mod.Engine(plan.built(plans[r], "env%d" % r, seed=r), 1) for r in range(R)]
    vec.track_trips(True)
    ph = one_plan_per_environment(vec, singles, plan, plans)[-1]
    att = vec.get_average_travel_time_tensor().cpu().numpy()
    want = np.array([e.get_average_travel_time() for e in singles])
    assert np.array_equal(att, want), (att, want)
    assert want.min() > 0.0
    assert not np.array_equal(ph[0], ph[1]) and not np.array_equal(ph[1], ph[2]), "the environments' lights never differed"


def rejections(plan, T_now, interval):
    """(name, kwargs as numpy arrays, the words the error must hold).  One invalid entry each, among valid rows."""
    c, first = plan.big, plan.small
    assert c != first and plan.count[c] > 2 and plan.count[first] == 2
    ids = plan.ids
    out = []
    d = plan.dirty(plan.other(3))
    d[c, 2] = -0.5
    out.append(("negative duration", dict(durations=d, phase=np.zeros(plan.I, dtype=np.int64)),
                ("durations", "'%s'" % ids[c], "phase 2")))
    d = plan.dirty(plan.other(3))
    d[first, 1] = np.inf
    out.append(("infinite duration", dict(durations=d, phase_remain=np.full(plan.I, 1.0)), ("durations", "'%s'" % ids[first], "phase 1")))
    d = plan.dirty(plan.other(3))
    d[c, :plan.count[c]] = 0.0
    d[c, 1] = interval / 2
    out.append(("sum below the interval", dict(durations=d), ("durations", "'%s'" % ids[c], "sum")))
    # NaN keeps leave the old entries in the sum: phase 0 in force (T_now[c, 0] < interval) and zeros elsewhere
    d = plan.dirty(plan.other(3))
    d[c, :plan.count[c]] = 0.0
    d[c, 0] = NAN
    assert T_now[c, 0] < interval
    out.append(("sum below the interval with a kept entry", dict(durations=d), ("durations", "'%s'" % ids[c], "sum")))
    p = np.full(plan.I, -1, dtype=np.int32)
    p[first] = 1
    p[c] = plan.count[c]
    out.append(("phase == P_i", dict(phase=p, durations=plan.dirty(plan.other(3))), ("phase", "'%s'" % ids[c], str(plan.count[c]))))
    r = np.full(plan.I, NAN)
    r[first] = 2.0
    r[c] = -0.25
    out.append(("negative phase_remain", dict(phase_remain=r, phase=np.zeros(plan.I, dtype=np.int32)),
                ("phase_remain", "'%s'" % ids[c], "-0.25")))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_an_invalid_entry_rejects_the_whole_call(mod, scen, workdir, layout):
    cfg = network(scen, workdir, "star5", layout)
    eng, untouched = on_device(mod.Engine(cfg, 1)), mod.Engine(cfg, 1)
    plan = Plan(eng, cfg)
    c = plan.big
    base = plan.file()
    base[c, 0] = 0.25  # (a valid plan with a phase shorter than the interval, given to both engines)
    for e in (eng, untouched):
        e.set_tl_plan(durations=base)
    for s in range(30):
        eng.next_step()
        untouched.next_step()
    for name, kwargs, words in rejections(plan, base, 1.0):
        before = lights(eng)
        eng.set_tl_plan_tensor(**{k: dev(eng, v) for k, v in kwargs.items()})
        with pytest.raises(ValueError) as err:
            eng.sync()
        msg = str(err.value)
        for w in words + ("not applied",):
            assert w in msg, "%s: %r lacks %r" % (name, msg, w)
        eng.sync()  # (the record was read: nothing is raised twice)
        assert np.array_equal(durations_of(eng), base), name + ": durations changed"
        after = lights(eng)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), name + ": the lights changed"
        with pytest.raises(ValueError):  # the numpy form raises at once, and applies as little
            eng.set_tl_plan(**kwargs)
        assert np.array_equal(durations_of(eng), base), name + ": durations changed (numpy form)"
        # the next valid call applies (and is taken back before a light could read it)
        probe = np.full_like(base, NAN)
        probe[c, 1] = 99.0
        eng.set_tl_plan_tensor(durations=dev(eng, probe))
        eng.sync()
        assert durations_of(eng)[c, 1] == 99.0, name + ": the next valid call did not apply"
        eng.set_tl_plan_tensor(durations=dev(eng, base))
        for s in range(5):
            eng.next_step()
            untouched.next_step()
        assert_same_state(eng, untouched, "after " + name)
    assert eng.get_vehicle_count() > 0


@pytest.mark.gpu
def test_a_rejection_names_the_env_on_a_vector_engine(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    vec = on_device(mod.VectorEngine(cfg, 3))
    plan = Plan(mod.Engine(cfg, 1), cfg)
    base = np.stack([plan.file()] * 3)
    d = np.stack([plan.other(k) for k in range(3)])
    i = plan.real[5]
    d[2, i, 3] = -1.0
    vec.set_tl_plan_tensor(durations=dev(vec, d))
    with pytest.raises(ValueError) as err:
        vec.sync()
    for w in ("durations", "'%s'" % plan.ids[i], "phase 3", "env 2", "not applied"):
        assert w in str(err.value), str(err.value)
    assert np.array_equal(durations_of(vec), base)
    p = np.full((3, plan.I), -1, dtype=np.int64)
    p[1, i] = 2 ** 40  # (beyond int32: stays invalid instead of wrapping into range)
    vec.set_tl_plan_tensor(phase=dev(vec, p))
    with pytest.raises(ValueError) as err:
        vec.get_lane_vehicle_count_array()  # (any call that waits for the device)
    for w in ("phase", "'%s'" % plan.ids[i], "env 1", "not applied"):
        assert w in str(err.value), str(err.value)
    assert not vec._tl_state()[0].any()


@pytest.mark.gpu
def test_padding_and_virtual_rows_are_ignored(mod, scen, workdir):
    cfg = network(scen, workdir, "star5")
    eng = on_device(mod.Engine(cfg, 1))
    plan = Plan(eng, cfg)
    virtual = [i for i in range(plan.I) if plan.count[i] == 0]
    assert virtual and min(plan.count[i] for i in plan.real) < plan.P
    T = plan.other(4)
    phase = np.zeros(plan.I, dtype=np.int32)
    remain = np.array(T[:, 0])
    phase[virtual] = 99
    remain[virtual] = -3.0
    before = lights(eng)
    eng.set_tl_plan_tensor(durations=dev(eng, plan.dirty(T)), phase=dev(eng, phase), phase_remain=dev(eng, remain))
    eng.sync()  # (nothing to raise)
    got = durations_of(eng)
    assert np.array_equal(got, T)
    assert not got[virtual].any() and all(not got[i, plan.count[i]:].any() for i in plan.real)
    after = lights(eng)
    assert np.array_equal(after[0][virtual], before[0][virtual]) and np.array_equal(after[1][virtual], before[1][virtual])
    assert np.array_equal(after[1][plan.real], T[plan.real, 0])


@pytest.mark.gpu
def test_plan_from_a_side_stream_without_a_host_wait(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng, ref = on_device(mod.Engine(cfg, 1)), mod.Engine(cfg, 1)
    plan = Plan(ref, cfg)
    for s in range(20):  # warm: rings built, tables uploaded
        eng.next_step()
        ref.next_step()
    T = plan.other(5)
    half = dev(eng, T / 2)
    out = torch.full((plan.I, plan.P), -7.0, dtype=torch.float64, device=tensor_device(eng))
    remain = torch.empty(plan.I, dtype=torch.float64, device=tensor_device(eng))
    eng.get_tl_phase_durations_tensor(out=out)
    eng.observe_intersections_tensor(phase_remain=remain)
    eng.sync()
    device = tensor_device(eng)
    torch.cuda.synchronize(device)
    side = torch.cuda.Stream(device=device)
    with torch.cuda.stream(side):  # (torch loads a kernel's code at its first launch and waits for the device to do so: not timed)
        warm = (half + half)[:, 0].contiguous()
        del warm
    side.synchronize()
    eng._device_spin(200000)  # 200 ms of device work in front of everything below
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        made = half + half  # the plan is the output of torch ops on `side`, handed over as it is
        eng.set_tl_plan_tensor(durations=made, phase_remain=made[:, 0].contiguous())
        del made  # (its memory may be handed out again by work enqueued on `side` from here on)
        scribble = torch.full((plan.I, plan.P), -1.0, dtype=torch.float64, device=device)
        eng.next_step()
        eng.get_tl_phase_durations_tensor(out=out)
        eng.observe_intersections_tensor(phase_remain=remain)
    elapsed = time.perf_counter() - t0
    assert elapsed < 0.1, "the calls waited for the device (%.1f ms behind a 200 ms spin)" % (elapsed * 1e3)
    side.synchronize()
    eng.sync()
    assert bool((scribble == -1.0).all())
    ref.set_tl_plan(durations=T, phase_remain=T[:, 0])
    ref.next_step()
    assert np.array_equal(out.cpu().numpy(), T)
    assert np.array_equal(remain.cpu().numpy(), lights(ref)[1])
    run_equal([ref, eng], 60, "after the unsynchronised calls")


@pytest.mark.gpu
def test_with_rl_traffic_light_the_plan_serves_reset(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    eng = on_device(mod.Engine(cfg, 1))
    plan = Plan(eng, cfg)
    T = plan.other(6)
    start = lights(eng)
    eng.set_tl_plan_tensor(durations=dev(eng, T))
    assert np.array_equal(durations_of(eng), T)
    for s in range(30):
        eng.next_step()
    now = lights(eng)
    assert np.array_equal(now[0], start[0]) and np.array_equal(now[1], start[1]), "the lights advanced under rlTrafficLight"
    eng.reset()
    assert np.array_equal(lights(eng)[1][plan.real], T[plan.real, 0])
    assert np.array_equal(durations_of(eng), T)
    # the phase part does not need set_tl_phases_tensor's permission, and shows where phases are read
    x = plan.real[3]
    eng.set_tl_phase(plan.ids[x], 0)
    assert lights(eng)[0][x] == 0
    p = np.full(plan.I, -1, dtype=np.int32)
    p[x] = 2
    eng.set_tl_plan_tensor(phase=dev(eng, p))
    assert eng.get_tl_phases_tensor().cpu().numpy()[x] == 2
    eng.set_tl_phase(plan.ids[x], 0)  # (the host's record of that light was forgotten: this set is sent, not taken for a repeat)
    assert lights(eng)[0][x] == 0


@pytest.mark.gpu
def test_built_equals_set_with_lane_change(mod, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir, laneChange=True)
    given = on_device(mod.Engine(cfg, 1))
    assert given._layout() == "dense"
    plan = Plan(given, cfg)
    T = plan.other(7)
    built = mod.Engine(plan.built(T, "lanechange"), 1)
    given.set_tl_plan_tensor(durations=dev(given, T), phase_remain=dev(given, T[:, 0]))
    run_equal([built, given], 150, "lane change")


# ----------------------------------------------------------------------------------------------------------------- CPU (twin)
def test_argument_errors_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = twin(mod, cfg)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    plan = Plan(eng, cfg)
    I, P = plan.I, plan.P
    assert (P,) == tuple(eng._intersection_dims()[1:])
    good = {"durations": torch.zeros((I, P), dtype=torch.float64), "phase": torch.zeros(I, dtype=torch.int32),
            "phase_remain": torch.zeros(I, dtype=torch.float64)}
    with pytest.raises(ValueError):
        eng.set_tl_plan_tensor()
    with pytest.raises(ValueError):
        eng.set_tl_plan()
    for name, t in good.items():
        with pytest.raises(TypeError):  # not a tensor
            eng.set_tl_plan_tensor(**{name: t.numpy()})
        with pytest.raises(TypeError):  # wrong device (the twin's tensors live on the CPU)
            eng.set_tl_plan_tensor(**{name: t.to("meta")})
        with pytest.raises(TypeError):  # wrong dtype
            eng.set_tl_plan_tensor(**{name: t.to(torch.float32)})
        with pytest.raises(ValueError):  # wrong shape
            eng.set_tl_plan_tensor(**{name: torch.cat([t, t])})
        with pytest.raises(ValueError):  # [R, ...] wanted
            vec.set_tl_plan_tensor(**{name: t})
        wide = torch.zeros(tuple(t.shape)[::-1] + (2,), dtype=t.dtype) if t.dim() == 1 else torch.zeros((P, I), dtype=t.dtype).t()
        noncontig = wide[:, 0] if t.dim() == 1 else wide
        assert tuple(noncontig.shape) == tuple(t.shape) and not noncontig.is_contiguous()
        with pytest.raises(ValueError):
            eng.set_tl_plan_tensor(**{name: noncontig})
        # a later argument that is wrong: still an argument error, not the missing backend call
        other = "phase" if name != "phase" else "durations"
        with pytest.raises(ValueError):
            eng.set_tl_plan_tensor(**{name: t, other: torch.zeros((3, 3), dtype=good[other].dtype)})
    with pytest.raises(TypeError):
        eng.set_tl_plan_tensor(phase=torch.zeros(I, dtype=torch.bool))
    with pytest.raises(TypeError):
        eng.get_tl_phase_durations_tensor(out=torch.zeros((I, P), dtype=torch.float32))
    with pytest.raises(ValueError):
        eng.get_tl_phase_durations_tensor(out=torch.zeros((I, P + 1), dtype=torch.float64))
    with pytest.raises(ValueError):
        vec.get_tl_phase_durations_tensor(out=torch.zeros((I, P), dtype=torch.float64))
    with pytest.raises(TypeError):
        eng.set_tl_plan(durations=np.zeros((I, P), dtype=np.int32))
    with pytest.raises(TypeError):
        eng.set_tl_plan(phase=np.zeros(I))
    with pytest.raises(ValueError):
        eng.set_tl_plan(phase_remain=np.zeros(I + 1))


def test_a_backend_without_the_calls_says_so_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    plan = Plan(twin(mod, cfg), cfg)
    I, P = plan.I, plan.P
    for eng, lead in ((twin(mod, cfg), ()), (mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB), (2,))):
        with pytest.raises(NotImplementedError):
            eng.set_tl_plan_tensor(durations=torch.ones(lead + (I, P), dtype=torch.float64), phase=torch.zeros(lead + (I,), dtype=torch.int64),
                                   phase_remain=torch.ones(lead + (I,), dtype=torch.float64))
        with pytest.raises(NotImplementedError):
            eng.set_tl_plan(durations=np.ones(lead + (I, P)))
        with pytest.raises(NotImplementedError):
            eng.get_tl_phase_durations_tensor()
        with pytest.raises(NotImplementedError):
            eng.get_tl_phase_durations_tensor(out=torch.zeros(lead + (I, P), dtype=torch.float64))
        with pytest.raises(NotImplementedError):
            eng.get_tl_phase_durations_array()
        with pytest.raises(NotImplementedError):
            eng.restore_tl_plan()
        for s in range(3):  # (and the engine is none the worse for it)
            eng.next_step()


def test_import_does_not_import_torch():
    import subprocess
    import sys

    from conftest import ROOT
    code = ("import sys, cityflow_amd; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert all(hasattr(c, n) for c in (cityflow_amd.Engine, cityflow_amd.VectorEngine) for n in "
            "('set_tl_plan_tensor', 'get_tl_phase_durations_tensor', 'set_tl_plan', 'get_tl_phase_durations_array', 'restore_tl_plan')); "
            "assert not hasattr(cityflow_amd.TiledEngine, 'set_tl_plan_tensor')")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def vector_equals_singles(vec, singles, steps, where):
    for s in range(steps):
        vec.next_step()
        for e in {id(e): e for e in singles}.values():  # (one engine may stand for several environments)
            e.next_step()
    counts = vec.get_lane_vehicle_count_array()
    for r, e in enumerate(singles):
        assert np.array_equal(counts[r], e.get_lane_vehicle_count_array()), "%s: env %d lane counts" % (where, r)
        assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "%s: env %d vehicle speeds" % (where, r)
    assert counts.sum() > 0


def test_vector_engine_seeds_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    s = 7
    vec = mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB, seeds=[s, s, s])
    single = [twin(mod, scen.materialize("grid_6x6", workdir, seed=s))]
    vector_equals_singles(vec, single * 3, 80, "equal seeds")
    counts = vec.get_lane_vehicle_count_array()
    assert np.array_equal(counts[0], counts[1]) and np.array_equal(counts[0], counts[2])
    # reset(seed=True) reseeds every environment with ITS seed
    vec.reset(True)
    single[0].reset(True)
    vector_equals_singles(vec, single * 3, 40, "equal seeds after reset")
    # different seeds, in an order seed + r could not give
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB, seeds=[9, 4])
    vector_equals_singles(vec, [twin(mod, scen.materialize("grid_6x6", workdir, seed=x)) for x in (9, 4)], 60, "seeds 9, 4")
    # None is today's seed + r
    default, none = mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB), mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB, None)
    singles = [twin(mod, scen.materialize("grid_6x6", workdir, seed=r)) for r in range(3)]
    for step in range(60):
        default.next_step()
    vector_equals_singles(none, singles, 60, "seeds=None")
    assert np.array_equal(default.get_lane_vehicle_count_array(), none.get_lane_vehicle_count_array())
    for r in range(3):
        assert default.get_vehicle_speed(r) == none.get_vehicle_speed(r)
    for bad in ([], [1, 2], [1, 2, 3, 4]):
        with pytest.raises(ValueError):
            mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB, seeds=bad)
        with pytest.raises(ValueError):
            mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB, bad)
