"""Per-movement throughput and delay statistics across steps: track_movement_flow / observe_movement_flow_tensor /
observe_movement_flow_array on Engine and VectorEngine (cityflow_amd/torch_io.py; kr_movement_flow / kd_movement_flow /
k_movement_flow_drain on the device, the host tracker of csrc/host/movement_flow.cpp on the twin).

After every step, with s = steps taken and D(v) the drivable (lane or laneLink) vehicle v is on, D'(v) the one before:
  1. D(v) = d != D'(v) = p: since(v) = s, wait(v) = 0, and off the old record
       d laneLink k, p a lane:      entered[k] += 1, entered_lane_steps[k] += s - since_p(v), entered_lane_waiting_steps[k] += wait_p(v)
       d laneLink k, p not a lane:  entered[k] += 1
       d a lane, p another lane:    k = the first laneLink of p's list that ends on d: the three additions and left[k] += 1
  2. v no longer on laneLink k:     left[k] += 1, left_steps[k] += s - since(v), left_waiting_steps[k] += wait(v)
  3. v on a drivable, speed < 0.1:  wait(v) += 1
waiting_steps / max_waiting_steps are the sum / the maximum of wait over the vehicles on the laneLink.  The outputs are the sums
(the maximum) over a roadLink's laneLinks, [I, M].  A baseline (tracking turned on, reset, load) starts every vehicle on a
drivable at since = s, wait = 0 without counting it, with all accumulators zero.

Everything is an integer: every check is array_equal.  The oracle is the small model of these rules below, fed only by
getters that existed before the feature (_vehicle_state()'s vid / drivable / speed, or the reference's get_lane_vehicles +
get_vehicle_speed + get_vehicle_info, and _flat_net()'s laneLink tables) — never by the feature's own arrays or
intersection_layout()."""
import collections
import json
import os

import numpy as np
import pytest

import star_networks
from conftest import SHADOW_GPU, TWIN_LIB, assert_hip_backend

torch = pytest.importorskip("torch")

from test_device_tensors import tensor_device  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_lane_flow import drain_plan, hip_engine, layout_config  # noqa: E402

NAMES = ("entered", "entered_lane_steps", "entered_lane_waiting_steps", "left", "left_steps", "left_waiting_steps", "waiting_steps",
         "max_waiting_steps")
ACCUMULATED = NAMES[:6]
DTYPES = {k: np.int32 if k in ("entered", "left", "max_waiting_steps") else np.int64 for k in NAMES}
NARROW4 = dict(arms=4, lanes=[1, 2, 1, 2], lengths=[200, 150, 200, 120], width=4, mid=False)


# ------------------------------------------------------------------------------------------------------------------ oracle
class Model:
    """The rules over {vehicle: drivable} and {vehicle: speed}; lanes are drivables [0, L), laneLink k is L + k."""

    def __init__(self, net, n_inters):
        self.L = len(net["lane_ll_start"]) - 1
        self.lane_ll_start, self.lane_ll, self.ll_end = net["lane_ll_start"], net["lane_ll"], net["ll_end_lane"]
        self.ll_inter, self.ll_roadlink = net["ll_inter"].astype(np.int64), net["ll_roadlink"].astype(np.int64)
        self.K = len(self.ll_end)
        self.shape = (n_inters, int(self.ll_roadlink.max()) + 1)
        self.rec = {}  # vehicle -> [drivable, since, wait]
        self.acc = {k: np.zeros(self.K, dtype=np.int64) for k in ACCUMULATED}
        # what a run must have looked at
        self.skips = 0
        self.refills = 0
        self._filled = [0] * self.K  # 0 never held a vehicle, 1 holds some, 2 held some and is empty

    def baseline(self, now, s):
        self.rec = {v: [d, s, 0] for v, d in now.items()}
        for a in self.acc.values():
            a[:] = 0

    def tick(self, now, speed, s):
        L, acc, new = self.L, self.acc, {}
        for v, d in now.items():
            r = self.rec.get(v)
            if r is not None and r[0] == d:
                new[v] = r
                continue
            p = r[0] if r is not None else -1
            k = -1
            if d >= L:
                k = d - L
                acc["entered"][k] += 1
            elif 0 <= p < L:
                for q in self.lane_ll[self.lane_ll_start[p]:self.lane_ll_start[p + 1]]:
                    if self.ll_end[q] == d:
                        k = int(q)
                        acc["entered"][k] += 1
                        acc["left"][k] += 1
                        self.skips += 1
                        break
            if k >= 0 and 0 <= p < L:
                acc["entered_lane_steps"][k] += s - r[1]
                acc["entered_lane_waiting_steps"][k] += r[2]
            new[v] = [d, s, 0]
        for v, r in self.rec.items():
            if r[0] >= L and now.get(v) != r[0]:
                acc["left"][r[0] - L] += 1
                acc["left_steps"][r[0] - L] += s - r[1]
                acc["left_waiting_steps"][r[0] - L] += r[2]
        for v, r in new.items():
            if speed[v] < 0.1:
                r[2] += 1
        self.rec = new
        held = np.zeros(self.K, dtype=bool)
        for r in new.values():
            if r[0] >= L:
                held[r[0] - L] = True
        for k in range(self.K):
            if held[k]:
                self.refills += self._filled[k] == 2
                self._filled[k] = 1
            elif self._filled[k] == 1:
                self._filled[k] = 2

    def _rows(self, per_link, how=np.add):
        out = np.zeros(self.shape, dtype=np.int64)
        how.at(out, (self.ll_inter, self.ll_roadlink), per_link)
        return out

    def outputs(self):
        o = {k: self._rows(a).astype(DTYPES[k]) for k, a in self.acc.items()}
        w, m = np.zeros(self.K, dtype=np.int64), np.zeros(self.K, dtype=np.int64)
        for r in self.rec.values():
            if r[0] >= self.L:
                w[r[0] - self.L] += r[2]
                m[r[0] - self.L] = max(m[r[0] - self.L], r[2])
        o["waiting_steps"] = self._rows(w)
        o["max_waiting_steps"] = self._rows(m, np.maximum).astype(np.int32)
        return o

    def drain(self, reset):
        o = self.outputs()
        if reset:
            for a in self.acc.values():
                a[:] = 0
        return o


def own_feed(eng):
    """-> a call giving ({vid: drivable}, {vid: speed}) of `eng` now, from _vehicle_state()."""
    def feed():
        st = eng._vehicle_state()
        vid = [int(v) for v in st["vid"]]
        return dict(zip(vid, (int(d) for d in st["drivable"]))), dict(zip(vid, (float(x) for x in st["speed"])))
    return feed


def reference_feed(ref, eng):
    """... of the reference in lockstep: get_lane_vehicles + get_vehicle_speed, and get_vehicle_info(v)["drivable"] for the
    running vehicles on no lane (the reference's laneLink id is <start lane>_TO_<end lane>)."""
    net, lanes = eng._flat_net(), list(eng.lane_ids())
    lane_of = {lane: l for l, lane in enumerate(lanes)}
    link_of = {"%s_TO_%s" % (lanes[a], lanes[b]): len(lanes) + k for k, (a, b) in enumerate(zip(net["ll_start_lane"], net["ll_end_lane"]))}
    assert len(link_of) == len(net["ll_end_lane"])

    def feed():
        now = {v: lane_of[lane] for lane, vs in ref.get_lane_vehicles().items() for v in vs}
        speed = ref.get_vehicle_speed()
        for v in speed:
            if v not in now:
                now[v] = link_of[ref.get_vehicle_info(v)["drivable"]]
        return now, speed
    return feed


def empty_outputs(eng, lead=()):
    shape = lead + (len(eng.intersection_ids()), eng._intersection_dims()[0])
    # (filled with a value no output takes: every element must be written)
    return {k: torch.full(shape, -7, dtype=torch.int64 if DTYPES[k] is np.int64 else torch.int32, device=tensor_device(eng)) for k in NAMES}


def check_drain(eng, want_peek, want, reset, where):
    """The array call without a reset, then the tensor call with `reset`; both against the model.  Returns what the engine gave."""
    got = eng.observe_movement_flow_array()
    assert sorted(got) == sorted(NAMES)
    for k in NAMES:
        assert got[k].dtype == DTYPES[k] and got[k].shape == want_peek[k].shape, "%s: %s is %s %s" % (where, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want_peek[k]), "%s: %s differs (array call)" % (where, k)
    t = empty_outputs(eng)
    eng.observe_movement_flow_tensor(reset=reset, **t)
    for k in NAMES:
        assert np.array_equal(t[k].cpu().numpy(), want[k]), "%s: %s differs (tensor call, reset=%s)" % (where, k, reset)
    return {k: t[k].cpu().numpy() for k in NAMES}  # (the engine's own values: the identities are checked on them)


def assert_no_route_ends_on_a_feeding_lane(eng, cfg, net):
    """What the identity against the lane tracker rests on: a vehicle leaves a lane that has laneLinks only into one of them."""
    c = json.load(open(cfg))
    flows = json.load(open(os.path.join(c["dir"], c["flowFile"])))
    feeding = np.diff(net["lane_ll_start"]) > 0
    roads = {lane.rsplit("_", 1)[0] for lane, f in zip(eng.lane_ids(), feeding) if f}
    assert flows and roads
    for f in flows:
        assert f["route"][-1] not in roads, f["route"]


class Identities:
    """At every drain, on the engine's own values: per roadLink, sum entered - sum left == movement_inside now - at the baseline;
    per intersection, with track_lane_flow on from the same baseline (never reset): sum_m entered == sum of the lane tracker's
    left over the lanes with a laneLink into it, likewise the lane steps and the lane waiting steps."""

    def __init__(self, eng, cfg, net):
        assert_no_route_ends_on_a_feeding_lane(eng, cfg, net)
        self.inside0 = eng.observe_intersections_array()["movement_inside"].astype(np.int64)
        self.tot = {k: np.zeros(self.inside0.shape, dtype=np.int64) for k in ACCUMULATED}
        feeding = np.diff(net["lane_ll_start"]) > 0
        self.lanes = np.nonzero(feeding)[0]
        self.inter = net["ll_inter"][net["lane_ll"][net["lane_ll_start"][:-1][feeding]]].astype(np.int64)

    def _per_inter(self, per_lane):
        out = np.zeros(self.inside0.shape[0], dtype=np.int64)
        np.add.at(out, self.inter, per_lane[self.lanes])
        return out

    def drained(self, eng, out, reset, where):
        cum = {k: self.tot[k] + out[k] for k in ACCUMULATED}
        inside = eng.observe_intersections_array()["movement_inside"].astype(np.int64)
        assert np.array_equal(cum["entered"] - cum["left"], inside - self.inside0), where + ": entered - left != change of movement_inside"
        lane = eng.observe_lane_flow_array()
        for mine, theirs in (("entered", "left"), ("entered_lane_steps", "left_steps"), ("entered_lane_waiting_steps", "left_waiting_steps")):
            assert np.array_equal(cum[mine].sum(axis=1), self._per_inter(lane[theirs])), "%s: %s against the lane tracker's %s" % (where, mine, theirs)
        if reset:
            self.tot = cum


def run_against_model(eng, feed, cfg, steps, where):
    """-> (model, {output: its sum over all drains' engine values}, the largest max_waiting_steps seen at a drain)"""
    net = eng._flat_net()
    eng.track_movement_flow(True)
    eng.track_lane_flow(True)
    assert eng.movement_flow_tracking()
    model = Model(net, len(eng.intersection_ids()))
    model.baseline(feed()[0], 0)
    ident = Identities(eng, cfg, net)
    plan, kinds = drain_plan(steps), set()
    total, largest = {k: 0 for k in ACCUMULATED}, 0
    for s in range(steps):
        eng.next_step()
        model.tick(*feed(), s + 1)
        if s in plan:
            at = "%s, step %d" % (where, s)
            peek = model.outputs()
            out = check_drain(eng, peek, model.drain(plan[s]), plan[s], at)
            ident.drained(eng, out, plan[s], at)
            kinds.add(plan[s])
            largest = max(largest, int(out["max_waiting_steps"].max()))
            if plan[s] or s == steps - 1:
                for k in ACCUMULATED:
                    total[k] += int(out[k].sum())
    assert kinds == {True, False}, "drains of both kinds are needed: %s" % kinds
    return model, total, largest


def lockstep(eng, ref):
    """feed() of the reference that also steps it: called once per step of `eng`, and once before the first."""
    inner, first = reference_feed(ref, eng), [True]

    def feed():
        if not first[0]:
            ref.next_step()
        first[0] = False
        return inner()
    return feed


def star_body(make, workdir, name, layout):
    cfg = star_networks.make(workdir, name, layout=layout)
    eng = make(cfg)
    model, total, largest = run_against_model(eng, own_feed(eng), cfg, 300, "%s %s" % (name, layout))
    shared = int((np.diff(eng._flat_net()["lane_ll_start"]) > 1).sum())
    assert shared == {"star7": 7, "star5": 13, "star3": 21}[name], shared
    net = eng._flat_net()
    links_of = collections.Counter(zip(net["ll_inter"].tolist(), net["ll_roadlink"].tolist()))  # laneLinks per roadLink
    if name == "star7":  # ragged rows
        assert sorted(set(collections.Counter(i for i, _ in links_of).values())) == [2, 42]
    if name == "star3":  # roadLinks with more laneLinks than the drain's group has threads
        assert {18, 36} <= set(links_of.values()), sorted(set(links_of.values()))
    assert total["left_waiting_steps"] > 0, "no vehicle ever waited inside the intersection"
    assert model.refills > 0, "no laneLink held a vehicle, emptied and held one again"
    if name == "star3":
        assert largest >= 2, "max_waiting_steps never reached 2 at a drain"


def narrow_body(make, workdir, layout):
    cfg = star_networks.star(workdir, "narrow4", layout=layout, **NARROW4)
    eng = make(cfg)
    model, total, _ = run_against_model(eng, own_feed(eng), cfg, 300, "narrow4 " + layout)
    assert model.skips >= 1, "no vehicle crossed a whole laneLink inside one step"
    assert total["entered"] > 0


# ---------------------------------------------------------------------------------------------------------------- CPU (twin)
@pytest.mark.parametrize("name", ["grid_6x6", "example_1x1"])
def test_equals_the_model_fed_by_the_reference(mod, ref_module, scen, workdir, name):
    cfg = scen.materialize(name, workdir)
    eng = twin(mod, cfg)
    _, total, _ = run_against_model(eng, lockstep(eng, ref_module.Engine(cfg, 1)), cfg, 400, name)
    assert total["entered"] > 0 and total["left_steps"] > 0


@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("name", ["star7", "star5", "star3"])
def test_star_junctions(mod, workdir, name, layout):
    star_body(lambda cfg: twin(mod, cfg), workdir, name, layout)


@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_skipped_lanelink(mod, workdir, layout):
    narrow_body(lambda cfg: twin(mod, cfg), workdir, layout)


def accumulators_are_zero(eng, where):
    got = eng.observe_movement_flow_array()
    for k in NAMES:
        assert not got[k].any(), "%s: %s is not zero after a baseline" % (where, k)
    assert eng.movement_flow_tracking(), where


def follow(eng, model, steps, where, first_step):
    feed = own_feed(eng)
    for s in range(steps):
        eng.next_step()
        model.tick(*feed(), first_step + s + 1)
    want = model.outputs()
    got = eng.observe_movement_flow_array()
    for k in NAMES:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (where, k)
    return want


def baseline_rules_body(make, cfg, tmp_path):
    eng = make(cfg)
    feed = own_feed(eng)
    assert not eng.movement_flow_tracking()
    on_at = 120
    for s in range(on_at):
        eng.next_step()
    while not eng.observe_intersections_array()["movement_inside"].any():  # (the first step from 120 on with a vehicle inside)
        eng.next_step()
        on_at += 1
        assert on_at < 180, "no vehicle inside an intersection between steps 120 and 180"
    # turned on mid-run: the vehicles already there, inside an intersection too, are not counted as entered and have not waited
    eng.track_movement_flow(True)
    model = Model(eng._flat_net(), len(eng.intersection_ids()))
    model.baseline(feed()[0], on_at)
    accumulators_are_zero(eng, "turned on at step %d" % on_at)
    want = follow(eng, model, 40, "after turning on at step %d" % on_at, on_at)
    assert want["left"].sum() > 0 and want["entered_lane_waiting_steps"].sum() > 0
    archive = eng.snapshot()
    path = str(tmp_path / "movement_flow_archive.json")
    archive.dump(path)
    follow(eng, model, 30, "after the snapshot", on_at + 40)
    # load: a baseline on the archive's state, at the archive's step
    eng.load(archive)
    accumulators_are_zero(eng, "load")
    model.baseline(feed()[0], on_at + 40)
    follow(eng, model, 30, "after load", on_at + 40)
    eng.load_from_file(path)
    accumulators_are_zero(eng, "load_from_file")
    model.baseline(feed()[0], on_at + 40)
    follow(eng, model, 30, "after load_from_file", on_at + 40)
    eng.reset()
    accumulators_are_zero(eng, "reset")
    model.baseline(feed()[0], 0)
    want = follow(eng, model, 60, "after reset", 0)
    assert want["entered"].sum() > 0
    # off and on again: a new baseline; off: the observe calls raise
    eng.track_movement_flow(False)
    assert not eng.movement_flow_tracking()
    with pytest.raises(RuntimeError):
        eng.observe_movement_flow_array()
    with pytest.raises(RuntimeError):
        eng.observe_movement_flow_tensor(**empty_outputs(eng))
    eng.next_step()
    eng.track_movement_flow(True)
    accumulators_are_zero(eng, "turned on again")
    model.baseline(feed()[0], 61)
    follow(eng, model, 20, "after turning on again", 61)


def test_baseline_rules(mod, scen, workdir, tmp_path):
    baseline_rules_body(lambda cfg: twin(mod, cfg), scen.materialize("grid_6x6", workdir), tmp_path)


def compaction_body(make, scen, workdir, steps=300):
    a = make(scen.materialize("grid_6x6", workdir, cfx={"compactVehicles": 40}))
    b = make(scen.materialize("grid_6x6", workdir, cfx={"compactVehicles": 0}))
    a.track_movement_flow(True)
    b.track_movement_flow(True)
    plan = drain_plan(steps)
    for s in range(steps):
        a.next_step()
        b.next_step()
        if s in plan:
            ga, gb = a.observe_movement_flow_array(reset=plan[s]), b.observe_movement_flow_array(reset=plan[s])
            for k in NAMES:
                assert np.array_equal(ga[k], gb[k]), "step %d: %s differs from the engine that never compacts" % (s, k)
    assert a._vehicle_table()[1] >= 2 and b._vehicle_table()[1] == 0, (a._vehicle_table(), b._vehicle_table())
    assert gb["left"].sum() + gb["entered"].sum() > 0


def test_compaction_is_invisible(mod, scen, workdir):
    compaction_body(lambda cfg: twin(mod, cfg), scen, workdir)


def vector_body(vec, singles, steps, every):
    R = len(singles)
    vec.track_movement_flow(True)
    for e in singles:
        e.track_movement_flow(True)
    seen = 0
    for s in range(steps):
        vec.next_step()
        for e in singles:
            e.next_step()
        if s % every != every - 1:
            continue
        reset = (s // every) % 2 == 0
        peek = [e.observe_movement_flow_array() for e in singles]
        got = vec.observe_movement_flow_array()
        t = empty_outputs(singles[0], lead=(R,))
        vec.observe_movement_flow_tensor(reset=reset, **t)
        if reset:
            for e in singles:
                e.observe_movement_flow_array(reset=True)
        for k in NAMES:
            w = np.stack([x[k] for x in peek])
            assert got[k].shape == w.shape and got[k].dtype == w.dtype == DTYPES[k], k
            assert tuple(t[k].shape) == w.shape, k
            assert np.array_equal(got[k], w), "step %d: %s (array)" % (s, k)
            assert np.array_equal(t[k].cpu().numpy(), w), "step %d: %s (tensor)" % (s, k)
        seen += int(np.stack([x["left"] for x in peek]).sum())
    assert seen > 0


def vector_configs(scen, workdir, name, seed=0):
    return star_networks.make(workdir, name, seed=seed) if name.startswith("star") else scen.materialize(name, workdir, seed=seed)


@pytest.mark.parametrize("name", ["star5", "grid_6x6"])
def test_vector_engine_equals_standalone_twins(mod, scen, workdir, name):
    vec = mod.VectorEngine._with_backend(vector_configs(scen, workdir, name), 3, 1, TWIN_LIB)
    singles = [twin(mod, vector_configs(scen, workdir, name, seed=e)) for e in range(3)]
    vector_body(vec, singles, 120, 20)


def argument_errors_body(eng, vec, other_device):
    shape = tuple(empty_outputs(eng)["entered"].shape)
    dev = tensor_device(eng)

    def zeros(sh=shape, dtype=torch.int32, device=dev):
        return torch.zeros(sh, dtype=dtype, device=device)
    with pytest.raises(RuntimeError):  # tracking is off
        eng.observe_movement_flow_tensor(entered=zeros())
    with pytest.raises(RuntimeError):
        eng.observe_movement_flow_array()
    with pytest.raises(RuntimeError):
        vec.observe_movement_flow_array()
    eng.track_movement_flow()
    vec.track_movement_flow(True)
    for s in range(40):
        eng.next_step()
    with pytest.raises(ValueError):
        eng.observe_movement_flow_tensor()
    with pytest.raises(ValueError):
        eng.observe_movement_flow_tensor(reset=True)
    with pytest.raises(TypeError):
        eng.observe_movement_flow_tensor(entered=zeros(dtype=torch.int64))
    with pytest.raises(TypeError):
        eng.observe_movement_flow_tensor(entered_lane_steps=zeros())
    with pytest.raises(TypeError):
        eng.observe_movement_flow_tensor(waiting_steps=zeros(dtype=torch.float64))
    with pytest.raises(TypeError):
        eng.observe_movement_flow_tensor(left=np.zeros(shape, dtype=np.int32))
    if other_device is not None:
        with pytest.raises(TypeError):
            eng.observe_movement_flow_tensor(left=zeros(device=other_device))
    with pytest.raises(TypeError):
        eng.observe_movement_flow_tensor(left=zeros(device="meta"))
    with pytest.raises(ValueError):
        eng.observe_movement_flow_tensor(max_waiting_steps=zeros((shape[0], shape[1] + 1)))
    with pytest.raises(ValueError):
        eng.observe_movement_flow_tensor(entered=zeros((shape[0], 2 * shape[1]))[:, ::2])  # not contiguous
    with pytest.raises(ValueError):
        vec.observe_movement_flow_tensor(entered=zeros())  # [R, I, M] wanted
    # nothing is written, and nothing is reset, when a later argument is wrong
    before = eng.observe_movement_flow_array()
    assert before["entered"].sum() > 0
    good = torch.full(shape, -7, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        eng.observe_movement_flow_tensor(entered=good, max_waiting_steps=zeros((shape[0], shape[1] + 2)), reset=True)
    assert bool((good == -7).all())
    assert np.array_equal(eng.observe_movement_flow_array()["entered"], before["entered"])
    # reset zeroes all six accumulators, asked for or not
    eng.observe_movement_flow_tensor(waiting_steps=zeros(dtype=torch.int64), reset=True)
    after = eng.observe_movement_flow_array()
    assert not any(after[k].any() for k in ACCUMULATED)


def test_argument_errors_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    argument_errors_body(twin(mod, cfg), mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB), "cuda" if torch.cuda.is_available() else None)


def test_lane_change_is_not_implemented(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, laneChange=True)
    eng = twin(mod, cfg)
    with pytest.raises(NotImplementedError):
        eng.track_movement_flow(True)
    assert not eng.movement_flow_tracking()
    eng.track_movement_flow(False)  # (turning it off is no error)
    vec = mod.VectorEngine._with_backend(cfg, 2, 1, TWIN_LIB)
    with pytest.raises(NotImplementedError):
        vec.track_movement_flow(True)


def test_tiled_engine_has_no_such_method():
    import cityflow_amd
    for name in ("track_movement_flow", "movement_flow_tracking", "observe_movement_flow_tensor", "observe_movement_flow_array"):
        assert hasattr(cityflow_amd.Engine, name) and hasattr(cityflow_amd.VectorEngine, name), name
        assert not hasattr(cityflow_amd.TiledEngine, name), name


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("name", ["star7", "star5", "star3"])
def test_star_junctions_on_the_device(mod, workdir, name, layout):
    star_body(lambda cfg: hip_engine(mod, cfg, layout), workdir, name, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_skipped_lanelink_on_the_device(mod, workdir, layout):
    narrow_body(lambda cfg: hip_engine(mod, cfg, layout), workdir, layout)


@pytest.mark.gpu
def test_baseline_rules_on_the_device(mod, scen, workdir, tmp_path):
    baseline_rules_body(lambda cfg: mod.Engine(cfg, 1), scen.materialize("grid_6x6", workdir), tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_compaction_is_invisible_on_the_device(mod, scen, workdir, layout):
    class S:  # (scen with the layout added to every config)
        @staticmethod
        def materialize(name, wd, cfx):
            return layout_config(scen, wd, name, layout, **cfx)
    compaction_body(lambda cfg: hip_engine(mod, cfg, layout), S, workdir)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["star5", "grid_6x6"])
def test_vector_engine_equals_standalone(mod, scen, workdir, name):
    vec = mod.VectorEngine(vector_configs(scen, workdir, name), 3)
    singles = [mod.Engine(vector_configs(scen, workdir, name, seed=e), 1) for e in range(3)]
    vector_body(vec, singles, 120, 20)


@pytest.mark.gpu
def test_argument_errors_on_the_device(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    eng = mod.Engine(cfg, 1)
    argument_errors_body(eng, mod.VectorEngine(cfg, 2), "cpu" if eng._device_buffers() else None)


@pytest.mark.gpu
def test_tables_grow_while_tracking(mod, scen, workdir):
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense.json"), 400, seed=7, interval=2.0,
                            base_flow=os.path.join(d, "flow.json"))
    small = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring", "ringCapacityPercent": 30}), 1)
    large = mod.Engine(scen.materialize("grid_6x6", workdir, flow_file=flow, cfx={"layout": "ring"}), 1)
    small.track_movement_flow(True)
    large.track_movement_flow(True)
    plan = drain_plan(300)
    for s in range(300):
        small.next_step()
        large.next_step()
        if s in plan:
            a, b = small.observe_movement_flow_array(reset=plan[s]), large.observe_movement_flow_array(reset=plan[s])
            for k in NAMES:
                assert np.array_equal(a[k], b[k]), "step %d: %s differs from the engine that starts large" % (s, k)
    assert b["entered"].sum() > 0
    if small._device_buffers():
        assert small._vehicle_table()[0] > 4096  # (the start-small knob starts the vehicle tables at 4096 numbers)


@pytest.mark.gpu
@pytest.mark.parametrize("tracking", [True, False])
def test_step_launches(mod, scen, workdir, tracking):
    """The tick adds no timing slot: with the tracker on the slot table is that of an engine that tracks lane flow (the commit
    a launch of its own), with it off that of the plain engine."""
    if SHADOW_GPU:
        pytest.skip("about the device library's launches: the twin has none")
    from test_step_launches import LAUNCHES
    eng = mod.Engine(scen.materialize("grid_6x6", workdir), 1)
    assert_hip_backend(eng)
    if tracking:
        eng.track_movement_flow(True)
    for _ in range(12):
        eng.next_step()
    eng.sync()
    eng._profile_enable(True)
    for _ in range(20):
        eng.next_step()
    prof, syms = eng._profile_read(), eng._profile_symbols()
    got = {k: (syms.get(k, ""), prof[k][1]) for k in prof}
    assert got == LAUNCHES["lane-flow" if tracking else "auto"]
    if tracking:
        assert eng.observe_movement_flow_array()["entered"].sum() > 0
