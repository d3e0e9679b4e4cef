"""VectorEngine.rollback(checkpoint, envs=...): a rollback in which environment r takes the state environment envs[r] had when
the checkpoint was saved (cityflow_amd/torch_io.py, cfx_checkpoint_restore_envs of include/cityflow_amd.h, the k_env_gather_*
kernels).  The oracle is ALWAYS standalone CPU twins that never leave their run: slot r after the rollback must go on bit for
bit like a twin seeded as envs[r] that was given envs[r]'s controls up to the checkpoint and slot r's from there on.  A twin is
never put into a state with load(snapshot()) (that moves route positions); where a slot changes the state it follows, its
twin is built anew and given the recorded controls from step 0, which costs little on one intersection.  Every comparison is
array_equal or ==.

The network is example_1x1 throughout, most tests with eight more flows on it (scenarios.dense_flows): the file's own demand
never leaves a vehicle in an entry buffer, and a gather that lost the buffers would pass.

The GPU tests skip themselves on a backend without checkpoints in device memory (the twin standing in for the device under
CFX_SHADOW_GPU).  What a gathered rollback cannot split by environment — _scalars()'s cumulative_travel_time and vehicle_steps —
is compared only where the map is a permutation of the environments."""
import json
import os
import time

import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB

TRIP_KEYS = ("entered", "admitted", "finished", "in_system", "buffered", "finished_travel_steps", "in_system_travel_steps",
             "average_travel_time")


# ----------------------------------------------------------------------------------------------------------------- helpers
def dense_config(scen, workdir, **config):
    """example_1x1 with eight more flows, one vehicle per second each: entry buffers hold vehicles from the first steps on."""
    base = scen.materialize("example_1x1", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense_envs.json"), 8, seed=7, interval=1.0,
                            base_flow=os.path.join(d, "flow.json"))
    return scen.materialize("example_1x1", workdir, flow_file=flow, **config)


def plain_config(scen, workdir, **config):
    return scen.materialize("example_1x1", workdir, **config)


def twin(mod, cfg):
    return mod.Engine._with_backend(cfg, 1, TWIN_LIB)


def device_vec(mod, cfg, R):
    vec = mod.VectorEngine(cfg, R, 1)  # (environment r runs on seed + r)
    assert SHADOW_GPU or vec.backend_name() == "hip-gfx950", vec.backend_name()
    if not vec._checkpoint_calls():
        pytest.skip("the backend %s has no checkpoints in device memory" % vec.backend_name())
    return vec


def random_phases(rng, counts, rows):
    return np.array([[int(rng.integers(0, c)) if c > 0 else 0 for c in counts] for _ in range(rows)], dtype=np.int32)


def assert_slot(vec, r, tw, where, trips=False, got=None):
    """Slot r of the batched engine against a standalone twin; `got`: the batched arrays read once for all slots."""
    got = got or read_all(vec, trips)
    assert np.array_equal(got["lanes"][r], tw.get_lane_vehicle_count_array()), "%s: slot %d lane counts" % (where, r)
    assert np.array_equal(got["waiting"][r], tw.get_lane_waiting_vehicle_count_array()), "%s: slot %d waiting counts" % (where, r)
    assert vec.get_vehicle_speed(r) == tw.get_vehicle_speed(), "%s: slot %d vehicle speeds" % (where, r)
    ph, rem = tw._tl_state()
    assert np.array_equal(got["tl"][0][r], ph) and np.array_equal(got["tl"][1][r], rem), "%s: slot %d lights" % (where, r)
    if trips:
        want = tw.observe_trips_array()
        for k in TRIP_KEYS:
            assert np.array_equal(got["trips"][k][r], want[k]), "%s: slot %d trips %s (%r, %r)" % (where, r, k, got["trips"][k][r], want[k])


def read_all(vec, trips=False):
    out = {"lanes": vec.get_lane_vehicle_count_array(), "waiting": vec.get_lane_waiting_vehicle_count_array(), "tl": vec._tl_state()}
    if trips:
        out["trips"] = vec.observe_trips_array()
    return out


def assert_counts_add_up(vec, twins, where):
    """The engine-wide scalars are the sums over the environments taken."""
    sc, each = vec._scalars(), [t._scalars() for t in twins]
    for k in ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count"):
        assert sc[k] == sum(x[k] for x in each), "%s: scalar %s: %r, the twins' sum %r" % (where, k, sc[k], sum(x[k] for x in each))


class History:
    """Phases given to every environment before each of the steps up to a checkpoint, and twins that are given a column of it."""

    def __init__(self, mod, cfg_of_seed, counts):
        self.mod, self.cfg_of_seed, self.counts, self.rows = mod, cfg_of_seed, counts, []

    def drive(self, vec, rng, steps, twins=None):
        for _ in range(steps):
            ph = random_phases(rng, self.counts, vec.num_envs)
            vec.set_tl_phases(ph)
            vec.next_step()
            self.rows.append(ph)
            for r, t in enumerate(twins or ()):
                t.set_tl_phases(ph[r])
                t.next_step()

    def twin_of(self, env, trackers=()):
        """A twin seeded as `env` that has been given env's phases of every step so far; then the trackers are turned on."""
        t = twin(self.mod, self.cfg_of_seed(env))
        for ph in self.rows:
            t.set_tl_phases(ph[env])
            t.next_step()
        for name in trackers:
            getattr(t, name)(True)
        return t


def follow(vec, twins, rng, counts, steps, where, trips=False, per_slot=None):
    """`steps` steps with another random phase row per slot (`per_slot`: slot -> the slot whose row it is given, for slots that
    share a twin); after every step slot r equals twins[r]."""
    R = vec.num_envs
    for s in range(steps):
        ph = random_phases(rng, counts, R)
        if per_slot is not None:
            ph = ph[per_slot]
        vec.set_tl_phases(ph)
        vec.next_step()
        given = set()
        for r, t in enumerate(twins):
            if id(t) not in given:
                given.add(id(t))
                t.set_tl_phases(ph[r])
                t.next_step()
        got = read_all(vec, trips)
        for r, t in enumerate(twins):
            assert_slot(vec, r, t, "%s, step %d after the rollback" % (where, s + 1), trips, got)
        if per_slot is None:
            assert_counts_add_up(vec, twins, "%s, step %d after the rollback" % (where, s + 1))


# --------------------------------------------------------------------------------------------------------------- CPU tests
def test_envs_is_checked_before_anything_else(mod, scen, workdir):
    cfg = plain_config(scen, workdir)
    vec = mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB)
    with pytest.raises(ValueError):
        vec.rollback(None, envs=[0, 1])
    with pytest.raises(ValueError, match="position 2"):
        vec.rollback(None, envs=[0, 1, 3])
    with pytest.raises(ValueError, match=r"envs\[0\]"):
        vec.rollback(None, envs=np.array([-1, 1, 2]))
    with pytest.raises(TypeError):
        vec.rollback(None, envs=[0.0, 1.0, 2.0])
    with pytest.raises(TypeError):
        vec.rollback(None, envs=[True, False, True])
    with pytest.raises(TypeError):
        vec.rollback(None, envs=np.array([True, False, True]))
    with pytest.raises(TypeError):
        vec.rollback(None, envs=np.array([0.0, 1.0, 2.0]))
    with pytest.raises(TypeError):  # (the type before the length)
        vec.rollback(None, envs=[0, 1.5])
    with pytest.raises(TypeError):
        vec.rollback(None, envs=2)
    with pytest.raises(TypeError):
        vec.rollback(None, envs="012")
    for valid in ([2, 2, 0], (0, 1, 2), np.array([1, 0, 1]), np.array([1, 0, 1], dtype=np.uint8), [np.int64(0), 1, 2]):
        with pytest.raises(NotImplementedError, match=vec.backend_name()):
            vec.rollback(None, envs=valid)
    with pytest.raises(NotImplementedError):  # (and the plain call as before)
        vec.rollback(None)
    lc = mod.VectorEngine._with_backend(scen.materialize("example_1x1", workdir, laneChange=True), 3, 1, TWIN_LIB)
    with pytest.raises(ValueError):
        lc.rollback(None, envs=[0, 1])
    with pytest.raises(NotImplementedError):
        lc.rollback(None, envs=[0, 1, 2])


def test_a_cpu_tensor_is_taken_and_a_device_tensor_is_named(mod, scen, workdir):
    torch = pytest.importorskip("torch")
    vec = mod.VectorEngine._with_backend(plain_config(scen, workdir), 3, 1, TWIN_LIB)
    with pytest.raises(NotImplementedError):
        vec.rollback(None, envs=torch.tensor([2, 2, 0]))
    with pytest.raises(TypeError):
        vec.rollback(None, envs=torch.tensor([True, False, True]))
    with pytest.raises(ValueError):
        vec.rollback(None, envs=torch.tensor([0, 1]))

    class OnADevice:  # (what the check looks at, without a device)
        device = torch.device("cuda", 0)

        def tolist(self):
            raise AssertionError("read from the device")

    with pytest.raises(TypeError, match="tolist"):
        vec.rollback(None, envs=OnADevice())


def test_engine_rollback_takes_no_envs(mod, scen, workdir):
    import inspect

    import cityflow_amd
    assert list(inspect.signature(cityflow_amd.Engine.rollback).parameters) == ["self", "checkpoint"]
    assert list(inspect.signature(cityflow_amd.VectorEngine.rollback).parameters) == ["self", "checkpoint", "envs"]
    tw = twin(mod, plain_config(scen, workdir))
    with pytest.raises(TypeError):
        tw.rollback(None, envs=[0])
    assert hasattr(cityflow_amd.VectorEngine, "_lane_history") and not hasattr(cityflow_amd.Engine, "_rollback_envs")


# --------------------------------------------------------------------------------------------------------------- GPU tests
BEFORE, AFTER = 50, 40


@pytest.mark.gpu
def test_duplicate_drop_and_shift_both_ways(mod, scen, workdir):
    """R = 3, envs = [2, 2, 0]: environment 2 is taken twice (once shifted down two places, once one), 0 shifted up, 1 dropped."""
    cfg = dense_config(scen, workdir, rlTrafficLight=True)
    vec = device_vec(mod, cfg, 3)
    counts = vec._phase_counts()
    hist = History(mod, lambda s: dense_config(scen, workdir, rlTrafficLight=True, seed=s), counts)
    rng = np.random.default_rng(11)
    trackers = ("track_trips",)
    vec.track_trips(True)
    hist.drive(vec, rng, BEFORE)
    # the plain state holds what the gather must move: vehicles in entry buffers, on the intersection, finished ones
    trips, inter = vec.observe_trips_array(), vec.observe_intersections_array()
    inside = inter["movement_inside"].reshape(3, -1).sum(axis=1)
    assert trips["buffered"].min() > 0 and inside.min() > 0 and trips["finished"].min() > 0, (trips["buffered"], inside, trips["finished"])
    assert len({tuple(row) for row in vec.get_lane_vehicle_count_array().tolist()}) == 3, "the environments do not differ"
    ck = vec.checkpoint()
    envs = [2, 2, 0]
    for _ in range(7):  # (leave the checkpointed state)
        vec.next_step()
    vec.rollback(ck, envs=envs)
    assert vec._scalars()["step"] == BEFORE and vec.get_current_time() == float(BEFORE)
    twins = [hist.twin_of(s, trackers) for s in envs]
    assert vec.trip_tracking()
    got = read_all(vec, True)
    for r, t in enumerate(twins):
        assert_slot(vec, r, t, "right after the rollback", True, got)
    assert_counts_add_up(vec, twins, "right after the rollback")
    assert np.array_equal(got["lanes"][0], got["lanes"][1])
    follow(vec, twins, rng, counts, AFTER, "envs=[2, 2, 0]", trips=True)
    lanes = vec.get_lane_vehicle_count_array()
    assert not np.array_equal(lanes[0], lanes[1]) and vec.get_vehicle_speed(0) != vec.get_vehicle_speed(1), \
        "slots 0 and 1 never diverged under their own phases"
    assert ck.step == BEFORE and not ck.released


def _everything(v):
    out = {"lanes": v.get_lane_vehicle_count_array(), "waiting": v.get_lane_waiting_vehicle_count_array(),
           "speed_sum": v.get_lane_speed_sum_array(), "phase": v._tl_state()[0], "remain": v._tl_state()[1]}
    for name, got in (("inter", v.observe_intersections_array()), ("trips", v.observe_trips_array()),
                      ("lane_flow", v.observe_lane_flow_array(reset=False)), ("move_flow", v.observe_movement_flow_array(reset=False))):
        for k, a in got.items():
            out[name + "." + k] = a
    return out


def _assert_everything_equal(a, b, where):
    ea, eb = _everything(a), _everything(b)
    assert sorted(ea) == sorted(eb)
    for k in ea:
        assert np.array_equal(ea[k], eb[k], equal_nan=True), "%s: %s" % (where, k)
    assert a._scalars() == b._scalars(), "%s: scalars %r / %r" % (where, a._scalars(), b._scalars())
    for r in range(a.num_envs):
        assert a.get_vehicle_speed(r) == b.get_vehicle_speed(r), "%s: env %d speeds" % (where, r)
        assert a.get_lane_vehicle_count(r) == b.get_lane_vehicle_count(r), "%s: env %d counts" % (where, r)


@pytest.mark.gpu
def test_identity_equals_the_plain_rollback_and_the_checkpoint_is_not_modified(mod, scen, workdir):
    cfg = dense_config(scen, workdir, rlTrafficLight=True)
    a, b = device_vec(mod, cfg, 3), device_vec(mod, cfg, 3)
    counts = a._phase_counts()
    hist = History(mod, lambda s: dense_config(scen, workdir, rlTrafficLight=True, seed=s), counts)
    rng = np.random.default_rng(12)
    for v in (a, b):
        v.track_trips(True)
        v.track_lane_flow(True)
        v.track_movement_flow(True)
    _drive_pair(hist, a, b, rng, BEFORE)
    cka, ckb = a.checkpoint(), b.checkpoint()

    def leave(v):
        for _ in range(5):
            v.next_step()

    def together(steps, where):
        for s in range(steps):
            ph = random_phases(rng, counts, 3)
            for v in (a, b):
                v.set_tl_phases(ph)
                v.next_step()
            _assert_everything_equal(a, b, "%s, step %d" % (where, s + 1))

    leave(a), leave(b)
    a.rollback(cka, envs=list(range(3)))
    b.rollback(ckb)
    _assert_everything_equal(a, b, "identity map, right after the rollback")
    together(20, "identity map")
    # another map on the same checkpoint, against twins ...
    a.rollback(cka, envs=np.array([1, 0, 1]))
    twins = [hist.twin_of(s, ("track_trips",)) for s in (1, 0, 1)]
    got = read_all(a, True)
    for r, t in enumerate(twins):
        assert_slot(a, r, t, "envs=[1, 0, 1] right after the rollback", True, got)
    follow(a, twins, rng, counts, 10, "envs=[1, 0, 1]", trips=True)
    # ... and the plain rollback to it afterwards: the checkpoint still holds every environment's own state
    a.rollback(cka)
    leave(b)
    b.rollback(ckb)
    _assert_everything_equal(a, b, "plain rollback after two gathered ones")
    together(20, "plain rollback after two gathered ones")


def _drive_pair(hist, a, b, rng, steps):
    for _ in range(steps):
        ph = random_phases(rng, hist.counts, a.num_envs)
        for v in (a, b):
            v.set_tl_phases(ph)
            v.next_step()
        hist.rows.append(ph)


@pytest.mark.gpu
def test_the_fullest_environment_everywhere_after_a_reset(mod, scen, workdir):
    """Checkpoints belong to their engine, so the checkpoint is taken in the same engine before the reset.  What the code
    guarantees, and what is asserted: the rings never shrink (a reset keeps their capacity scale) and every environment's rings
    have the geometry of the source's, so a state of this engine's checkpoint fits the rings as they are — the scale after
    the rollback is the scale at the checkpoint.  The engine starts with rings a tenth of the usual size, so that by the
    checkpoint they HAVE grown (asserted): the state would not fit rings of the initial size."""
    cfg = dense_config(scen, workdir, rlTrafficLight=True, cfx={"layout": "ring", "ringCapacityPercent": 10})
    R = 4
    vec = device_vec(mod, cfg, R)
    counts = vec._phase_counts()
    hist = History(mod, lambda s: dense_config(scen, workdir, rlTrafficLight=True, seed=s), counts)
    rng = np.random.default_rng(13)
    first_scale = vec._ring_info()[1]
    hist.drive(vec, rng, 60)
    ck = vec.checkpoint()
    scale = vec._ring_info()[1]
    per_env = vec.get_lane_vehicle_count_array().sum(axis=1)
    k = int(np.argmax(per_env))
    vec.reset()
    assert vec.get_vehicle_count() == 0 and vec._scalars()["step"] == 0
    vec.rollback(ck, envs=[k] * R)
    assert vec._ring_info()[1] == scale > first_scale, (first_scale, scale, vec._ring_info())
    t = hist.twin_of(k)
    twins = [t] * R
    got = read_all(vec)
    for r in range(R):
        assert_slot(vec, r, t, "[%d] * %d right after the rollback" % (k, R), False, got)
    assert vec._scalars()["active_vehicle_count"] == R * t._scalars()["active_vehicle_count"] > 0
    follow(vec, twins, rng, counts, 20, "[%d] * %d" % (k, R), per_slot=[0] * R)
    print("ring scale at creation %d, at the checkpoint and after the rollback %d; environment %d of %s vehicles" % (first_scale, scale, k, per_env))


@pytest.mark.gpu
def test_sixty_seven_environments_with_a_random_map(mod, scen, workdir):
    """Beyond k_trip_tick's 64 rows in LDS and the 32 environments from which the host's thread pool carries the spawners."""
    R = 67
    t0 = time.perf_counter()
    cfg = dense_config(scen, workdir, rlTrafficLight=True)
    vec = device_vec(mod, cfg, R)
    counts = vec._phase_counts()
    hist = History(mod, lambda s: dense_config(scen, workdir, rlTrafficLight=True, seed=s), counts)
    rng = np.random.default_rng(14)
    envs = rng.integers(0, R, R)
    taken = np.bincount(envs, minlength=R)
    assert (taken == 0).any() and (taken >= 3).any(), taken
    assert taken[envs[64:]].max() >= 1 and len(set(envs[64:].tolist())) >= 2
    vec.track_trips(True)
    hist.drive(vec, rng, 15)
    ck = vec.checkpoint()
    vec.next_step()
    vec.rollback(ck, envs=envs)
    sources = {int(s): hist.twin_of(int(s), ("track_trips",)) for s in sorted(set(envs.tolist()))}
    twins = [sources[int(s)] for s in envs]
    first_slot = {int(s): int(np.argmax(envs == s)) for s in sources}  # (slots that share a source are given one row)
    per_slot = [first_slot[int(s)] for s in envs]
    got = read_all(vec, True)
    for r, t in enumerate(twins):
        assert_slot(vec, r, t, "x67 right after the rollback", True, got)
    assert got["trips"]["buffered"][64:].min() > 0
    sc = vec._scalars()
    assert sc["active_vehicle_count"] == sum(t._scalars()["active_vehicle_count"] for t in twins)
    assert sc["spawned_vehicle_count"] == sum(t._scalars()["spawned_vehicle_count"] for t in twins)
    follow(vec, twins, rng, counts, 15, "x67", trips=True, per_slot=per_slot)
    print("x67, %d distinct sources: %.1f s" % (len(sources), time.perf_counter() - t0))


@pytest.mark.gpu
def test_the_plan_stays_the_slots_and_the_phase_moves(mod, scen, workdir):
    """Fixed-time lights.  The twin of slot r is a DRIVEN twin, as in tests/test_device_sequences.py: a twin in rlTrafficLight
    mode seeded as envs[r], given before every step the phase that the pass_time model (TrafficLight::passTime restated,
    tests/test_tl_plan.py) holds — under envs[r]'s durations up to the checkpoint, under slot r's from there on, the model's
    phase and remaining time carried across.  (A twin cannot read another plan than its roadnet file's in the middle of a run,
    so no twin "whose roadnet carries slot r's durations" can start from another environment's light state; the lights
    themselves are compared with the model, the traffic with the driven twin.)"""
    from test_tl_plan import Plan, pass_time
    R, before, envs = 3, 45, [1, 2, 0]
    cfg = dense_config(scen, workdir)
    vec = device_vec(mod, cfg, R)
    if not vec._tl_plan_calls():
        pytest.skip("the backend keeps no signal plan")
    plan = Plan(vec, cfg)
    count, real = plan.count, plan.real
    T = np.stack([plan.other(r) for r in range(R)])
    assert len({T[r].tobytes() for r in range(R)}) == R
    vec.set_tl_plan(durations=np.stack([plan.dirty(T[r]) for r in range(R)]))
    phase, remain = np.zeros((R, plan.I), dtype=np.int64), np.stack([plan.file()[:, 0]] * R)

    def driven(seed):
        return twin(mod, dense_config(scen, workdir, rlTrafficLight=True, seed=seed))

    def driven_step(t, ph, rem, durations):
        t.set_tl_phases(ph.astype(np.int32))
        t.next_step()
        pass_time(ph, rem, durations, count, 1.0)

    twins = [driven(r) for r in range(R)]
    for s in range(before):
        vec.next_step()
        for r in range(R):
            driven_step(twins[r], phase[r], remain[r], T[r])
    got_phase, got_remain = (np.asarray(x) for x in vec._tl_state())
    assert np.array_equal(got_phase[:, real], phase[:, real]) and np.array_equal(got_remain[:, real], remain[:, real])
    assert len({(tuple(phase[r, real]), tuple(remain[r, real])) for r in range(R)}) == R, "the lights of the environments do not differ"
    for r in range(R):
        assert np.array_equal(vec.get_lane_vehicle_count_array()[r], twins[r].get_lane_vehicle_count_array())
    ck = vec.checkpoint()
    for _ in range(6):
        vec.next_step()
    vec.rollback(ck, envs=envs)
    assert np.array_equal(vec.get_tl_phase_durations_array(), T), "the durations moved with the state"
    got_phase, got_remain = (np.asarray(x) for x in vec._tl_state())
    for r, s in enumerate(envs):
        assert np.array_equal(got_phase[r, real], phase[s, real]) and np.array_equal(got_remain[r, real], remain[s, real]), \
            "slot %d does not show environment %d's lights" % (r, s)
    # slot r: the traffic and the light state of envs[r], the durations of r
    after = [driven(s) for s in envs]
    ph2, rem2 = np.zeros((R, plan.I), dtype=np.int64), np.stack([plan.file()[:, 0]] * R)
    for r, s in enumerate(envs):
        for _ in range(before):
            driven_step(after[r], ph2[r], rem2[r], T[s])
        assert np.array_equal(ph2[r], phase[s]) and np.array_equal(rem2[r], remain[s])
    changed = 0
    for step in range(10):
        vec.next_step()
        start = ph2.copy()
        for r in range(R):
            driven_step(after[r], ph2[r], rem2[r], T[r])
        changed += int((start[:, real] != ph2[:, real]).sum())
        got_phase, got_remain = (np.asarray(x) for x in vec._tl_state())
        assert np.array_equal(got_phase[:, real], ph2[:, real]), "phases differ from pass_time's at step %d" % step
        assert np.array_equal(got_remain[:, real], rem2[:, real]), "remaining times differ from pass_time's at step %d" % step
        lanes = vec.get_lane_vehicle_count_array()
        for r in range(R):
            assert np.array_equal(lanes[r], after[r].get_lane_vehicle_count_array()), "slot %d lane counts at step %d" % (r, step)
            assert vec.get_vehicle_speed(r) == after[r].get_vehicle_speed(), "slot %d speeds at step %d" % (r, step)
    assert changed > 0, "no light changed its phase in ten steps"


@pytest.mark.gpu
def test_lane_history_moves_with_the_lanes(mod, scen, workdir):
    cfg = dense_config(scen, workdir, rlTrafficLight=True, cfx={"laneHistory": True})
    vec = device_vec(mod, cfg, 3)
    assert vec._keeps_lane_history()
    rng = np.random.default_rng(16)
    counts = vec._phase_counts()
    for _ in range(30):
        vec.set_tl_phases(random_phases(rng, counts, 3))
        vec.next_step()
    ck = vec.checkpoint()
    for _ in range(9):
        vec.next_step()
    vec.rollback(ck)
    rows = [vec._lane_history(r) for r in range(3)]
    L = len(vec.lane_ids())
    assert rows[0]["len"].shape == (L,) and rows[0]["vehicle_num"].size == L * 241 and rows[0]["len"].max() == 30
    assert any(not np.array_equal(rows[0][k], rows[2][k]) for k in rows[0]), "the environments' histories do not differ"
    for _ in range(4):
        vec.next_step()
    envs = [2, 0, 0]
    vec.rollback(ck, envs=envs)
    for r, s in enumerate(envs):
        got = vec._lane_history(r)
        assert sorted(got) == sorted(rows[s])
        for k in got:
            assert np.array_equal(got[k], rows[s][k]), "slot %d: %s is not environment %d's" % (r, k, s)
    # ... and goes on from there: two slots with one state and one phase sequence keep one history
    for _ in range(5):
        ph = random_phases(rng, counts, 3)
        ph[2] = ph[1]
        vec.set_tl_phases(ph)
        vec.next_step()
    h1, h2 = vec._lane_history(1), vec._lane_history(2)
    for k in h1:
        assert np.array_equal(h1[k], h2[k]), k
    assert h1["len"].max() == 35


# ----------------------------------------------------------------------------------------- a random call sequence (R = 4)
SEQUENCE_OPS = (("steps", 6.0), ("phases", 2.0), ("rollback", 1.2), ("rollback_envs", 2.5), ("checkpoint", 1.0), ("checkpoint_into", 1.0),
                ("track", 1.5), ("drain", 2.0), ("reset", 0.4), ("compare", 1.0))
TRACK = {"lane": "track_lane_flow", "move": "track_movement_flow", "trip": "track_trips"}


class Follower:
    """The standalone twin of one slot with the controls it was given since step 0, from which it can be built again (the twins
    are REBUILT from step 0 where a slot takes another state, never loaded from a snapshot)."""

    def __init__(self, mod, cfg_of_seed, seed, log=()):
        self.mod, self.cfg_of_seed, self.seed, self.log = mod, cfg_of_seed, seed, []
        self.eng = twin(mod, cfg_of_seed(seed))
        for op in log:
            self.apply(op)

    def apply(self, op):
        self.log.append(op)
        if op[0] == "phases":
            self.eng.set_tl_phases(op[1])
        elif op[0] == "step":
            self.eng.next_step()
        else:
            self.eng.reset(False)

    def saved(self):
        return self.seed, tuple(self.log)


def run_rollback_sequence(mod, vec, cfg_of_seed, seed, calls, where):
    rng = np.random.default_rng(seed)
    R = vec.num_envs
    counts = vec._phase_counts()
    slots = [Follower(mod, cfg_of_seed, r) for r in range(R)]
    on = dict.fromkeys(TRACK, False)
    tally = dict.fromkeys([k for k, _ in SEQUENCE_OPS], 0)
    tally.update(gathered_with_repeat=0, rollback_while_tracking=0, steps=0, gathered_vehicles=0, most_vehicles=0)
    names, weights = [k for k, _ in SEQUENCE_OPS], np.array([w for _, w in SEQUENCE_OPS])
    ck, held = None, None  # the checkpoint, and per environment what its twin had been given when it was saved

    def compare(at):
        got = read_all(vec, on["trip"])
        for r, f in enumerate(slots):
            assert_slot(vec, r, f.eng, at, on["trip"], got)
        assert_counts_add_up(vec, [f.eng for f in slots], at)

    def save(into):
        nonlocal ck, held
        ck = vec.checkpoint(into=into)
        held = [f.saved() for f in slots]

    def restore(envs):
        for r in range(R):
            s, log = held[r if envs is None else envs[r]]
            slots[r] = Follower(mod, cfg_of_seed, s, log)
            for k in TRACK:
                if on[k]:
                    getattr(slots[r].eng, TRACK[k])(True)

    save(None)
    for call in range(calls):
        op = names[int(rng.choice(len(names), p=weights / weights.sum()))]
        at = "%s seed %d, call %d (%s)" % (where, seed, call, op)
        tally[op] += 1
        if op == "steps":
            for _ in range(int(rng.integers(1, 7))):
                vec.next_step()
                for f in slots:
                    f.apply(("step",))
                tally["steps"] += 1
        elif op == "phases":
            ph = random_phases(rng, counts, R)
            vec.set_tl_phases(ph)
            for r, f in enumerate(slots):
                f.apply(("phases", ph[r]))
        elif op == "rollback":
            vec.rollback(ck)
            restore(None)
            tally["rollback_while_tracking"] += any(on.values())
        elif op == "rollback_envs":
            envs = rng.integers(0, R, R)
            vec.rollback(ck, envs=envs if rng.random() < 0.5 else envs.tolist())
            restore(envs.tolist())
            tally["gathered_with_repeat"] += len(set(envs.tolist())) < R
            tally["gathered_vehicles"] += ck.num_running > 0 and len(set(envs.tolist())) < R
            tally["rollback_while_tracking"] += any(on.values())
        elif op == "checkpoint":
            save(None)
        elif op == "checkpoint_into":
            save(ck)
        elif op == "track":
            which = list(TRACK)[int(rng.integers(0, 3))]
            on[which] = not on[which]
            for e in [vec] + [f.eng for f in slots]:
                getattr(e, TRACK[which])(on[which])
        elif op == "drain":
            live = [k for k in TRACK if on[k]]
            if live:
                which = live[int(rng.integers(0, len(live)))]
                reset = bool(rng.integers(0, 2)) and which != "trip"
                if which == "trip":
                    got, want = vec.observe_trips_array(), [f.eng.observe_trips_array() for f in slots]
                elif which == "lane":
                    got, want = vec.observe_lane_flow_array(reset=reset), [f.eng.observe_lane_flow_array(reset=reset) for f in slots]
                else:
                    got, want = vec.observe_movement_flow_array(reset=reset), [f.eng.observe_movement_flow_array(reset=reset) for f in slots]
                for k in got:
                    assert np.array_equal(got[k], np.stack([w[k] for w in want]), equal_nan=True), "%s: %s %s" % (at, which, k)
        elif op == "reset":
            vec.reset(False)
            for f in slots:
                f.apply(("reset",))
        compare(at)
        tally["most_vehicles"] = max(tally["most_vehicles"], int(vec.get_vehicle_count()))
    assert tally["rollback"] >= 3 and tally["rollback_envs"] >= 8 and tally["gathered_with_repeat"] >= 5, tally
    assert tally["checkpoint_into"] >= 2 and tally["reset"] >= 1 and tally["drain"] >= 5 and tally["rollback_while_tracking"] >= 3, tally
    assert tally["steps"] >= 100 and tally["gathered_vehicles"] >= 3 and tally["most_vehicles"] > 100 * R, tally
    return tally


@pytest.mark.gpu
def test_a_random_call_sequence_equals_rebuilt_twins(mod, scen, workdir):
    t0 = time.perf_counter()
    cfg = dense_config(scen, workdir, rlTrafficLight=True)
    vec = device_vec(mod, cfg, 4)
    tally = run_rollback_sequence(mod, vec, lambda s: dense_config(scen, workdir, rlTrafficLight=True, seed=s), 41, 150, "rollback sequence")
    print("rollback sequence x4: %s, %.1f s" % (json.dumps(tally), time.perf_counter() - t0))
