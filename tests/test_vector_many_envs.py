"""VectorEngine at 67 environments of example_1x1: the smallest shape at which the device paths that depend on the number of
environments all run — more than k_trip_tick's 64 LDS rows (environments 64, 65 and 66 take its road straight to memory),
more than the 32 from which the host thread pool carries spawners and record translation, an odd count, and rows that differ
(seed + env picks other first lanes).  The network is one intersection, so the oracle — ALWAYS 67 standalone twin engines,
plus the Python models of the trip tracker and of TrafficLight::passTime, never a HIP engine — costs little.

Every test marked gpu builds its batched engine through the `mod` fixture and has an unmarked sibling that runs the same body
with a batched twin in its place: that holds the harness, the models, the pinned numbers and every end-of-test condition on a
machine without a GPU, where the seeds and step counts below were chosen.  (The signal plan is state only the device library
keeps: the plan sequences' siblings run the stream, the models and the driven twins alone, and the rejection test has none.)
All comparisons are array_equal or ==."""
import time

import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB

torch = pytest.importorskip("torch")

import test_device_sequences as sequences  # noqa: E402
import test_trip_stats as trip_stats  # noqa: E402
import test_vector_engine as vector_engine  # noqa: E402
from test_device_tensors import twin  # noqa: E402
from test_tl_plan import NAN, Plan, dev, durations_of, on_device  # noqa: E402

R = 67
HIGH = sequences.HIGH_ENV  # 64: the first environment beyond k_trip_tick's LDS table
assert R > HIGH + 2 and R % 2 == 1


def vec_twin(mod):
    return lambda cfg, n: mod.VectorEngine._with_backend(cfg, n, 1, TWIN_LIB)


def vec_default(mod):
    """The batched engine on the default backend: the HIP library, or the twin in the shadow run of the gpu tests."""
    def make(cfg, n):
        vec = mod.VectorEngine(cfg, n)
        assert SHADOW_GPU or vec.backend_name() == "hip-gfx950", vec.backend_name()
        return vec
    return make


# ------------------------------------------------------------------- 1. trip statistics across the kTripLdsEnvs boundary
# The smallest multiple of 50 steps after which, on the twin, every environment from 64 on has entered, admitted and finished
# vehicles, two of them differ in finished_travel_steps and one of them differs from an environment below 64; and the twin's
# `finished` of environments 64, 65, 66 at that step.
TRIP_STEPS = 50
TRIP_FINISHED_HIGH = [12, 12, 12]


def high_rows_are_live(got, where):
    for k in ("entered", "admitted", "finished"):
        assert got[k][HIGH:].min() > 0, "%s: an environment from %d on has no %s vehicle: %s" % (where, HIGH, k, got[k][HIGH:])
    fts = got["finished_travel_steps"]
    assert len(set(fts[HIGH:].tolist())) >= 2, "%s: the rows from %d on are equal: %s" % (where, HIGH, fts[HIGH:])
    assert set(fts[:HIGH].tolist()) - set(fts[HIGH:].tolist()), "%s: no row below %d differs from one beyond" % (where, HIGH)


def trips_body(mod, make_vec, scen, workdir):
    engines = []
    models, got = trip_stats.vector_body(make_vec, lambda cfg: twin(mod, cfg), scen, workdir, "example_1x1", TRIP_STEPS, rl=False,
                                         vec_twin=vec_twin(mod), R=R, engines=engines)
    high_rows_are_live(got, "tracking since creation")
    assert got["finished"][HIGH:].tolist() == TRIP_FINISHED_HIGH  # what the CPU twin showed
    vec, other, singles = engines[0]
    # reset while tracking is on: tracking stays on, every output restarts; without a new seed the generators go on, with one
    # every environment repeats its first run
    for reseed in (False, True):
        for e in [vec, other] + singles:
            e.reset(reseed)
        assert vec.trip_tracking()
        where = "after reset(%s)" % reseed
        models = [trip_stats.Model() for _ in range(R)]
        got = trip_stats.read(vec, where, shape=(R,))
        trip_stats.check(got, trip_stats.stack([m.outputs() for m in models]), where)
        assert not any(got[k].any() for k in trip_stats.NAMES), where
        got, _ = trip_stats.vector_follow(vec, other, singles, models, 0, TRIP_STEPS, where)
        high_rows_are_live(got, where)
    assert got["finished"][HIGH:].tolist() == TRIP_FINISHED_HIGH


def test_trips_twin_against_twins(mod, scen, workdir):
    trips_body(mod, vec_twin(mod), scen, workdir)


@pytest.mark.gpu
def test_trips_across_the_lds_table_on_the_device(mod, scen, workdir):
    t0 = time.perf_counter()
    trips_body(mod, vec_default(mod), scen, workdir)
    print("trips example_1x1 x%d: %.1f s" % (R, time.perf_counter() - t0))


# The baseline launch (tracking turned on in the middle of a run) counts the vehicles alive and, apart, those that wait in a
# lane's buffer.  Under example_1x1's own signal plan nothing ever waits in a buffer (tests/test_trip_stats.py::example_body),
# in none of 67 environments in 400 steps; with rlTrafficLight and no phase ever set the signal holds phase 0, the lanes it
# never serves fill up, and from step 340 on every environment from 64 on has vehicles in its buffers (at 360 the twin
# shows 13, 9 and 14).  Hence this leg's engines and its step; baselines_body's step 60 has none.
BASELINE_AT = 360
BASELINE_BUFFERED_HIGH = [13, 9, 14]


def trips_baseline_body(mod, make_vec, scen, workdir):
    cfg = scen.materialize("example_1x1", workdir, rlTrafficLight=True)
    vec, other = make_vec(cfg, R), vec_twin(mod)(cfg, R)
    singles = [twin(mod, scen.materialize("example_1x1", workdir, rlTrafficLight=True, seed=r)) for r in range(R)]
    models = [trip_stats.Model() for _ in range(R)]
    assert not vec.trip_tracking()

    def untracked_step(s):
        vec.next_step()
        other.next_step()
        for r in range(R):
            singles[r].next_step()
            models[r].tick(singles[r], s)

    def turn_on(where):
        for e in (vec, other):
            e.track_trips(True)
        for m in models:
            m.baseline()
        got = trip_stats.read(vec, where, shape=(R,))
        trip_stats.check(got, trip_stats.stack([m.outputs() for m in models]), where)
        assert not any(got[k].any() for k in trip_stats.ACCUMULATED), where
        return got

    for s in range(1, BASELINE_AT + 1):
        untracked_step(s)
    got = turn_on("turned on at step %d" % BASELINE_AT)
    assert got["buffered"][HIGH:].tolist() == BASELINE_BUFFERED_HIGH and min(BASELINE_BUFFERED_HIGH) > 0
    assert (got["in_system"][HIGH:] > got["buffered"][HIGH:]).all() and (got["in_system_travel_steps"][HIGH:] > got["in_system"][HIGH:]).all()
    # (followed under vector_body's phase plan, another phase per environment every 10 steps: the lanes that phase 0 never
    # served begin to drain; the first vehicle that waited in a buffer is admitted some 60 steps later, in the second leg)
    got, differed = trip_stats.vector_follow(vec, other, singles, models, BASELINE_AT, 40, "after turning on at step %d" % BASELINE_AT,
                                             rl=True, exact=False)
    assert differed
    for k in ("admitted", "finished"):
        assert got[k][HIGH:].min() > 0, (k, got[k][HIGH:])
    for e in (vec, other):
        e.track_trips(False)
    with pytest.raises(RuntimeError):
        vec.observe_trips_array()
    untracked_step(BASELINE_AT + 41)
    turn_on("turned on again")
    got, _ = trip_stats.vector_follow(vec, other, singles, models, BASELINE_AT + 41, 60, "after turning on again", rl=True, exact=False)
    for k in ("admitted", "admitted_buffer_steps", "finished"):
        assert got[k][HIGH:].min() > 0, (k, got[k][HIGH:])


def test_trips_baseline_twin_against_twins(mod, scen, workdir):
    trips_baseline_body(mod, vec_twin(mod), scen, workdir)


@pytest.mark.gpu
def test_trips_baseline_across_the_lds_table_on_the_device(mod, scen, workdir):
    t0 = time.perf_counter()
    trips_baseline_body(mod, vec_default(mod), scen, workdir)
    print("trips baseline example_1x1 x%d: %.1f s" % (R, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------ 2. random call sequences, and the plan
def vector_sequence(mod, make_vec, scen, workdir, where):
    vec, cfgs = sequences.vector_engines(scen, workdir, make_vec, "example_1x1", R)
    return sequences.run_vector_sequence(vec, [twin(mod, c) for c in cfgs], sequences.VECTOR_SEEDS["example_1x1", R],
                                         sequences.VECTOR_ROUNDS, where)


def test_vector_sequence_twin_against_twins(mod, scen, workdir):
    vector_sequence(mod, vec_twin(mod), scen, workdir, "vector x%d twin" % R)


@pytest.mark.gpu
def test_vector_sequence_equals_standalone_twins(mod, scen, workdir):
    t0 = time.perf_counter()
    vector_sequence(mod, vec_default(mod), scen, workdir, "vector x%d" % R)
    print("vector example_1x1 x%d: %.1f s" % (R, time.perf_counter() - t0))


@pytest.mark.parametrize("net,envs,interval", sorted(sequences.VECTOR_PLAN_SEEDS))
def test_vector_plan_sequence_stream_on_the_driven_twins(mod, scen, workdir, net, envs, interval):
    _, singles, cfg = sequences.vector_plan_engines(mod, scen, workdir, net, envs, interval, None)
    sequences.run_vector_plan_sequence(None, singles, cfg, sequences.VECTOR_PLAN_SEEDS[net, envs, interval],
                                       sequences.VECTOR_PLAN_ROUNDS, interval, "plan %s x%d" % (net, envs))


@pytest.mark.gpu
@pytest.mark.parametrize("net,envs,interval", sorted(sequences.VECTOR_PLAN_SEEDS))
def test_vector_plan_sequence_equals_pass_time_and_the_driven_twins(mod, scen, workdir, net, envs, interval):
    vec, singles, cfg = sequences.vector_plan_engines(mod, scen, workdir, net, envs, interval, lambda c, n: on_device(vec_default(mod)(c, n)))
    t0 = time.perf_counter()
    sequences.run_vector_plan_sequence(vec, singles, cfg, sequences.VECTOR_PLAN_SEEDS[net, envs, interval],
                                       sequences.VECTOR_PLAN_ROUNDS, interval, "plan %s x%d" % (net, envs))
    print("plan %s x%d %s s: %.1f s" % (net, envs, interval, time.perf_counter() - t0))


@pytest.mark.gpu
def test_a_rejection_names_an_env_beyond_64(mod, scen, workdir):
    """tests/test_tl_plan.py::test_a_rejection_names_the_env_on_a_vector_engine at 67 environments: the invalid entry sits in
    environment 65 among 66 valid plans that all differ; none of them is applied, and the next valid call is."""
    cfg = scen.materialize("example_1x1", workdir)
    vec = on_device(vec_default(mod)(cfg, R))
    t0 = time.perf_counter()
    plan = Plan(twin(mod, cfg), cfg)
    i = plan.real[0]
    assert plan.count[i] > 3
    base = np.stack([plan.file()] * R)
    for s in range(5):
        vec.next_step()
    before = vec._tl_state()
    d = np.stack([plan.other(k) for k in range(R)])
    assert len({d[r].tobytes() for r in range(R)}) > 8
    d[65, i, 3] = -1.0
    vec.set_tl_plan_tensor(durations=dev(vec, d), phase_remain=dev(vec, d[:, :, 0]))
    with pytest.raises(ValueError) as err:
        vec.sync()
    for w in ("durations", "'%s'" % plan.ids[i], "phase 3", "env 65", "not applied"):
        assert w in str(err.value), str(err.value)
    assert np.array_equal(durations_of(vec), base), "durations changed in an environment"
    p = np.full((R, plan.I), -1, dtype=np.int64)
    p[:, i] = np.arange(R) % plan.count[i]
    p[65, i] = plan.count[i]
    vec.set_tl_plan_tensor(phase=dev(vec, p))
    with pytest.raises(ValueError) as err:
        vec.get_lane_vehicle_count_array()  # (any call that waits for the device)
    for w in ("phase", "'%s'" % plan.ids[i], "env 65", "not applied"):
        assert w in str(err.value), str(err.value)
    rem = np.full((R, plan.I), NAN)
    rem[:, i] = 1.0 + 0.25 * np.arange(R)
    rem[65, i] = -0.25
    vec.set_tl_plan_tensor(phase_remain=dev(vec, rem), durations=dev(vec, np.stack([plan.other(k) for k in range(R)])))
    with pytest.raises(ValueError) as err:
        vec.sync()
    for w in ("phase_remain", "'%s'" % plan.ids[i], "env 65", "-0.25", "not applied"):
        assert w in str(err.value), str(err.value)
    after = vec._tl_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the lights changed in an environment"
    assert np.array_equal(durations_of(vec), base)
    # the next valid call applies, in environment 65 and in its neighbours, each with its own row
    d[65, i, 3] = 7.75
    p[65, i] = 1
    rem[65, i] = 0.5
    vec.set_tl_plan_tensor(durations=dev(vec, d), phase=dev(vec, p), phase_remain=dev(vec, rem))
    vec.sync()
    want = np.array(base)
    for r in range(R):
        want[r] = plan.other(r)
    want[65, i, 3] = 7.75
    assert np.array_equal(durations_of(vec), want)
    ph, re = vec._tl_state()
    assert np.array_equal(np.asarray(ph)[:, i], p[:, i]) and np.array_equal(np.asarray(re)[:, i], rem[:, i])
    print("rejection example_1x1 x%d: %.1f s" % (R, time.perf_counter() - t0))


# ------------------------------------------------------------------------------- 3. lane change under random control, batched
# The seed of the 67 case: the first below 20 with which, on the twins, four resets fall into the middle of lane changes and
# some step creates shadows in two or more of the environments 64 to 66.  Every seed below 20 gives steps that create some 400
# shadows in all (seed 3: 414): far more than the 64 by which k_lc_insert's rankOf strides over the step's insertions.
LANE_CHANGE_SEED, LANE_CHANGE_STEPS = 3, 200


def lane_change_body(mod, make_vec, scen, workdir, seed, envs, steps):
    held = vector_engine.lane_change_random_control(mod, scen, workdir, make_vec, seed, envs, steps)
    if envs > HIGH:
        assert any(sum(e >= HIGH for e in step) >= 2 for step in held["inserting_envs"]), \
            "no step created shadows in two environments from %d on" % HIGH
        assert held["most_inserted"] > 64, "no step created more than 64 shadows (%d)" % held["most_inserted"]


def test_lane_change_random_control_twin_against_twins(mod, scen, workdir):
    lane_change_body(mod, vec_twin(mod), scen, workdir, LANE_CHANGE_SEED, R, LANE_CHANGE_STEPS)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,envs,steps", [(1, 3, 260), (2, 3, 260), (LANE_CHANGE_SEED, R, LANE_CHANGE_STEPS)])
def test_lane_change_random_control_on_the_device(mod, scen, workdir, seed, envs, steps):
    t0 = time.perf_counter()
    lane_change_body(mod, vec_default(mod), scen, workdir, seed, envs, steps)
    print("lane change example_1x1 x%d seed %d: %.1f s" % (envs, seed, time.perf_counter() - t0))
