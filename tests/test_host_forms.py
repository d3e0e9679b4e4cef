"""The host forms of the observation and command calls, interleaved on ONE engine.

Every host form (get_lane_front_vehicles_array, observe_intersections_array, get_lane_vehicle_bins_array, get_lane_speed_sum_array,
observe_movement_flow_array, set_vehicle_speeds, set_tl_plan, get_tl_phase_durations_array) has a test file of its own that
calls it alone.  On the device library they all stage their host arrays in one arena (cfx_engine::stage, cfx_stage_layout.h),
so what could newly go wrong is one call's leftovers or sizes leaking into the next.  Here one engine takes them in turn with
request sizes that go up and down: 40 steps with the lane-flow and movement-flow trackers on, the sequence of SCRIPT, 5 steps,
the sequence again in reverse order.  Every return value is held with array_equal against the CPU twin driven in lockstep with
the same calls, and the whole state after the 5 steps and at the end (and once more a step later, when the last commands have
acted).  The unmarked tests run the same body with a second twin in the HIP engine's place and so hold the harness.

The twin has no signal plan calls, so set_tl_plan is held against its device form (set_tl_plan_tensor, which test_tl_plan.py
holds against its models and which stages nothing): two HIP engines of one config in lockstep, one given the plan from numpy
arrays between front-vehicle calls of changing size, the other from tensors."""
import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB, assert_same_state

torch = pytest.importorskip("torch")

from test_device_tensors import twin  # noqa: E402
from test_lane_flow import hip_engine, layout_config  # noqa: E402
from test_tl_plan import Plan, dev, on_device, same_lights  # noqa: E402

MAX_FRONT = 64  # CFX_MAX_LANE_FRONT
MAX_BINS = 32   # CFX_MAX_LANE_BINS
NAN = float("nan")


def same_dict(got, want, where):
    assert sorted(got) == sorted(want), "%s: %s against %s" % (where, sorted(got), sorted(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, "%s %s: %s %s against %s %s" % (where, k, g.dtype, g.shape, w.dtype, w.shape)
        assert np.array_equal(g, w), "%s: %s differs" % (where, k)


def same_rows(a, b, where):
    """observe_vehicles_array of both: every vehicle's number, drivable, environment, distance, speed, leader and gap."""
    ra, rb = a.observe_vehicles_array(), b.observe_vehicles_array()
    has = np.asarray(rb["leader"]) >= 0
    assert sorted(ra) == sorted(rb), where
    for k in rb:
        x, y = np.asarray(ra[k]), np.asarray(rb[k])
        assert x.shape == y.shape, "%s: %s holds %s against %s" % (where, k, x.shape, y.shape)
        if k == "gap":
            x, y = x[has], y[has]
        assert np.array_equal(x, y), "%s: vehicle rows, %s differs" % (where, k)


def same_state(a, b, where):
    """assert_same_state; a VectorEngine has no _vehicle_state(), there the vehicle rows carry every vehicle's state."""
    same_rows(a, b, where)
    if not hasattr(b, "num_envs"):
        assert_same_state(a, b, where)
        return
    assert np.array_equal(a.get_lane_vehicle_count_array(), b.get_lane_vehicle_count_array()), where + ": lane counts"
    assert np.array_equal(a.get_lane_waiting_vehicle_count_array(), b.get_lane_waiting_vehicle_count_array()), where + ": waiting counts"
    (pa, ra), (pb, rb) = a._tl_state(), b._tl_state()
    assert np.array_equal(pa, pb) and np.array_equal(ra, rb), where + ": traffic-light state differs"
    for r in range(b.num_envs):
        assert a.get_vehicle_speed(r) == b.get_vehicle_speed(r), "%s: env %d vehicle speeds" % (where, r)
    sa, sb = a._scalars(), b._scalars()
    for k in ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time"):
        assert sa[k] == sb[k], "%s: scalar %s differs (%r vs %r)" % (where, k, sa[k], sb[k])


def running(b):
    v = np.asarray(b.observe_vehicles_array()["vehicle"]).reshape(-1)
    return v[v >= 0].astype(np.int32)


def one_row(b, rng):
    live = running(b)
    return live[len(live) // 2:len(live) // 2 + 1], rng.uniform(0.0, 12.0, 1)


def every_vehicle(b, rng):
    """Every running vehicle, then a padding row, a masked row and one vehicle named a second time (the higher row wins)."""
    live = running(b)
    vehicle = np.concatenate([live, np.array([-1, live[0], live[-1]], dtype=np.int32)]).astype(np.int32)
    speed = rng.uniform(0.0, 12.0, len(vehicle))
    speed[len(live)] = 5.0
    speed[len(live) + 1] = NAN
    return vehicle, speed


def speeds(rows):
    def call(e, b, rng):
        vehicle, speed = rows(b, rng)  # (from the twin: both engines are given the same rows)
        return {"ignored": np.int64(e.set_vehicle_speeds(vehicle, speed)), "rows": np.int64(len(vehicle))}
    return call


def script(edges):
    """[(name, call(engine, twin, rng) -> dict of arrays)]"""
    return [
        ("fronts 1", lambda e, b, rng: e.get_lane_front_vehicles_array(1)),
        ("intersections", lambda e, b, rng: e.observe_intersections_array()),
        ("fronts 64", lambda e, b, rng: e.get_lane_front_vehicles_array(MAX_FRONT)),  # (the arena grows)
        ("bins 32", lambda e, b, rng: {"bins": e.get_lane_vehicle_bins_array(edges)}),
        ("speed sum", lambda e, b, rng: {"speed_sum": e.get_lane_speed_sum_array()}),
        ("fronts 1 again", lambda e, b, rng: e.get_lane_front_vehicles_array(1)),  # (small after large)
        ("movement flow", lambda e, b, rng: e.observe_movement_flow_array(reset=False)),
        ("movement flow, reset", lambda e, b, rng: e.observe_movement_flow_array(reset=True)),
        ("speeds, one row", speeds(one_row)),
        ("speeds, every vehicle", speeds(every_vehicle)),
    ]


def interleaved_body(a, b, where, seed=17):
    """`a`: the engine under test; `b`: the twin it is held against."""
    L = len(b.lane_ids())
    # a row of edges per lane, neighbouring lanes' rows differ; the last bin is open
    edges = b.lane_lengths()[:, None] * np.append(np.arange(MAX_BINS) / MAX_BINS, np.inf) * (0.7 + 0.1 * (np.arange(L) % 4))[:, None]
    assert edges.shape == (L, MAX_BINS + 1)
    for e in (a, b):
        e.track_lane_flow(True)
        e.track_movement_flow(True)
    for _ in range(40):
        a.next_step()
        b.next_step()
    assert len(running(b)) > 2, where + ": no traffic"
    calls = script(edges)
    seen = {"moved": 0, "fronts": 0}
    for leg, order in (("forward", calls), ("reverse", calls[::-1])):
        rng_a, rng_b = np.random.default_rng(seed), np.random.default_rng(seed)
        for name, call in order:
            at = "%s, %s, %s" % (where, leg, name)
            want = call(b, b, rng_b)
            got = call(a, b, rng_a)
            same_dict(got, want, at)
            if name == "movement flow":
                seen["moved"] += int(want["left"].sum())
            if name == "fronts 64":
                assert sorted(want) == ["front_distance", "front_lane_steps", "front_speed", "front_waiting_steps"], at
                seen["fronts"] += int((want["front_distance"] >= 0).sum())
            if name.startswith("speeds"):
                assert want["ignored"] == 0, at
        if leg == "forward":
            for _ in range(5):
                a.next_step()
                b.next_step()
            same_state(a, b, where + ", after the 5 steps")
    same_state(a, b, where + ", at the end")
    a.next_step()
    b.next_step()
    same_state(a, b, where + ", a step after the end")
    assert seen["moved"] > 0 and seen["fronts"] > 0, "%s: %s" % (where, seen)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_interleaved_twin_against_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    interleaved_body(twin(mod, cfg), twin(mod, cfg), "grid_6x6 twin")


def test_interleaved_vector_twin_against_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    make = lambda: mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB)  # noqa: E731
    interleaved_body(make(), make(), "grid_6x6 x3 twin")


# ---------------------------------------------------------------------------------------------------------------- GPU
CASES = [("grid_6x6", "auto"), ("grid_6x6", "dense"), ("example_1x1", "auto")]


@pytest.mark.gpu
@pytest.mark.parametrize("net,layout", CASES)
def test_interleaved_host_forms_equal_the_twin(mod, scen, workdir, net, layout):
    cfg = layout_config(scen, workdir, net, layout)
    interleaved_body(hip_engine(mod, cfg, layout), twin(mod, cfg), "%s %s" % (net, layout))


@pytest.mark.gpu
def test_interleaved_host_forms_vector_engine(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    vec = mod.VectorEngine(cfg, 3)
    assert SHADOW_GPU or vec.backend_name() == "hip-gfx950"
    interleaved_body(vec, mod.VectorEngine._with_backend(cfg, 3, 1, TWIN_LIB), "grid_6x6 x3")


@pytest.mark.gpu
@pytest.mark.parametrize("net,layout", CASES)
def test_plan_from_arrays_between_front_calls_equals_the_tensor_form(mod, scen, workdir, net, layout):
    cfg = layout_config(scen, workdir, net, layout)
    a, b = on_device(hip_engine(mod, cfg, layout)), hip_engine(mod, cfg, layout)
    where = "%s %s" % (net, layout)
    plan = Plan(a, cfg)
    T1, T2 = plan.other(1), plan.other(2)
    assert not np.array_equal(T1, T2) and not np.array_equal(T2, plan.file())
    phase = np.array([i % c if c else -1 for i, c in enumerate(plan.count)], dtype=np.int32)
    remain = 2.0 + 0.5 * (np.arange(plan.I) % 4)
    later = remain[::-1] + 1.0

    def fronts(k, at):
        same_dict(a.get_lane_front_vehicles_array(k), b.get_lane_front_vehicles_array(k), "%s: fronts %d %s" % (where, k, at))

    for _ in range(40):
        a.next_step()
        b.next_step()
    fronts(1, "before the plan")
    a.set_tl_plan(durations=plan.dirty(T1), phase=phase, phase_remain=remain)
    b.set_tl_plan_tensor(durations=dev(b, plan.dirty(T1)), phase=dev(b, phase), phase_remain=dev(b, remain))
    fronts(MAX_FRONT, "after the whole plan")
    a.set_tl_plan(durations=plan.dirty(T2))
    b.set_tl_plan_tensor(durations=dev(b, plan.dirty(T2)))
    assert np.array_equal(a.get_tl_phase_durations_array(), T2), where + ": the durations right after the call"
    fronts(1, "after the durations")
    a.set_tl_plan(phase_remain=later)
    b.set_tl_plan_tensor(phase_remain=dev(b, later))
    b.sync()
    same_lights(a, b, where + ", after the plan calls")
    assert np.array_equal(np.asarray(a._tl_state()[1])[plan.real], later[plan.real]), where + ": the remaining times are the last call's"
    for s in range(20):
        a.next_step()
        b.next_step()
        same_lights(a, b, "%s, step %d" % (where, s))
    fronts(MAX_FRONT, "after 20 steps")
    got = a.get_tl_phase_durations_array()
    assert np.array_equal(got, b.get_tl_phase_durations_tensor().cpu().numpy()), where + ": durations, array form against tensor form"
    assert np.array_equal(got, T2), where + ": durations in force"
    assert_same_state(a, b, where + ", 20 steps after the plan")
