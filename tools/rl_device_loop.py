"""RL loop with a torch policy on the GPU: the numpy calls (observation to the host and into torch, phases back through the
host) against the tensor calls (get_lane_*_tensor / set_tl_phases_tensor: no host wait).  us per iteration, on the headline
RL network (bench.py's 30x30 workload, rlTrafficLight) and on VectorEngine 16 x the same.
usage: python tools/rl_device_loop.py [--iters N] [--envs R]      (the probe tools/rl_probe.py is the numpy side's own story)
       python tools/rl_device_loop.py --features [--features-only all|counts_waiting]
--features: observe_lanes_tensor (one launch of kr_lane_features) against the two count getters, on the Engine only;
--features-only runs just that observe_lanes_tensor loop (with all four outputs, B = 3, or counts + waiting), for a kernel trace;
--lib PATH runs either on another build of the device library.
       python tools/rl_device_loop.py --intersections [--runs N] [--intersections-only lanes|four|seven|no_waiting]
--intersections: a max-pressure loop built two ways, alternated --runs times — A: observe_lanes_tensor(counts, waiting) and torch
ops over index tensors made once (movement_in, movement_in_waiting, movement_out, phase_pressure); B: observe_intersections_tensor
with the same four outputs (one launch of kr_intersection_features), and with all seven; A's tensors are asserted equal to B's
first.  --intersections-only runs one of the loops alone, for a kernel trace.
       python tools/rl_device_loop.py --lane-flow [--runs N] [--lane-flow-only trace]
--lane-flow: what track_lane_flow costs and saves — next_step alone with tracking off and on, alternated --runs times; then a
max-pressure loop whose reward (vehicles that left each lane, and the steps they waited there) comes from
observe_lane_flow_tensor(left, left_waiting_steps, reset=True), against the same loop with the reward built from
get_lane_vehicles() + get_vehicle_speed() and a Python diff every step; both rewards are asserted equal first.
--lane-flow-only trace runs next_step + observe_lanes_tensor(counts, waiting) + observe_lane_flow_tensor(reset=True) alone, so
that a kernel trace shows kr_lane_features, kr_lane_flow and k_lane_flow_drain side by side.
       python tools/rl_device_loop.py --fronts [--runs N] [--fronts-only four|k8|k32|all8|all32|fronts32]
--fronts: what the front-K outputs of observe_lanes_tensor cost and replace — the launch alone (host clock, 1 launch + events) with
the four per-lane outputs, with front_distance + front_speed added at K = 8 and K = 32, with all four front outputs added
(tracking on), alternated --runs times; then the host path on the same state: get_lane_vehicles() + get_vehicle_distance() +
get_vehicle_speed() and a Python gather of the first K per lane, asserted equal to the tensors first.  --fronts-only runs one
output set in the observe -> policy -> set -> next_step loop of --features-only, for a kernel trace (`four` runs on any
version of the package: it is the launch --features-only all measures).
       python tools/rl_device_loop.py --trips [--runs N] [--envs R] [--skip-vector | --skip-single] [--trips-only trace]
--trips: what track_trips costs and replaces, on the Engine and on VectorEngine --envs x the same — tracking is on from the first
step, and get_average_travel_time_tensor() is asserted equal to Engine.get_average_travel_time() after the warm-up steps; then
next_step alone with tracking off and on, alternated --runs times; then get_average_travel_time_tensor() per call against
Engine.get_average_travel_time() per call on the same state.  --trips-only trace runs next_step + observe_trips_tensor(all nine)
alone, so that a kernel trace shows k_trip_tick and k_trip_drain beside the step's kernels.
       python tools/rl_device_loop.py --movement-flow [--runs N] [--movement-flow-only trace]
--movement-flow: what track_movement_flow costs and saves — next_step alone with tracking off and on, alternated --runs times;
then a max-pressure loop whose reward (vehicles that crossed a stop line, and the steps they waited on their approach lane)
comes from observe_movement_flow_tensor(entered, entered_lane_waiting_steps, reset=True), against the same loop with the reward
built from _vehicle_state() and a numpy diff every step; both rewards are asserted equal over 12 steps first.
--movement-flow-only trace runs next_step + observe_lane_flow_tensor(reset=True) + observe_movement_flow_tensor(reset=True) alone,
so that a kernel trace shows kr_lane_flow, k_lane_flow_drain, kr_movement_flow and k_movement_flow_drain side by side.
       python tools/rl_device_loop.py --detectors [--runs N] [--lib PATH] [--detectors-only trace]
--detectors: what track_detectors costs and saves, with two detectors on every lane, (len - 10, inf) and (len - 100, len - 90) —
next_step alone with tracking off and on (and, with --lib, tracking off on that other build of the device library), alternated
--runs times; observe_detectors_tensor(all six, reset=True) alone; then a decision loop that drains every 10 steps against
get_lane_vehicles() + get_vehicle_distance() + get_vehicle_speed() after every step and the same numbers computed in Python;
both loops set the lights by max pressure at every drain, and the two are asserted equal over four decisions first.
--detectors-only trace runs next_step + observe_detectors_tensor alone, so that a kernel trace shows kr_detectors and
k_detectors_drain beside the step's kernels."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=400)
ap.add_argument("--envs", type=int, default=16)
ap.add_argument("--skip-vector", action="store_true")
ap.add_argument("--features", action="store_true")
ap.add_argument("--features-only", choices=["all", "counts_waiting"], default=None)
ap.add_argument("--intersections", action="store_true")
ap.add_argument("--intersections-only", choices=["lanes", "four", "seven", "no_waiting"], default=None)
ap.add_argument("--lane-flow", action="store_true")
ap.add_argument("--lane-flow-only", choices=["trace"], default=None)
ap.add_argument("--fronts", action="store_true")
ap.add_argument("--fronts-only", choices=["four", "k8", "k32", "all8", "all32", "fronts32"], default=None)
ap.add_argument("--trips", action="store_true")
ap.add_argument("--trips-only", choices=["trace"], default=None)
ap.add_argument("--movement-flow", action="store_true")
ap.add_argument("--movement-flow-only", choices=["trace"], default=None)
ap.add_argument("--detectors", action="store_true")
ap.add_argument("--detectors-only", choices=["trace"], default=None)
ap.add_argument("--skip-single", action="store_true", help="--trips: the VectorEngine alone")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--lib", default="", help="--features: a differently built device library (an A/B against another build)")
args = ap.parse_args()
sys.argv = [sys.argv[0]]
import bench  # noqa: E402
import torch  # noqa: E402
from cityflow_amd import _cityflow  # noqa: E402

cfg = bench.with_config(bench.build_workload("/tmp/cfa_rl_dev", 0), "rl", rlTrafficLight=True)


def measure(label, eng, body, n):
    for s in range(20):
        body(s)
    eng.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(n):
        body(s)
    eng.sync()
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / n * 1e6
    print("%-66s %8.1f us" % (label, us), flush=True)
    return us


def loops(name, eng, n):
    handle, dev = eng._stream_handle()
    device = torch.device("cuda", dev)
    n_phases = torch.from_numpy(eng._phase_counts()).to(device).long()
    npos = torch.clamp(n_phases, min=1)
    obs_shape = tuple(eng._tensor_shapes()[0])
    L = obs_shape[-1]
    I = n_phases.shape[0]
    idx = (torch.arange(I, device=device) * 7) % L
    envs = obs_shape[0] if len(obs_shape) == 2 else 0

    def policy(c, w, s):  # trivial: one lane's count (+ waiting) picks each signal's phase
        if envs:
            p = (c[:, idx].long() + w[:, idx].long() + s) % npos
            return torch.where(n_phases >= 0, p, -1)
        p = (c[idx].long() + w[idx].long() + s) % npos
        return torch.where(n_phases >= 0, p, -1)

    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    measure("next_step alone", eng, lambda s: eng.next_step(), n)

    def numpy_iter(s):
        c = torch.from_numpy(eng.get_lane_vehicle_count_array()).to(device)
        w = torch.from_numpy(eng.get_lane_waiting_vehicle_count_array()).to(device)
        eng.set_tl_phases(policy(c, w, s).to(torch.int32).cpu().numpy())
        eng.next_step()

    out_c = torch.empty(obs_shape, dtype=torch.int32, device=device)
    out_w = torch.empty(obs_shape, dtype=torch.int32, device=device)

    def tensor_iter(s):
        c = eng.get_lane_vehicle_count_tensor(out=out_c)
        w = eng.get_lane_waiting_vehicle_count_tensor(out=out_w)
        eng.set_tl_phases_tensor(policy(c, w, s))
        eng.next_step()

    a = measure("numpy loop: 2 array getters -> torch policy -> set_tl_phases -> next_step", eng, numpy_iter, n)
    b = measure("tensor loop: 2 tensor getters -> torch policy -> set_tl_phases_tensor -> next_step", eng, tensor_iter, n)
    measure("tensor getters alone (2 launches + events, no step)", eng,
            lambda s: (eng.get_lane_vehicle_count_tensor(out=out_c), eng.get_lane_waiting_vehicle_count_tensor(out=out_w)), n)
    ph = policy(out_c, out_w, 0)
    measure("set_tl_phases_tensor alone (1 launch + event, no step)", eng, lambda s: eng.set_tl_phases_tensor(ph), n)
    measure("torch policy alone", eng, lambda s: policy(out_c, out_w, s), n)
    print("%-66s %8.2fx" % ("numpy loop / tensor loop", a / b), flush=True)


def features(name, eng, n, only):
    device = torch.device("cuda", eng._stream_handle()[1])
    n_phases = torch.from_numpy(eng._phase_counts()).to(device).long()
    npos = torch.clamp(n_phases, min=1)
    L = len(eng.lane_ids())
    idx = (torch.arange(n_phases.shape[0], device=device) * 7) % L
    edges = torch.from_numpy(eng.lane_lengths()[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, np.inf])).to(device)

    def policy(c, w, s):  # as loops(): the same few eager ops whichever call produced c and w
        return torch.where(n_phases >= 0, (c[idx].long() + w[idx].long() + s) % npos, -1)

    out_c = torch.empty(L, dtype=torch.int32, device=device)
    out_w = torch.empty(L, dtype=torch.int32, device=device)
    out_s = torch.empty(L, dtype=torch.float64, device=device)
    out_b = torch.empty((L, 3), dtype=torch.int32, device=device)

    def obs_cw():
        eng.observe_lanes_tensor(counts=out_c, waiting=out_w)

    def obs_all():
        eng.observe_lanes_tensor(counts=out_c, waiting=out_w, speed_sum=out_s, bins=out_b, edges=edges)

    def getters():
        eng.get_lane_vehicle_count_tensor(out=out_c)
        eng.get_lane_waiting_vehicle_count_tensor(out=out_w)

    def loop(observe):
        def body(s):
            observe()
            eng.set_tl_phases_tensor(policy(out_c, out_w, s))
            eng.next_step()
        return body

    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    if only:
        measure("observe_lanes_tensor loop, outputs: %s" % only, eng, loop(obs_all if only == "all" else obs_cw), n)
        return
    measure("next_step alone", eng, lambda s: eng.next_step(), n)
    a = measure("2 count getters -> torch policy -> set_tl_phases_tensor -> next_step", eng, loop(getters), n)
    b = measure("observe_lanes_tensor(counts, waiting) -> policy -> set -> next_step", eng, loop(obs_cw), n)
    c = measure("observe_lanes_tensor(all four, B=3) -> policy -> set -> next_step", eng, loop(obs_all), n)
    measure("2 count getters alone (2 launches + events, no step)", eng, lambda s: getters(), n)
    measure("observe_lanes_tensor(counts, waiting) alone (1 launch + events)", eng, lambda s: obs_cw(), n)
    measure("observe_lanes_tensor(all four, B=3) alone (1 launch + events)", eng, lambda s: obs_all(), n)
    print("%-66s %8.2fx" % ("2 getters loop / observe_lanes_tensor(counts, waiting) loop", a / b), flush=True)
    print("%-66s %8.2fx" % ("2 getters loop / observe_lanes_tensor(all four) loop", a / c), flush=True)


def intersections(name, eng, n, runs, only):
    device = torch.device("cuda", eng._stream_handle()[1])
    lay = eng.intersection_layout()
    L = len(eng.lane_ids())
    I, P, M = lay["phase_avail"].shape
    pad = torch.iinfo(torch.int32).min
    # loop A's tables: lane indices with the padding pointing at one extra, always-zero element behind the counts
    in_idx = torch.from_numpy(np.where(lay["in_lanes"] >= 0, lay["in_lanes"], L)).to(device).long()
    out_idx = torch.from_numpy(np.where(lay["out_lanes"] >= 0, lay["out_lanes"], L)).to(device).long()
    avail = torch.from_numpy(lay["phase_avail"].astype(np.int32)).to(device)
    no_phase = torch.from_numpy(np.arange(P)[None, :] >= np.maximum(lay["n_phases"], 0)[:, None]).to(device)
    c1 = torch.zeros(L + 1, dtype=torch.int32, device=device)
    w1 = torch.zeros(L + 1, dtype=torch.int32, device=device)
    a_out = {}

    def loop_a(s):
        eng.observe_lanes_tensor(counts=c1[:L], waiting=w1[:L])
        a_out["in"] = c1[in_idx].sum(-1, dtype=torch.int32)
        a_out["wait"] = w1[in_idx].sum(-1, dtype=torch.int32)
        a_out["out"] = c1[out_idx].sum(-1, dtype=torch.int32)
        pp = (avail * (a_out["in"] - a_out["out"])[:, None, :]).sum(-1, dtype=torch.int32)
        a_out["pp"] = pp.masked_fill(no_phase, pad)
        eng.set_tl_phases_tensor(a_out["pp"].argmax(-1))
        eng.next_step()

    b = {k: torch.empty((I, M), dtype=torch.int32, device=device) for k in ("in", "wait", "out", "inside")}
    b["pp"] = torch.empty((I, P), dtype=torch.int32, device=device)
    b["phase"] = torch.empty(I, dtype=torch.int32, device=device)
    b["remain"] = torch.empty(I, dtype=torch.float64, device=device)

    def observe_four():
        eng.observe_intersections_tensor(movement_in=b["in"], movement_in_waiting=b["wait"], movement_out=b["out"],
                                         phase_pressure=b["pp"])

    def loop_b(observe):
        def body(s):
            observe()
            eng.set_tl_phases_tensor(b["pp"].argmax(-1))
            eng.next_step()
        return body

    def observe_seven():
        eng.observe_intersections_tensor(phase=b["phase"], phase_remain=b["remain"], movement_in=b["in"], movement_in_waiting=b["wait"],
                                         movement_out=b["out"], movement_inside=b["inside"], phase_pressure=b["pp"])

    def observe_no_waiting():
        eng.observe_intersections_tensor(phase=b["phase"], phase_remain=b["remain"], movement_in=b["in"], movement_out=b["out"],
                                         movement_inside=b["inside"], phase_pressure=b["pp"])

    def lanes_only(s):  # (kr_lane_features beside the new kernel in one trace)
        eng.observe_lanes_tensor(counts=c1[:L], waiting=w1[:L])
        eng.next_step()

    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    if only:
        body = {"lanes": lanes_only, "four": loop_b(observe_four), "seven": loop_b(observe_seven),
                "no_waiting": loop_b(observe_no_waiting)}[only]
        measure("intersections loop: %s" % only, eng, body, n)
        return
    observe_four()
    loop_a(0)  # (observes the same state, then steps)
    torch.cuda.synchronize()
    for k in ("in", "wait", "out", "pp"):
        assert torch.equal(a_out[k], b[k]), "loop A's %s differs from observe_intersections_tensor's" % k
    print("loop A's four tensors equal loop B's", flush=True)
    measure("next_step alone", eng, lambda s: eng.next_step(), n)
    res = {"A": [], "B4": [], "B7": []}
    for r in range(runs):
        res["A"].append(measure("A  observe_lanes_tensor + torch ops -> argmax -> set -> next_step (run %d)" % r, eng, loop_a, n))
        res["B4"].append(measure("B  observe_intersections_tensor(4) -> argmax -> set -> next_step (run %d)" % r, eng, loop_b(observe_four), n))
        res["B7"].append(measure("B  observe_intersections_tensor(7) -> argmax -> set -> next_step (run %d)" % r, eng, loop_b(observe_seven), n))
    measure("observe_intersections_tensor(7) alone (1 launch + events)", eng, lambda s: observe_seven(), n)
    measure("observe_lanes_tensor(counts, waiting) alone (1 launch + events)", eng,
            lambda s: eng.observe_lanes_tensor(counts=c1[:L], waiting=w1[:L]), n)
    for k, v in res.items():
        print("%-4s median %8.1f us   min %8.1f   max %8.1f   (spread %.1f)" % (k, float(np.median(v)), min(v), max(v), max(v) - min(v)),
              flush=True)


def lane_flow(name, eng, n, runs, only):
    device = torch.device("cuda", eng._stream_handle()[1])
    lay = eng.intersection_layout()
    L = len(eng.lane_ids())
    I, P, M = lay["phase_avail"].shape
    pp = torch.empty((I, P), dtype=torch.int32, device=device)
    left = torch.empty(L, dtype=torch.int32, device=device)
    left_wait = torch.empty(L, dtype=torch.int64, device=device)
    c = torch.empty(L, dtype=torch.int32, device=device)
    w = torch.empty(L, dtype=torch.int32, device=device)
    reward = {}

    def control():
        eng.observe_intersections_tensor(phase_pressure=pp)
        eng.set_tl_phases_tensor(pp.argmax(-1))
        eng.next_step()

    def tensor_loop(s):
        control()
        eng.observe_lane_flow_tensor(left=left, left_waiting_steps=left_wait, reset=True)
        reward["tensor"] = torch.stack((left.sum(), left_wait.sum()))  # (stays on the device)

    lanes = eng.lane_ids()
    on = {}  # lane -> {vehicle: steps waited on it}

    def python_reward():
        lv, speed = eng.get_lane_vehicles(), eng.get_vehicle_speed()
        n_left = waited = 0
        for lane in lanes:
            prev, now = on.get(lane, {}), lv[lane]
            cur = {v: prev.get(v, 0) + (speed[v] < 0.1) for v in now}
            gone = [v for v in prev if v not in cur]
            n_left += len(gone)
            waited += sum(prev[v] for v in gone)
            on[lane] = cur
        return n_left, waited

    def python_loop(s):
        control()
        reward["python"] = python_reward()

    def trace(s):
        eng.next_step()
        eng.observe_lanes_tensor(counts=c, waiting=w)
        eng.observe_lane_flow_tensor(left=left, left_waiting_steps=left_wait, reset=True)

    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    if only:
        eng.track_lane_flow(True)
        measure("next_step + observe_lanes_tensor(counts, waiting) + observe_lane_flow_tensor(2, reset)", eng, trace, n)
        return
    res = {"off": [], "on": []}
    for r in range(runs):
        eng.track_lane_flow(False)
        res["off"].append(measure("next_step alone, tracking off (run %d)" % r, eng, lambda s: eng.next_step(), n))
        eng.track_lane_flow(True)
        res["on"].append(measure("next_step alone, tracking on  (run %d)" % r, eng, lambda s: eng.next_step(), n))
    for k, v in res.items():
        print("%-4s median %8.1f us   min %8.1f   max %8.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("tracking on - off (medians) %8.1f us per step" % (float(np.median(res["on"])) - float(np.median(res["off"]))), flush=True)
    measure("observe_lane_flow_tensor(left, left_waiting_steps, reset) alone (1 launch + events)", eng,
            lambda s: eng.observe_lane_flow_tensor(left=left, left_waiting_steps=left_wait, reset=True), n)
    # both rewards from one engine, step by step, before anything is timed
    eng.track_lane_flow(False)
    eng.track_lane_flow(True)  # (a baseline for both)
    on.clear()
    on.update({lane: {v: 0 for v in vs} for lane, vs in eng.get_lane_vehicles().items()})
    total = 0
    for s in range(12):
        control()
        eng.observe_lane_flow_tensor(left=left, left_waiting_steps=left_wait, reset=True)
        got, want = (int(left.sum()), int(left_wait.sum())), python_reward()
        assert got == want, "step %d: the tensor reward %s is not the Python diff's %s" % (s, got, want)
        total += want[0]
    assert total > 0
    print("the two rewards are equal over 12 steps (%d vehicles left a lane)" % total, flush=True)
    n_py = max(n // 20, 10)
    res = {"tensor": [], "python": []}
    for r in range(runs):
        res["tensor"].append(measure("observe_intersections -> argmax -> set -> next_step -> observe_lane_flow_tensor (run %d)" % r, eng, tensor_loop, n))
        res["python"].append(measure("... -> next_step -> get_lane_vehicles + get_vehicle_speed + Python diff (run %d)" % r, eng, python_loop, n_py))
    for k, v in res.items():
        print("%-6s median %10.1f us   min %10.1f   max %10.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("python loop / tensor loop %8.1fx" % (float(np.median(res["python"])) / float(np.median(res["tensor"]))), flush=True)


def detectors(name, eng, parent, n, runs, only):
    """`parent`: an engine on another build of the device library (--lib), never tracked, or None."""
    device = torch.device("cuda", eng._stream_handle()[1])
    lanes, length = eng.lane_ids(), eng.lane_lengths()
    L = len(lanes)
    # two detectors on every lane: a stop-bar zone and an advance detector
    lane = np.repeat(np.arange(L, dtype=np.int32), 2)
    start = np.stack((np.maximum(length - 10.0, 0.0), np.maximum(length - 100.0, 0.0)), axis=1).reshape(-1)
    end = np.stack((np.full(L, np.inf), np.maximum(length - 90.0, 1.0)), axis=1).reshape(-1)
    N = len(lane)
    dtypes = {"passed": torch.int32, "occupied_steps": torch.int32, "vehicle_steps": torch.int64, "waiting_vehicle_steps": torch.int64,
              "speed_sum": torch.float64, "count": torch.int32}
    out = {k: torch.empty(N, dtype=t, device=device) for k, t in dtypes.items()}
    every = 10

    lay = eng.intersection_layout()
    pp = torch.empty(lay["phase_avail"].shape[:2], dtype=torch.int32, device=device)

    def decide():  # (max pressure, so that the traffic keeps moving)
        eng.observe_intersections_tensor(phase_pressure=pp)
        eng.set_tl_phases_tensor(pp.argmax(-1))

    def tensor_loop(s):
        eng.next_step()
        if s % every == every - 1:
            eng.observe_detectors_tensor(reset=True, **out)
            decide()

    prev = {}  # lane -> {vehicle: distance}
    acc = {k: np.zeros(N, dtype=np.float64 if k == "speed_sum" else np.int64) for k in list(dtypes)[:5]}

    def python_tick():
        lv, dis, speed = eng.get_lane_vehicles(), eng.get_vehicle_distance(), eng.get_vehicle_speed()
        for i in range(N):
            lid, a, b = lanes[lane[i]], start[i], end[i]
            was, now = prev.get(lid, {}), lv[lid]
            here = set(now)
            passed = sum(1 for v in now if dis[v] >= a and (v not in was or was[v] < a)) + sum(1 for v, d in was.items() if v not in here and d < a)
            zone = [speed[v] for v in now if a <= dis[v] < b]
            t = 0.0
            for x in zone:
                t = t + x
            acc["passed"][i] += passed
            acc["occupied_steps"][i] += 1 if zone else 0
            acc["vehicle_steps"][i] += len(zone)
            acc["waiting_vehicle_steps"][i] += sum(1 for x in zone if x < 0.1)
            acc["speed_sum"][i] = acc["speed_sum"][i] + t
        prev.clear()
        prev.update({lid: {v: dis[v] for v in vs} for lid, vs in lv.items()})

    def python_loop(s):
        eng.next_step()
        python_tick()
        if s % every == every - 1:
            for a in acc.values():
                a[:] = 0
            decide()

    for _ in range(300):
        eng.next_step()
        if parent is not None:
            parent.next_step()
    eng.sync()
    print("# %s, %d detectors" % (name, N), flush=True)
    if only:
        eng.track_detectors(lane, start, end)
        measure("next_step + observe_detectors_tensor(6, reset) every step", eng,
                lambda s: (eng.next_step(), eng.observe_detectors_tensor(reset=True, **out)), n)
        return
    res = {"off": [], "on": [], "parent": []}
    for r in range(runs):
        if parent is not None:
            res["parent"].append(measure("next_step alone, the other library, tracking off (run %d)" % r, parent, lambda s: parent.next_step(), n))
        eng.track_detectors(on=False)
        res["off"].append(measure("next_step alone, tracking off (run %d)" % r, eng, lambda s: eng.next_step(), n))
        eng.track_detectors(lane, start, end)
        res["on"].append(measure("next_step alone, tracking on  (run %d)" % r, eng, lambda s: eng.next_step(), n))
    for k, v in res.items():
        if v:
            print("%-6s median %8.1f us   min %8.1f   max %8.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("tracking on - off (medians) %8.1f us per step" % (float(np.median(res["on"])) - float(np.median(res["off"]))), flush=True)
    drain = [measure("observe_detectors_tensor(6 outputs, reset) alone (1 launch + events) (run %d)" % r, eng,
                     lambda s: eng.observe_detectors_tensor(reset=True, **out), n) for r in range(runs)]
    print("drain  median %8.1f us   min %8.1f   max %8.1f" % (float(np.median(drain)), min(drain), max(drain)), flush=True)
    # both sets of numbers from one engine over four decisions, before anything is timed
    for s in range(4 * every):  # (the lights have stood still so far)
        tensor_loop(s)
    eng.track_detectors(lane, start, end)  # (a baseline for both)
    lv, dis = eng.get_lane_vehicles(), eng.get_vehicle_distance()
    prev.update({lid: {v: dis[v] for v in vs} for lid, vs in lv.items()})
    total = 0
    for s in range(4 * every):
        eng.next_step()
        python_tick()
        if s % every == every - 1:
            eng.observe_detectors_tensor(reset=True, **out)
            decide()
            for k, a in acc.items():
                assert np.array_equal(out[k].cpu().numpy(), a.astype(out[k].cpu().numpy().dtype)), "decision %d: %s differs" % (s // every, k)
                total += int(a.sum()) if k == "passed" else 0
                a[:] = 0
    assert total > 0
    print("the detector outputs equal the Python loop's over four decisions (%d passages)" % total, flush=True)
    n_py = max(n // 20, 2 * every)
    res = {"tensor": [], "python": []}
    for r in range(runs):
        res["tensor"].append(measure("next_step x 10 + observe_detectors_tensor(6, reset), per step (run %d)" % r, eng, tensor_loop, n))
        res["python"].append(measure("next_step + 3 getters + the same numbers in Python, per step (run %d)" % r, eng, python_loop, n_py))
    for k, v in res.items():
        print("%-6s median %10.1f us   min %10.1f   max %10.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("python loop / tensor loop %8.1fx" % (float(np.median(res["python"])) / float(np.median(res["tensor"]))), flush=True)


def fronts(name, eng, n, runs, only):
    device = torch.device("cuda", eng._stream_handle()[1])
    n_phases = torch.from_numpy(eng._phase_counts()).to(device).long()
    npos = torch.clamp(n_phases, min=1)
    lanes = eng.lane_ids()
    L = len(lanes)
    idx = (torch.arange(n_phases.shape[0], device=device) * 7) % L
    edges = torch.from_numpy(eng.lane_lengths()[:, None] * np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, np.inf])).to(device)
    four = {"counts": torch.empty(L, dtype=torch.int32, device=device), "waiting": torch.empty(L, dtype=torch.int32, device=device),
            "speed_sum": torch.empty(L, dtype=torch.float64, device=device), "bins": torch.empty((L, 3), dtype=torch.int32, device=device),
            "edges": edges}

    def front_outputs(k, tracker):
        t = {"front_distance": torch.empty((L, k), dtype=torch.float64, device=device),
             "front_speed": torch.empty((L, k), dtype=torch.float64, device=device)}
        if tracker:
            t["front_lane_steps"] = torch.empty((L, k), dtype=torch.int32, device=device)
            t["front_waiting_steps"] = torch.empty((L, k), dtype=torch.int32, device=device)
        return t

    sets = {"four": dict(four), "k8": dict(four, **front_outputs(8, False)), "k32": dict(four, **front_outputs(32, False)),
            "all8": dict(four, **front_outputs(8, True)), "all32": dict(four, **front_outputs(32, True)),
            "fronts32": front_outputs(32, False)}

    def host_path(k):
        lv, dist, speed = eng.get_lane_vehicles(), eng.get_vehicle_distance(), eng.get_vehicle_speed()
        d, v = np.full((L, k), -1.0), np.zeros((L, k))
        for l, lane in enumerate(lanes):
            for j, veh in enumerate(lv[lane][:k]):
                d[l, j], v[l, j] = dist[veh], speed[veh]
        return d, v

    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    if only:
        if only.startswith("all"):
            eng.track_lane_flow(True)
        out = sets[only]
        c, w = four["counts"], four["waiting"]
        if only == "fronts32":
            c.zero_()
            w.zero_()

        def body(s):
            eng.observe_lanes_tensor(**out)
            eng.set_tl_phases_tensor(torch.where(n_phases >= 0, (c[idx].long() + w[idx].long() + s) % npos, -1))
            eng.next_step()
        measure("observe_lanes_tensor loop, outputs: %s" % only, eng, body, n)
        return
    eng.track_lane_flow(True)
    for k in (8, 32):  # the tensors are what the host path gives, before anything is timed
        eng.observe_lanes_tensor(**sets["k%d" % k])
        d, v = host_path(k)
        assert np.array_equal(sets["k%d" % k]["front_distance"].cpu().numpy(), d) and np.array_equal(sets["k%d" % k]["front_speed"].cpu().numpy(), v)
    print("front_distance / front_speed equal the host path's at K = 8 and 32 (%d vehicles on lanes, fullest lane %d)"
          % (int(four["counts"].sum()), int(four["counts"].max())), flush=True)
    res = {k: [] for k in sets}
    for r in range(runs):
        for k, out in sets.items():
            res[k].append(measure("observe_lanes_tensor(%s) alone (1 launch + events) (run %d)" % (k, r), eng,
                                  lambda s, out=out: eng.observe_lanes_tensor(**out), n))
    for k, v in res.items():
        print("%-9s median %8.1f us   min %8.1f   max %8.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    for k in (8, 32):
        measure("host path: 3 dict getters + Python gather of the first %d per lane" % k, eng, lambda s, k=k: host_path(k), max(n // 40, 5))


def trips(name, eng, n, runs, only):
    device = torch.device("cuda", eng._stream_handle()[1])
    shape = tuple(eng._tensor_shapes()[0])[:-1]
    int64 = ("admitted_buffer_steps", "finished_travel_steps", "in_system_travel_steps")
    names = ("entered", "admitted", "admitted_buffer_steps", "finished", "finished_travel_steps", "in_system", "buffered",
             "in_system_travel_steps")
    out = {k: torch.empty(shape, dtype=torch.int64 if k in int64 else torch.int32, device=device) for k in names}
    out["average_travel_time"] = torch.empty(shape, dtype=torch.float64, device=device)
    avg = out["average_travel_time"]
    eng.track_trips(True)  # (from the first step on: only then is the average the reference's)
    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    eng.observe_trips_tensor(**out)
    torch.cuda.synchronize()
    print("after 300 steps: entered %d, admitted %d, finished %d, in_system %d, buffered %d" % tuple(
        int(out[k].sum()) for k in ("entered", "admitted", "finished", "in_system", "buffered")), flush=True)
    if not shape:
        want = eng.get_average_travel_time()
        assert float(avg) == want, "get_average_travel_time_tensor %r is not get_average_travel_time %r" % (float(avg), want)
        print("get_average_travel_time_tensor() == get_average_travel_time() == %.6f" % want, flush=True)
    if only:
        def trace(s):
            eng.next_step()
            eng.observe_trips_tensor(**out)
        measure("next_step + observe_trips_tensor(all nine)", eng, trace, n)
        return
    res = {"off": [], "on": []}
    for r in range(runs):
        eng.track_trips(False)
        res["off"].append(measure("next_step alone, tracking off (run %d)" % r, eng, lambda s: eng.next_step(), n))
        eng.track_trips(True)
        res["on"].append(measure("next_step alone, tracking on  (run %d)" % r, eng, lambda s: eng.next_step(), n))
    for k, v in res.items():
        print("%-4s median %8.1f us   min %8.1f   max %8.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("tracking on - off (medians) %8.1f us per step" % (float(np.median(res["on"])) - float(np.median(res["off"]))), flush=True)
    measure("get_average_travel_time_tensor(out) alone (1 launch + events)", eng, lambda s: eng.get_average_travel_time_tensor(out=avg), n)
    measure("observe_trips_tensor(all nine) alone (1 launch + events)", eng, lambda s: eng.observe_trips_tensor(**out), n)
    if not shape:
        measure("Engine.get_average_travel_time() alone (status bytes to the host, sort, sum)", eng,
                lambda s: eng.get_average_travel_time(), max(n // 20, 10))


def movement_flow(name, eng, n, runs, only):
    device = torch.device("cuda", eng._stream_handle()[1])
    lay = eng.intersection_layout()
    L = len(eng.lane_ids())
    I, P, M = lay["phase_avail"].shape
    pp = torch.empty((I, P), dtype=torch.int32, device=device)
    entered = torch.empty((I, M), dtype=torch.int32, device=device)
    lane_wait = torch.empty((I, M), dtype=torch.int64, device=device)
    left = torch.empty(L, dtype=torch.int32, device=device)
    reward = {}

    def control():
        eng.observe_intersections_tensor(phase_pressure=pp)
        eng.set_tl_phases_tensor(pp.argmax(-1))
        eng.next_step()

    def tensor_loop(s):
        control()
        eng.observe_movement_flow_tensor(entered=entered, entered_lane_waiting_steps=lane_wait, reset=True)
        reward["tensor"] = torch.stack((entered.sum(), lane_wait.sum()))  # (stays on the device)

    # the same reward by vehicle number over _vehicle_state(): the drivable and the steps waited on it at the last step
    host = {"drv": np.full(0, -1, dtype=np.int64), "wait": np.zeros(0, dtype=np.int64)}

    def numpy_reward(baseline=False):
        st = eng._vehicle_state()
        vid, drv = st["vid"].astype(np.int64), st["drivable"].astype(np.int64)
        size = max(int(vid.max()) + 1 if vid.size else 0, host["drv"].size)
        grow = size - host["drv"].size
        prev = np.concatenate([host["drv"], np.full(grow, -1, dtype=np.int64)])
        wait = np.concatenate([host["wait"], np.zeros(grow, dtype=np.int64)])
        now = np.full(size, -1, dtype=np.int64)
        now[vid] = drv
        slow = np.zeros(size, dtype=bool)
        slow[vid] = st["speed"] < 0.1
        new = (now != prev) & (now >= 0)
        # (lane -> lane inside one step: the vehicle crossed the whole laneLink that joins the two, and a route has one)
        crossed = new & ((now >= L) | ((prev >= 0) & (prev < L)))
        from_lane = crossed & (prev >= 0) & (prev < L)
        result = (int(crossed.sum()), int(wait[from_lane].sum()))
        wait[new | baseline] = 0
        wait[slow & (now >= 0) & (not baseline)] += 1
        host["drv"], host["wait"] = now, wait
        return result

    def numpy_loop(s):
        control()
        reward["numpy"] = numpy_reward()

    lf_left = torch.empty(L, dtype=torch.int32, device=device)

    def trace(s):
        eng.next_step()
        eng.observe_lane_flow_tensor(left=lf_left, reset=True)
        eng.observe_movement_flow_tensor(entered=entered, entered_lane_waiting_steps=lane_wait, reset=True)

    for _ in range(300):
        eng.next_step()
    eng.sync()
    print("# %s" % name, flush=True)
    if only:
        eng.track_lane_flow(True)
        eng.track_movement_flow(True)
        measure("next_step + observe_lane_flow_tensor(1, reset) + observe_movement_flow_tensor(2, reset)", eng, trace, n)
        return
    res = {"off": [], "on": []}
    for r in range(runs):
        eng.track_movement_flow(False)
        res["off"].append(measure("next_step alone, tracking off (run %d)" % r, eng, lambda s: eng.next_step(), n))
        eng.track_movement_flow(True)
        res["on"].append(measure("next_step alone, tracking on  (run %d)" % r, eng, lambda s: eng.next_step(), n))
    for k, v in res.items():
        print("%-4s median %8.1f us   min %8.1f   max %8.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("tracking on - off (medians) %8.1f us per step" % (float(np.median(res["on"])) - float(np.median(res["off"]))), flush=True)
    measure("observe_movement_flow_tensor(entered, entered_lane_waiting_steps, reset) alone (1 launch + events)", eng,
            lambda s: eng.observe_movement_flow_tensor(entered=entered, entered_lane_waiting_steps=lane_wait, reset=True), n)
    # both rewards from one engine, step by step, before anything is timed
    eng.track_movement_flow(False)
    eng.track_movement_flow(True)  # (a baseline for both)
    numpy_reward(baseline=True)
    total = 0
    for s in range(12):
        control()
        eng.observe_movement_flow_tensor(entered=entered, entered_lane_waiting_steps=lane_wait, reset=True)
        got, want = (int(entered.sum()), int(lane_wait.sum())), numpy_reward()
        assert got == want, "step %d: the tensor reward %s is not the numpy diff's %s" % (s, got, want)
        total += want[0]
    assert total > 0
    print("the two rewards are equal over 12 steps (%d vehicles crossed a stop line)" % total, flush=True)
    n_np = max(n // 10, 10)
    res = {"tensor": [], "numpy": []}
    for r in range(runs):
        res["tensor"].append(measure("observe_intersections -> argmax -> set -> next_step -> observe_movement_flow_tensor (run %d)" % r, eng, tensor_loop, n))
        res["numpy"].append(measure("... -> next_step -> _vehicle_state() + numpy diff (run %d)" % r, eng, numpy_loop, n_np))
    for k, v in res.items():
        print("%-6s median %10.1f us   min %10.1f   max %10.1f" % (k, float(np.median(v)), min(v), max(v)), flush=True)
    print("numpy loop / tensor loop %8.1fx" % (float(np.median(res["numpy"])) / float(np.median(res["tensor"]))), flush=True)


if args.detectors or args.detectors_only:
    e = _cityflow.Engine(cfg, 1)
    p = _cityflow.Engine._with_backend(cfg, 1, os.path.abspath(args.lib)) if args.lib else None
    detectors("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, p, args.iters,
              args.runs, args.detectors_only)
    sys.exit(0)

if args.movement_flow or args.movement_flow_only:
    e = _cityflow.Engine(cfg, 1)
    movement_flow("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters,
                  args.runs, args.movement_flow_only)
    sys.exit(0)

if args.trips or args.trips_only:
    if not args.skip_single:
        e = _cityflow.Engine(cfg, 1)
        trips("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters,
              args.runs, args.trips_only)
        del e
    if not args.skip_vector:
        v = _cityflow.VectorEngine(cfg, args.envs, 1)
        trips("VectorEngine, %d x 30x30 RL workload" % args.envs, v, max(args.iters // 4, 50), args.runs, args.trips_only)
    sys.exit(0)

if args.fronts or args.fronts_only:
    e = _cityflow.Engine(cfg, 1)
    fronts("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters,
           args.runs, args.fronts_only)
    sys.exit(0)

if args.lane_flow or args.lane_flow_only:
    e = _cityflow.Engine(cfg, 1)
    lane_flow("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters,
              args.runs, args.lane_flow_only)
    sys.exit(0)

if args.intersections or args.intersections_only:
    e = _cityflow.Engine(cfg, 1)
    intersections("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters,
                  args.runs, args.intersections_only)
    sys.exit(0)

if args.features or args.features_only:
    e = _cityflow.Engine._with_backend(cfg, 1, os.path.abspath(args.lib)) if args.lib else _cityflow.Engine(cfg, 1)
    features("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters,
             args.features_only)
    sys.exit(0)

e = _cityflow.Engine(cfg, 1)
loops("Engine, 30x30 RL workload (%d signals, %d lanes)" % (len(e.intersection_ids()), len(e.lane_ids())), e, args.iters)
del e
if not args.skip_vector:
    v = _cityflow.VectorEngine(cfg, args.envs, 1)
    loops("VectorEngine, %d x 30x30 RL workload" % args.envs, v, max(args.iters // 4, 50))
