"""What set_lane_speed_limits_tensor costs, what a variable-speed-limit loop on the device costs, and what the only route a
user had before costs: a rewritten roadnet file, a new engine and load(snapshot()).

  python tools/speed_limit_loop.py [--which bench|vector16|all] [--repeats 5] [--steps 50] [--rebuilds 3]
      bench     the benchmark workload (bench.build_workload: 30x30 after bench.BUILD_UP_STEPS steps)
      vector16  a 16-environment VectorEngine of the same 30x30 network after as many steps
      Every measurement starts from the same state (checkpoint / rollback), median / min / max over `repeats` after one
      warm-up:
        (a) one call that sets every lane's limit: the time until the call returns, the device time between two events
            recorded on the torch stream around the call (the kernel, its 4-byte fill and the two stream hand-overs), and
            the time until `rejected` is read;
        (b) per step of `steps` steps: observe_lanes_tensor(counts) -> a torch rule (a lane holding more than 8 vehicles
            gets 8 m/s, every other lane its file limit back) -> set_lane_speed_limits_tensor -> next_step;
        (c) per step of `steps` free-running steps;
        (d) Engine only, `rebuilds` times: the limits of (b)'s rule written into a roadnet file, an engine built from it,
            snapshot() of the running engine and load() into the new one.

  python tools/speed_limit_loop.py --trace [--which bench|vector16] [--iters 50]
      the workload for a `rocprofv3 --kernel-trace --stats` run of its own: `iters` calls as in (a) (k_set_lane_limits), as
      many get_lane_speed_limits_tensor calls (k_get_lane_limits) and restore_lane_speed_limits calls (k_restore_lane_limits)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import cityflow_amd  # noqa: E402

CROWDED, SLOW = 8, 8.0


def spread(name, ts, unit=1e3, unit_name="ms"):
    print("  %-66s median %9.3f %s   min %9.3f   max %9.3f   (n = %d)" % (
        name, statistics.median(ts) * unit, unit_name, min(ts) * unit, max(ts) * unit, len(ts)), flush=True)


def rule(torch, counts, file_limits):
    return torch.where(counts > CROWDED, torch.full_like(file_limits, SLOW), file_limits)


def rebuilt(cfg, eng, limits, tag):
    """The route without the call: the limits into a roadnet file of their own, an engine from it, the state carried over."""
    with open(cfg) as f:
        doc = json.load(f)
    with open(os.path.join(doc["dir"], doc["roadnetFile"])) as f:
        net = json.load(f)
    at = {i: n for n, i in enumerate(eng.lane_ids())}
    for road in net["roads"]:
        for k, lane in enumerate(road["lanes"]):
            lane["maxSpeed"] = float(limits[at["%s_%d" % (road["id"], k)]])
    doc["roadnetFile"] = "roadnet_%s.json" % tag
    with open(os.path.join(doc["dir"], doc["roadnetFile"]), "w") as f:
        json.dump(net, f)
    path = cfg[:-5] + "_" + tag + ".json"
    with open(path, "w") as f:
        json.dump(doc, f)
    new = cityflow_amd.Engine(path, 1)
    new.load(eng.snapshot())
    new.sync()
    return new


def measure(args):
    import torch
    work = tempfile.mkdtemp(prefix="speed_limit_loop_")
    for which in (("bench", "vector16") if args.which == "all" else (args.which,)):
        cfg = bench.build_workload(work, 0, scenario="grid_30x30")
        eng = cityflow_amd.Engine(cfg, 1) if which == "bench" else cityflow_amd.VectorEngine(cfg, 16, 1)
        for _ in range(bench.BUILD_UP_STEPS):
            eng.next_step()
        eng.sync()
        device = torch.device("cuda", eng._stream_handle()[1])
        file_limits = eng.get_lane_speed_limits_tensor()
        counts = torch.empty(tuple(file_limits.shape), dtype=torch.int32, device=device)
        rejected = torch.empty(1, dtype=torch.int32, device=device)
        eng.observe_lanes_tensor(counts=counts)
        print("%s: %s, %d vehicles running, %d lane limits, %d lanes above %d vehicles" % (
            which, type(eng).__name__, eng.get_vehicle_count(), file_limits.numel(), int((counts > CROWDED).sum()), CROWDED), flush=True)
        every = rule(torch, counts, file_limits)
        if args.trace:
            for _ in range(args.iters):
                eng.set_lane_speed_limits_tensor(every, rejected)
            for _ in range(args.iters):
                eng.get_lane_speed_limits_tensor(out=file_limits)
            for _ in range(args.iters):
                eng.restore_lane_speed_limits()
            torch.cuda.synchronize(device)
            eng.sync()
            return
        ck = eng.checkpoint()
        call, between, read, loop, free = [], [], [], [], []
        before, after = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for warm in (True, False):
            for _ in range(1 if warm else args.repeats):
                eng.rollback(ck)
                eng.restore_lane_speed_limits()
                torch.cuda.synchronize(device)
                eng.sync()
                before.record()
                t0 = time.perf_counter()
                eng.set_lane_speed_limits_tensor(every, rejected)
                t1 = time.perf_counter()
                after.record()
                refused = int(rejected.item())
                t2 = time.perf_counter()
                after.synchronize()
                on_device = before.elapsed_time(after) * 1e-3
                eng.rollback(ck)
                eng.restore_lane_speed_limits()
                eng.sync()
                t3 = time.perf_counter()
                for s in range(args.steps):
                    eng.observe_lanes_tensor(counts=counts)
                    eng.set_lane_speed_limits_tensor(rule(torch, counts, file_limits))
                    eng.next_step()
                torch.cuda.synchronize(device)
                eng.sync()
                t4 = time.perf_counter()
                eng.rollback(ck)
                eng.restore_lane_speed_limits()
                eng.sync()
                t5 = time.perf_counter()
                for _ in range(args.steps):
                    eng.next_step()
                eng.sync()
                t6 = time.perf_counter()
                if not warm:
                    call.append(t1 - t0), between.append(on_device), read.append(t2 - t0)
                    loop.append((t4 - t3) / args.steps), free.append((t6 - t5) / args.steps)
        assert refused == 0
        spread("set_lane_speed_limits_tensor, every lane: until the call returns", call, 1e6, "us")
        spread("  ... device time between events around the call", between, 1e6, "us")
        spread("  ... until `rejected` is read", read, 1e6, "us")
        spread("observe -> rule -> set -> step, per step", loop, 1e6, "us")
        spread("free-running step", free, 1e6, "us")
        if which == "bench":
            eng.rollback(ck)
            eng.restore_lane_speed_limits()
            limits = every.cpu().numpy()
            whole = []
            for r in range(args.rebuilds):
                t0 = time.perf_counter()
                new = rebuilt(cfg, eng, limits, "limits%d" % r)
                whole.append(time.perf_counter() - t0)
                del new
            spread("rewritten roadnet file -> new engine -> load(snapshot())", whole, 1e3, "ms")
        del ck, eng


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("bench", "vector16", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rebuilds", type=int, default=3)
    a = ap.parse_args()
    if a.trace and a.which == "all":
        a.which = "bench"
    measure(a)
