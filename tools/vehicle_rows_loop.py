"""What observe_vehicles_tensor costs beside the host's means to the same data.

  python tools/vehicle_rows_loop.py [--which bench|vector16|all] [--repeats 9]
      bench     the benchmark workload (bench.build_workload: 30x30 after bench.BUILD_UP_STEPS steps)
      vector16  a 16-environment VectorEngine of the same 30x30 network after as many steps
      Per workload, after a warm-up of each, `repeats` times in turn, median / min / max:
        (a) observe_vehicles_tensor with all outputs: the call's host time (it returns without waiting), and the time to
            the device's completion (call + torch.cuda.synchronize);
        (b) _vehicle_state(), which is cfx_get_vehicles (offsets, gather, wait, copies), and — Engine only —
            get_lane_vehicles() + get_vehicle_speed() + get_vehicle_distance().

  python tools/vehicle_rows_loop.py --trace [--which bench|vector16] [--iters 50]
      the workload for a `rocprofv3 --kernel-trace --stats` run of its own: `iters` observe_vehicles_tensor calls with all
      outputs (k_vehicle_tile_sums, kr_vehicle_rows), then as many _vehicle_state() calls where the engine has one (kr_offsets,
      kr_gather)."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
import cityflow_amd  # noqa: E402


def spread(name, ts, unit=1e3, unit_name="ms"):
    print("  %-58s median %9.3f %s   min %9.3f   max %9.3f   (n = %d)" % (
        name, statistics.median(ts) * unit, unit_name, min(ts) * unit, max(ts) * unit, len(ts)), flush=True)


def workload(which, work):
    cfg = bench.build_workload(work, 0, scenario="grid_30x30")
    eng = cityflow_amd.Engine(cfg, 1) if which == "bench" else cityflow_amd.VectorEngine(cfg, 16, 1)
    for _ in range(bench.BUILD_UP_STEPS):
        eng.next_step()
    eng.sync()
    return eng


def outputs(eng):
    import torch
    device = torch.device("cuda", eng._stream_handle()[1])
    lanes, links = eng._drivable_counts()
    lead = tuple(eng._tensor_shapes()[0])[:-1]
    n_rows = int(eng.get_vehicle_count() * 1.25) + 1024
    t = {"start": torch.empty(lead + (lanes + links + 1,), dtype=torch.int32, device=device),
         "count": torch.empty((), dtype=torch.int32, device=device)}
    for name in ("vehicle", "drivable", "env", "leader"):
        t[name] = torch.empty(n_rows, dtype=torch.int32, device=device)
    for name in ("distance", "speed", "gap"):
        t[name] = torch.empty(n_rows, dtype=torch.float64, device=device)
    return t, device


def measure(args):
    import torch
    work = tempfile.mkdtemp(prefix="vehicle_rows_loop_")
    for which in (("bench", "vector16") if args.which == "all" else (args.which,)):
        eng = workload(which, work)
        t, device = outputs(eng)
        single = hasattr(eng, "_vehicle_state")
        print("%s: %s, %d vehicles running, %d drivables, rows of %d" % (
            which, type(eng).__name__, eng.get_vehicle_count(), t["start"].numel(), t["vehicle"].numel()), flush=True)
        call, done, state, dicts = [], [], [], []
        for warm in (True, False):
            for _ in range(2 if warm else args.repeats):
                torch.cuda.synchronize(device)
                eng.sync()
                t0 = time.perf_counter()
                eng.observe_vehicles_tensor(**t)
                t1 = time.perf_counter()
                torch.cuda.synchronize(device)
                t2 = time.perf_counter()
                if single:
                    eng._vehicle_state()
                t3 = time.perf_counter()
                if single:
                    eng.get_lane_vehicles(), eng.get_vehicle_speed(), eng.get_vehicle_distance()
                t4 = time.perf_counter()
                if not warm:
                    call.append(t1 - t0), done.append(t2 - t0), state.append(t3 - t2), dicts.append(t4 - t3)
        assert int(t["count"]) == eng.get_vehicle_count()
        spread("observe_vehicles_tensor, all outputs: the call", call, 1e6, "us")
        spread("  ... until the device has finished", done, 1e6, "us")
        if single:
            spread("_vehicle_state()", state)
            spread("get_lane_vehicles() + get_vehicle_speed() + _distance()", dicts)
        del eng


def trace(args):
    import torch
    work = tempfile.mkdtemp(prefix="vehicle_rows_trace_")
    which = "bench" if args.which == "all" else args.which
    eng = workload(which, work)
    t, device = outputs(eng)
    eng.observe_vehicles_tensor(**t)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(args.iters):
        eng.observe_vehicles_tensor(**t)
    torch.cuda.synchronize(device)
    print("%s: %d observe_vehicles_tensor calls at %d running vehicles: %.1f us each on the host's clock" % (
        which, args.iters, int(t["count"]), (time.perf_counter() - t0) / args.iters * 1e6), flush=True)
    if hasattr(eng, "_vehicle_state"):
        for _ in range(args.iters):
            eng._vehicle_state()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("bench", "vector16", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    trace(a) if a.trace else measure(a)
