"""What the trip log costs and what it buys: the measurements of DESIGN.md 6b "Trip log" (profiles/trip_log.txt).

  python tools/trip_log_loop.py --tick off|on [--lib LIBRARY] [--steps 200]
      the workload for a `rocprofv3 --kernel-trace` run of its own: the benchmark workload (bench.build_workload: 30x30 after
      bench.BUILD_UP_STEPS steps) with track_trips on, then `steps` steps.  `off`: no log (with --lib: another build of the
      device library, such as the parent commit's, which has no log).  `on`: log=65536, drained every 10 steps with
      reset=True into tensors (k_trip_log_drain).

  python tools/trip_log_loop.py --summary RESULTS.db [--last 200]
      k_trip_tick and k_trip_log_drain of such a trace: launches, median / min / max microseconds of the last `last` launches.

  python tools/trip_log_loop.py [--repeats 7] [--steps 100]
      The decision loop.  Every measurement starts from the same state (checkpoint / rollback), median / min / max over
      `repeats`, per step of `steps` steps:
        (a) next_step, and every 10 steps observe_trip_log_tensor(reset=True) plus the mean travel time per origin-destination
            pair in torch on the device (two index_add_ over the rows), the pairs that had a trip read back once at the end;
        (b) the same numbers from Python: get_vehicles(True) after every step, set differences, a dict per pair;
        (c) free-running steps with trip tracking on and no log.
      The Python loop starts in the middle of a run, so it takes 0 for the enter step of the vehicles alive at its start: its
      sums are not the log's, its work is that of a loop that ran from the first step, and both must count the same trips.
      Also: the host time of one drain call and the time until the device has finished it."""
import argparse
import os
import sqlite3
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAPACITY = 65536
EVERY = 10


def spread(name, ts, unit=1e6, unit_name="us"):
    print("  %-62s median %9.2f %s   min %9.2f   max %9.2f   (n = %d)" % (
        name, statistics.median(ts) * unit, unit_name, min(ts) * unit, max(ts) * unit, len(ts)), flush=True)


def workload(lib=None):
    import bench
    import cityflow_amd
    cfg = bench.build_workload(tempfile.mkdtemp(prefix="trip_log_loop_"), 0, scenario="grid_30x30")
    eng = cityflow_amd.Engine._with_backend(cfg, 1, os.path.abspath(lib)) if lib else cityflow_amd.Engine(cfg, 1)
    eng.track_trips(True)
    for _ in range(bench.BUILD_UP_STEPS):
        eng.next_step()
    eng.sync()
    return eng, cfg


def columns(torch, eng, names=("count", "origin_road", "destination_road", "travel_steps")):
    device = torch.device("cuda", eng._stream_handle()[1])
    return {k: torch.empty(() if k in ("count", "dropped") else (eng.trip_log_capacity(),), dtype=torch.int32, device=device)
            for k in names}, device


def tick(args):
    import torch
    eng, _cfg = workload(args.lib)
    if args.tick == "on":
        eng.track_trips(True, log=CAPACITY)
        t, device = columns(torch, eng)
    rows = []
    for s in range(1, args.steps + 1):
        eng.next_step()
        if args.tick == "on" and s % EVERY == 0:
            eng.observe_trip_log_tensor(reset=True, **t)
            rows.append(int(t["count"]))
    eng.sync()
    print("tick leg %s%s: %d steps, %d vehicles running, %d finished since tracking is on; rows per drain %s" % (
        args.tick, " (" + os.path.basename(args.lib) + ")" if args.lib else "", args.steps, eng.get_vehicle_count(),
        int(eng.observe_trips_array()["finished"]), rows), flush=True)


def summary(args):
    cur = sqlite3.connect(args.summary).cursor()
    for kernel in ("k_trip_tick", "k_trip_log_drain"):
        d = [r[0] / 1e3 for r in cur.execute("select duration from kernels where name like ? order by start desc limit ?",
                                             ("%" + kernel + "%", args.last))]
        if d:
            print("%-18s launches %4d   median %7.2f us   min %7.2f   max %7.2f" % (kernel, len(d), statistics.median(d), min(d), max(d)))


def loop(args):
    import torch
    eng, _cfg = workload()
    eng.track_trips(True, log=CAPACITY)
    n_roads = len(eng.road_ids())
    t, device = columns(torch, eng)
    ck = eng.checkpoint()
    print("decision loop: %d vehicles running, %d roads, log of %d rows, drained every %d steps" % (
        eng.get_vehicle_count(), n_roads, CAPACITY, EVERY), flush=True)

    def on_device():
        total = torch.zeros(n_roads * n_roads, dtype=torch.float64, device=device)
        trips = torch.zeros(n_roads * n_roads, dtype=torch.float64, device=device)
        for s in range(1, args.steps + 1):
            eng.next_step()
            if s % EVERY == 0:
                eng.observe_trip_log_tensor(reset=True, **t)
                held = (torch.arange(CAPACITY, device=device) < t["count"]).to(torch.float64)
                pair = (t["origin_road"].clamp(min=0).long() * n_roads + t["destination_road"].clamp(min=0).long())
                total.index_add_(0, pair, t["travel_steps"].to(torch.float64) * held)
                trips.index_add_(0, pair, held)
        seen = trips > 0  # the means of the pairs that had a trip, read back once: the loop's one wait
        return (total[seen] / trips[seen]).cpu(), trips[seen].cpu()

    def in_python():
        alive, total, trips = set(eng.get_vehicles(True)), {}, {}
        enter = dict.fromkeys(alive, 0)  # (a loop that ran from the first step would know them)
        for s in range(1, args.steps + 1):
            eng.next_step()
            now = set(eng.get_vehicles(True))
            for v in now - alive:
                enter[v] = s - 1
            for v in alive - now:
                f = int(v.split("_")[1])  # (the flow, which stands for the origin-destination pair)
                total[f] = total.get(f, 0) + (s - 1) - enter.pop(v)
                trips[f] = trips.get(f, 0) + 1
            alive = now
        return total, trips

    dev, py, free, call, done = [], [], [], [], []
    for warm in (True, False):
        for _ in range(1 if warm else args.repeats):
            eng.rollback(ck)
            eng.sync()
            t0 = time.perf_counter()
            means, trips = on_device()
            t1 = time.perf_counter()
            eng.rollback(ck)
            eng.sync()
            t2 = time.perf_counter()
            ptotal, ptrips = in_python()
            t3 = time.perf_counter()
            eng.rollback(ck)
            eng.track_trips(True, log=0)
            eng.sync()
            t4 = time.perf_counter()
            for _ in range(args.steps):
                eng.next_step()
            eng.sync()
            t5 = time.perf_counter()
            eng.track_trips(True, log=CAPACITY)
            # one drain alone, at the rows EVERY steps leave
            eng.rollback(ck)
            for _ in range(EVERY):
                eng.next_step()
            eng.sync()
            torch.cuda.synchronize(device)
            t6 = time.perf_counter()
            eng.observe_trip_log_tensor(reset=True, **t)
            t7 = time.perf_counter()
            torch.cuda.synchronize(device)
            t8 = time.perf_counter()
            if not warm:
                dev.append((t1 - t0) / args.steps), py.append((t3 - t2) / args.steps), free.append((t5 - t4) / args.steps)
                call.append(t7 - t6), done.append(t8 - t6)
    print("  %d trips between %d origin-destination pairs finished in the %d steps (mean of the pairs' means %.1f steps), %d in the "
          "last drain alone" % (int(trips.sum()), trips.numel(), args.steps, float(means.mean()), int(t["count"])), flush=True)
    assert int(trips.sum()) == sum(ptrips.values()) > 0, (int(trips.sum()), sum(ptrips.values()))
    spread("step + drain every %d steps + per-pair means in torch, per step" % EVERY, dev)
    spread("step + get_vehicles(True) set differences in Python, per step", py)
    spread("free-running step, trip tracking on, no log", free)
    spread("observe_trip_log_tensor(reset=True), 4 outputs: the call", call)
    spread("  ... until the device has finished", done)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tick", choices=("off", "on"))
    ap.add_argument("--lib", default="")
    ap.add_argument("--summary", default="")
    ap.add_argument("--last", type=int, default=200)
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if a.summary:
        summary(a)
    elif a.tick:
        a.steps = a.steps or 200
        tick(a)
    else:
        a.steps = a.steps or 100
        loop(a)
