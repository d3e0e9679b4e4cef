"""What set_vehicle_routes_tensor costs beside set_vehicle_route() per vehicle, and what a routing loop on the device costs.

  python tools/vehicle_routes_loop.py [--which bench|vector16|all] [--repeats 5] [--steps 50] [--sample 1000] [--dense]
      bench     the benchmark workload (bench.build_workload: 30x30 after bench.BUILD_UP_STEPS steps)
      vector16  a 16-environment VectorEngine of the same 30x30 network after as many steps
      The candidate set: around every road g[k] of every flow route g, [g[k-1], g[k], g[k+1]] — registered with add_routes
      (VectorEngine: routes=) before the first step.  Every measurement starts from the same state (checkpoint / rollback;
      --dense: snapshot / load), median / min / max over `repeats` after one warm-up:
        (a) one call that gives every running vehicle a random handle from the candidate set: the call's host time, and
            the time until `ignored` is read;
        (b) per step of `steps` steps: observe_vehicles_tensor -> a torch rule picking among the candidates (a hash of the
            vehicle's number, its drivable and the step) -> set_vehicle_routes_tensor -> next_step;
        (c) per step of `steps` free-running steps;
        (d) Engine only: set_vehicle_route(id, [the last road of its route]) per vehicle over `sample` running vehicles.

  python tools/vehicle_routes_loop.py --trace [--which bench|vector16] [--iters 50] [--dense]
      the workload for a `rocprofv3 --kernel-trace --stats` run of its own: `iters` calls as in (a) (k_routes_claim and
      kr_routes_apply; with --dense k_routes_claim, k_routes_superseded and k_routes_apply_dense), then as many
      get_vehicle_routes_tensor calls (k_get_routes)."""
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


def spread(name, ts, unit=1e3, unit_name="ms"):
    print("  %-58s median %9.3f %s   min %9.3f   max %9.3f   (n = %d)" % (
        name, statistics.median(ts) * unit, unit_name, min(ts) * unit, max(ts) * unit, len(ts)), flush=True)


def candidates(cfg):
    """The three-road windows of every flow route, read from a throw-away engine's route tables."""
    probe = cityflow_amd.Engine(cfg, 1)
    lists = []
    for h in range(probe.route_count()):
        g = probe.route_roads(h)
        lists += [g[k - 1:k + 2] for k in range(1, len(g) - 1)]
    return lists


def workload(which, work, dense):
    cfg = bench.build_workload(work, 0, scenario="grid_30x30")
    if dense:
        with open(cfg) as f:
            doc = json.load(f)
        doc.setdefault("cfx", {})["layout"] = "dense"
        with open(cfg, "w") as f:
            json.dump(doc, f)
    lists = candidates(cfg)
    if which == "bench":
        eng = cityflow_amd.Engine(cfg, 1)
        handles = eng.add_routes(lists)
    else:
        eng = cityflow_amd.VectorEngine(cfg, 16, 1, routes=lists)
        handles = eng.added_routes()
    for _ in range(bench.BUILD_UP_STEPS):
        eng.next_step()
    eng.sync()
    return eng, handles


def buffers(eng, handles):
    import torch
    device = torch.device("cuda", eng._stream_handle()[1])
    n_rows = int(eng.get_vehicle_count() * 1.25) + 1024
    t = {name: torch.empty(n_rows, dtype=torch.int32, device=device) for name in ("vehicle", "drivable")}
    t["count"] = torch.empty((), dtype=torch.int32, device=device)
    cand = torch.tensor(sorted(set(handles)), dtype=torch.int32, device=device)
    return t, cand, device


def rule(torch, t, cand, step):
    pick = (t["vehicle"].to(torch.int64) * 7 + t["drivable"] + step) % cand.numel()
    return torch.where(t["vehicle"] >= 0, cand[pick], torch.full_like(t["vehicle"], -1))


def restorer(eng):
    try:
        ck = eng.checkpoint()
        return lambda: eng.rollback(ck)
    except NotImplementedError:  # (the dense layout has no checkpoints in device memory)
        ck = eng.snapshot()
        return lambda: eng.load(ck)


def measure(args):
    import torch
    work = tempfile.mkdtemp(prefix="vehicle_routes_loop_")
    for which in (("bench", "vector16") if args.which == "all" else (args.which,)):
        eng, handles = workload(which, work, args.dense)
        t, cand, device = buffers(eng, handles)
        n_rows = t["vehicle"].numel()
        status = torch.empty(n_rows, dtype=torch.int32, device=device)
        ignored = torch.empty(1, dtype=torch.int32, device=device)
        restore = restorer(eng)
        eng.observe_vehicles_tensor(**t)
        print("%s%s: %s, %d vehicles running, rows of %d, %d candidate routes of %d" % (
            which, " (dense layout)" if args.dense else "", type(eng).__name__, int(t["count"]), n_rows, cand.numel(),
            eng.route_count()), flush=True)
        if args.trace:
            random = cand[torch.randint(0, cand.numel(), (n_rows,), device=device)]
            for _ in range(args.iters):
                eng.set_vehicle_routes_tensor(t["vehicle"], random, status, ignored)
            for _ in range(args.iters):
                eng.get_vehicle_routes_tensor(t["vehicle"], status)
            torch.cuda.synchronize(device)
            return
        call, read, loop, free = [], [], [], []
        for warm in (True, False):
            for _ in range(1 if warm else args.repeats):
                restore()
                eng.observe_vehicles_tensor(**t)
                random = cand[torch.randint(0, cand.numel(), (n_rows,), device=device)]
                torch.cuda.synchronize(device)
                eng.sync()
                t0 = time.perf_counter()
                eng.set_vehicle_routes_tensor(t["vehicle"], random, status, ignored)
                t1 = time.perf_counter()
                refused = int(ignored.item())
                t2 = time.perf_counter()
                applied = int((status[:int(t["count"])] == 1).sum())
                restore()
                eng.sync()
                t3 = time.perf_counter()
                for s in range(args.steps):
                    eng.observe_vehicles_tensor(**t)
                    eng.set_vehicle_routes_tensor(t["vehicle"], rule(torch, t, cand, s))
                    eng.next_step()
                torch.cuda.synchronize(device)
                eng.sync()
                t4 = time.perf_counter()
                restore()
                eng.sync()
                t5 = time.perf_counter()
                for _ in range(args.steps):
                    eng.next_step()
                eng.sync()
                t6 = time.perf_counter()
                if not warm:
                    call.append(t1 - t0), read.append(t2 - t0)
                    loop.append((t4 - t3) / args.steps), free.append((t6 - t5) / args.steps)
        print("  a random candidate to every running vehicle: %d applied, %d refused" % (applied, refused))
        spread("set_vehicle_routes_tensor, every running vehicle: the call", call, 1e6, "us")
        spread("  ... until `ignored` is read", read, 1e6, "us")
        spread("observe -> rule -> set -> step, per step", loop, 1e6, "us")
        spread("free-running step", free, 1e6, "us")
        if hasattr(eng, "set_vehicle_route"):
            import numpy as np
            each = []
            for _ in range(args.repeats):
                restore()
                rows = eng.observe_vehicles_array()
                numbers = np.ascontiguousarray(rows["vehicle"][:args.sample])
                ids = eng._vehicle_ids(numbers)
                last = [[eng.route_roads(int(h))[-1]] for h in eng.get_vehicle_routes(numbers)]
                eng.sync()
                t0 = time.perf_counter()
                done = sum(eng.set_vehicle_route(v, anchors) for v, anchors in zip(ids, last))
                t1 = time.perf_counter()
                each.append((t1 - t0) / max(len(ids), 1))
            spread("set_vehicle_route(), per vehicle (%d sampled, %d took it)" % (len(ids), done), each, 1e6, "us")
        del restore, eng


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("bench", "vector16", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sample", type=int, default=1000)
    a = ap.parse_args()
    if a.trace and a.which == "all":
        a.which = "bench"
    measure(a)
