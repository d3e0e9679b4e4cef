"""What observe_vehicles_tensor costs beside the host's means to the same data.

  python tools/vehicle_rows_loop.py [--which bench|vector16|all] [--repeats 9]
      bench     the benchmark workload (bench.build_workload: 30x30 after bench.BUILD_UP_STEPS steps)
      vector16  a 16-environment VectorEngine of the same 30x30 network after as many steps
      Per workload, after a warm-up of each, `repeats` times in turn, median / min / max:
        (a) observe_vehicles_tensor with all outputs: the call's host time (it returns without waiting), and the time to
            the device's completion (call + torch.cuda.synchronize);
        (b) _vehicle_state(), which is cfx_get_vehicles (offsets, gather, wait, copies), and — Engine only —
            get_lane_vehicles() + get_vehicle_speed() + get_vehicle_distance().
      --poses   beside (a), in the same turn: the call with the six pose outputs as well (x, y, dir_x, dir_y, length, width:
                thirteen row outputs), and the call of (a) once more behind it — the first one follows the host's getters of
                (b), these two follow a call like themselves.  Then — Engine only — the host's route to the same positions,
                on an engine of its own with saveReplay: what a step costs more with set_save_replay(True) than with set_save_replay(False), turn by
                turn, and reading the step's line of the replay file and parsing its vehicle records.

  python tools/vehicle_rows_loop.py --trace [--which bench|vector16] [--iters 50]
      the workload for a `rocprofv3 --kernel-trace --stats` run of its own: `iters` observe_vehicles_tensor calls with all
      outputs (k_vehicle_tile_sums, kr_vehicle_rows; with --poses the six pose outputs too: kr_vehicle_poses), then as many
      _vehicle_state() calls where the engine has one (kr_offsets, kr_gather).

  python tools/vehicle_rows_loop.py --control [--which bench|vector16|all] [--repeats 5] [--steps 50] [--sample 300]
      What set_vehicle_speeds_tensor buys a vehicle-level control loop.  The rule, in torch on the device: command half its
      speed to every vehicle that follows its leader with a gap below 10 m, NaN (leave alone) to the others.  Every
      measurement starts from the same state (checkpoint / rollback; --dense: snapshot / load), median / min / max over `repeats`:
        (a) one call that commands every running vehicle: the call's host time, and the time until `ignored` is read;
        (b) per step of `steps` steps: observe_vehicles_tensor -> the rule -> set_vehicle_speeds_tensor -> next_step;
        (c) per step of `steps` free-running steps;
        (d) Engine only, the per-vehicle loop: the get_vehicle_speed() dict (the host has no dict of the gaps), and
            set_vehicle_speed() per vehicle over `sample` vehicles (the whole loop is the dict plus that, times the vehicles
            commanded).

  python tools/vehicle_rows_loop.py --control --trace [--which bench|vector16] [--iters 50]
      the workload for a kernel trace of its own: `iters` calls that command every running vehicle (k_speeds_claim,
      k_speeds_apply, and k_speeds_flag_dense with "cfx": {"layout": "dense"} through --dense)."""
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


def workload(which, work, dense=False, replay=None):
    """replay: a list that takes the path of the replay file the engine then writes ("saveReplay": true)"""
    cfg = bench.build_workload(work, 0, scenario="grid_30x30")
    if dense or replay is not None:
        import json
        with open(cfg) as f:
            doc = json.load(f)
        if dense:
            doc.setdefault("cfx", {})["layout"] = "dense"
        if replay is not None:
            doc.update(saveReplay=True, roadnetLogFile="roadnet_log.json", replayLogFile="replay.txt")
            replay.append(doc["dir"] + "replay.txt")
        with open(cfg, "w") as f:
            json.dump(doc, f)
    eng = cityflow_amd.Engine(cfg, 1) if which == "bench" else cityflow_amd.VectorEngine(cfg, 16, 1)
    for _ in range(bench.BUILD_UP_STEPS):
        eng.next_step()
    eng.sync()
    return eng


def outputs(eng, poses=False):
    import torch
    device = torch.device("cuda", eng._stream_handle()[1])
    lanes, links = eng._drivable_counts()
    lead = tuple(eng._tensor_shapes()[0])[:-1]
    n_rows = int(eng.get_vehicle_count() * 1.25) + 1024
    t = {"start": torch.empty(lead + (lanes + links + 1,), dtype=torch.int32, device=device),
         "count": torch.empty((), dtype=torch.int32, device=device)}
    for name in ("vehicle", "drivable", "env", "leader"):
        t[name] = torch.empty(n_rows, dtype=torch.int32, device=device)
    for name in ("distance", "speed", "gap") + (cityflow_amd.torch_io.VEHICLE_POSE_OUTPUTS if poses else ()):
        t[name] = torch.empty(n_rows, dtype=torch.float64, device=device)
    return t, device


def replay_route(args, work):
    """The host's route to the positions: a step with the replay writer on against one with it off, and the line's parsing."""
    log = []
    eng = workload("bench", work, replay=log)
    on, off, parse = [], [], []
    for warm in (True, False):
        for _ in range(2 if warm else args.repeats):
            eng.set_save_replay(False)
            eng.sync()
            t0 = time.perf_counter()
            eng.next_step()
            eng.sync()
            t1 = time.perf_counter()
            eng.set_save_replay(True)
            written = os.path.getsize(log[0]) if os.path.exists(log[0]) else 0
            eng.next_step()
            eng.sync()
            t2 = time.perf_counter()
            with open(log[0]) as f:
                f.seek(written)  # (the step's line alone)
                line = f.read().splitlines()[-1]
            records = [v.split(" ") for v in line.split(";")[0].split(",") if v]
            xy = [(float(r[0]), float(r[1]), float(r[2]), r[3], float(r[5]), float(r[6])) for r in records]
            t3 = time.perf_counter()
            assert len(xy) == eng.get_vehicle_count()
            if not warm:
                off.append(t1 - t0), on.append(t2 - t1), parse.append(t3 - t2)
    print("the replay route, %d vehicles running:" % eng.get_vehicle_count(), flush=True)
    spread("next_step() + sync, set_save_replay(False)", off)
    spread("next_step() + sync, set_save_replay(True)", on)
    spread("reading the file and parsing the step's line", parse)


def measure(args):
    import torch
    work = tempfile.mkdtemp(prefix="vehicle_rows_loop_")
    for which in (("bench", "vector16") if args.which == "all" else (args.which,)):
        eng = workload(which, work)
        t, device = outputs(eng)
        t13 = dict(t, **{k: v for k, v in outputs(eng, True)[0].items() if k not in t}) if args.poses else None
        single = hasattr(eng, "_vehicle_state")
        print("%s: %s, %d vehicles running, %d drivables, rows of %d" % (
            which, type(eng).__name__, eng.get_vehicle_count(), t["start"].numel(), t["vehicle"].numel()), flush=True)
        call, done, state, dicts, call13, done13, call7, done7 = [], [], [], [], [], [], [], []
        for warm in (True, False):
            for _ in range(2 if warm else args.repeats):
                torch.cuda.synchronize(device)
                eng.sync()
                t0 = time.perf_counter()
                eng.observe_vehicles_tensor(**t)
                t1 = time.perf_counter()
                torch.cuda.synchronize(device)
                t2 = time.perf_counter()
                if t13:
                    eng.sync()  # (as in front of the call above)
                    p0 = time.perf_counter()
                    eng.observe_vehicles_tensor(**t13)
                    p1 = time.perf_counter()
                    torch.cuda.synchronize(device)
                    p2 = time.perf_counter()
                    eng.sync()
                    p3 = time.perf_counter()
                    eng.observe_vehicles_tensor(**t)  # (once more: the first call above follows the host's getters of (b),
                    p4 = time.perf_counter()          # this one follows a call like itself, as the pose call does)
                    torch.cuda.synchronize(device)
                    p5 = time.perf_counter()
                    if not warm:
                        call13.append(p1 - p0), done13.append(p2 - p0), call7.append(p4 - p3), done7.append(p5 - p3)
                ts = time.perf_counter()
                if single:
                    eng._vehicle_state()
                t3 = time.perf_counter()
                if single:
                    eng.get_lane_vehicles(), eng.get_vehicle_speed(), eng.get_vehicle_distance()
                t4 = time.perf_counter()
                if not warm:
                    call.append(t1 - t0), done.append(t2 - t0), state.append(t3 - ts), dicts.append(t4 - t3)
        assert int(t["count"]) == eng.get_vehicle_count()
        spread("observe_vehicles_tensor, all outputs: the call", call, 1e6, "us")
        spread("  ... until the device has finished", done, 1e6, "us")
        if t13:
            spread("observe_vehicles_tensor, the six pose outputs too: the call", call13, 1e6, "us")
            spread("  ... until the device has finished", done13, 1e6, "us")
            spread("observe_vehicles_tensor, all outputs once more, behind that call: the call", call7, 1e6, "us")
            spread("  ... until the device has finished", done7, 1e6, "us")
        if single:
            spread("_vehicle_state()", state)
            spread("get_lane_vehicles() + get_vehicle_speed() + _distance()", dicts)
        del eng
        if t13 and single:
            replay_route(args, tempfile.mkdtemp(prefix="vehicle_rows_replay_"))


def trace(args):
    import torch
    work = tempfile.mkdtemp(prefix="vehicle_rows_trace_")
    which = "bench" if args.which == "all" else args.which
    eng = workload(which, work)
    t, device = outputs(eng, args.poses)
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


def rule(torch, t):
    follows = (t["leader"] >= 0) & (t["gap"] >= 0) & (t["gap"] < 10.0)
    return torch.where(follows, 0.5 * t["speed"], torch.full_like(t["speed"], float("nan")))


def control(args):
    import torch
    work = tempfile.mkdtemp(prefix="vehicle_speeds_loop_")
    for which in (("bench", "vector16") if args.which == "all" else (args.which,)):
        eng = workload(which, work, args.dense)
        t, device = outputs(eng)
        ignored = torch.empty((), dtype=torch.int32, device=device)
        try:
            ck = eng.checkpoint()
            restore = lambda: eng.rollback(ck)  # noqa: E731
        except NotImplementedError:  # (the dense layout has no checkpoints in device memory)
            ck = eng.snapshot()
            restore = lambda: eng.load(ck)  # noqa: E731
        eng.observe_vehicles_tensor(**t)
        commanded = int(torch.isfinite(rule(torch, t))[:int(t["count"])].sum())
        print("%s%s: %s, %d vehicles running, the rule commands %d of them" % (
            which, " (dense layout)" if args.dense else "", type(eng).__name__, int(t["count"]), commanded), flush=True)
        if args.trace:
            every = t["speed"].clone()
            for _ in range(args.iters):
                eng.set_vehicle_speeds_tensor(t["vehicle"], every, ignored)
            torch.cuda.synchronize(device)
            assert int(ignored) == 0
            return
        call, read, loop, free = [], [], [], []
        for warm in (True, False):
            for _ in range(1 if warm else args.repeats):
                restore()
                eng.observe_vehicles_tensor(**t)
                every = t["speed"].clone()  # (its own speed to every running vehicle; the padding rows name -1)
                torch.cuda.synchronize(device)
                eng.sync()
                t0 = time.perf_counter()
                eng.set_vehicle_speeds_tensor(t["vehicle"], every, ignored)
                t1 = time.perf_counter()
                assert int(ignored.item()) == 0
                t2 = time.perf_counter()
                restore()
                eng.sync()
                t3 = time.perf_counter()
                for _ in range(args.steps):
                    eng.observe_vehicles_tensor(**t)
                    eng.set_vehicle_speeds_tensor(t["vehicle"], rule(torch, t))
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
        spread("set_vehicle_speeds_tensor, every running vehicle: the call", call, 1e6, "us")
        spread("  ... until `ignored` is read", read, 1e6, "us")
        spread("observe -> rule -> set -> step, per step", loop, 1e6, "us")
        spread("free-running step", free, 1e6, "us")
        if hasattr(eng, "set_vehicle_speed"):
            dicts, each = [], []
            for _ in range(args.repeats):
                restore()
                eng.sync()
                t0 = time.perf_counter()
                speeds = eng.get_vehicle_speed()
                t1 = time.perf_counter()
                ids = sorted(speeds)[:args.sample]
                t2 = time.perf_counter()
                for v in ids:
                    eng.set_vehicle_speed(v, 0.5 * speeds[v])
                t3 = time.perf_counter()
                dicts.append(t1 - t0), each.append((t3 - t2) / max(len(ids), 1))
            spread("get_vehicle_speed()", dicts)
            spread("set_vehicle_speed(), per vehicle (%d sampled)" % len(ids), each, 1e6, "us")
        del restore, ck, eng


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("bench", "vector16", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--poses", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--control", action="store_true")
    ap.add_argument("--dense", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--sample", type=int, default=300)
    a = ap.parse_args()
    control(a) if a.control else trace(a) if a.trace else measure(a)
