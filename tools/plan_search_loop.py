"""What set_tl_plan_tensor buys: evaluating many fixed-time signal plans under the same demand.

  python tools/plan_search_loop.py [--envs 64] [--steps 300] [--seed 3] [--runs 3]
      leg A  ONE VectorEngine(grid_6x6, R, seeds=[s] * R): R random plans set with one set_tl_plan_tensor, `steps` steps, the [R]
             average travel times read with get_average_travel_time_tensor — plans, steps and result never leave the device;
      leg B  the only route without the call: R engines, each built from a roadnet file rewritten with its plan (seed s), stepped
             one after the other, get_average_travel_time() of each.
      Both times are printed (engine construction and file writing counted apart), and leg A's travel times must equal leg B's
      per environment, exactly.

  python tools/plan_search_loop.py --rounds 2 [--keep 8] [--envs 64] [--steps 300] [--seed 3] [--runs 3]
      the search loop that rollback(ck, envs=) closes: per round R candidate plans run `steps` steps side by side, the `keep`
      environments with the lowest average travel time of the round survive, and EVERY slot goes on from a survivor's state
      (checkpoint(into=) + rollback(ck, envs=the survivors tiled)) under a new candidate: the survivor's plan, with some phases
      redrawn in all but the survivor's first slot.  Timed beside the only route without the call: every round starts with
      reset(True) and the earlier rounds again from step 0, each slot under the plans its state came from (round n costs n
      rounds of steps).  Both must end in the same lane counts.

  python tools/plan_search_loop.py --trace [--iters 220] [--which engine|vector]
      the workload for a `rocprofv3 --kernel-trace --stats` run of its own: set_tl_plan_tensor(durations, phase, phase_remain),
      get_tl_phase_durations_tensor and set_tl_phases_tensor, `iters` times each, on an Engine(grid_30x30) and on a
      VectorEngine(grid_6x6, 256) (both with rlTrafficLight, which set_tl_phases_tensor needs); tools/rocpd_summary.py lists
      k_set_tl_plan / k_get_phase_durations / k_set_phases_dense per grid size."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import cityflow_amd  # noqa: E402
from cityflow_amd import scenarios  # noqa: E402


def random_plans(rng, n_phases, P, R):
    """[R, I, P] float64: 5 to 40 s in whole seconds for every phase of every signalised intersection, 0 elsewhere."""
    T = np.zeros((R, len(n_phases), P))
    for i, n in enumerate(n_phases):
        if n > 0:
            T[:, i, :n] = rng.integers(5, 41, size=(R, n)).astype(np.float64)
    return T


def write_plan(cfg, ids, n_phases, T, tag, seed):
    with open(cfg) as f:
        c = json.load(f)
    with open(os.path.join(c["dir"], c["roadnetFile"])) as f:
        net = json.load(f)
    by_id = {it["id"]: it for it in net["intersections"]}
    for i, n in enumerate(n_phases):
        for p in range(max(n, 0)):
            by_id[ids[i]]["trafficLight"]["lightphases"][p]["time"] = float(T[i, p])
    c["roadnetFile"] = "roadnet_%s.json" % tag
    c["seed"] = seed
    with open(os.path.join(c["dir"], c["roadnetFile"]), "w") as f:
        json.dump(net, f)
    path = os.path.join(c["dir"], "config_%s.json" % tag)
    with open(path, "w") as f:
        json.dump(c, f)
    return path


def search(args):
    work = tempfile.mkdtemp(prefix="plan_search_")
    cfg = scenarios.materialize("grid_6x6", work, seed=args.seed)
    R = args.envs
    vec = cityflow_amd.VectorEngine(cfg, R, 1, seeds=[args.seed] * R)
    device = torch.device("cuda", vec._stream_handle()[1])
    n_phases = vec._phase_counts()
    P = vec._intersection_dims()[1]
    ids = vec.intersection_ids()
    plans = random_plans(np.random.default_rng(args.seed), n_phases, P, R)
    t0 = time.perf_counter()
    cfgs = [write_plan(cfg, ids, n_phases, plans[r], "plan%d" % r, args.seed) for r in range(R)]
    t_files = time.perf_counter() - t0
    t0 = time.perf_counter()
    singles = [cityflow_amd.Engine(c, 1) for c in cfgs]
    t_build = time.perf_counter() - t0
    vec.track_trips(True)
    d = torch.from_numpy(plans).to(device)
    a_times, b_times = [], []
    for run in range(args.runs):
        # leg A
        vec.reset(True)
        vec.sync()
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        vec.set_tl_plan_tensor(durations=d, phase_remain=d[:, :, 0].contiguous())
        for s in range(args.steps):
            vec.next_step()
        att = vec.get_average_travel_time_tensor()
        best = int(att.argmin())  # (the first wait for the device)
        a_times.append(time.perf_counter() - t0)
        # leg B
        for e in singles:
            e.reset(True)
            e.sync()
        t0 = time.perf_counter()
        want = []
        for e in singles:
            for s in range(args.steps):
                e.next_step()
            want.append(e.get_average_travel_time())
        b_times.append(time.perf_counter() - t0)
        got = att.cpu().numpy()
        assert np.array_equal(got, np.array(want)), "travel times differ:\n%s\n%s" % (got, want)
        print("run %d: one VectorEngine %8.1f ms   %d engines in turn %8.1f ms   best plan %d (%.3f s); travel times equal per env"
              % (run, a_times[-1] * 1e3, R, b_times[-1] * 1e3, best, got[best]), flush=True)
    print("%d plans x %d steps on grid_6x6, seeds all %d: %d distinct travel times, %.3f to %.3f s" % (
        R, args.steps, args.seed, len(set(got.tolist())), got.min(), got.max()))
    print("one VectorEngine, plans set on the device   median %8.1f ms  min %8.1f  max %8.1f" % (
        statistics.median(a_times) * 1e3, min(a_times) * 1e3, max(a_times) * 1e3))
    print("%d engines from rewritten files, in turn    median %8.1f ms  min %8.1f  max %8.1f   (+ once: %.1f ms writing the files, "
          "%.1f ms building the engines)" % (R, statistics.median(b_times) * 1e3, min(b_times) * 1e3, max(b_times) * 1e3,
                                             t_files * 1e3, t_build * 1e3))
    print("ratio of the medians %.1fx" % (statistics.median(b_times) / statistics.median(a_times)))


def search_rounds(args):
    work = tempfile.mkdtemp(prefix="plan_rounds_")
    cfg = scenarios.materialize("grid_6x6", work, seed=args.seed)
    R, k = args.envs, min(args.keep, args.envs)
    vec = cityflow_amd.VectorEngine(cfg, R, 1, seeds=[args.seed] * R)
    device = torch.device("cuda", vec._stream_handle()[1])
    n_phases = vec._phase_counts()
    P = vec._intersection_dims()[1]
    vec.track_trips(True)

    def run_round(plans):
        vec.set_tl_plan_tensor(durations=torch.from_numpy(plans).to(device))
        for s in range(args.steps):
            vec.next_step()
        return vec.get_average_travel_time_tensor().cpu().numpy()  # (of the round: the trackers took a baseline at its start)

    search_ms, gather_ms, rebuilt_ms = [], [], []
    ck = None
    for run in range(args.runs + 1):  # (run 0 warms up)
        rng = np.random.default_rng(args.seed + run)
        vec.restore_tl_plan()  # (a reset restarts the lights from the durations in force: both legs start from the file's)
        vec.reset(True)
        vec.sync()
        t0 = time.perf_counter()
        plans = random_plans(rng, n_phases, P, R)
        history, histories, t_gather = [], [], 0.0  # per round: the plans whose states the slots go on from
        for rnd in range(args.rounds):
            att = run_round(plans)
            history.append(plans)
            histories.append(list(history))
            if rnd + 1 == args.rounds:
                break
            best = np.argsort(att, kind="stable")[:k]
            envs = [int(best[r % k]) for r in range(R)]
            t1 = time.perf_counter()
            ck = vec.checkpoint(into=ck)
            vec.rollback(ck, envs=envs)
            t_gather += time.perf_counter() - t1
            history = [h[envs] for h in history]
            plans = plans[envs].copy()
            fresh = random_plans(rng, n_phases, P, R)
            redraw = rng.random(plans.shape) < 0.25
            redraw[:k] = False  # (the survivors themselves go on unchanged in the first k slots)
            plans = np.where(redraw & (plans > 0), fresh, plans)
        vec.sync()
        t_search = time.perf_counter() - t0
        lanes = vec.get_lane_vehicle_count_array()
        winner = int(att.argmin())
        # the same rounds without the call: each from step 0 again, every slot under the plans its state came from
        t0 = time.perf_counter()
        for upto in histories:
            vec.restore_tl_plan()
            vec.reset(True)
            for h in upto:
                run_round(h)
        vec.sync()
        t_rebuilt = time.perf_counter() - t0
        assert np.array_equal(vec.get_lane_vehicle_count_array(), lanes), "the searched and the rebuilt run end in different lane counts"
        if run:
            search_ms.append(t_search * 1e3), gather_ms.append(t_gather * 1e3), rebuilt_ms.append(t_rebuilt * 1e3)
            print("run %d: %d rounds of %d plans x %d steps, keep %d: %8.1f ms, of which checkpoint + gathered rollback %6.1f ms; "
                  "rebuilt from step 0 %8.1f ms; best of the last round: slot %d, %.3f s; end states equal"
                  % (run, args.rounds, R, args.steps, k, search_ms[-1], gather_ms[-1], rebuilt_ms[-1], winner, att[winner]), flush=True)
    for name, ts in (("search loop", search_ms), ("  checkpoint(into=) + rollback(ck, envs=)", gather_ms), ("rebuilt from step 0", rebuilt_ms)):
        print("%-44s median %8.1f ms  min %8.1f  max %8.1f" % (name, statistics.median(ts), min(ts), max(ts)))


def trace(args):
    work = tempfile.mkdtemp(prefix="plan_trace_")
    engines = [("Engine 30x30", cityflow_amd.Engine(scenarios.materialize("grid_30x30", work, rlTrafficLight=True), 1)),
               ("VectorEngine 256 x 6x6", cityflow_amd.VectorEngine(scenarios.materialize("grid_6x6", work, rlTrafficLight=True), 256))]
    for name, eng in engines:
        if args.which not in ("both", "engine" if name.startswith("Engine") else "vector"):
            continue
        device = torch.device("cuda", eng._stream_handle()[1])
        lead = tuple(eng._tensor_shapes()[1])
        P = eng._intersection_dims()[1]
        for s in range(5):
            eng.next_step()
        d = torch.full(lead + (P,), 7.0, dtype=torch.float64, device=device)
        ph = torch.zeros(lead, dtype=torch.int32, device=device)
        rem = torch.full(lead, 3.0, dtype=torch.float64, device=device)
        out = torch.empty(lead + (P,), dtype=torch.float64, device=device)
        t0 = time.perf_counter()
        for it in range(args.iters):
            eng.set_tl_plan_tensor(durations=d, phase=ph, phase_remain=rem)
            eng.get_tl_phase_durations_tensor(out=out)
            eng.set_tl_phases_tensor(ph)
        eng.sync()
        print("%s: %d intersections x %d phases = %d doubles; %.1f us per (set plan + get durations + set phases) on the host's clock"
              % (name, ph.numel(), P, d.numel(), (time.perf_counter() - t0) / args.iters * 1e6), flush=True)
        assert float(out.max()) == 7.0 and float(out.min()) == 0.0  # (the plan as set, 0.0 at the virtual intersections)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=0, help="the keep-the-best search loop with this many rounds (0: the plan evaluation)")
    ap.add_argument("--keep", type=int, default=8)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=220)
    ap.add_argument("--which", choices=("both", "engine", "vector"), default="both", help="--trace: one engine alone (a trace per size)")
    a = ap.parse_args()
    trace(a) if a.trace else search_rounds(a) if a.rounds else search(a)
