"""What checkpoint() / rollback() cost beside snapshot() / load(), and what they buy a rollout loop.

  python tools/checkpoint_loop.py [--which bench|6x6|vector|vector16|all] [--repeats 5] [--rollout-steps 300] [--candidates 3]
      bench   the benchmark workload (bench.build_workload: 30x30, ~96 k running vehicles after bench.BUILD_UP_STEPS steps,
              Lane::history on)
      6x6     the stock grid_6x6 after 300 steps
      vector  a 64-environment grid_6x6 VectorEngine after 300 steps (no snapshot / load there: absolute times only)
      vector16  the same with 16 environments
      Per workload: checkpoint() + rollback() + sync() and snapshot() + load() + sync() timed as pairs, alternating in the same
      process after a warm-up of each, `repeats` times, median / min / max printed with device_bytes; then a rollout of
      `rollout-steps` steps per candidate in the form "checkpoint once, roll back per candidate" against rebuilding the state
      from step 0 (reset(True) and the steps up to it) for every candidate.  The two forms must end in the same state.
      A VectorEngine also gets rollback(ck), rollback(ck, envs=identity) and rollback(ck, envs=the 8 environments with the
      fewest vehicles, tiled over the slots), each ending in sync(), timed in turn in every repeat after a warm-up of each;
      then "continue every slot from the 8 survivors": the gathered rollback and `rollout-steps` steps, beside the rollout
      rebuilt from step 0 above.

  python tools/checkpoint_loop.py --trace [--iters 20]
      the workload for a `rocprofv3 --kernel-trace --stats` run of its own: `iters` checkpoint(into=) + rollback() pairs on the
      benchmark workload (k_pack_segments, kr_gather, kr_offsets, kr_scatter_in, k_checkpoint_state_gap).

  python tools/checkpoint_loop.py --trace-envs [--iters 20] [--envs 64]
      the same for rollback(ck, envs=the 8 survivors tiled) on the 64-environment VectorEngine (k_env_gather_running,
      k_env_gather_table, k_env_gather_net, kr_scatter_in)."""
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
from cityflow_amd import scenarios  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(name, ts):
    print("  %-44s median %9.3f ms   min %9.3f   max %9.3f   (n = %d)" % (
        name, statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, len(ts)), flush=True)


def signature(eng):
    """Enough of the state to tell two runs apart: the two lane arrays and the counters."""
    sc = eng._scalars()
    return (eng.get_lane_vehicle_count_array().tobytes(), eng.get_lane_waiting_vehicle_count_array().tobytes(),
            sc["active_vehicle_count"], sc["finished_vehicle_count"], sc["cumulative_travel_time"])


def pairs(eng, repeats, with_archive):
    ck = eng.checkpoint()
    eng.rollback(ck)
    if with_archive:
        eng.load(eng.snapshot())
    eng.sync()
    new, old, save, back = [], [], [], []
    for _ in range(repeats):
        def new_pair():
            eng.checkpoint(into=ck)
            eng.rollback(ck)
            eng.sync()
        new.append(timed(new_pair))
        if with_archive:
            def old_pair():
                eng.load(eng.snapshot())
                eng.sync()
            old.append(timed(old_pair))
        save.append(timed(lambda: (eng.checkpoint(into=ck), eng.sync())))
        back.append(timed(lambda: (eng.rollback(ck), eng.sync())))
    print("  checkpoint: step %d, %d running vehicles, %d vehicle numbers, device_bytes %d (%.1f MB)" % (
        ck.step, ck.num_running, ck.num_vehicle_numbers, ck.device_bytes, ck.device_bytes / 1e6))
    spread("checkpoint() + rollback() + sync()", new)
    spread("  of which checkpoint(into=) + sync()", save)
    spread("  of which rollback() + sync()", back)
    if with_archive:
        spread("snapshot() + load() + sync()", old)
        print("  ratio of the medians %.1fx" % (statistics.median(old) / statistics.median(new)))
    return ck


def rollouts(eng, ck, steps_before, rollout_steps, candidates):
    from_ck, from_zero, sig = [], [], []
    for c in range(candidates):
        def a():
            eng.rollback(ck)
            for _ in range(rollout_steps):
                eng.next_step()
            eng.sync()
        from_ck.append(timed(a))
        sig.append(signature(eng))
    for c in range(candidates):
        def b():
            eng.reset(True)
            for _ in range(steps_before + rollout_steps):
                eng.next_step()
            eng.sync()
        from_zero.append(timed(b))
        assert signature(eng) == sig[c], "the rollout from the checkpoint and the one from step 0 end in different states"
    spread("rollout of %d steps from the checkpoint" % rollout_steps, from_ck)
    spread("... rebuilt from step 0 (%d + %d steps)" % (steps_before, rollout_steps), from_zero)


def survivors(eng, k=8):
    """envs of "keep the k environments with the fewest vehicles, continue every slot from them": the k tiled over the slots."""
    import numpy as np
    per_env = eng.get_lane_vehicle_count_array().sum(axis=1)
    best = np.argsort(per_env, kind="stable")[:k]
    return [int(best[r % len(best)]) for r in range(eng.num_envs)]


def gathered(eng, ck, repeats, rollout_steps):
    import inspect
    R = eng.num_envs
    eng.rollback(ck)
    identity, top = list(range(R)), survivors(eng)
    forms = (("rollback(ck) + sync()", None), ("rollback(ck, envs=identity) + sync()", identity),
             ("rollback(ck, envs=8 survivors tiled) + sync()", top))
    if "envs" not in inspect.signature(type(eng).rollback).parameters:  # (this tool beside an older build, for the A/B of the plain call)
        forms = forms[:1]
    times = {name: [] for name, _ in forms}
    for warm in (True, False):
        for _ in range(1 if warm else repeats):
            for name, envs in forms:
                t = timed(lambda: (eng.rollback(ck) if envs is None else eng.rollback(ck, envs=envs), eng.sync()))
                if not warm:
                    times[name].append(t)
    for name, _ in forms:
        spread(name, times[name])
    cont = []
    for _ in range(max(repeats // 2, 2) if len(forms) > 1 else 0):
        def a():
            eng.rollback(ck, envs=top)
            for _ in range(rollout_steps):
                eng.next_step()
            eng.sync()
        cont.append(timed(a))
    if cont:
        spread("every slot continued from the 8 survivors, %d steps" % rollout_steps, cont)
    eng.rollback(ck)
    eng.sync()


def workload(which, work):
    if which == "bench":
        eng = cityflow_amd.Engine(bench.build_workload(work, 0, scenario="grid_30x30"), 1)
        return eng, bench.BUILD_UP_STEPS, True
    cfg = scenarios.materialize("grid_6x6", work)
    if which == "6x6":
        return cityflow_amd.Engine(cfg, 1), 300, True
    return cityflow_amd.VectorEngine(cfg, 16 if which == "vector16" else 64, 1), 300, False


def measure(args):
    work = tempfile.mkdtemp(prefix="checkpoint_loop_")
    for which in (("bench", "6x6", "vector", "vector16") if args.which == "all" else (args.which,)):
        eng, before, with_archive = workload(which, work)
        eng.reset(True)  # (the same seeding as the rebuilt runs below)
        for _ in range(before):
            eng.next_step()
        eng.sync()
        print("%s: %s after %d steps, %d vehicles running%s" % (
            which, type(eng).__name__, before, eng.get_vehicle_count(),
            ", Lane::history %s" % ("on" if eng._keeps_lane_history() else "off") if with_archive else ""), flush=True)
        ck = pairs(eng, args.repeats, with_archive)
        if which.startswith("vector"):
            gathered(eng, ck, args.repeats, args.rollout_steps)
        rollouts(eng, ck, before, args.rollout_steps, args.candidates)
        ck.release()
        del eng


def trace(args):
    work = tempfile.mkdtemp(prefix="checkpoint_trace_")
    eng, before, _ = workload("bench", work)
    for _ in range(before):
        eng.next_step()
    ck = eng.checkpoint()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        eng.checkpoint(into=ck)
        eng.rollback(ck)
    eng.sync()
    print("%d checkpoint(into=) + rollback() pairs at %d running vehicles: %.3f ms each on the host's clock; device_bytes %d" % (
        args.iters, ck.num_running, (time.perf_counter() - t0) / args.iters * 1e3, ck.device_bytes), flush=True)


def trace_envs(args):
    work = tempfile.mkdtemp(prefix="checkpoint_trace_envs_")
    eng = cityflow_amd.VectorEngine(scenarios.materialize("grid_6x6", work), args.envs, 1)
    for _ in range(300):
        eng.next_step()
    ck = eng.checkpoint()
    top = survivors(eng)
    eng.rollback(ck, envs=top)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        eng.rollback(ck, envs=top)
    eng.sync()
    print("%d rollback(ck, envs=8 survivors tiled) at %d environments, %d running vehicles in the checkpoint, %d after: %.3f ms each on "
          "the host's clock" % (args.iters, args.envs, ck.num_running, eng.get_vehicle_count(), (time.perf_counter() - t0) / args.iters * 1e3),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", choices=("bench", "6x6", "vector", "vector16", "all"), default="all")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rollout-steps", type=int, default=300)
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-envs", action="store_true")
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    trace_envs(a) if a.trace_envs else trace(a) if a.trace else measure(a)
