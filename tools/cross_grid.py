"""Developer tool: what kr_cross's grids do on the bench workload (profiles/cross_grid.txt).

  python tools/cross_grid.py run [lib=PATH] [steps=200] [warmup=20]
      the bench workload stepped free-running as bench.py steps it (300 build-up steps, warm-up, the timed steps); prints the
      device's own counters over the timed steps (Engine._host_stats: launches in which a group took a second job, the most
      jobs a group took) and the time per step.  Under `rocprofv3 --kernel-trace -- python tools/cross_grid.py run ...` the
      trace's last `steps` kr_cross launches are the timed steps.
  python tools/cross_grid.py jobs OUT.json [steps=200] [warmup=20]
      the same steps with the scalars read after every step: the cross phase's job count of every timed step (the run is
      deterministic, so these are the counts of the free-running launches too)
  python tools/cross_grid.py table RESULTS.db JOBS.json [first_step=320] [cycle=35]
      the trace and the counts side by side, launch by launch: blocks, groups, jobs, the passes the busiest group needs at
      least (jobs over groups, rounded up: the shards are not quite even), duration; then the launches by their place in the
      signal cycle, and one-pass against several-pass launches"""
import json
import os
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _options(args):
    opt = {"steps": 200, "warmup": 20, "lib": "", "first_step": 320, "cycle": 35}
    for a in args:
        k, v = a.split("=", 1)
        opt[k] = v if k == "lib" else int(v)
    return opt


def _engine(lib):
    argv, sys.argv = sys.argv, [sys.argv[0]]
    import bench
    sys.argv = argv
    from cityflow_amd import _cityflow
    cfg = bench.build_workload("/tmp/cfa_cross_grid", 0)
    eng = _cityflow.Engine._with_backend(cfg, 1, os.path.abspath(lib)) if lib else _cityflow.Engine(cfg, 1)
    for _ in range(bench.BUILD_UP_STEPS):
        eng.next_step()
    eng.sync()
    return eng


def run(opt):
    eng = _engine(opt["lib"])
    for _ in range(opt["warmup"]):
        eng.next_step()
    eng.sync()
    eng._host_stats(True)
    t0 = time.perf_counter()
    for _ in range(opt["steps"]):
        eng.next_step()
    eng.sync()
    us = (time.perf_counter() - t0) / opt["steps"] * 1e6
    hs = eng._host_stats(False)
    print("%s: %d timed steps, %.2f us per step; kr_cross launches in which a group took a second job: %s, most jobs one group took: %s, "
          "last launch %s blocks for %s jobs, held peak %s; kr_action blocks over one pass: %s at %s lanes per block" % (
              opt["lib"] or "the tree's library", opt["steps"], us, hs.get("cross_multi_pass_launches"), hs.get("cross_max_passes"),
              hs.get("cross_last_grid_blocks"), hs.get("cross_last_jobs"), hs.get("cross_held_jobs"), hs.get("action_multi_pass_blocks"),
              hs.get("action_lanes_per_block")))


def jobs(out, opt):
    eng = _engine(opt["lib"])
    counts = []
    for s in range(opt["warmup"] + opt["steps"]):
        eng.next_step()
        n = eng._scalars()["diag_cross_jobs"]
        if s >= opt["warmup"]:
            counts.append(int(n))
    with open(out, "w") as f:
        json.dump(counts, f)
    print("jobs of %d steps: min %d, max %d -> %s" % (len(counts), min(counts), max(counts), out))


def table(db_path, jobs_path, opt):
    with open(jobs_path) as f:
        counts = json.load(f)
    n = len(counts)
    cur = sqlite3.connect(db_path).cursor()
    rows = cur.execute("select grid_x, workgroup_x, duration from kernels where name like '%kr_cross%' order by start desc limit ?", (n,)).fetchall()
    rows.reverse()
    assert len(rows) == n, "the trace has %d kr_cross launches, %d wanted" % (len(rows), n)
    cyc = opt["cycle"]
    print("%5s %6s %7s %7s %7s %7s %9s" % ("step", "cycle", "blocks", "groups", "jobs", "passes", "us"))
    one, several, by_place = [], [], {}
    for i, ((gx, wg, dur), nj) in enumerate(zip(rows, counts)):
        step = opt["first_step"] + i
        blocks = gx // wg if gx % wg == 0 and gx >= wg * 16 else gx  # (threads or blocks, whichever the trace holds)
        groups = blocks * 16
        passes = (nj + groups - 1) // groups
        (several if passes > 1 else one).append(dur / 1e3)
        by_place.setdefault(step % cyc, []).append((dur / 1e3, passes))
        print("%5d %6d %7d %7d %7d %7d %9.2f" % (step, step % cyc, blocks, groups, nj, passes, dur / 1e3))
    print("\nby place in the %d-step signal cycle: launches, of them with several passes, mean us" % cyc)
    for place in sorted(by_place):
        v = by_place[place]
        print("%5d %4d %4d %9.2f" % (place, len(v), sum(1 for _d, p in v if p > 1), sum(d for d, _p in v) / len(v)))
    allv = one + several
    print("\nall      %4d launches: mean %6.2f  min %6.2f  max %6.2f us" % (len(allv), sum(allv) / len(allv), min(allv), max(allv)))
    for name, v in (("one pass", one), ("several ", several)):
        if v:
            print("%s %4d launches: mean %6.2f  min %6.2f  max %6.2f us" % (name, len(v), sum(v) / len(v), min(v), max(v)))
        else:
            print("%s    0 launches" % name)
    print("peak jobs %d against %d groups resident at once (1024 blocks of 16)" % (max(counts), 16 * 1024))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "run":
        run(_options(sys.argv[2:]))
    elif mode == "jobs":
        jobs(sys.argv[2], _options(sys.argv[3:]))
    elif mode == "table":
        table(sys.argv[2], sys.argv[3], _options(sys.argv[4:]))
    else:
        sys.exit(__doc__)
