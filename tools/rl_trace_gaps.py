"""Where the tensor loop of tools/rl_device_loop.py spends its time on the device timeline: a rocprofv3 kernel trace of
`python tools/rl_device_loop.py --skip-vector --iters 200` (rocpd / sqlite), the 200 timed iterations of the tensor loop, busy
time against idle gaps, the gaps grouped by the two kernels around them.
usage: python tools/rl_trace_gaps.py <results.db>"""
import sqlite3, sys, collections
db = sqlite3.connect(sys.argv[1])
ks = db.execute("select name, start, end, queue_id, stream_id from kernels order by start").fetchall()
def short(n):
    n = n.split("(")[0].replace("void ", "")
    return n.split("<")[0].replace("cfxd::", "").replace("at::native::", "torch:")
obs = [i for i, k in enumerate(ks) if short(k[0]) == "kr_lane_features"]
obs = obs[220:]                     # the numpy loop before it: 220 iterations, one launch each (the waiting counts)
lo, hi = obs[40], obs[440]          # tensor loop: 20 warm-up iterations (2 observations each) skipped, 200 timed
win = ks[lo:hi]
span = win[-1][2] - win[0][1]
busy, last_end = 0, win[0][1]
gaps = collections.defaultdict(lambda: [0, 0])
prev = None
for k in win:
    s, e = k[1], k[2]
    if s > last_end:
        busy += e - s
        g = s - last_end
        key = "%s -> %s" % (prev, short(k[0]))
        gaps[key][0] += g; gaps[key][1] += 1
    else:
        busy += max(0, e - last_end)
    last_end = max(last_end, e)
    prev = short(k[0])
n = 200
print("tensor loop, 200 iterations from the kernel trace: %.1f us per iteration on the device timeline, %.1f us busy, %.1f us idle"
      % (span / n / 1e3, busy / n / 1e3, (span - busy) / n / 1e3))
print("kernels per iteration: %.1f" % (len(win) / n))
print("idle gaps per iteration, by the two kernels around them (largest first):")
for key, (g, c) in sorted(gaps.items(), key=lambda x: -x[1][0])[:12]:
    print("  %-60s %7.1f us per iteration (%d gaps)" % (key, g / n / 1e3, c))
