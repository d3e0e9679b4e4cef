// Stand-alone check of csrc/hip/cfx_launch_policy.h (tests/test_cross_grid_policy.py builds and runs it): synthetic job-count
// traces go through the policy the way launchRingCross feeds it — before every launch the newest report the host can see, which
// is `lag` steps old, repeats while the device is behind and skips steps when it catches up — and every launch's grid is held
// against the step's TRUE job count.  Prints "ok" and returns 0, or the first violated bound and 1.
#include <cstdio>
#include <functional>
#include <vector>

#include "cfx_launch_policy.h"

using namespace cfx_policy;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (failures++ < 20) {            \
                printf("FAILED %s: ", #cond); \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

constexpr size_t kPlenty = 40000000;  // running vehicles: the bound by them (a quarter) is far above every trace
constexpr int kLag = 18;              // kMaxLead + the two steps the commit's report trails its launch

struct Launch {
    int blocks;     // what the policy launched
    int oldBlocks;  // what the last report alone would have launched
};

// every step t: the report of step reportOf(t) (none below 0), then the launch
static std::vector<Launch> run(const std::vector<int> &jobs, const std::function<int(int)> &reportOf, CrossGridPolicy *keep = nullptr) {
    CrossGridPolicy p;
    std::vector<Launch> out;
    for (int t = 0; t < (int) jobs.size(); ++t) {
        const int r = reportOf(t);
        if (r >= 0) p.report(r, jobs[r]);
        out.push_back(Launch{crossBlocks(p.groups(kPlenty)), crossBlocks(crossGroups(kPlenty, r >= 0 ? (size_t) jobs[r] : 0))});
    }
    if (keep) *keep = p;
    return out;
}
static int lagged(int t) { return t - kLag; }
static int groupsOf(int blocks) { return blocks * (kCrossThreads / kCrossLanes); }

// (a) a signal cycle of 35 steps, trough to peak 1 : 3, reported 18 steps late: no launch after the first cycle is undersized
static void sawtooth(const char *name, int peak, const std::function<int(int)> &shape, const std::function<int(int)> &reportOf, int from) {
    std::vector<int> jobs;
    for (int t = 0; t < 35 * 40; ++t) jobs.push_back(shape(t));
    const std::vector<Launch> l = run(jobs, reportOf);
    int oldUnder = 0;
    for (int t = from; t < (int) jobs.size(); ++t) {
        CHECK(groupsOf(l[t].blocks) >= jobs[t], "%s peak %d: step %d has %d jobs and %d groups", name, peak, t, jobs[t], groupsOf(l[t].blocks));
        oldUnder += groupsOf(l[t].oldBlocks) < jobs[t];
    }
    // (what the trace is for: above the floor of 64 blocks the last report alone IS undersized in every cycle)
    if (peak > 2 * (int) kCrossMinBlocks * 16) CHECK(oldUnder > 0, "%s peak %d: the last report alone was never undersized", name, peak);
}

int main() {
    // ---- floor, cap, margin, forcing
    CHECK(crossBlocks(0) == 64, "floor");
    CHECK(crossBlocks(1000) == 64, "floor at 1000 groups");
    CHECK(crossBlocks(1025) == 65, "one group over 64 blocks");
    CHECK(crossBlocks((size_t) 1 << 30) == 32768, "cap");
    CHECK(crossGroups(kPlenty, 10000) == 10000 + 2500 + 256, "margin");
    CHECK(crossGroups(8000, 10000) == 2000, "the running vehicles bound the groups");
    CHECK(crossGroups(8000, 0) == 2000, "no report");
    CHECK(crossBlocks(123456, 16) == 16 && crossBlocks(0, 4096) == 4096, "forced blocks");
    CHECK(crossBlocks(0, 5) == 16, "forced below one block per shard");
    CHECK(crossBlocks(0, 100000) == 32768, "forced above the cap");

    // ---- (d) before a report, and after reset(): by the running vehicles alone
    {
        CrossGridPolicy p;
        CHECK(p.groups(96000) == 24000, "no report yet: %zu", p.groups(96000));
        p.report(7, 14000);
        CHECK(p.groups(96000) == 14000 + 3500 + 256, "first report: %zu", p.groups(96000));
        p.reset();
        CHECK(p.groups(96000) == 24000, "after reset: %zu", p.groups(96000));
        p.report(1000, 5000);
        p.report(3, 100);  // (the step counter went back: reset, load)
        CHECK(p.held == 100 && p.lastStep == 3, "step went back: held %lld", (long long) p.held);
        p.report(3 + kPeakForgetSteps, 7);
        CHECK(p.held == 7, "a gap of %lld steps: held %lld", (long long) kPeakForgetSteps, (long long) p.held);
    }

    // ---- (a)
    for (int peak : {900, 3000, 15000, 48000, 300000}) {
        const int trough = peak / 3;
        // the bench network's plan: 30 steps open, 5 steps all red; and the same starting inside the red phase
        sawtooth("30 + 5", peak, [=](int t) { return t % 35 < 30 ? peak : trough; }, lagged, 35);
        sawtooth("5 + 30", peak, [=](int t) { return t % 35 < 5 ? trough : peak; }, lagged, 35);
        // a linear ramp from trough to peak, dropping at once; and one rising at once and draining
        sawtooth("ramp up", peak, [=](int t) { return trough + (int) ((long long) (peak - trough) * (t % 35) / 34); }, lagged, 35);
        sawtooth("ramp down", peak, [=](int t) { return peak - (int) ((long long) (peak - trough) * (t % 35) / 34); }, lagged, 35);
        // reports that repeat twice and then skip two steps; reports whose lag wanders between 14 and 22 steps
        sawtooth("30 + 5, every third report", peak, [=](int t) { return t % 35 < 30 ? peak : trough; },
                 [](int t) { return t < kLag ? -1 : (t - kLag) / 3 * 3; }, 35 + 3);
        sawtooth("ramp up, wandering lag", peak, [=](int t) { return trough + (int) ((long long) (peak - trough) * (t % 35) / 34); },
                 [newest = -1](int t) mutable {  // (the newest report never goes back)
                     newest = std::max(newest, t - kLag + 4 - (t * 7) % 9);
                     return newest;
                 }, 35 + 4);
    }

    // ---- a constant trace: exactly the last report's grid, from the first report on
    for (int n : {0, 1, 700, 14000, 500000}) {
        const std::vector<int> jobs(2000, n);
        const std::vector<Launch> l = run(jobs, lagged);
        for (int t = 0; t < (int) jobs.size(); ++t)
            CHECK(l[t].blocks == l[t].oldBlocks, "constant %d: step %d has %d blocks, the last report alone %d", n, t, l[t].blocks, l[t].oldBlocks);
    }

    // ---- (c) the count falls to a quarter for good: within 2x of the last report's grid after at most 512 steps, never undersized
    for (int peak : {2000, 16000, 60000, 200000, 1200000}) {
        std::vector<int> jobs(200, peak);
        jobs.resize(200 + 2000, peak / 4);
        const std::vector<Launch> l = run(jobs, lagged);
        for (int t = kLag; t < (int) jobs.size(); ++t) {
            CHECK(groupsOf(l[t].blocks) >= jobs[t] || l[t].blocks == (int) kCrossMaxBlocks, "fall from %d: step %d undersized", peak, t);
            CHECK(l[t].blocks >= l[t].oldBlocks, "fall from %d: step %d below the last report's grid", peak, t);
            if (t >= 200 + 512)
                CHECK(l[t].blocks <= 2 * l[t].oldBlocks, "fall from %d: step %d still has %d blocks, the last report alone %d", peak, t,
                      l[t].blocks, l[t].oldBlocks);
        }
        // and the peak is forgotten altogether in the end
        std::vector<int> longRun(200, peak);
        longRun.resize(200 + 12000, peak / 4);
        CrossGridPolicy p;
        run(longRun, lagged, &p);
        CHECK(p.held == peak / 4, "fall from %d: held %lld after 12000 steps", peak, (long long) p.held);
    }
    // a network that empties: the same against the floor
    {
        std::vector<int> jobs(100, 9000);
        jobs.resize(100 + 12000, 0);
        CrossGridPolicy p;
        run(jobs, lagged, &p);
        CHECK(p.held == 0 && crossBlocks(crossGroupsFor((size_t) p.held)) == 64, "emptied: held %lld", (long long) p.held);
    }

    // ---- a single spike: nobody foresees it; from its report on it is covered, and 512 steps later it costs at most 2x
    for (int base : {1500, 14000}) {
        std::vector<int> jobs(1500, base);
        jobs[300] = 3 * base;
        const std::vector<Launch> l = run(jobs, lagged);
        for (int t = kLag; t < (int) jobs.size(); ++t) {
            if (t != 300) CHECK(groupsOf(l[t].blocks) >= jobs[t], "spike over %d: step %d undersized", base, t);
            if (t >= 300 + kLag && t < 300 + kLag + 35) CHECK(groupsOf(l[t].blocks) >= 3 * base, "spike over %d: not held at step %d", base, t);
            if (t >= 300 + kLag + 512) CHECK(l[t].blocks <= 2 * l[t].oldBlocks, "spike over %d: step %d still has %d blocks", base, t, l[t].blocks);
        }
    }
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
