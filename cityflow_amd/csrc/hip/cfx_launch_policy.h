// How many 16-lane groups a kr_cross launch gets (plain C++: the host side of cfx_hip.hip and a stand-alone test include it).
//
// The device reports the cross phase's job count of a step when that step's commit has run; a free-running host is up to
// kMaxLead + 2 steps ahead of it, so the count a launch is sized from is about 18 steps old.  Where every signal of a network
// switches at once the queue collapses for the few steps of an all-red phase and comes back at once: sized from the last
// report alone (count + 25 % + 256), the launches 18 steps behind the collapse get a grid for the short queue while the
// long one is back, and every group of such a launch walks two vehicles' chains one after the other.
//
// So the grid follows the PEAK of the reports, and forgets it slowly: 1/512 per reported step (at least one job), which
// loses less than 11 % + 53 jobs over a 35-step signal cycle plus the lead — inside the margin — and more than half within
// 400 steps, so that a network that empties stops paying for a grid of idle blocks.  A window maximum does the same with a
// ring of one entry per step of the longest cycle it is to cover (and a cycle length to choose); the decaying peak is two words.
//
// Time is counted in REPORTED steps: a report that repeats (the host ran ahead of the device) decays nothing, one that
// skips steps decays once for every step skipped, and a step number that goes back (reset, load) starts over.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cfx_policy {

constexpr int kCrossLanes = 16;          // lanes of a group (kCrossGroup)
constexpr int kCrossThreads = 256;       // threads of a block (kCrossBlock): 16 groups
constexpr size_t kCrossMinBlocks = 64;   // floor of the grid
constexpr size_t kCrossMaxBlocks = 32768;  // and its cap
constexpr int kCrossShards = 16;         // a block serves the shard its index names: fewer blocks would leave a shard unserved
constexpr int kPeakDecayShift = 9;       // the held peak loses 1/512 per reported step
constexpr int64_t kPeakForgetSteps = 1 << 14;  // a gap this long forgets the peak outright

// the margin over a job count: a quarter and 256 groups
inline size_t crossGroupsFor(size_t jobs) { return jobs + jobs / 4 + 256; }

// the groups a launch gets from one job count (0: none reported) and the running vehicles' estimate
inline size_t crossGroups(size_t activeEst, size_t jobs) {
    const size_t byActive = activeEst / 4;
    return jobs > 0 ? std::min(byActive, crossGroupsFor(jobs)) : byActive;
}

// groups -> blocks of the launch; `forced` > 0 (developer knob) names the blocks outright
inline int crossBlocks(size_t groups, int forced = 0) {
    if (forced > 0) return (int) std::min<size_t>(std::max<size_t>((size_t) forced, (size_t) kCrossShards), kCrossMaxBlocks);
    const size_t blocks = (groups * kCrossLanes + kCrossThreads - 1) / kCrossThreads;
    return (int) std::min(std::max(kCrossMinBlocks, blocks), kCrossMaxBlocks);
}

struct CrossGridPolicy {
    int64_t held = 0;       // the decayed peak of the reports
    int64_t lastStep = -1;  // step of the newest report taken (-1: none)

    void reset() {
        held = 0;
        lastStep = -1;
    }
    // a report of the device: `jobs` vehicles were queued for the cross phase of `step`
    void report(int64_t step, int64_t jobs) {
        if (jobs < 0) jobs = 0;
        if (lastStep < 0 || step < lastStep || step - lastStep >= kPeakForgetSteps) {
            held = jobs;
            lastStep = step;
            return;
        }
        for (int64_t i = lastStep; i < step && held > jobs; ++i) held -= (held >> kPeakDecayShift) + 1;
        held = std::max(held, jobs);
        lastStep = step;
    }
    // the groups of the next launch; without a report (or with none above zero) as by the running vehicles alone
    size_t groups(size_t activeEst) const { return crossGroups(activeEst, lastStep < 0 ? 0 : (size_t) held); }
};

}  // namespace cfx_policy
