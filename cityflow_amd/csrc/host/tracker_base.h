// What the four trackers of statistics kept across steps share on the host (lane_flow.h, movement_flow.h, trip_stats.h,
// detectors.h; DESIGN.md "One scaffold for the trackers").  On a backend that exports a tracker's optional entry points the device
// keeps it and the class is a thin dispatcher.  A backend without them (the CPU twin) gets the HOST tracker: the same rules in
// C++ over the backend's getters, ticked by the owner after every step and given a baseline after a reset or a load.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "cityflow_amd.h"

namespace cfa {

struct Backend;

class TrackerBase {
public:
    virtual ~TrackerBase() = default;
    bool on() const { return on_; }
    bool onDevice() const { return onDevice_; }  // the backend keeps the tracker (all its entry points)
    bool onHost() const { return on_ && !onDevice_; }
    // ---- host tracker (no-ops while the device keeps it, which ticks inside cfx_step and takes its own baselines)
    void afterStep(int64_t step) {
        if (onHost()) walk(step, false);
    }
    void baseline(int64_t step) {
        if (onHost()) walk(step, true);
    }

protected:
    // `name`, `pyCall`: as messages name the tracker and the Python call that turns it on ("lane-flow", "track_lane_flow")
    TrackerBase(const char *name, const char *pyCall) : name_(name), pyCall_(pyCall) {}
    template <typename Enable, typename... Rest>
    void bindBackend(const Backend *be, cfx_engine *dev, const char *enableName, Enable enable, Rest... rest) {
        be_ = be;
        dev_ = dev;
        enableName_ = enableName;
        enable_ = enable;
        onDevice_ = enable != nullptr && (... && (rest != nullptr));
    }
    // cfx_*_enable where the device keeps the tracker.  True: the HOST tracker is to be set up (on) or torn down by the caller
    bool switchTo(bool on);
    void requireOn(const char *what) const;    // "<what>: <name> tracking is off (<pyCall>(True) turns it on)"
    void requireDevice(const char *noun) const;  // "... has no device-side <noun>"
    void fail(const char *what) const;         // the backend's last error
    virtual void walk(int64_t step, bool baseline) = 0;  // one tick (or baseline) of the host tracker
    const Backend *be_ = nullptr;
    cfx_engine *dev_ = nullptr;
    bool on_ = false;

private:
    const char *name_, *pyCall_, *enableName_ = "";
    int32_t (*enable_)(cfx_engine *, int32_t) = nullptr;
    bool onDevice_ = false;
};

// A {drivable, tick last seen on it, since, wait} record per vehicle number, as both flow trackers keep it on the device and
// on the host: a host that renumbers the vehicles (EngineHost::compactVehicles) carries either through renumber()
struct VehicleRecords {
    std::vector<int32_t> records;  // [4 * vehicle numbers]; -1: never seen
    int32_t tick = 0;
    int32_t *of(int32_t vid) {     // (grown on access)
        const size_t at = 4 * (size_t) vid;
        if (at + 3 >= records.size()) records.resize(std::max(at + 4, 2 * records.size()), -1);
        return &records[at];
    }
    // record v moves to newOfOld[v] (-1: forgotten)
    void renumber(const std::vector<int32_t> &newOfOld, int nLive);
};

// The closing update of a lane's or a laneLink's record from what one tick of a HOST tracker found on it (`n` vehicles, `entered`
// of them new, `inc` waiting increments, sums `since` / `wait`, `mx`): who left is the difference of the sums
// (include/cityflow_amd.h).  Restated here on purpose: the twin-side trackers share no code with the HIP library.
template <typename A>
void closeFlowRecord(A &a, bool baseline, int32_t step, int32_t n, int32_t entered, int32_t inc, int64_t since, int64_t wait, int32_t mx) {
    if (!baseline) {
        const int32_t left = a.count + entered - n;
        a.entered += entered;
        a.left += left;
        a.left_steps += (int64_t) step * left - (a.since_sum + (int64_t) step * entered - since);
        a.left_waiting_steps += a.waiting_steps - (wait - inc);
    }
    a.since_sum = since;
    a.waiting_steps = wait;
    a.count = n;
    a.max_waiting_steps = mx;
}

}  // namespace cfa
