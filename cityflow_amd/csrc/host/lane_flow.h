// Per-lane flow and waiting-time statistics across steps (include/cityflow_amd.h "cfx_lane_flow_enable" has the rules), as
// Engine and VectorEngine hold them.  On a backend that exports the five optional entry points the device keeps the tracker
// and this is a thin dispatcher.  A backend without them (the CPU twin) gets the HOST tracker below: the same rules in C++
// over cfx_get_vehicles (vid, drivable, speed), ticked by the owner after every step.  Both keep the tracker in the same form —
// a {lane, tick last seen on it, since, wait} record per vehicle number and a cfx_lane_flow_lane per lane — so a host that
// renumbers the vehicles (EngineHost::compactVehicles) carries either through the same few lines.
#pragma once

#include <cstdint>
#include <vector>

#include "cityflow_amd.h"

namespace cfa {

struct Backend;

// the six outputs, [n_lanes] each (of every environment); any may be null
struct LaneFlowOut {
    int32_t *entered = nullptr, *left = nullptr;
    int64_t *leftSteps = nullptr, *leftWaitingSteps = nullptr, *waitingSteps = nullptr;
    int32_t *maxWaitingSteps = nullptr;
};

struct LaneFlowState {
    std::vector<int32_t> records;  // [4 * vehicle numbers]
    std::vector<cfx_lane_flow_lane> lanes;
    int32_t tick = 0;
    // the vehicles renumbered: record v moves to newOfOld[v] (-1: forgotten); the lanes stay as they are
    void renumber(const std::vector<int32_t> &newOfOld, int nLive);
};

class LaneFlow {
public:
    void bind(const Backend *be, cfx_engine *dev, int nLanes) {
        be_ = be;
        dev_ = dev;
        nLanes_ = nLanes;
    }
    bool on() const { return on_; }
    bool onDevice() const;                    // the backend keeps the tracker (all five entry points)
    void enable(bool on, int64_t step);       // on: a baseline at `step`; off: everything is freed
    void afterStep(int64_t step);             // the tick (host tracker; the device ticks inside cfx_step)
    void baseline(int64_t step);              // after a reset / load (host tracker; the device takes its own)
    void features(const LaneFlowOut &out, bool reset);
    void observeDevice(const LaneFlowOut &out, bool reset, uintptr_t consumerStream);
    // s - since and wait of the first k vehicles of every lane from the front, as of the last tick ([n_lanes * k] each, either may
    // be null; 0, 0 in the padding and for a vehicle whose record is not this lane's at that tick).  Changes nothing
    void fronts(int k, int32_t *laneSteps, int32_t *waitingSteps);
    LaneFlowState state(int nVehicles);       // ... around a renumbering load
    void setState(const LaneFlowState &s);

private:
    void requireOn(const char *what) const;
    void fail(const char *what) const;
    void walk(int64_t step, bool baseline);
    const Backend *be_ = nullptr;
    cfx_engine *dev_ = nullptr;
    int nLanes_ = 0;
    bool on_ = false;
    LaneFlowState host_;                      // the host tracker
    int32_t hostStep_ = 0;                    // ... the step of its last tick
    std::vector<int32_t> vid_, drv_, n_, entered_, inc_, max_;  // scratch of a tick
    std::vector<double> speed_;
    std::vector<int64_t> since_, wait_;
};

}  // namespace cfa
