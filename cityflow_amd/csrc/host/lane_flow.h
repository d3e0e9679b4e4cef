// Per-lane flow and waiting-time statistics across steps (include/cityflow_amd.h "cfx_lane_flow_enable" has the rules), as
// Engine and VectorEngine hold them (tracker_base.h has the lifecycle).  The host tracker walks cfx_get_vehicles (vid, drivable,
// speed).  Device and host keep the tracker in the same form: a vehicle record per number and a cfx_lane_flow_lane per lane.
#pragma once

#include "tracker_base.h"

namespace cfa {

// the six outputs, [n_lanes] each (of every environment); any may be null
struct LaneFlowOut {
    int32_t *entered = nullptr, *left = nullptr;
    int64_t *leftSteps = nullptr, *leftWaitingSteps = nullptr, *waitingSteps = nullptr;
    int32_t *maxWaitingSteps = nullptr;
};

struct LaneFlowState : VehicleRecords {
    std::vector<cfx_lane_flow_lane> lanes;  // (a renumbering leaves them as they are)
};

class LaneFlow : public TrackerBase {
public:
    LaneFlow() : TrackerBase("lane-flow", "track_lane_flow") {}
    void bind(const Backend *be, cfx_engine *dev, int nLanes);
    void enable(bool on, int64_t step);       // on: a baseline at `step`; off: everything is freed
    void features(const LaneFlowOut &out, bool reset);
    void observeDevice(const LaneFlowOut &out, bool reset, uintptr_t consumerStream);
    // s - since and wait of the first k vehicles of every lane from the front, as of the last tick ([n_lanes * k] each, either may
    // be null; 0, 0 in the padding and for a vehicle whose record is not this lane's at that tick).  Changes nothing
    void fronts(int k, int32_t *laneSteps, int32_t *waitingSteps);
    LaneFlowState state(int nVehicles);       // ... around a renumbering load
    void setState(const LaneFlowState &s);

private:
    void walk(int64_t step, bool baseline) override;
    int nLanes_ = 0;
    LaneFlowState host_;                      // the host tracker
    int32_t hostStep_ = 0;                    // ... the step of its last tick
    std::vector<int32_t> n_, entered_, inc_, max_;  // scratch of a tick
    std::vector<int64_t> since_, wait_;
};

}  // namespace cfa
