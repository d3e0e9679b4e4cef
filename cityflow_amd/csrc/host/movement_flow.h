// Per-movement (roadLink) throughput and delay statistics across steps (include/cityflow_amd.h "cfx_movement_flow_enable" has the
// rules), as Engine and VectorEngine hold them (tracker_base.h has the lifecycle).  The host tracker walks cfx_get_vehicles (vid,
// drivable, speed).  Device and host keep the tracker in the same form: a vehicle record per number and a
// cfx_movement_flow_link per laneLink.
#pragma once

#include <cstddef>

#include "tracker_base.h"

namespace cfa {

// the eight outputs, [n_inters * max_roadlinks] each (of every environment); any may be null
struct MoveFlowOut {
    int32_t *entered = nullptr;
    int64_t *enteredLaneSteps = nullptr, *enteredLaneWaitingSteps = nullptr;
    int32_t *left = nullptr;
    int64_t *leftSteps = nullptr, *leftWaitingSteps = nullptr, *waitingSteps = nullptr;
    int32_t *maxWaitingSteps = nullptr;
};

struct MoveFlowState : VehicleRecords {
    std::vector<cfx_movement_flow_link> links;  // (a renumbering leaves them as they are)
};

class MoveFlow : public TrackerBase {
public:
    MoveFlow() : TrackerBase("movement-flow", "track_movement_flow") {}
    // `net`: ONE environment's network (it outlives this object); the backend numbers the drivables of `nEnvs` copies lanes
    // copy by copy, then laneLinks copy by copy
    void bind(const Backend *be, cfx_engine *dev, const cfx_net *net, int nEnvs);
    int maxRoadLinks() const { return M_; }
    size_t rows() const { return (size_t) R_ * I_ * M_; }
    void enable(bool on, int64_t step);       // on: a baseline at `step`; off: everything is freed
    void features(const MoveFlowOut &out, bool reset);
    void observeDevice(const MoveFlowOut &out, bool reset, uintptr_t consumerStream);
    MoveFlowState state(int nVehicles);       // ... around a renumbering load
    void setState(const MoveFlowState &s);

private:
    void walk(int64_t step, bool baseline) override;
    cfx_movement_flow_out descriptor(const MoveFlowOut &out, bool reset) const;
    const cfx_net *net_ = nullptr;
    int R_ = 0, L_ = 0, K_ = 0, I_ = 0, M_ = 0;  // environments; lanes, laneLinks, intersections of one; the longest roadLink row
    MoveFlowState host_;                      // the host tracker
    std::vector<int32_t> n_, entered_, inc_, max_;  // scratch of a tick, per laneLink
    std::vector<int64_t> since_, wait_;
};

}  // namespace cfa
