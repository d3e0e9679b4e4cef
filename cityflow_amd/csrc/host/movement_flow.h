// Per-movement (roadLink) throughput and delay statistics across steps (include/cityflow_amd.h "cfx_movement_flow_enable" has the
// rules), as Engine and VectorEngine hold them.  On a backend that exports the five optional entry points the device keeps the
// tracker and this is a thin dispatcher.  A backend without them (the CPU twin) gets the HOST tracker below: the same rules in
// C++ over cfx_get_vehicles (vid, drivable, speed), ticked by the owner after every step.  Both keep the tracker in the same form —
// a {drivable, tick last seen, since, wait} record per vehicle number and a cfx_movement_flow_link per laneLink — so a host that
// renumbers the vehicles (EngineHost::compactVehicles) carries either through the same few lines.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "cityflow_amd.h"

namespace cfa {

struct Backend;

// the eight outputs, [n_inters * max_roadlinks] each (of every environment); any may be null
struct MoveFlowOut {
    int32_t *entered = nullptr;
    int64_t *enteredLaneSteps = nullptr, *enteredLaneWaitingSteps = nullptr;
    int32_t *left = nullptr;
    int64_t *leftSteps = nullptr, *leftWaitingSteps = nullptr, *waitingSteps = nullptr;
    int32_t *maxWaitingSteps = nullptr;
};

struct MoveFlowState {
    std::vector<int32_t> records;  // [4 * vehicle numbers]
    std::vector<cfx_movement_flow_link> links;
    int32_t tick = 0;
    // the vehicles renumbered: record v moves to newOfOld[v] (-1: forgotten); the laneLinks stay as they are
    void renumber(const std::vector<int32_t> &newOfOld, int nLive);
};

class MoveFlow {
public:
    // `net`: ONE environment's network (it outlives this object); the backend numbers the drivables of `nEnvs` copies lanes
    // copy by copy, then laneLinks copy by copy
    void bind(const Backend *be, cfx_engine *dev, const cfx_net *net, int nEnvs);
    bool on() const { return on_; }
    bool onDevice() const;                    // the backend keeps the tracker (all five entry points)
    int maxRoadLinks() const { return M_; }
    size_t rows() const { return (size_t) R_ * I_ * M_; }
    void enable(bool on, int64_t step);       // on: a baseline at `step`; off: everything is freed
    void afterStep(int64_t step);             // the tick (host tracker; the device ticks inside cfx_step)
    void baseline(int64_t step);              // after a reset / load (host tracker; the device takes its own)
    void features(const MoveFlowOut &out, bool reset);
    void observeDevice(const MoveFlowOut &out, bool reset, uintptr_t consumerStream);
    MoveFlowState state(int nVehicles);       // ... around a renumbering load
    void setState(const MoveFlowState &s);

private:
    void requireOn(const char *what) const;
    void fail(const char *what) const;
    void walk(int64_t step, bool baseline);
    cfx_movement_flow_out descriptor(const MoveFlowOut &out, bool reset) const;
    const Backend *be_ = nullptr;
    cfx_engine *dev_ = nullptr;
    const cfx_net *net_ = nullptr;
    int R_ = 0, L_ = 0, K_ = 0, I_ = 0, M_ = 0;  // environments; lanes, laneLinks, intersections of one; the longest roadLink row
    bool on_ = false;
    MoveFlowState host_;                      // the host tracker
    std::vector<int32_t> n_, entered_, inc_, max_;  // scratch of a tick, per laneLink
    std::vector<int64_t> since_, wait_;
};

}  // namespace cfa
