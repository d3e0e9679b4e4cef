// Lane-flow tracker: dispatcher over the backend's entry points and the host tracker (lane_flow.h).
#include "lane_flow.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine_host.h"

namespace cfa {

void LaneFlow::bind(const Backend *be, cfx_engine *dev, int nLanes) {
    bindBackend(be, dev, "cfx_lane_flow_enable", be->cfx_lane_flow_enable, be->cfx_observe_lane_flow_device, be->cfx_get_lane_flow,
                be->cfx_lane_flow_get_state, be->cfx_lane_flow_set_state);
    nLanes_ = nLanes;
}

void LaneFlow::enable(bool on, int64_t step) {
    if (!switchTo(on)) return;
    host_ = LaneFlowState{};
    if (!on) {
        for (std::vector<int32_t> *v : {&n_, &entered_, &inc_, &max_}) std::vector<int32_t>().swap(*v);
        std::vector<int64_t>().swap(since_);
        std::vector<int64_t>().swap(wait_);
        return;
    }
    host_.lanes.assign((size_t) nLanes_, cfx_lane_flow_lane{});
    walk(step, true);
}

// one tick (or baseline) of the host tracker: the rules of include/cityflow_amd.h over the running vehicles as the backend lists them
void LaneFlow::walk(int64_t step, bool baseline) {
    const VehicleColumns v = vehicleColumnsOf(*be_, dev_, true, false, true);
    const size_t L = (size_t) nLanes_;
    n_.assign(L, 0);
    entered_.assign(L, 0);
    inc_.assign(L, 0);
    max_.assign(L, 0);
    since_.assign(L, 0);
    wait_.assign(L, 0);
    const int32_t tick = ++host_.tick, s = (int32_t) step;
    hostStep_ = s;
    for (int i = 0; i < v.count; ++i) {
        const int32_t l = v.drivable[(size_t) i], id = v.vid[(size_t) i];
        if (l < 0 || l >= nLanes_ || id < 0) continue;  // (on a laneLink: on no lane)
        int32_t *r = host_.of(id);
        if (baseline || r[0] != l || r[1] != tick - 1) {
            r[2] = s;
            r[3] = 0;
            entered_[(size_t) l] += 1;
        }
        r[0] = l;
        r[1] = tick;
        if (!baseline && v.speed[(size_t) i] < 0.1) {
            r[3] += 1;
            inc_[(size_t) l] += 1;
        }
        n_[(size_t) l] += 1;
        since_[(size_t) l] += r[2];
        wait_[(size_t) l] += r[3];
        max_[(size_t) l] = std::max(max_[(size_t) l], r[3]);
    }
    for (size_t l = 0; l < L; ++l) {
        cfx_lane_flow_lane &a = host_.lanes[l];
        if (baseline) {
            a.left_steps = a.left_waiting_steps = 0;
            a.entered = a.left = 0;
        }
        closeFlowRecord(a, baseline, s, n_[l], entered_[l], inc_[l], since_[l], wait_[l], max_[l]);
    }
}

void LaneFlow::features(const LaneFlowOut &o, bool reset) {
    requireOn("observe_lane_flow");
    if (onDevice()) {
        if (be_->cfx_get_lane_flow(dev_, o.entered, o.left, o.leftSteps, o.leftWaitingSteps, o.waitingSteps, o.maxWaitingSteps,
                                   reset ? 1 : 0) != CFX_OK)
            fail("cfx_get_lane_flow");
        return;
    }
    for (size_t l = 0; l < host_.lanes.size(); ++l) {
        cfx_lane_flow_lane &a = host_.lanes[l];
        if (o.entered) o.entered[l] = a.entered;
        if (o.left) o.left[l] = a.left;
        if (o.leftSteps) o.leftSteps[l] = a.left_steps;
        if (o.leftWaitingSteps) o.leftWaitingSteps[l] = a.left_waiting_steps;
        if (o.waitingSteps) o.waitingSteps[l] = a.waiting_steps;
        if (o.maxWaitingSteps) o.maxWaitingSteps[l] = a.max_waiting_steps;
        if (reset) {
            a.left_steps = a.left_waiting_steps = 0;
            a.entered = a.left = 0;
        }
    }
}

void LaneFlow::observeDevice(const LaneFlowOut &o, bool reset, uintptr_t consumerStream) {
    requireOn("observe_lane_flow_tensor");
    requireDevice("lane-flow statistics");
    if (be_->cfx_observe_lane_flow_device(dev_, o.entered, o.left, o.leftSteps, o.leftWaitingSteps, o.waitingSteps, o.maxWaitingSteps,
                                          reset ? 1 : 0, (void *) consumerStream) != CFX_OK)
        fail("cfx_observe_lane_flow_device");
}

void LaneFlow::fronts(int k, int32_t *laneSteps, int32_t *waitingSteps) {
    requireOn("lane fronts");
    if (onDevice()) {
        if (!be_->cfx_get_lane_obs) throw std::runtime_error("cityflow_amd: '" + be_->path + "' has no front-vehicle observations");
        cfx_lane_obs a{};
        a.struct_size = (int32_t) sizeof a;
        a.n_front = k;
        a.front_lane_steps = laneSteps;
        a.front_waiting_steps = waitingSteps;
        if (be_->cfx_get_lane_obs(dev_, &a) != CFX_OK) fail("cfx_get_lane_obs");
        return;
    }
    const size_t n = (size_t) nLanes_ * k;
    if (laneSteps) std::fill(laneSteps, laneSteps + n, 0);
    if (waitingSteps) std::fill(waitingSteps, waitingSteps + n, 0);
    const VehicleColumns v = vehicleColumnsOf(*be_, dev_, true, false, false);
    n_.assign((size_t) nLanes_, 0);  // (vehicles seen per lane: front to back inside one)
    for (int i = 0; i < v.count; ++i) {
        const int32_t l = v.drivable[(size_t) i], id = v.vid[(size_t) i];
        if (l < 0 || l >= nLanes_) continue;
        const int slot = n_[(size_t) l]++;
        if (slot >= k || id < 0 || 4 * (size_t) id + 3 >= host_.records.size()) continue;
        const int32_t *r = &host_.records[4 * (size_t) id];
        if (r[0] != l || r[1] != host_.tick) continue;
        if (laneSteps) laneSteps[(size_t) l * k + slot] = hostStep_ - r[2];
        if (waitingSteps) waitingSteps[(size_t) l * k + slot] = r[3];
    }
}

LaneFlowState LaneFlow::state(int nVehicles) {
    requireOn("lane flow");
    if (!onDevice()) {
        LaneFlowState s = host_;
        s.records.resize((size_t) nVehicles * 4, -1);
        return s;
    }
    LaneFlowState s;
    s.records.assign((size_t) nVehicles * 4, -1);
    s.lanes.assign((size_t) nLanes_, cfx_lane_flow_lane{});
    if (be_->cfx_lane_flow_get_state(dev_, s.records.data(), nVehicles, s.lanes.data(), &s.tick) != CFX_OK) fail("cfx_lane_flow_get_state");
    return s;
}

void LaneFlow::setState(const LaneFlowState &s) {
    requireOn("lane flow");
    if (!onDevice()) {
        host_ = s;
        return;
    }
    if (be_->cfx_lane_flow_set_state(dev_, s.records.data(), (int32_t) (s.records.size() / 4), s.lanes.data(), s.tick) != CFX_OK)
        fail("cfx_lane_flow_set_state");
}

}  // namespace cfa
