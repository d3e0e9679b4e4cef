// Lane-flow tracker: dispatcher over the backend's entry points and the host tracker (lane_flow.h).
#include "lane_flow.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine_host.h"

namespace cfa {

void LaneFlowState::renumber(const std::vector<int32_t> &newOfOld, int nLive) {
    std::vector<int32_t> moved((size_t) nLive * 4, -1);
    for (size_t v = 0; v < newOfOld.size() && 4 * v + 3 < records.size(); ++v)
        if (newOfOld[v] >= 0 && newOfOld[v] < nLive) std::copy(records.begin() + 4 * v, records.begin() + 4 * v + 4, moved.begin() + 4 * (size_t) newOfOld[v]);
    records.swap(moved);
}

bool LaneFlow::onDevice() const {
    return be_->cfx_lane_flow_enable && be_->cfx_observe_lane_flow_device && be_->cfx_get_lane_flow && be_->cfx_lane_flow_get_state &&
           be_->cfx_lane_flow_set_state;
}

void LaneFlow::fail(const char *what) const {
    const char *msg = be_->cfx_last_error(dev_);
    throw std::runtime_error(std::string("cityflow_amd: ") + what + " failed: " + (msg ? msg : ""));
}

void LaneFlow::requireOn(const char *what) const {
    if (!on_) throw std::runtime_error(std::string(what) + ": lane-flow tracking is off (track_lane_flow(True) turns it on)");
}

void LaneFlow::enable(bool on, int64_t step) {
    if (on == on_) return;
    if (onDevice()) {
        if (be_->cfx_lane_flow_enable(dev_, on ? 1 : 0) != CFX_OK) fail("cfx_lane_flow_enable");
        on_ = on;
        return;
    }
    on_ = on;
    host_ = LaneFlowState{};
    if (!on) {
        for (std::vector<int32_t> *v : {&vid_, &drv_, &n_, &entered_, &inc_, &max_}) std::vector<int32_t>().swap(*v);
        std::vector<double>().swap(speed_);
        std::vector<int64_t>().swap(since_);
        std::vector<int64_t>().swap(wait_);
        return;
    }
    host_.lanes.assign((size_t) nLanes_, cfx_lane_flow_lane{});
    walk(step, true);
}

void LaneFlow::afterStep(int64_t step) {
    if (on_ && !onDevice()) walk(step, false);
}

void LaneFlow::baseline(int64_t step) {
    if (on_ && !onDevice()) walk(step, true);
}

// one tick (or baseline) of the host tracker: the rules of include/cityflow_amd.h over the running vehicles as the backend lists them
void LaneFlow::walk(int64_t step, bool baseline) {
    cfx_scalars sc{};
    if (be_->cfx_get_scalars(dev_, &sc) != CFX_OK) fail("cfx_get_scalars");
    cfx_vehicle_view v{};
    for (int cap = (int) sc.active_vehicle_count + 16;;) {
        vid_.resize((size_t) cap);
        drv_.resize((size_t) cap);
        speed_.resize((size_t) cap);
        v = cfx_vehicle_view{};
        v.capacity = cap;
        v.vid = vid_.data();
        v.drivable = drv_.data();
        v.speed = speed_.data();
        const int32_t rc = be_->cfx_get_vehicles(dev_, &v);
        if (rc == CFX_ERR_CAPACITY && v.count > cap) {
            cap = v.count + 16;
            continue;
        }
        if (rc != CFX_OK) fail("cfx_get_vehicles");
        break;
    }
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
        const int32_t l = drv_[(size_t) i], id = vid_[(size_t) i];
        if (l < 0 || l >= nLanes_ || id < 0) continue;  // (on a laneLink: on no lane)
        if (4 * (size_t) id + 3 >= host_.records.size()) host_.records.resize(std::max(4 * (size_t) id + 4, 2 * host_.records.size()), -1);
        int32_t *r = &host_.records[4 * (size_t) id];
        if (baseline || r[0] != l || r[1] != tick - 1) {
            r[2] = s;
            r[3] = 0;
            entered_[(size_t) l] += 1;
        }
        r[0] = l;
        r[1] = tick;
        if (!baseline && speed_[(size_t) i] < 0.1) {
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
        } else {  // who left is the difference of the lane's sums (include/cityflow_amd.h; laneFlowTick of the HIP library)
            const int32_t left = a.count + entered_[l] - n_[l];
            a.entered += entered_[l];
            a.left += left;
            a.left_steps += (int64_t) s * left - (a.since_sum + (int64_t) s * entered_[l] - since_[l]);
            a.left_waiting_steps += a.waiting_steps - (wait_[l] - inc_[l]);
        }
        a.since_sum = since_[l];
        a.waiting_steps = wait_[l];
        a.count = n_[l];
        a.max_waiting_steps = max_[l];
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
    if (!onDevice()) throw std::runtime_error("cityflow_amd: '" + be_->path + "' has no device-side lane-flow statistics");
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
