// Movement-flow tracker: dispatcher over the backend's entry points and the host tracker (movement_flow.h).
#include "movement_flow.h"

#include <algorithm>
#include <stdexcept>
#include <string>

#include "engine_host.h"

namespace cfa {

void MoveFlow::bind(const Backend *be, cfx_engine *dev, const cfx_net *net, int nEnvs) {
    bindBackend(be, dev, "cfx_movement_flow_enable", be->cfx_movement_flow_enable, be->cfx_observe_movement_flow_device,
                be->cfx_get_movement_flow, be->cfx_movement_flow_get_state, be->cfx_movement_flow_set_state);
    net_ = net;
    R_ = nEnvs;
    L_ = net->n_lanes;
    K_ = net->n_lanelinks;
    I_ = net->n_inters;
    M_ = 0;
    for (int i = 0; i < I_; ++i) M_ = std::max(M_, (int) net->inter_n_roadlinks[i]);
}

void MoveFlow::enable(bool on, int64_t step) {
    if (!switchTo(on)) return;
    host_ = MoveFlowState{};
    if (!on) {
        for (std::vector<int32_t> *v : {&n_, &entered_, &inc_, &max_}) std::vector<int32_t>().swap(*v);
        std::vector<int64_t>().swap(since_);
        std::vector<int64_t>().swap(wait_);
        return;
    }
    host_.links.assign((size_t) R_ * K_, cfx_movement_flow_link{});
    walk(step, true);
}

// one tick (or baseline) of the host tracker: the rules of include/cityflow_amd.h over the running vehicles as the backend lists
// them; the laneLink records in the difference form
void MoveFlow::walk(int64_t step, bool baseline) {
    const VehicleColumns v = vehicleColumnsOf(*be_, dev_, true, false, true);
    const int Lt = R_ * L_, Kt = R_ * K_;
    const size_t nK = (size_t) Kt;
    n_.assign(nK, 0);
    entered_.assign(nK, 0);
    inc_.assign(nK, 0);
    max_.assign(nK, 0);
    since_.assign(nK, 0);
    wait_.assign(nK, 0);
    if (baseline) host_.links.assign(nK, cfx_movement_flow_link{});
    const int32_t tick = ++host_.tick, s = (int32_t) step;
    for (int i = 0; i < v.count; ++i) {
        const int32_t d = v.drivable[(size_t) i], id = v.vid[(size_t) i];
        if (d < 0 || d >= Lt + Kt || id < 0) continue;
        int32_t *r = host_.of(id);
        if (baseline) {
            r[2] = s;
            r[3] = 0;
        } else if (r[1] != tick - 1 || r[0] != d) {  // new on d: where it was is read off the record before it is overwritten
            const int32_t p = r[1] == tick - 1 ? r[0] : -1;
            const bool fromLane = p >= 0 && p < Lt;
            if (d >= Lt) {
                cfx_movement_flow_link &a = host_.links[(size_t) (d - Lt)];
                entered_[(size_t) (d - Lt)] += 1;
                if (fromLane) {
                    a.entered_lane_steps += s - r[2];
                    a.entered_lane_waiting_steps += r[3];
                }
            } else if (fromLane) {  // lane -> lane: the first laneLink of p that ends on d
                const int env = p / L_, pl = p % L_;
                for (int q = net_->lane_ll_start[pl]; q < net_->lane_ll_start[pl + 1]; ++q) {
                    const int k = net_->lane_ll[q];
                    if (env * L_ + net_->ll_end_lane[k] != d) continue;
                    cfx_movement_flow_link &a = host_.links[(size_t) env * K_ + k];
                    a.entered += 1;
                    a.left += 1;
                    a.entered_lane_steps += s - r[2];
                    a.entered_lane_waiting_steps += r[3];
                    break;
                }
            }
            r[2] = s;
            r[3] = 0;
        }
        r[0] = d;
        r[1] = tick;
        const bool waiting = !baseline && v.speed[(size_t) i] < 0.1;
        if (waiting) r[3] += 1;
        if (d < Lt) continue;
        const size_t k = (size_t) (d - Lt);
        inc_[k] += waiting;
        n_[k] += 1;
        since_[k] += r[2];
        wait_[k] += r[3];
        max_[k] = std::max(max_[k], r[3]);
    }
    for (size_t k = 0; k < nK; ++k) closeFlowRecord(host_.links[k], baseline, s, n_[k], entered_[k], inc_[k], since_[k], wait_[k], max_[k]);
}

cfx_movement_flow_out MoveFlow::descriptor(const MoveFlowOut &o, bool reset) const {
    cfx_movement_flow_out a{};
    a.struct_size = (int32_t) sizeof a;
    a.max_roadlinks = M_;
    a.reset = reset ? 1 : 0;
    a.entered = o.entered;
    a.entered_lane_steps = o.enteredLaneSteps;
    a.entered_lane_waiting_steps = o.enteredLaneWaitingSteps;
    a.left = o.left;
    a.left_steps = o.leftSteps;
    a.left_waiting_steps = o.leftWaitingSteps;
    a.waiting_steps = o.waitingSteps;
    a.max_waiting_steps = o.maxWaitingSteps;
    return a;
}

void MoveFlow::features(const MoveFlowOut &o, bool reset) {
    requireOn("observe_movement_flow");
    if (onDevice()) {
        const cfx_movement_flow_out a = descriptor(o, reset);
        if (be_->cfx_get_movement_flow(dev_, &a) != CFX_OK) fail("cfx_get_movement_flow");
        return;
    }
    const size_t n = rows();
    auto zero = [n](auto *p) {
        if (p) std::fill(p, p + n, 0);
    };
    zero(o.entered);
    zero(o.enteredLaneSteps);
    zero(o.enteredLaneWaitingSteps);
    zero(o.left);
    zero(o.leftSteps);
    zero(o.leftWaitingSteps);
    zero(o.waitingSteps);
    zero(o.maxWaitingSteps);
    for (size_t k = 0; k < host_.links.size(); ++k) {
        cfx_movement_flow_link &a = host_.links[k];
        const size_t env = k / (size_t) K_, kk = k % (size_t) K_;
        const int i = net_->ll_inter[kk], m = net_->ll_roadlink[kk];
        if (i >= 0 && i < I_ && m >= 0 && m < M_ && !net_->inter_virtual[i]) {
            const size_t row = (env * I_ + (size_t) i) * M_ + (size_t) m;
            if (o.entered) o.entered[row] += a.entered;
            if (o.enteredLaneSteps) o.enteredLaneSteps[row] += a.entered_lane_steps;
            if (o.enteredLaneWaitingSteps) o.enteredLaneWaitingSteps[row] += a.entered_lane_waiting_steps;
            if (o.left) o.left[row] += a.left;
            if (o.leftSteps) o.leftSteps[row] += a.left_steps;
            if (o.leftWaitingSteps) o.leftWaitingSteps[row] += a.left_waiting_steps;
            if (o.waitingSteps) o.waitingSteps[row] += a.waiting_steps;
            if (o.maxWaitingSteps) o.maxWaitingSteps[row] = std::max(o.maxWaitingSteps[row], a.max_waiting_steps);
        }
        if (reset) {
            a.left_steps = a.left_waiting_steps = a.entered_lane_steps = a.entered_lane_waiting_steps = 0;
            a.entered = a.left = 0;
        }
    }
}

void MoveFlow::observeDevice(const MoveFlowOut &o, bool reset, uintptr_t consumerStream) {
    requireOn("observe_movement_flow_tensor");
    requireDevice("movement-flow statistics");
    const cfx_movement_flow_out a = descriptor(o, reset);
    if (be_->cfx_observe_movement_flow_device(dev_, &a, (void *) consumerStream) != CFX_OK) fail("cfx_observe_movement_flow_device");
}

MoveFlowState MoveFlow::state(int nVehicles) {
    requireOn("movement flow");
    if (!onDevice()) {
        MoveFlowState s = host_;
        s.records.resize((size_t) nVehicles * 4, -1);
        return s;
    }
    MoveFlowState s;
    s.records.assign((size_t) nVehicles * 4, -1);
    s.links.assign((size_t) R_ * K_ + 1, cfx_movement_flow_link{});  // (+1: never an empty array)
    if (be_->cfx_movement_flow_get_state(dev_, s.records.data(), nVehicles, s.links.data(), &s.tick) != CFX_OK)
        fail("cfx_movement_flow_get_state");
    s.links.resize((size_t) R_ * K_);
    return s;
}

void MoveFlow::setState(const MoveFlowState &s) {
    requireOn("movement flow");
    if (!onDevice()) {
        host_ = s;
        return;
    }
    std::vector<cfx_movement_flow_link> links = s.links;
    links.resize((size_t) R_ * K_ + 1);
    if (be_->cfx_movement_flow_set_state(dev_, s.records.data(), (int32_t) (s.records.size() / 4), links.data(), s.tick) != CFX_OK)
        fail("cfx_movement_flow_set_state");
}

}  // namespace cfa
