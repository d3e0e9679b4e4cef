// Detector tracker: dispatcher over the backend's entry points and the host tracker (detectors.h).
#include "detectors.h"

#include <cmath>
#include <stdexcept>
#include <string>

#include "engine_host.h"

namespace cfa {

void Detectors::bind(const Backend *be, cfx_engine *dev, int lanesPerEnv, int nEnvs) {
    bindBackend(be, dev, "cfx_detectors_enable", be->cfx_detectors_enable, be->cfx_detectors_define, be->cfx_observe_detectors_device,
                be->cfx_get_detectors, be->cfx_detectors_get_state, be->cfx_detectors_set_state);
    lanesPerEnv_ = lanesPerEnv;
    nEnvs_ = nEnvs;
}

void Detectors::define(const int32_t *lane, const double *start, const double *end, int n, int64_t step) {
    if (n < 1) throw std::invalid_argument("track_detectors: at least one detector");
    for (int i = 0; i < n; ++i) {  // (every entry before anything changes)
        const char *bad = (lane[i] < 0 || lane[i] >= lanesPerEnv_) ? "lane is not an index into lane_ids()"
                          : !(std::isfinite(start[i]) && start[i] >= 0.0) ? "start is not finite and >= 0"
                          : !(end[i] > start[i]) ? "end is not beyond start" : nullptr;
        if (bad) throw std::invalid_argument("track_detectors: position " + std::to_string(i) + ": " + bad);
    }
    if (onDevice() && be_->cfx_detectors_define(dev_, lane, start, end, n) != CFX_OK) fail("cfx_detectors_define");
    lane_.assign(lane, lane + n);
    start_.assign(start, start + n);
    end_.assign(end, end + n);
    switchTo(true);  // (the device: on takes the first baseline, and defining while on has taken one)
    if (onDevice()) return;
    hostTables();
    walk(step, true);
}

void Detectors::disable() {
    const bool host = switchTo(false);
    std::vector<int32_t>().swap(lane_);
    for (std::vector<double> *v : {&start_, &end_}) std::vector<double>().swap(*v);
    if (!host) return;
    host_ = DetectorState{};
    for (std::vector<int32_t> *v : {&first_, &order_, &entered_, &c_, &w_, &u_}) std::vector<int32_t>().swap(*v);
    std::vector<double>().swap(t_);
}

void Detectors::hostTables() {
    const size_t n = lane_.size(), L = (size_t) lanesPerEnv_ * nEnvs_;
    host_.dets.assign(n * nEnvs_, cfx_detector{});
    first_.assign(L + 1, 0);
    for (int r = 0; r < nEnvs_; ++r)
        for (size_t i = 0; i < n; ++i) {
            cfx_detector &a = host_.dets[(size_t) r * n + i];
            a.start = start_[i];
            a.end = end_[i];
            a.lane = r * lanesPerEnv_ + lane_[i];
            first_[(size_t) a.lane + 1] += 1;
        }
    for (size_t l = 0; l < L; ++l) first_[l + 1] += first_[l];
    order_.assign(host_.dets.size(), 0);
    std::vector<int32_t> at(first_.begin(), first_.end() - 1);
    for (size_t d = 0; d < host_.dets.size(); ++d) order_[(size_t) at[(size_t) host_.dets[d].lane]++] = (int32_t) d;
}

// one tick (or baseline) of the host tracker: the rules of include/cityflow_amd.h over the running vehicles as the backend lists them
void Detectors::walk(int64_t, bool baseline) {
    const VehicleColumns v = vehicleColumnsOf(*be_, dev_, true, true, true);
    const int nLanes = lanesPerEnv_ * nEnvs_;
    const size_t nDet = host_.dets.size();
    entered_.assign((size_t) nLanes, 0);
    c_.assign(nDet, 0);
    w_.assign(nDet, 0);
    u_.assign(nDet, 0);
    t_.assign(nDet, 0.0);
    const int32_t tick = ++host_.tick;
    for (int i = 0; i < v.count; ++i) {  // (front to back inside a lane: t is added in that order)
        const int32_t l = v.drivable[(size_t) i], id = v.vid[(size_t) i];
        if (l < 0 || l >= nLanes || id < 0) continue;  // (on a laneLink: on no lane)
        if (first_[(size_t) l] == first_[(size_t) l + 1]) continue;  // (a lane without detectors keeps no records)
        int32_t *r = host_.of(id);
        if (r[0] != l || r[1] != tick - 1) entered_[(size_t) l] += 1;
        r[0] = l;
        r[1] = tick;
        r[2] = r[3] = 0;
        const double dis = v.dis[(size_t) i], speed = v.speed[(size_t) i];
        for (int32_t j = first_[(size_t) l]; j < first_[(size_t) l + 1]; ++j) {
            const size_t d = (size_t) order_[(size_t) j];
            const cfx_detector &a = host_.dets[d];
            if (dis < a.start) u_[d] += 1;
            if (!(a.start <= dis && dis < a.end)) continue;
            c_[d] += 1;
            if (speed < 0.1) w_[d] += 1;
            t_[d] += speed;
        }
    }
    for (size_t d = 0; d < nDet; ++d) {
        cfx_detector &a = host_.dets[d];
        if (baseline) {
            a.passed = a.occupied_steps = 0;
            a.vehicle_steps = a.waiting_vehicle_steps = 0;
            a.speed_sum = 0.0;
        } else {
            a.passed += a.upstream - u_[d] + entered_[(size_t) a.lane];
            a.occupied_steps += c_[d] > 0 ? 1 : 0;
            a.vehicle_steps += c_[d];
            a.waiting_vehicle_steps += w_[d];
            a.speed_sum = a.speed_sum + t_[d];
        }
        a.upstream = u_[d];
        a.count = c_[d];
    }
}

void Detectors::features(const cfx_detectors_out &o, bool reset) {
    requireOn("observe_detectors");
    if (onDevice()) {
        if (be_->cfx_get_detectors(dev_, &o, reset ? 1 : 0) != CFX_OK) fail("cfx_get_detectors");
        return;
    }
    for (size_t d = 0; d < host_.dets.size(); ++d) {
        cfx_detector &a = host_.dets[d];
        if (o.passed) o.passed[d] = a.passed;
        if (o.occupied_steps) o.occupied_steps[d] = a.occupied_steps;
        if (o.vehicle_steps) o.vehicle_steps[d] = a.vehicle_steps;
        if (o.waiting_vehicle_steps) o.waiting_vehicle_steps[d] = a.waiting_vehicle_steps;
        if (o.speed_sum) o.speed_sum[d] = a.speed_sum;
        if (o.count) o.count[d] = a.count;
        if (reset) {
            a.passed = a.occupied_steps = 0;
            a.vehicle_steps = a.waiting_vehicle_steps = 0;
            a.speed_sum = 0.0;
        }
    }
}

void Detectors::observeDevice(const cfx_detectors_out &o, bool reset, uintptr_t consumerStream) {
    requireOn("observe_detectors_tensor");
    requireDevice("detectors");
    if (be_->cfx_observe_detectors_device(dev_, &o, reset ? 1 : 0, (void *) consumerStream) != CFX_OK) fail("cfx_observe_detectors_device");
}

DetectorState Detectors::state(int nVehicles) {
    requireOn("detectors");
    if (!onDevice()) {
        DetectorState s = host_;
        s.records.resize((size_t) nVehicles * 4, -1);
        return s;
    }
    DetectorState s;
    s.records.assign((size_t) nVehicles * 4, -1);
    s.dets.assign(lane_.size() * nEnvs_, cfx_detector{});
    if (be_->cfx_detectors_get_state(dev_, s.records.data(), nVehicles, s.dets.data(), (int32_t) s.dets.size(), &s.tick) != CFX_OK)
        fail("cfx_detectors_get_state");
    return s;
}

void Detectors::setState(const DetectorState &s) {
    requireOn("detectors");
    if (!onDevice()) {
        host_ = s;
        return;
    }
    if (be_->cfx_detectors_set_state(dev_, s.records.data(), (int32_t) (s.records.size() / 4), s.dets.data(), (int32_t) s.dets.size(), s.tick) !=
        CFX_OK)
        fail("cfx_detectors_set_state");
}

}  // namespace cfa
