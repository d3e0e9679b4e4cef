// Trip-statistics tracker: dispatcher over the backend's entry points and the host tracker (trip_stats.h).
#include "trip_stats.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "engine_host.h"

namespace cfa {

void TripStats::bind(const Backend *be, cfx_engine *dev, int nEnvs, double interval) {
    bindBackend(be, dev, "cfx_trip_stats_enable", be->cfx_trip_stats_enable, be->cfx_observe_trip_stats_device, be->cfx_get_trip_stats,
                be->cfx_trip_stats_get_state, be->cfx_trip_stats_set_state);
    nEnvs_ = nEnvs;
    interval_ = interval;
    logOnDevice_ = onDevice() && be->cfx_trip_log_enable && be->cfx_observe_trip_log_device && be->cfx_get_trip_log && be->cfx_trip_log_set_state;
}

void TripStats::enable(bool on) {
    if (on == on_) return;
    const bool host = switchTo(on);
    logCap_ = 0;  // (the log goes with the tracker: the backend frees its own)
    log_.clear();
    if (!host) return;
    std::vector<cfx_trip_stats_env>().swap(rec_);
    std::vector<uint8_t>().swap(seen_);
    std::vector<uint8_t>().swap(status_);
    forget();
    if (on) rec_.assign((size_t) nEnvs_, cfx_trip_stats_env{});
}

void TripStats::note(int32_t vid, double enterTime, int env, int32_t originRoad, int32_t destinationRoad) {
    if (!on_ || onDevice() || vid < 0) return;
    if ((size_t) vid >= enter_.size()) {
        enter_.resize((size_t) vid + 1, 0);
        env_.resize((size_t) vid + 1, 0);
        origin_.resize((size_t) vid + 1, -1);
        destination_.resize((size_t) vid + 1, -1);
    }
    origin_[(size_t) vid] = originRoad;
    destination_[(size_t) vid] = destinationRoad;
    enter_[(size_t) vid] = (int32_t) std::llrint(enterTime / interval_);
    env_[(size_t) vid] = std::min(std::max(env, 0), nEnvs_ - 1);
}

void TripStats::forget() {
    std::vector<int32_t>().swap(enter_);
    std::vector<int32_t>().swap(env_);
    std::vector<int32_t>().swap(origin_);
    std::vector<int32_t>().swap(destination_);
}

// one tick (or baseline) of the host tracker: the rules of include/cityflow_amd.h over the status of every vehicle number noted
void TripStats::walk(int64_t step, bool baseline) {
    const size_t n = enter_.size();
    status_.resize(n);
    if (n && be_->cfx_get_vehicle_status(dev_, 0, (int32_t) n, status_.data()) != CFX_OK) fail("cfx_get_vehicle_status");
    step_ = step;
    if (baseline) {
        rec_.assign((size_t) nEnvs_, cfx_trip_stats_env{});
        seen_.assign(n, 0xFF);
        log_.clear();  // (a baseline empties the log, and logs nothing itself)
    } else {
        seen_.resize(n, 0xFF);
    }
    for (size_t v = 0; v < n; ++v) {
        const uint8_t prev = seen_[v], cur = status_[v];
        if (prev == cur) continue;
        seen_[v] = cur;
        cfx_trip_stats_env &a = rec_[(size_t) env_[v]];
        const int64_t e = enter_[v];
        if (baseline) {
            if (cur != 2) {
                a.base_in_system += 1;
                a.enter_sum_created += e;
                if (cur == 0) a.base_buffered += 1;
            }
            continue;
        }
        if (prev == 0xFF) {
            a.entered += 1;
            a.enter_sum_created += e;
        }
        if (cur == 1 && prev != 1) {
            a.admitted += 1;
            a.admitted_buffer_steps += (step - 1) - e;
        }
        if (cur == 2 && prev != 2) {
            a.finished += 1;
            a.finished_travel_steps += (step - 1) - e;
            a.enter_sum_finished += e;
            if (logCap_ > 0) {  // the log's row of this finish (restated here: no code shared with the HIP library)
                if (log_.rows() < (size_t) logCap_) {
                    log_.env.push_back(env_[v]);
                    log_.vehicle.push_back((int32_t) v);
                    log_.originRoad.push_back(origin_[v]);
                    log_.destinationRoad.push_back(destination_[v]);
                    log_.enterStep.push_back((int32_t) e);
                    log_.finishStep.push_back((int32_t) step);
                    log_.travelSteps.push_back((int32_t) ((step - 1) - e));
                } else {
                    log_.dropped += 1;
                }
            }
        }
    }
}

void TripStats::features(const cfx_trip_stats_out &o) {
    requireOn("observe_trips");
    if (onDevice()) {
        if (be_->cfx_get_trip_stats(dev_, &o) != CFX_OK) fail("cfx_get_trip_stats");
        return;
    }
    for (size_t r = 0; r < rec_.size(); ++r) {  // (the present values follow from the record: k_trip_drain of the HIP library)
        const cfx_trip_stats_env &a = rec_[r];
        const int32_t inSystem = a.base_in_system + a.entered - a.finished;
        const int64_t inSteps = (int64_t) inSystem * step_ - (a.enter_sum_created - a.enter_sum_finished);
        const int64_t n = (int64_t) a.finished + inSystem;
        if (o.entered) o.entered[r] = a.entered;
        if (o.admitted) o.admitted[r] = a.admitted;
        if (o.admitted_buffer_steps) o.admitted_buffer_steps[r] = a.admitted_buffer_steps;
        if (o.finished) o.finished[r] = a.finished;
        if (o.finished_travel_steps) o.finished_travel_steps[r] = a.finished_travel_steps;
        if (o.in_system) o.in_system[r] = inSystem;
        if (o.buffered) o.buffered[r] = a.base_buffered + a.entered - a.admitted;
        if (o.in_system_travel_steps) o.in_system_travel_steps[r] = inSteps;
        if (o.average_travel_time)
            o.average_travel_time[r] = n == 0 ? 0.0 : (double) (a.finished_travel_steps + inSteps) * interval_ / (double) n;
    }
}

void TripStats::observeDevice(const cfx_trip_stats_out &o, uintptr_t consumerStream) {
    requireOn("observe_trips_tensor");
    requireDevice("trip statistics");
    if (be_->cfx_observe_trip_stats_device(dev_, &o, (void *) consumerStream) != CFX_OK) fail("cfx_observe_trip_stats_device");
}

std::vector<cfx_trip_stats_env> TripStats::state() {
    requireOn("trip statistics");
    if (!onDevice()) return rec_;
    std::vector<cfx_trip_stats_env> s((size_t) nEnvs_);
    if (be_->cfx_trip_stats_get_state(dev_, s.data(), nEnvs_) != CFX_OK) fail("cfx_trip_stats_get_state");
    return s;
}

void TripStats::setState(const std::vector<cfx_trip_stats_env> &s) {
    requireOn("trip statistics");
    if (!onDevice()) {
        rec_ = s;
        return;
    }
    if (be_->cfx_trip_stats_set_state(dev_, s.data(), (int32_t) s.size()) != CFX_OK) fail("cfx_trip_stats_set_state");
}

// ---- the trip log
void TripStats::enableLog(int64_t capacity) {
    requireOn("track_trips(log=)");
    if (capacity < 0 || capacity > CFX_TRIP_LOG_MAX_CAPACITY)
        throw std::invalid_argument("track_trips: log capacity " + std::to_string(capacity) + " is outside [0, " +
                                    std::to_string(CFX_TRIP_LOG_MAX_CAPACITY) + "]");
    if (onDevice()) {
        // (such a backend ticks by itself, so the host cannot keep the log for it)
        if (!logOnDevice_) throw std::runtime_error("cityflow_amd: '" + be_->path + "' has no device-side trip log");
        if (be_->cfx_trip_log_enable(dev_, (int32_t) capacity) != CFX_OK) fail("cfx_trip_log_enable");
    }
    log_.clear();
    logCap_ = (int32_t) capacity;
}

void TripStats::requireLog(const char *what) const {
    requireOn(what);
    if (logCap_ <= 0) throw std::runtime_error(std::string(what) + ": there is no trip log (track_trips(True, log=N) turns it on)");
}

void TripStats::logFeatures(const cfx_trip_log_out &o, bool reset) {
    requireLog("observe_trip_log");
    if (logOnDevice_) {
        if (be_->cfx_get_trip_log(dev_, &o, reset ? 1 : 0) != CFX_OK) fail("cfx_get_trip_log");
        return;
    }
    const size_t n = log_.rows();
    auto column = [&](int32_t *out, const std::vector<int32_t> &rows) {  // (k_trip_log_drain of the HIP library: -1 behind the count)
        if (!out) return;
        std::copy(rows.begin(), rows.end(), out);
        std::fill(out + n, out + logCap_, -1);
    };
    if (o.count) *o.count = (int32_t) n;
    if (o.dropped) *o.dropped = log_.dropped;
    column(o.env, log_.env);
    column(o.vehicle, log_.vehicle);
    column(o.origin_road, log_.originRoad);
    column(o.destination_road, log_.destinationRoad);
    column(o.enter_step, log_.enterStep);
    column(o.finish_step, log_.finishStep);
    column(o.travel_steps, log_.travelSteps);
    if (reset) log_.clear();
}

void TripStats::observeLogDevice(const cfx_trip_log_out &o, bool reset, uintptr_t consumerStream) {
    requireLog("observe_trip_log_tensor");
    if (!logOnDevice_) throw std::runtime_error("cityflow_amd: '" + be_->path + "' has no device-side trip log");
    if (be_->cfx_observe_trip_log_device(dev_, &o, reset ? 1 : 0, (void *) consumerStream) != CFX_OK) fail("cfx_observe_trip_log_device");
}

TripLogState TripStats::logState() {
    if (logCap_ <= 0) return TripLogState{};
    if (!logOnDevice_) return log_;
    const size_t cap = (size_t) logCap_;
    TripLogState s;
    int32_t count = 0;
    for (std::vector<int32_t> *c : {&s.env, &s.vehicle, &s.originRoad, &s.destinationRoad, &s.enterStep, &s.finishStep, &s.travelSteps}) c->resize(cap);
    cfx_trip_log_out o{&count, &s.dropped, s.env.data(), s.vehicle.data(), s.originRoad.data(), s.destinationRoad.data(), s.enterStep.data(),
                       s.finishStep.data(), s.travelSteps.data()};
    if (be_->cfx_get_trip_log(dev_, &o, 0) != CFX_OK) fail("cfx_get_trip_log");
    for (std::vector<int32_t> *c : {&s.env, &s.vehicle, &s.originRoad, &s.destinationRoad, &s.enterStep, &s.finishStep, &s.travelSteps})
        c->resize((size_t) std::max(count, 0));
    return s;
}

void TripStats::setLogState(const TripLogState &s) {
    if (logCap_ <= 0) return;
    if (!logOnDevice_) {
        log_ = s;
        return;
    }
    cfx_trip_log_out o{nullptr, nullptr, const_cast<int32_t *>(s.env.data()), const_cast<int32_t *>(s.vehicle.data()),
                       const_cast<int32_t *>(s.originRoad.data()), const_cast<int32_t *>(s.destinationRoad.data()),
                       const_cast<int32_t *>(s.enterStep.data()), const_cast<int32_t *>(s.finishStep.data()),
                       const_cast<int32_t *>(s.travelSteps.data())};
    if (be_->cfx_trip_log_set_state(dev_, &o, (int32_t) s.rows(), s.dropped) != CFX_OK) fail("cfx_trip_log_set_state");
}

}  // namespace cfa
