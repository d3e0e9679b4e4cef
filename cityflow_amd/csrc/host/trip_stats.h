// Per-environment trip statistics and the average travel time across steps (include/cityflow_amd.h "cfx_trip_stats_enable" has
// the rules), as Engine and VectorEngine hold them.  On a backend that exports the five optional entry points the device keeps
// the tracker and this is a thin dispatcher.  A backend without them (the CPU twin) gets the HOST tracker below: the same rules
// in C++ over cfx_get_vehicle_status, ticked by the owner after every step.  The owner tells it every vehicle number's enter
// time and environment (note) before the tick that first sees the number.  Both keep a status byte per vehicle number (the
// status at the previous tick, 0xFF = never seen) and a cfx_trip_stats_env per environment.
#pragma once

#include <cstdint>
#include <vector>

#include "cityflow_amd.h"

namespace cfa {

struct Backend;

class TripStats {
public:
    void bind(const Backend *be, cfx_engine *dev, int nEnvs, double interval) {
        be_ = be;
        dev_ = dev;
        nEnvs_ = nEnvs;
        interval_ = interval;
    }
    bool on() const { return on_; }
    bool onDevice() const;             // the backend keeps the tracker (all five entry points)
    // on: the device takes its baseline; the owner of a HOST tracker notes the vehicles alive and calls baseline().  off: freed
    void enable(bool on);
    // ---- host tracker (no-ops while the device keeps it)
    int32_t noted() const { return (int32_t) enter_.size(); }
    void note(int32_t vid, double enterTime, int env);
    void forget();                     // the vehicle numbers are about to mean something else (reset, load)
    void baseline(int64_t step);       // on the statuses as they stand: nothing is counted as entered
    void afterStep(int64_t step);      // the tick
    // ----
    void features(const cfx_trip_stats_out &out);  // any pointer may be null; host memory
    void observeDevice(const cfx_trip_stats_out &out, uintptr_t consumerStream);
    std::vector<cfx_trip_stats_env> state();       // ... around a renumbering load (the records only)
    void setState(const std::vector<cfx_trip_stats_env> &s);

private:
    void requireOn(const char *what) const;
    void fail(const char *what) const;
    void walk(int64_t step, bool baseline);
    const Backend *be_ = nullptr;
    cfx_engine *dev_ = nullptr;
    int nEnvs_ = 1;
    double interval_ = 1.0;
    bool on_ = false;
    // the host tracker
    std::vector<cfx_trip_stats_env> rec_;
    std::vector<uint8_t> seen_, status_;
    std::vector<int32_t> enter_, env_;  // e(v), r(v)
    int64_t step_ = 0;                  // the step counter of the last tick
};

}  // namespace cfa
