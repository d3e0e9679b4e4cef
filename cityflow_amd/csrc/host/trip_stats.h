// Per-environment trip statistics and the average travel time across steps (include/cityflow_amd.h "cfx_trip_stats_enable" has
// the rules), as Engine and VectorEngine hold them (tracker_base.h has the lifecycle).  The host tracker walks
// cfx_get_vehicle_status; the owner tells it every vehicle number's enter time and environment (note) before the tick that
// first sees the number.  Device and host keep a status byte per vehicle number (the status at the previous tick, 0xFF = never
// seen) and a cfx_trip_stats_env per environment.
#pragma once

#include "tracker_base.h"

namespace cfa {

class TripStats : public TrackerBase {
public:
    TripStats() : TrackerBase("trip", "track_trips") {}
    void bind(const Backend *be, cfx_engine *dev, int nEnvs, double interval);
    // on: the device takes its baseline; the owner of a HOST tracker notes the vehicles alive and calls baseline().  off: freed
    void enable(bool on);
    // ---- host tracker (no-ops while the device keeps it)
    int32_t noted() const { return (int32_t) enter_.size(); }
    void note(int32_t vid, double enterTime, int env);
    void forget();                     // the vehicle numbers are about to mean something else (reset, load)
    // (baseline(): on the statuses as they stand, nothing is counted as entered)
    // ----
    void features(const cfx_trip_stats_out &out);  // any pointer may be null; host memory
    void observeDevice(const cfx_trip_stats_out &out, uintptr_t consumerStream);
    std::vector<cfx_trip_stats_env> state();       // ... around a renumbering load (the records only)
    void setState(const std::vector<cfx_trip_stats_env> &s);

private:
    void walk(int64_t step, bool baseline) override;
    int nEnvs_ = 1;
    double interval_ = 1.0;
    // the host tracker
    std::vector<cfx_trip_stats_env> rec_;
    std::vector<uint8_t> seen_, status_;
    std::vector<int32_t> enter_, env_;  // e(v), r(v)
    int64_t step_ = 0;                  // the step counter of the last tick
};

}  // namespace cfa
