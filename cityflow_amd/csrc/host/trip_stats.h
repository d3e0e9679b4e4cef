// Per-environment trip statistics and the average travel time across steps (include/cityflow_amd.h "cfx_trip_stats_enable" has
// the rules), as Engine and VectorEngine hold them (tracker_base.h has the lifecycle).  The host tracker walks
// cfx_get_vehicle_status; the owner tells it every vehicle number's enter time and environment (note) before the tick that
// first sees the number.  Device and host keep a status byte per vehicle number (the status at the previous tick, 0xFF = never
// seen) and a cfx_trip_stats_env per environment.
// The trip LOG (one row per finished vehicle; "cfx_trip_log_enable" in the header has the rules) belongs to this tracker: the
// backend keeps it where it exports the log's four entry points, the host tracker's walk otherwise.
#pragma once

#include "tracker_base.h"

namespace cfa {

// The trip log as it goes round a renumbering load (Trackers::Carry) and as the host tracker keeps it: rows in log order
struct TripLogState {
    std::vector<int32_t> env, vehicle, originRoad, destinationRoad, enterStep, finishStep, travelSteps;
    int32_t dropped = 0;
    size_t rows() const { return env.size(); }
    void clear() { *this = TripLogState{}; }
};

class TripStats : public TrackerBase {
public:
    TripStats() : TrackerBase("trip", "track_trips") {}
    void bind(const Backend *be, cfx_engine *dev, int nEnvs, double interval);
    // on: the device takes its baseline; the owner of a HOST tracker notes the vehicles alive and calls baseline().  off: freed
    void enable(bool on);
    // ---- host tracker (no-ops while the device keeps it)
    int32_t noted() const { return (int32_t) enter_.size(); }
    // `originRoad`, `destinationRoad`: the first and the last road of the route the vehicle holds, of ONE environment's roads
    // (noted again when the route changes: EngineHost::setRoute)
    void note(int32_t vid, double enterTime, int env, int32_t originRoad, int32_t destinationRoad);
    void forget();                     // the vehicle numbers are about to mean something else (reset, load)
    // (baseline(): on the statuses as they stand, nothing is counted as entered)
    // ----
    void features(const cfx_trip_stats_out &out);  // any pointer may be null; host memory
    void observeDevice(const cfx_trip_stats_out &out, uintptr_t consumerStream);
    std::vector<cfx_trip_stats_env> state();       // ... around a renumbering load (the records only)
    void setState(const std::vector<cfx_trip_stats_env> &s);
    // ---- the trip log (tracking must be on).  capacity > 0: an empty log of that many rows, replacing the one there; 0: none.
    // std::invalid_argument outside [0, CFX_TRIP_LOG_MAX_CAPACITY]
    void enableLog(int64_t capacity);
    int32_t logCapacity() const { return logCap_; }  // 0: no log
    bool logOnDevice() const { return logOnDevice_; }
    void logFeatures(const cfx_trip_log_out &out, bool reset);  // any pointer may be null; host memory, columns [capacity]
    void observeLogDevice(const cfx_trip_log_out &out, bool reset, uintptr_t consumerStream);
    TripLogState logState();                       // ... around a renumbering load (no log: empty)
    void setLogState(const TripLogState &s);

private:
    void walk(int64_t step, bool baseline) override;
    int nEnvs_ = 1;
    double interval_ = 1.0;
    // the host tracker
    std::vector<cfx_trip_stats_env> rec_;
    std::vector<uint8_t> seen_, status_;
    std::vector<int32_t> enter_, env_;  // e(v), r(v)
    int64_t step_ = 0;                  // the step counter of the last tick
    // the log: on the device where the backend has its entry points, otherwise rows appended by walk()
    void requireLog(const char *what) const;
    bool logOnDevice_ = false;
    int32_t logCap_ = 0;
    TripLogState log_;
    std::vector<int32_t> origin_, destination_;  // per vehicle number, as noted
};

}  // namespace cfa
