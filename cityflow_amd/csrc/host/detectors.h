// Virtual loop detectors: passage counts, occupancy and speed over zones of lanes across steps (include/cityflow_amd.h
// "cfx_detectors_define" has the rules), as Engine and VectorEngine hold them (tracker_base.h has the lifecycle).  The host tracker
// walks cfx_get_vehicles (vid, drivable, distance, speed, front to back inside a lane).  Device and host keep the tracker in the
// same form: a vehicle record per number, of which the first two fields are used, and a cfx_detector per detector.
#pragma once

#include "tracker_base.h"

namespace cfa {

struct DetectorState : VehicleRecords {
    std::vector<cfx_detector> dets;  // every environment's (a renumbering leaves them as they are)
};

class Detectors : public TrackerBase {
public:
    Detectors() : TrackerBase("detector", "track_detectors") {}
    // `lanesPerEnv`: the lanes of ONE environment, of which the backend runs `nEnvs` copies
    void bind(const Backend *be, cfx_engine *dev, int lanesPerEnv, int nEnvs);
    // The set of detectors of one environment, for every environment; turns the tracker on if it is off, and takes a baseline at
    // `step` either way.  Every entry is checked before anything changes (std::invalid_argument naming the position)
    void define(const int32_t *lane, const double *start, const double *end, int n, int64_t step);
    void disable();                           // everything is freed, the set forgotten
    int count() const { return (int) lane_.size(); }  // detectors of one environment
    const std::vector<int32_t> &lanes() const { return lane_; }
    const std::vector<double> &starts() const { return start_; }
    const std::vector<double> &ends() const { return end_; }
    void features(const cfx_detectors_out &out, bool reset);  // [nEnvs * count()] each; any may be null
    void observeDevice(const cfx_detectors_out &out, bool reset, uintptr_t consumerStream);
    DetectorState state(int nVehicles);       // ... around a renumbering load
    void setState(const DetectorState &s);

private:
    void walk(int64_t step, bool baseline) override;
    void hostTables();                        // host_.dets and the per-lane index from the set
    int lanesPerEnv_ = 0, nEnvs_ = 1;
    std::vector<int32_t> lane_;               // the set as it was defined
    std::vector<double> start_, end_;
    DetectorState host_;                      // the host tracker
    std::vector<int32_t> first_, order_;      // ... order_[first_[l] .. first_[l + 1]): the detectors of lane l
    std::vector<int32_t> entered_, c_, w_, u_;  // scratch of a tick: per lane, then per detector
    std::vector<double> t_;
};

}  // namespace cfa
