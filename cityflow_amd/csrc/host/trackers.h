// The four trackers as EngineHost and VectorEngineHost own them: one call per point of their common lifecycle, always in
// the order lane flow, movement flow, trips, detectors (DESIGN.md "One scaffold for the trackers").
#pragma once

#include "detectors.h"
#include "lane_flow.h"
#include "movement_flow.h"
#include "trip_stats.h"

namespace cfa {

struct Trackers {
    LaneFlow flow;
    MoveFlow move;
    TripStats trip;
    Detectors det;

    // `net`: ONE environment's network (it outlives this object), of which the backend runs `nEnvs` copies
    void bind(const Backend *be, cfx_engine *dev, const cfx_net *net, int nEnvs, double interval) {
        flow.bind(be, dev, nEnvs * net->n_lanes);
        move.bind(be, dev, net, nEnvs);
        trip.bind(be, dev, nEnvs, interval);
        det.bind(be, dev, net->n_lanes, nEnvs);
    }
    bool onHost() const { return flow.onHost() || move.onHost() || trip.onHost() || det.onHost(); }  // a host tracker has to be ticked
    // the host trackers' tick (a backend that keeps a tracker has ticked it inside cfx_step)
    void afterStep(int64_t step) {
        flow.afterStep(step);
        move.afterStep(step);
        trip.afterStep(step);
        det.afterStep(step);
    }
    // after a reset or a load.  `noteTrips`: the owner notes the vehicles that are alive now (TripStats::note), by their new numbers
    template <typename Note> void rebaseline(int64_t step, Note noteTrips) {
        flow.baseline(step);
        move.baseline(step);
        trip.forget();
        noteTrips();
        trip.baseline(step);
        det.baseline(step);
    }

    // EngineHost::compactVehicles: a load takes a baseline, a compaction must not show — the trackers that are on go round the
    // load as they stand, the vehicle records renumbered (the same vehicles are alive before and after: the trip records as they are)
    struct Carry {
        LaneFlowState flow;
        MoveFlowState move;
        std::vector<cfx_trip_stats_env> trips;
        TripLogState tripLog;  // (rows keep the vehicle numbers they were logged with)
        DetectorState det;
    };
    Carry take(int nVehicles, const std::vector<int32_t> &newOfOld, int nLive);
    void put(const Carry &c);
};

}  // namespace cfa
