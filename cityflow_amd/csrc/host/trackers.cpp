// What the trackers share on the host (tracker_base.h) and the owners' aggregate of the four (trackers.h).
#include "trackers.h"

#include <stdexcept>
#include <string>

#include "engine_host.h"

namespace cfa {

bool TrackerBase::switchTo(bool on) {
    if (on == on_) return false;
    if (onDevice_ && enable_(dev_, on ? 1 : 0) != CFX_OK) fail(enableName_);
    on_ = on;
    return !onDevice_;
}

void TrackerBase::requireOn(const char *what) const {
    if (!on_) throw std::runtime_error(std::string(what) + ": " + name_ + " tracking is off (" + pyCall_ + "(True) turns it on)");
}

void TrackerBase::requireDevice(const char *noun) const {
    if (!onDevice_) throw std::runtime_error("cityflow_amd: '" + be_->path + "' has no device-side " + noun);
}

void TrackerBase::fail(const char *what) const {
    const char *msg = be_->cfx_last_error(dev_);
    throw std::runtime_error(std::string("cityflow_amd: ") + what + " failed: " + (msg ? msg : ""));
}

void VehicleRecords::renumber(const std::vector<int32_t> &newOfOld, int nLive) {
    std::vector<int32_t> moved((size_t) nLive * 4, -1);
    for (size_t v = 0; v < newOfOld.size() && 4 * v + 3 < records.size(); ++v)
        if (newOfOld[v] >= 0 && newOfOld[v] < nLive) std::copy(records.begin() + 4 * v, records.begin() + 4 * v + 4, moved.begin() + 4 * (size_t) newOfOld[v]);
    records.swap(moved);
}

Trackers::Carry Trackers::take(int nVehicles, const std::vector<int32_t> &newOfOld, int nLive) {
    Carry c;
    if (flow.on()) {
        c.flow = flow.state(nVehicles);
        c.flow.renumber(newOfOld, nLive);
    }
    if (move.on()) {
        c.move = move.state(nVehicles);
        c.move.renumber(newOfOld, nLive);
    }
    if (trip.on()) {
        c.trips = trip.state();
        c.tripLog = trip.logState();
    }
    if (det.on()) {
        c.det = det.state(nVehicles);
        c.det.renumber(newOfOld, nLive);
    }
    return c;
}

void Trackers::put(const Carry &c) {
    if (flow.on()) flow.setState(c.flow);
    if (move.on()) move.setState(c.move);
    if (trip.on()) {
        trip.setState(c.trips);
        trip.setLogState(c.tripLog);
    }
    if (det.on()) det.setState(c.det);
}

}  // namespace cfa
