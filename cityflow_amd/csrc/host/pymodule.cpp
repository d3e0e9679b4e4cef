// pybind11 binding of the drop-in `cityflow` module.  Same class name, method names, argument names and
// defaults as the reference binding (reference src/cityflow.cpp:10-47); extra members are prefixed or
// clearly array-flavoured and never change the behaviour of the reference-named ones.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <chrono>
#include <iostream>
#include <optional>

#include "archive.h"
#include "engine_host.h"
#include "tile_engine.h"
#include "vector_engine.h"
#include "json.h"

namespace py = pybind11;
using namespace py::literals;
using cfa::EngineHost;

namespace {

template <typename T> py::array_t<T> toArray(const std::vector<T> &v) {
    py::array_t<T> a((py::ssize_t) v.size());
    if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
    return a;
}
template <typename T> py::array_t<T> toArray(const T *p, size_t n) {
    py::array_t<T> a((py::ssize_t) n);
    if (n) std::memcpy(a.mutable_data(), p, n * sizeof(T));
    return a;
}

py::dict flatNetToDict(const cfa::HostRoadNet &net) {
    const cfx_net &f = net.flat();
    const int D = f.n_lanes + f.n_lanelinks;
    py::dict d;
    d["n_roads"] = f.n_roads;
    d["n_lanes"] = f.n_lanes;
    d["n_lanelinks"] = f.n_lanelinks;
    d["n_inters"] = f.n_inters;
    d["n_xentries"] = f.n_xentries;
    d["drv_length"] = toArray(f.drv_length, D);
    d["drv_max_speed"] = toArray(f.drv_max_speed, D);
    d["lane_road"] = toArray(f.lane_road, f.n_lanes);
    d["lane_index"] = toArray(f.lane_index, f.n_lanes);
    d["lane_ll_start"] = toArray(f.lane_ll_start, f.n_lanes + 1);
    d["lane_ll"] = toArray(f.lane_ll, f.n_lanelinks);
    d["road_lane_start"] = toArray(f.road_lane_start, f.n_roads + 1);
    d["ll_start_lane"] = toArray(f.ll_start_lane, f.n_lanelinks);
    d["ll_end_lane"] = toArray(f.ll_end_lane, f.n_lanelinks);
    d["ll_inter"] = toArray(f.ll_inter, f.n_lanelinks);
    d["ll_roadlink"] = toArray(f.ll_roadlink, f.n_lanelinks);
    d["ll_type"] = toArray(f.ll_type, f.n_lanelinks);
    d["ll_x_start"] = toArray(f.ll_x_start, f.n_lanelinks + 1);
    d["x_dist"] = toArray(f.x_dist, f.n_xentries);
    d["x_peer"] = toArray(f.x_peer, f.n_xentries);
    d["x_ll"] = toArray(f.x_ll, f.n_xentries);
    d["inter_virtual"] = toArray(f.inter_virtual, f.n_inters);
    d["inter_n_roadlinks"] = toArray(f.inter_n_roadlinks, f.n_inters);
    d["inter_phase_start"] = toArray(f.inter_phase_start, f.n_inters + 1);
    d["inter_avail_start"] = toArray(f.inter_avail_start, f.n_inters);
    d["phase_time"] = toArray(f.phase_time, f.n_phases);
    d["phase_avail"] = toArray(f.phase_avail, f.n_avail);
    std::vector<std::string> laneIds(f.n_lanes), llIds(f.n_lanelinks), interIds(f.n_inters), roadIds(f.n_roads);
    for (int l = 0; l < f.n_lanes; ++l) laneIds[l] = net.laneId(l);
    for (int k = 0; k < f.n_lanelinks; ++k) llIds[k] = net.laneLinkId(k);
    for (int i = 0; i < f.n_inters; ++i) interIds[i] = net.inters[i].id;
    for (int r = 0; r < f.n_roads; ++r) roadIds[r] = net.roads[r].id;
    d["lane_ids"] = laneIds;
    d["lanelink_ids"] = llIds;
    d["inter_ids"] = interIds;
    d["road_ids"] = roadIds;
    return d;
}

// Reference getLaneVehicleCount returns std::map<std::string,int> (engine.cpp:628-648) which pybind11 turns into a dict
// by creating one Python string per lane and inserting every entry per call.  Here the key objects are created once per
// engine, a master dict per getter is kept up to date by rewriting only the entries whose value changed since the
// previous call (a step changes a small fraction of the lanes), and the caller gets a C-level copy of it: a fresh dict
// in std::map (lexicographic) key order every call, like the reference's.
struct LaneDictCache {
    py::list keys;
    py::object interIdx;  // {intersection id: index in net().inters}, for set_tl_phase (built at its first call)
    py::dict master[2];
    std::vector<int32_t> last[2];
    bool filled[2] = {false, false};
    // vehicle id strings, created once per vehicle (valid for one vehicleEpoch of the engine)
    std::vector<PyObject *> vidStr;
    std::vector<uint64_t> vidSortKey;  // Spawner::idSortKey, computed once per vehicle (never 0)
    uint64_t vidEpoch = 0;
    ~LaneDictCache() { clearVehicles(); }
    void clearVehicles() {
        for (PyObject *o : vidStr) Py_XDECREF(o);
        vidStr.clear();
        vidSortKey.clear();
    }
};

LaneDictCache &bindingCacheOf(EngineHost &e) {
    if (!e.bindingCache) {
        auto *c = new LaneDictCache();
        for (int32_t l : e.laneIdOrder()) c->keys.append(py::str(e.net().laneId(l)));
        e.bindingCache = std::shared_ptr<void>(c, [](void *p) { delete static_cast<LaneDictCache *>(p); });
    }
    return *static_cast<LaneDictCache *>(e.bindingCache.get());
}

// borrowed reference to the (cached) Python string of a vehicle's id
PyObject *vehicleKey(EngineHost &e, LaneDictCache &c, int vid) {
    if (c.vidEpoch != e.vehicleEpoch()) {
        c.clearVehicles();
        c.vidEpoch = e.vehicleEpoch();
    }
    if ((size_t) vid >= c.vidStr.size()) c.vidStr.resize((size_t) vid + 1 + c.vidStr.size() / 2, nullptr);
    PyObject *&o = c.vidStr[vid];
    if (!o) {
        const std::string id = e.vehicleId(vid);
        o = PyUnicode_FromStringAndSize(id.data(), (Py_ssize_t) id.size());
        if (!o) throw py::error_already_set();
    }
    return o;
}

uint64_t vehicleSortKey(EngineHost &e, LaneDictCache &c, int vid) {
    if (c.vidEpoch != e.vehicleEpoch()) {
        c.clearVehicles();
        c.vidEpoch = e.vehicleEpoch();
    }
    if ((size_t) vid >= c.vidSortKey.size()) c.vidSortKey.resize((size_t) vid + 1 + c.vidSortKey.size() / 2, 0);
    uint64_t &k = c.vidSortKey[vid];
    if (!k) k = e.spawner().idSortKey(vid);
    return k;
}

// get_vehicle_speed / get_vehicle_distance (engine.cpp:650-676): {vehicle id: value} in std::map (string) key order
py::dict vehicleValueDict(EngineHost &e, bool speed) {
    cfa::VehicleSnapshot s;
    e.snapshotVehicles(s, speed ? cfa::kSnapSpeed : cfa::kSnapDis);
    const std::vector<double> &val = speed ? s.speed : s.dis;
    LaneDictCache &c = bindingCacheOf(e);
    std::vector<std::pair<uint64_t, int>> order((size_t) s.count);
    for (int i = 0; i < s.count; ++i) order[i] = std::make_pair(vehicleSortKey(e, c, s.vid[i]), i);
    std::sort(order.begin(), order.end());
    py::dict d;
    for (auto &p : order) {
        PyObject *num = PyFloat_FromDouble(val[p.second]);
        if (!num || PyDict_SetItem(d.ptr(), vehicleKey(e, c, s.vid[p.second]), num) != 0) {
            Py_XDECREF(num);
            throw py::error_already_set();
        }
        Py_DECREF(num);
    }
    return d;
}

// get_vehicles (engine.cpp:619-626): ids in vehiclePool (= priority) order
py::list vehicleList(EngineHost &e, bool includeWaiting) {
    cfa::VehicleSnapshot s;
    e.snapshotVehicles(s, 0);
    std::vector<std::pair<int32_t, int32_t>> byPriority;
    byPriority.reserve((size_t) s.count);
    for (int i = 0; i < s.count; ++i) byPriority.emplace_back(e.spawner().vehicles[s.vid[i]].priority, s.vid[i]);
    if (includeWaiting) {
        std::vector<int32_t> wv, wl;
        e.waitingVehicles(wv, wl);
        for (int32_t v : wv) byPriority.emplace_back(e.spawner().vehicles[v].priority, v);
    }
    std::sort(byPriority.begin(), byPriority.end());
    LaneDictCache &c = bindingCacheOf(e);
    py::list out(byPriority.size());
    for (size_t i = 0; i < byPriority.size(); ++i) {
        PyObject *key = vehicleKey(e, c, byPriority[i].second);
        Py_INCREF(key);
        PyList_SET_ITEM(out.ptr(), (Py_ssize_t) i, key);
    }
    return out;
}

// get_lane_vehicles (engine.cpp:658-668): {lane id: [vehicle ids front to back]} for every lane, std::map key order
py::dict laneVehiclesDict(EngineHost &e) {
    cfa::VehicleSnapshot s;
    e.snapshotVehicles(s, cfa::kSnapDrivable);
    const std::vector<int32_t> &order = e.laneIdOrder();
    const int L = (int) order.size();
    std::vector<int32_t> start((size_t) L + 1, 0);
    for (int i = 0; i < s.count; ++i)
        if (s.drivable[i] < L) start[s.drivable[i] + 1]++;
    for (int l = 0; l < L; ++l) start[l + 1] += start[l];
    // the snapshot is ordered by drivable, front to back: the vehicles of lane l are a contiguous run
    std::vector<int32_t> first((size_t) L, -1);
    for (int i = s.count - 1; i >= 0; --i)
        if (s.drivable[i] < L) first[s.drivable[i]] = i;
    LaneDictCache &c = bindingCacheOf(e);
    py::dict d;
    for (int k = 0; k < L; ++k) {
        const int l = order[k];
        const int n = start[l + 1] - start[l];
        PyObject *lst = PyList_New(n);
        if (!lst) throw py::error_already_set();
        for (int j = 0; j < n; ++j) {
            PyObject *key = vehicleKey(e, c, s.vid[first[l] + j]);
            Py_INCREF(key);
            PyList_SET_ITEM(lst, j, key);
        }
        if (PyDict_SetItem(d.ptr(), PyList_GET_ITEM(c.keys.ptr(), (Py_ssize_t) k), lst) != 0) {
            Py_DECREF(lst);
            throw py::error_already_set();
        }
        Py_DECREF(lst);
    }
    return d;
}

py::dict laneDict(EngineHost &e, const std::vector<int32_t> &values, int which) {
    const std::vector<int32_t> &order = e.laneIdOrder();
    LaneDictCache &c = bindingCacheOf(e);
    std::vector<int32_t> &last = c.last[which];
    if (!c.filled[which]) last.assign(order.size(), INT32_MIN);
    PyObject *master = c.master[which].ptr();
    for (size_t i = 0; i < order.size(); ++i) {
        const int32_t v = values[order[i]];
        if (v == last[i]) continue;
        last[i] = v;
        PyObject *num = PyLong_FromLong(v);
        if (!num || PyDict_SetItem(master, PyList_GET_ITEM(c.keys.ptr(), (Py_ssize_t) i), num) != 0) {
            Py_XDECREF(num);
            throw py::error_already_set();
        }
        Py_DECREF(num);
    }
    c.filled[which] = true;
    PyObject *copy = PyDict_Copy(master);
    if (!copy) throw py::error_already_set();
    return py::reinterpret_steal<py::dict>(copy);
}

// ---- per-lane speed and position features as numpy arrays (Engine and VectorEngine; the tensors are cityflow_amd/torch_io.py)
using EdgesArray = py::array_t<double, py::array::c_style | py::array::forcecast>;

// edges: [nLanes, B + 1] (a row per lane) or [B + 1] (one row for every lane), 1 <= B <= CFX_MAX_LANE_BINS; returns B
int checkBinEdges(const EdgesArray &edges, size_t nLanes, bool &perLane) {
    if (edges.ndim() != 1 && edges.ndim() != 2)
        throw py::value_error("edges must have shape [B+1] or [" + std::to_string(nLanes) + ", B+1]");
    perLane = edges.ndim() == 2;
    if (perLane && (size_t) edges.shape(0) != nLanes)
        throw py::value_error("per-lane edges must have " + std::to_string(nLanes) + " rows, not " + std::to_string(edges.shape(0)));
    const py::ssize_t nBins = edges.shape(edges.ndim() - 1) - 1;
    if (nBins < 1 || nBins > CFX_MAX_LANE_BINS)
        throw py::value_error("edges must give 1 to " + std::to_string(CFX_MAX_LANE_BINS) + " bins (B+1 edges), not " +
                              std::to_string(nBins));
    return (int) nBins;
}

// `lead`: the leading dimensions of an observation ([L] or [R, L])
template <typename E> py::array_t<double> laneSpeedSumArray(E &e, std::vector<py::ssize_t> lead) {
    py::array_t<double> out(lead);
    e.laneFeatures(out.mutable_data(), nullptr, nullptr, 0, false);
    return out;
}

template <typename E> py::array_t<int32_t> laneBinsArray(E &e, const EdgesArray &edges, std::vector<py::ssize_t> lead) {
    bool perLane = false;
    const int nBins = checkBinEdges(edges, (size_t) lead.back(), perLane);
    lead.push_back(nBins);
    py::array_t<int32_t> out(lead);
    e.laneFeatures(nullptr, out.mutable_data(), edges.data(), nBins, perLane);
    return out;
}

// ---- per-intersection observations (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
template <typename E> py::tuple intersectionFeaturesTuple(E &e, py::ssize_t nEnvs) {
    const cfa::InterLayout &y = e.intersectionLayout();
    const py::ssize_t rows = nEnvs * y.I;
    py::array_t<int32_t> phase(rows), in(rows * y.M), wait(rows * y.M), out(rows * y.M), inside(rows * y.M), pressure(rows * y.P);
    py::array_t<double> remain(rows);
    cfa::InterFeatures f;
    f.phase = phase.mutable_data();
    f.remain = remain.mutable_data();
    f.in = in.mutable_data();
    f.inWaiting = wait.mutable_data();
    f.out = out.mutable_data();
    f.inside = inside.mutable_data();
    f.pressure = pressure.mutable_data();
    e.intersectionFeatures(f);
    return py::make_tuple(phase, remain, in, wait, out, inside, pressure);
}

template <typename E> py::dict intersectionLayoutDict(E &e) {
    const cfa::InterLayout &y = e.intersectionLayout();
    auto shaped = [](const auto &v, std::vector<py::ssize_t> shape) {
        using T = typename std::decay<decltype(v)>::type::value_type;
        py::array_t<T> a(shape);
        std::copy(v.begin(), v.end(), a.mutable_data());
        return a;
    };
    py::dict d;
    d["n_roadlinks"] = shaped(y.nRoadLinks, {y.I});
    d["n_phases"] = shaped(y.nPhases, {y.I});
    d["phase_avail"] = shaped(y.phaseAvail, {y.I, y.P, y.M});
    d["roadlink_type"] = shaped(y.roadLinkType, {y.I, y.M});
    d["in_lanes"] = shaped(y.inLanes, {y.I, y.M, y.Kin});
    d["out_lanes"] = shaped(y.outLanes, {y.I, y.M, y.Kout});
    return d;
}

// ---- per-lane flow statistics across steps (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
inline py::ssize_t laneFlowLanes(EngineHost &e) { return (py::ssize_t) e.net().lanes.size(); }
inline py::ssize_t laneFlowLanes(cfa::VectorEngineHost &e) { return (py::ssize_t) e.numEnvs() * e.numLanes(); }
// one output of a tracker's array call: a fresh array of n elements, and the descriptor's pointer to its data
template <typename T> py::array_t<T> column(T *&slot, py::ssize_t n) {
    py::array_t<T> a(n);
    slot = a.mutable_data();
    return a;
}
template <typename E> py::tuple laneFlowTuple(E &e, bool reset) {
    const py::ssize_t n = laneFlowLanes(e);
    cfa::LaneFlowOut o;
    py::tuple t = py::make_tuple(column(o.entered, n), column(o.left, n), column(o.leftSteps, n), column(o.leftWaitingSteps, n),
                                 column(o.waitingSteps, n), column(o.maxWaitingSteps, n));
    e.laneFlowFeatures(o, reset);
    return t;
}
template <typename E>
void observeLaneFlowDevice(E &e, uintptr_t entered, uintptr_t left, uintptr_t leftSteps, uintptr_t leftWait, uintptr_t waitNow,
                           uintptr_t maxWait, bool reset, uintptr_t consumerStream) {
    cfa::LaneFlowOut o;
    o.entered = (int32_t *) entered;
    o.left = (int32_t *) left;
    o.leftSteps = (int64_t *) leftSteps;
    o.leftWaitingSteps = (int64_t *) leftWait;
    o.waitingSteps = (int64_t *) waitNow;
    o.maxWaitingSteps = (int32_t *) maxWait;
    e.observeLaneFlowDevice(o, reset, consumerStream);
}

// ---- per-movement flow statistics across steps (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
template <typename E> py::tuple movementFlowTuple(E &e, bool reset) {
    const py::ssize_t n = (py::ssize_t) e.movementFlowRows();
    cfa::MoveFlowOut o;
    py::tuple t = py::make_tuple(column(o.entered, n), column(o.enteredLaneSteps, n), column(o.enteredLaneWaitingSteps, n), column(o.left, n),
                                 column(o.leftSteps, n), column(o.leftWaitingSteps, n), column(o.waitingSteps, n),
                                 column(o.maxWaitingSteps, n));
    e.movementFlowFeatures(o, reset);
    return t;
}
template <typename E>
void observeMovementFlowDevice(E &e, uintptr_t entered, uintptr_t laneSteps, uintptr_t laneWait, uintptr_t left, uintptr_t leftSteps,
                               uintptr_t leftWait, uintptr_t waitNow, uintptr_t maxWait, bool reset, uintptr_t consumerStream) {
    cfa::MoveFlowOut o;
    o.entered = (int32_t *) entered;
    o.enteredLaneSteps = (int64_t *) laneSteps;
    o.enteredLaneWaitingSteps = (int64_t *) laneWait;
    o.left = (int32_t *) left;
    o.leftSteps = (int64_t *) leftSteps;
    o.leftWaitingSteps = (int64_t *) leftWait;
    o.waitingSteps = (int64_t *) waitNow;
    o.maxWaitingSteps = (int32_t *) maxWait;
    e.observeMovementFlowDevice(o, reset, consumerStream);
}

// ---- the first k vehicles of every lane from the front (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
template <typename E> py::tuple laneFrontsTuple(E &e, int k, bool tracker) {
    if (k < 1 || k > CFX_MAX_LANE_FRONT)
        throw py::value_error("k must be 1 to " + std::to_string(CFX_MAX_LANE_FRONT) + ", not " + std::to_string(k));
    const py::ssize_t n = laneFlowLanes(e) * k;
    py::array_t<double> dis(n), speed(n);
    py::array_t<int32_t> steps(tracker ? n : 0), wait(tracker ? n : 0);
    cfa::LaneFronts o;
    o.distance = dis.mutable_data();
    o.speed = speed.mutable_data();
    if (tracker) {
        o.laneSteps = steps.mutable_data();
        o.waitingSteps = wait.mutable_data();
    }
    e.laneFronts(k, o);
    return py::make_tuple(dis, speed, steps, wait);
}

template <typename E>
void observeLanesDevice(E &e, uintptr_t counts, uintptr_t waiting, uintptr_t speedSum, uintptr_t bins, uintptr_t edges, int nBins,
                        bool perLaneEdges, uintptr_t frontDistance, uintptr_t frontSpeed, uintptr_t frontLaneSteps,
                        uintptr_t frontWaitingSteps, int nFront, uintptr_t consumerStream) {
    cfx_lane_obs a{};
    a.struct_size = (int32_t) sizeof a;
    a.counts = (int32_t *) counts;
    a.waiting = (int32_t *) waiting;
    a.speed_sum = (double *) speedSum;
    a.bins = (int32_t *) bins;
    a.edges = (const double *) edges;
    a.n_bins = nBins;
    a.per_lane_edges = perLaneEdges ? 1 : 0;
    a.front_distance = (double *) frontDistance;
    a.front_speed = (double *) frontSpeed;
    a.front_lane_steps = (int32_t *) frontLaneSteps;
    a.front_waiting_steps = (int32_t *) frontWaitingSteps;
    a.n_front = nFront;
    e.observeLanesDevice(a, consumerStream);
}

// ---- every running vehicle as a row (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
template <typename E> py::tuple vehicleRowsTuple(E &e, bool poses) {
    const cfa::VehicleRows r = e.vehicleRows(poses);
    py::tuple t = py::make_tuple(toArray(r.start), r.count, toArray(r.vehicle), toArray(r.drivable), toArray(r.env), toArray(r.distance),
                                 toArray(r.speed), toArray(r.leader), toArray(r.gap));
    if (!poses) return t;
    return t + py::make_tuple(toArray(r.x), toArray(r.y), toArray(r.dirX), toArray(r.dirY), toArray(r.length), toArray(r.width));
}
template <typename E> py::tuple drivableGeometryTuple(E &e) {
    const cfa::DrivableGeometry g = e.drivableGeometry();
    return py::make_tuple(toArray(g.pointStart), toArray(g.xy));
}
template <typename E>
void observeVehiclesDevice(E &e, uintptr_t start, uintptr_t count, uintptr_t vehicle, uintptr_t drivable, uintptr_t env, uintptr_t distance,
                           uintptr_t speed, uintptr_t leader, uintptr_t gap, int nRows, uintptr_t consumerStream, uintptr_t x, uintptr_t y,
                           uintptr_t dirX, uintptr_t dirY, uintptr_t length, uintptr_t width) {
    cfx_vehicle_rows a{};
    a.struct_size = (int32_t) sizeof a;
    a.n_rows = nRows;
    a.start = (int32_t *) start;
    a.count = (int32_t *) count;
    a.vehicle = (int32_t *) vehicle;
    a.drivable = (int32_t *) drivable;
    a.env = (int32_t *) env;
    a.distance = (double *) distance;
    a.speed = (double *) speed;
    a.leader = (int32_t *) leader;
    a.gap = (double *) gap;
    a.x = (double *) x;
    a.y = (double *) y;
    a.dir_x = (double *) dirX;
    a.dir_y = (double *) dirY;
    a.length = (double *) length;
    a.width = (double *) width;
    e.observeVehiclesDevice(a, consumerStream);
}

// ---- trip statistics across steps (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
inline py::ssize_t tripEnvs(EngineHost &) { return 1; }
inline py::ssize_t tripEnvs(cfa::VectorEngineHost &e) { return (py::ssize_t) e.numEnvs(); }
template <typename E> py::tuple tripTuple(E &e) {
    const py::ssize_t n = tripEnvs(e);
    cfx_trip_stats_out o{};
    py::tuple t = py::make_tuple(column(o.entered, n), column(o.admitted, n), column(o.admitted_buffer_steps, n), column(o.finished, n),
                                 column(o.finished_travel_steps, n), column(o.in_system, n), column(o.buffered, n),
                                 column(o.in_system_travel_steps, n), column(o.average_travel_time, n));
    e.tripFeatures(o);
    return t;
}
template <typename E>
void observeTripsDevice(E &e, uintptr_t entered, uintptr_t admitted, uintptr_t bufferSteps, uintptr_t finished, uintptr_t travelSteps,
                        uintptr_t inSystem, uintptr_t buffered, uintptr_t inSteps, uintptr_t average, uintptr_t consumerStream) {
    cfx_trip_stats_out o{};
    o.entered = (int32_t *) entered;
    o.admitted = (int32_t *) admitted;
    o.admitted_buffer_steps = (int64_t *) bufferSteps;
    o.finished = (int32_t *) finished;
    o.finished_travel_steps = (int64_t *) travelSteps;
    o.in_system = (int32_t *) inSystem;
    o.buffered = (int32_t *) buffered;
    o.in_system_travel_steps = (int64_t *) inSteps;
    o.average_travel_time = (double *) average;
    e.observeTripsDevice(o, consumerStream);
}

// ---- the trip log (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
template <typename E> void trackTripLog(E &e, int64_t capacity) { e.trackTripLog(capacity); }
// (count, dropped, then the seven columns [capacity] in log order, -1 behind count)
template <typename E> py::tuple tripLogTuple(E &e, bool reset) {
    const py::ssize_t cap = (py::ssize_t) e.tripLogCapacity();
    cfx_trip_log_out o{};
    py::tuple t = py::make_tuple(column(o.count, 1), column(o.dropped, 1), column(o.env, cap), column(o.vehicle, cap), column(o.origin_road, cap),
                                 column(o.destination_road, cap), column(o.enter_step, cap), column(o.finish_step, cap),
                                 column(o.travel_steps, cap));
    e.tripLogFeatures(o, reset);
    return t;
}
template <typename E>
void observeTripLogDevice(E &e, uintptr_t count, uintptr_t dropped, uintptr_t env, uintptr_t vehicle, uintptr_t origin, uintptr_t destination,
                          uintptr_t enter, uintptr_t finish, uintptr_t travel, bool reset, uintptr_t consumerStream) {
    cfx_trip_log_out o{};
    o.count = (int32_t *) count;
    o.dropped = (int32_t *) dropped;
    o.env = (int32_t *) env;
    o.vehicle = (int32_t *) vehicle;
    o.origin_road = (int32_t *) origin;
    o.destination_road = (int32_t *) destination;
    o.enter_step = (int32_t *) enter;
    o.finish_step = (int32_t *) finish;
    o.travel_steps = (int32_t *) travel;
    e.observeTripLogDevice(o, reset, consumerStream);
}

// ---- virtual loop detectors across steps (Engine and VectorEngine; the public calls, and the checks of the arguments' types and
//      lengths, are cityflow_amd/torch_io.py)
template <typename E>
void defineDetectors(E &e, py::array_t<int32_t, py::array::c_style> lane, py::array_t<double, py::array::c_style> start,
                     py::array_t<double, py::array::c_style> end) {
    if (lane.ndim() != 1 || start.ndim() != 1 || end.ndim() != 1 || start.size() != lane.size() || end.size() != lane.size())
        throw py::value_error("track_detectors: lane, start and end must be one-dimensional and of equal length");
    try {
        e.defineDetectors(lane.data(), start.data(), end.data(), (int) lane.size());
    } catch (const std::invalid_argument &) {
        throw;  // (a ValueError; it is a logic_error too)
    } catch (const std::logic_error &x) {  // lane change is out of scope, not a failure of the call
        PyErr_SetString(PyExc_NotImplementedError, x.what());
        throw py::error_already_set();
    }
}
template <typename E> py::tuple detectorLayoutTuple(E &e) {
    const cfa::Detectors &d = e.detectors();
    return py::make_tuple(toArray(d.lanes()), toArray(d.starts()), toArray(d.ends()));
}
template <typename E> py::tuple detectorTuple(E &e, bool reset) {
    const py::ssize_t n = tripEnvs(e) * (py::ssize_t) e.detectors().count();
    cfx_detectors_out o{};
    py::tuple t = py::make_tuple(column(o.passed, n), column(o.occupied_steps, n), column(o.vehicle_steps, n),
                                 column(o.waiting_vehicle_steps, n), column(o.speed_sum, n), column(o.count, n));
    e.detectorFeatures(o, reset);
    return t;
}
template <typename E>
void observeDetectorsDevice(E &e, uintptr_t passed, uintptr_t occupied, uintptr_t vehicleSteps, uintptr_t waitingSteps, uintptr_t speedSum,
                            uintptr_t count, bool reset, uintptr_t consumerStream) {
    cfx_detectors_out o{};
    o.passed = (int32_t *) passed;
    o.occupied_steps = (int32_t *) occupied;
    o.vehicle_steps = (int64_t *) vehicleSteps;
    o.waiting_vehicle_steps = (int64_t *) waitingSteps;
    o.speed_sum = (double *) speedSum;
    o.count = (int32_t *) count;
    e.observeDetectorsDevice(o, reset, consumerStream);
}

// VectorEngine(seeds=...): None -> empty (seed + env index); anything else must hold one seed per environment
std::vector<int> envSeeds(int envs, const std::optional<std::vector<int>> &seeds) {
    if (!seeds) return {};
    if (envs < 1 || seeds->size() != (size_t) envs)
        throw std::invalid_argument("VectorEngine: seeds must hold num_envs = " + std::to_string(envs) + " seeds, not " +
                                    std::to_string(seeds->size()));
    return *seeds;
}

// ---- the fixed-time signal plan as engine state (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
inline py::ssize_t planRows(EngineHost &e) { return (py::ssize_t) e.net().inters.size(); }
inline py::ssize_t planRows(cfa::VectorEngineHost &e) { return (py::ssize_t) e.numEnvs() * e.numIntersections(); }

template <typename E> void setTlPlanArrays(E &e, const py::object &durations, const py::object &phase, const py::object &remain) {
    using DArr = py::array_t<double, py::array::c_style | py::array::forcecast>;
    using IArr = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
    const py::ssize_t rows = planRows(e), P = e.intersectionLayout().P;
    DArr d, r;
    IArr p;
    if (!durations.is_none()) d = durations.cast<DArr>();
    if (!phase.is_none()) p = phase.cast<IArr>();
    if (!remain.is_none()) r = remain.cast<DArr>();
    if ((!durations.is_none() && d.size() != rows * P) || (!phase.is_none() && p.size() != rows) || (!remain.is_none() && r.size() != rows))
        throw std::invalid_argument("set_tl_plan: an array of the wrong size");
    e.setTlPlan(durations.is_none() ? nullptr : d.data(), phase.is_none() ? nullptr : p.data(), remain.is_none() ? nullptr : r.data());
}

template <typename E> py::array_t<double> tlPhaseDurationsArray(E &e) {
    py::array_t<double> out(planRows(e) * (py::ssize_t) e.intersectionLayout().P);
    e.tlPhaseDurations(out.mutable_data());
    return out;
}

// ---- the lanes' speed limits as engine state (Engine and VectorEngine; the public calls are cityflow_amd/torch_io.py)
template <typename E> int setLaneSpeedLimitsArray(E &e, const py::array_t<double, py::array::c_style | py::array::forcecast> &limits) {
    if (limits.size() != (py::ssize_t) e.laneLimitCount()) throw std::invalid_argument("set_lane_speed_limits: an array of the wrong size");
    return (int) e.setLaneSpeedLimits(limits.data());
}

template <typename E> py::array_t<double> laneSpeedLimitsArray(E &e) {
    py::array_t<double> out((py::ssize_t) e.laneLimitCount());
    e.laneSpeedLimits(out.mutable_data());
    return out;
}

// track_lane_flow / track_movement_flow / track_trips: lane change is out of scope (logic_error), not a failure of the call
template <typename E, void (E::*Track)(bool)> void trackOrNotImplemented(E &e, bool on) {
    try {
        (e.*Track)(on);
    } catch (const std::logic_error &x) {
        PyErr_SetString(PyExc_NotImplementedError, x.what());
        throw py::error_already_set();
    }
}

// Device buffers: raw pointers and streams under the tensor methods of cityflow_amd/torch_io.py (Engine and VectorEngine alike)
template <typename E> void defDeviceBuffers(py::class_<E> &c) {
    c.def("_device_buffers", &E::deviceBuffers, "the backend takes observations / signals in device memory")
        .def("_tl_plan_calls", &E::tlPlanCalls, "the backend keeps the signal plan as engine state (set_tl_plan_tensor and its kin)")
        .def("_set_tl_plan_device", &E::setTlPlanDevice, "durations_ptr"_a, "phase_ptr"_a, "phase_remain_ptr"_a, "producer_stream"_a)
        .def("_set_tl_plan", &setTlPlanArrays<E>, "durations"_a, "phase"_a, "phase_remain"_a,
             "float64 [.., I, P] / int32 [.., I] / float64 [.., I] or None each; waits for the device")
        .def("_tl_phase_durations_device", &E::tlPhaseDurationsDevice, "out_ptr"_a, "consumer_stream"_a)
        .def("_tl_phase_durations", &tlPhaseDurationsArray<E>, "float64, flat (env-major, then intersection, then phase)")
        .def("_restore_tl_plan", &E::restoreTlPlan)
        .def("_lane_limit_calls", &E::laneLimitCalls,
             "the backend keeps the lanes' speed limits as engine state (set_lane_speed_limits_tensor and its kin)")
        .def("_set_lane_speed_limits_device", &E::setLaneSpeedLimitsDevice, "limits_ptr"_a, "rejected_ptr"_a, "producer_stream"_a)
        .def("_set_lane_speed_limits", &setLaneSpeedLimitsArray<E>, "limits"_a,
             "float64 [.., L]; waits for the device and returns the number of rejected entries")
        .def("_lane_speed_limits_device", &E::laneSpeedLimitsDevice, "out_ptr"_a, "consumer_stream"_a)
        .def("_lane_speed_limits", &laneSpeedLimitsArray<E>, "float64, flat (env-major, then lane)")
        .def("_restore_lane_speed_limits", &E::restoreLaneSpeedLimits)
        .def("_checkpoint_calls", &E::checkpointCalls, "the backend has checkpoints in device memory (checkpoint() / rollback())")
        .def("_checkpoint_unsupported", &E::checkpointUnsupported, "why this engine has no checkpoints in device memory ('' = it has)")
        .def("_checkpoint", &E::checkpoint, "into"_a = py::none(), py::keep_alive<0, 1>(),
             "DeviceCheckpoint of the state as of now (into: overwritten in place); it keeps the engine alive")
        .def("_rollback", &E::rollback, "checkpoint"_a)
        .def("_stream_handle", &E::streamHandle, "(engine's hipStream_t as an int, HIP device ordinal)")
        .def("_set_tl_phases_device", &E::setTrafficLightPhasesDevice, "phases_ptr"_a, "n"_a, "producer_stream"_a)
        .def("_rl_traffic_light", &E::rlTrafficLight)
        .def("_phase_counts", [](E &e) { return toArray(e.phaseCounts()); }, "phases per intersection, -1 = virtual")
        .def("lane_lengths", [](E &e) { return toArray(e.laneLengths()); }, "float64 [L]: Lane::getLength (of one environment)")
        .def("_observe_lanes_device", &observeLanesDevice<E>, "counts_ptr"_a, "waiting_ptr"_a, "speed_sum_ptr"_a, "bins_ptr"_a,
             "edges_ptr"_a, "n_bins"_a, "per_lane_edges"_a, "front_distance_ptr"_a, "front_speed_ptr"_a, "front_lane_steps_ptr"_a,
             "front_waiting_steps_ptr"_a, "n_front"_a, "consumer_stream"_a)
        .def("_lane_fronts", [](E &e, int k, bool tracker) { return laneFrontsTuple(e, k, tracker); }, "k"_a, "tracker"_a,
             "(distance, speed, lane_steps, waiting_steps) of the first k vehicles of every lane, flat (env-major); the last two "
             "empty unless `tracker`")
        .def("_vehicle_rows_device", &E::vehicleRowsDevice, "the backend writes the vehicle rows in device memory")
        .def("_drivable_counts", &E::drivableCounts, "(lanes, laneLinks) of one environment")
        .def("_lane_change", &E::laneChange)
        .def("_vehicle_poses_device", &E::vehiclePosesDevice, "the backend writes the pose columns of the vehicle rows in device memory")
        .def("_vehicle_rows", [](E &e, bool poses) { return vehicleRowsTuple(e, poses); }, "poses"_a = false,
             "(start, count, vehicle, drivable, env, distance, speed, leader, gap): every running vehicle as a row, environment-"
             "major, `start` flat [envs * (D + 1)]; with `poses` also (x, y, dir_x, dir_y, length, width); waits for the device")
        .def("_drivable_geometry", [](E &e) { return drivableGeometryTuple(e); },
             "(point_start int32 [D + 1], xy float64 [2 * P]): the polylines of one environment's drivables, lanes first")
        .def("_observe_vehicles_device", &observeVehiclesDevice<E>, "start_ptr"_a, "count_ptr"_a, "vehicle_ptr"_a, "drivable_ptr"_a,
             "env_ptr"_a, "distance_ptr"_a, "speed_ptr"_a, "leader_ptr"_a, "gap_ptr"_a, "n_rows"_a, "consumer_stream"_a, "x_ptr"_a = 0,
             "y_ptr"_a = 0, "dir_x_ptr"_a = 0, "dir_y_ptr"_a = 0, "length_ptr"_a = 0, "width_ptr"_a = 0)
        .def("_vehicle_speeds_device", &E::vehicleSpeedsDevice, "the backend takes vehicle speed commands from device memory")
        .def("_set_vehicle_speeds_device", &E::setVehicleSpeedsDevice, "vehicle_ptr"_a, "speed_ptr"_a, "n"_a, "ignored_ptr"_a,
             "producer_stream"_a)
        .def("_set_vehicle_speeds",
             [](E &e, py::array_t<int32_t, py::array::c_style> vehicle, py::array_t<double, py::array::c_style> speed) {
                 if (vehicle.ndim() != 1 || speed.ndim() != 1 || vehicle.size() != speed.size())
                     throw std::invalid_argument("set_vehicle_speeds: vehicle and speed must be one-dimensional and of one length");
                 return e.setVehicleSpeeds(vehicle.data(), speed.data(), (int) vehicle.size());
             },
             "vehicle"_a, "speed"_a, "int32 [N] vehicle numbers, float64 [N] speeds; returns the rows ignored; waits for the device")
        .def("route_roads", &E::routeRoads, "handle"_a,
             "the road ids of the route behind a handle (add_routes / added_routes, or any route index below route_count(), flow "
             "routes included); IndexError for anything else")
        .def("route_count", &E::routeCount, "the route handles are 0 .. route_count() - 1 (of one environment)")
        .def("_set_vehicle_routes_device", &E::setVehicleRoutesDevice, "vehicle_ptr"_a, "route_ptr"_a, "n"_a, "status_ptr"_a,
             "ignored_ptr"_a, "producer_stream"_a)
        .def("_set_vehicle_routes",
             [](E &e, py::array_t<int32_t, py::array::c_style> vehicle, py::array_t<int32_t, py::array::c_style> route) {
                 if (vehicle.ndim() != 1 || route.ndim() != 1 || vehicle.size() != route.size())
                     throw std::invalid_argument("set_vehicle_routes: vehicle and route must be one-dimensional and of one length");
                 py::array_t<int32_t> status(vehicle.size());
                 const int ignored = e.setVehicleRoutes(vehicle.data(), route.data(), (int) vehicle.size(), status.mutable_data());
                 return py::make_tuple(status, ignored);
             },
             "vehicle"_a, "route"_a, "int32 [N] vehicle numbers, int32 [N] route handles; returns (status [N], rows refused); waits for the device")
        .def("_vehicle_routes_device", &E::vehicleRoutesDevice, "vehicle_ptr"_a, "n"_a, "out_ptr"_a, "consumer_stream"_a)
        .def("_vehicle_routes",
             [](E &e, py::array_t<int32_t, py::array::c_style> vehicle) {
                 if (vehicle.ndim() != 1) throw std::invalid_argument("get_vehicle_routes: vehicle must be one-dimensional");
                 py::array_t<int32_t> out(vehicle.size());
                 e.vehicleRoutes(vehicle.data(), (int) vehicle.size(), out.mutable_data());
                 return out;
             },
             "vehicle"_a, "int32 [N] vehicle numbers; returns the handles they hold, -1 where there is none; waits for the device")
        .def("_intersection_dims", [](E &e) { return py::make_tuple(e.intersectionLayout().M, e.intersectionLayout().P); },
             "(largest roadLink count, largest phase count) of an intersection: the row lengths of the intersection observations")
        .def("_intersection_layout", [](E &e) { return intersectionLayoutDict(e); })
        .def("_observe_intersections_device", &E::observeIntersectionsDevice, "phase_ptr"_a, "remain_ptr"_a, "in_ptr"_a,
             "in_waiting_ptr"_a, "out_ptr"_a, "inside_ptr"_a, "pressure_ptr"_a, "max_roadlinks"_a, "max_phases"_a, "consumer_stream"_a)
        .def("_track_lane_flow", &trackOrNotImplemented<E, &E::trackLaneFlow>, "on"_a)
        .def("_lane_flow_tracking", &E::laneFlowTracking)
        .def("_lane_flow_features", [](E &e, bool reset) { return laneFlowTuple(e, reset); }, "reset"_a,
             "(entered, left, left_steps, left_waiting_steps, waiting_steps, max_waiting_steps), flat (env-major)")
        .def("_observe_lane_flow_device", &observeLaneFlowDevice<E>, "entered_ptr"_a, "left_ptr"_a, "left_steps_ptr"_a,
             "left_waiting_steps_ptr"_a, "waiting_steps_ptr"_a, "max_waiting_steps_ptr"_a, "reset"_a, "consumer_stream"_a)
        .def("_track_movement_flow", &trackOrNotImplemented<E, &E::trackMovementFlow>, "on"_a)
        .def("_movement_flow_tracking", &E::movementFlowTracking)
        .def("_movement_flow_features", [](E &e, bool reset) { return movementFlowTuple(e, reset); }, "reset"_a,
             "(entered, entered_lane_steps, entered_lane_waiting_steps, left, left_steps, left_waiting_steps, waiting_steps, "
             "max_waiting_steps), flat (env-major, then intersection, then roadLink)")
        .def("_observe_movement_flow_device", &observeMovementFlowDevice<E>, "entered_ptr"_a, "entered_lane_steps_ptr"_a,
             "entered_lane_waiting_steps_ptr"_a, "left_ptr"_a, "left_steps_ptr"_a, "left_waiting_steps_ptr"_a, "waiting_steps_ptr"_a,
             "max_waiting_steps_ptr"_a, "reset"_a, "consumer_stream"_a)
        .def("_track_trips", &trackOrNotImplemented<E, &E::trackTrips>, "on"_a)
        .def("_trip_tracking", &E::tripTracking)
        .def("_trip_features", [](E &e) { return tripTuple(e); },
             "(entered, admitted, admitted_buffer_steps, finished, finished_travel_steps, in_system, buffered, "
             "in_system_travel_steps, average_travel_time), one element per environment")
        .def("_observe_trips_device", &observeTripsDevice<E>, "entered_ptr"_a, "admitted_ptr"_a, "admitted_buffer_steps_ptr"_a,
             "finished_ptr"_a, "finished_travel_steps_ptr"_a, "in_system_ptr"_a, "buffered_ptr"_a, "in_system_travel_steps_ptr"_a,
             "average_travel_time_ptr"_a, "consumer_stream"_a)
        .def("_track_trip_log", &trackTripLog<E>, "capacity"_a, "an empty trip log of that many rows (0: none); trip tracking must be on")
        .def("_trip_log_capacity", &E::tripLogCapacity)
        .def("_trip_log_features", [](E &e, bool reset) { return tripLogTuple(e, reset); }, "reset"_a,
             "(count, dropped, env, vehicle, origin_road, destination_road, enter_step, finish_step, travel_steps): the columns "
             "[capacity] in log order, -1 behind count")
        .def("_observe_trip_log_device", &observeTripLogDevice<E>, "count_ptr"_a, "dropped_ptr"_a, "env_ptr"_a, "vehicle_ptr"_a,
             "origin_road_ptr"_a, "destination_road_ptr"_a, "enter_step_ptr"_a, "finish_step_ptr"_a, "travel_steps_ptr"_a, "reset"_a,
             "consumer_stream"_a)
        .def("_define_detectors", &defineDetectors<E>, "lane"_a, "start"_a, "end"_a,
             "int32 / float64 / float64 [N], of one environment; turns the tracker on and takes a baseline")
        .def("_drop_detectors", &E::dropDetectors)
        .def("_detector_tracking", [](E &e) { return e.detectors().on(); })
        .def("_detector_count", [](E &e) { return e.detectors().count(); }, "detectors of one environment")
        .def("_detector_layout", [](E &e) { return detectorLayoutTuple(e); }, "(lane, start, end) as they were defined")
        .def("_detector_features", [](E &e, bool reset) { return detectorTuple(e, reset); }, "reset"_a,
             "(passed, occupied_steps, vehicle_steps, waiting_vehicle_steps, speed_sum, count), flat (env-major)")
        .def("_observe_detectors_device", &observeDetectorsDevice<E>, "passed_ptr"_a, "occupied_steps_ptr"_a, "vehicle_steps_ptr"_a,
             "waiting_vehicle_steps_ptr"_a, "speed_sum_ptr"_a, "count_ptr"_a, "reset"_a, "consumer_stream"_a);
}

// Engine.set_tl_phase(intersection_id, phase_id) (reference src/cityflow.cpp:35, engine.cpp:719-725) as a vectorcall method of its
// own.  An RL agent written for the reference calls it once per signal and step — 900 calls per step on the 30x30 grid — and
// the generic binding path (argument records, a std::string per call, a std::map lookup by string comparison) costs ~0.35 us
// per call: more than the whole device step for the 900 of them.  Here: the id's Python string is looked up in a dict kept with
// the engine (its hash is cached in the string object), ~0.1 us per call.  Same arguments (positional or by the reference's
// names), same errors (RuntimeError for an unknown intersection, IndexError for a phase out of range, TypeError otherwise).
PyObject *engineSetTlPhase(PyObject *self, PyObject *const *args, Py_ssize_t nargs, PyObject *kwnames) {
    try {
        PyObject *idObj = nargs >= 1 ? args[0] : nullptr, *phObj = nargs >= 2 ? args[1] : nullptr;
        const Py_ssize_t nkw = kwnames ? PyTuple_GET_SIZE(kwnames) : 0;
        bool bad = nargs > 2;
        for (Py_ssize_t i = 0; i < nkw && !bad; ++i) {
            PyObject *name = PyTuple_GET_ITEM(kwnames, i);
            if (PyUnicode_CompareWithASCIIString(name, "intersection_id") == 0 && !idObj) idObj = args[nargs + i];
            else if (PyUnicode_CompareWithASCIIString(name, "phase_id") == 0 && !phObj) phObj = args[nargs + i];
            else bad = true;
        }
        if (bad || !idObj || !phObj || !PyUnicode_Check(idObj) || PyFloat_Check(phObj) || !PyIndex_Check(phObj)) {
            PyErr_SetString(PyExc_TypeError, "set_tl_phase(intersection_id: str, phase_id: int): incompatible arguments");
            return nullptr;
        }
        // (the method descriptor has checked that `self` is an Engine; the generic caster's type lookup is a third of the call)
        auto *inst = reinterpret_cast<py::detail::instance *>(self);
        EngineHost *ep = inst->simple_layout ? static_cast<EngineHost *>(inst->simple_value_holder[0]) : nullptr;
        EngineHost &e = ep ? *ep : py::cast<EngineHost &>(py::handle(self));
        long ph;
        if (PyLong_CheckExact(phObj)) {
            ph = PyLong_AsLong(phObj);
        } else {
            PyObject *phIdx = PyNumber_Index(phObj);
            if (!phIdx) return nullptr;
            ph = PyLong_AsLong(phIdx);
            Py_DECREF(phIdx);
        }
        if (ph == -1 && PyErr_Occurred()) return nullptr;
        if (ph < INT32_MIN || ph > INT32_MAX) {
            PyErr_SetString(PyExc_TypeError, "set_tl_phase: phase_id does not fit an int");
            return nullptr;
        }
        LaneDictCache &c = bindingCacheOf(e);
        if (!c.interIdx) {
            py::dict d;
            for (size_t i = 0; i < e.net().inters.size(); ++i) d[py::str(e.net().inters[i].id)] = py::int_(i);
            c.interIdx = std::move(d);
        }
        PyObject *ix = PyDict_GetItemWithError(c.interIdx.ptr(), idObj);  // borrowed
        if (!ix && PyErr_Occurred()) return nullptr;
        if (ix) {
            e.setTrafficLightPhaseOf((int) PyLong_AsLong(ix), (int) ph);
        } else {  // (not an intersection: the message comes from where the reference's comes from)
            Py_ssize_t len = 0;
            const char *utf8 = PyUnicode_AsUTF8AndSize(idObj, &len);
            if (!utf8) return nullptr;
            e.setTrafficLightPhase(std::string(utf8, (size_t) len), (int) ph);
        }
        Py_RETURN_NONE;
    } catch (py::error_already_set &err) {
        err.restore();
    } catch (const py::cast_error &err) {
        PyErr_SetString(PyExc_TypeError, err.what());
    } catch (const std::out_of_range &err) {
        PyErr_SetString(PyExc_IndexError, err.what());
    } catch (const std::exception &err) {
        PyErr_SetString(PyExc_RuntimeError, err.what());
    }
    return nullptr;
}
PyMethodDef kEngineSetTlPhaseDef = {"set_tl_phase", (PyCFunction) (void (*)(void)) engineSetTlPhase, METH_FASTCALL | METH_KEYWORDS,
                                    "set_tl_phase(self, intersection_id: str, phase_id: int) -> None"};

// Host-only helpers (no device engine involved): used by the CPU test-suite to pin the loader and the
// spawner against the reference.
py::dict loadRoadnet(const std::string &path) {
    cfa::HostRoadNet net;
    net.load(path);
    return flatNetToDict(net);
}

// Same text format as oracle/probe_roadnet.cpp prints from the reference's own loader.
py::bytes roadnetProbe(const std::string &path) {
    cfa::HostRoadNet net;
    net.load(path);
    const cfx_net &f = net.flat();
    std::string out;
    char buf[512];
    for (int l = 0; l < f.n_lanes; ++l) {
        snprintf(buf, sizeof buf, "L %s %.17g %.17g %.17g %zu\n", net.laneId(l).c_str(), f.drv_length[l],
                 f.drv_max_speed[l], net.lanes[l].width, net.lanes[l].laneLinks.size());
        out += buf;
    }
    for (int k = 0; k < f.n_lanelinks; ++k) {
        snprintf(buf, sizeof buf, "K %s %.17g %d %d\n", net.laneLinkId(k).c_str(), f.drv_length[f.n_lanes + k],
                 f.ll_type[k], f.ll_x_start[k + 1] - f.ll_x_start[k]);
        out += buf;
        for (int e = f.ll_x_start[k]; e < f.ll_x_start[k + 1]; ++e) {
            snprintf(buf, sizeof buf, "X %.17g %s %.17g\n", f.x_dist[e], net.laneLinkId(f.x_ll[f.x_peer[e]]).c_str(),
                     f.x_dist[f.x_peer[e]]);
            out += buf;
        }
    }
    for (auto &in : net.inters) {
        snprintf(buf, sizeof buf, "T %s %d %zu\n", in.id.c_str(), (int) in.isVirtual, in.phases.size());
        out += buf;
    }
    return py::bytes(out);
}

// ahead: 0 every step taken plainly; 1 every step taken ahead and consumed (Spawner::beginAhead / commitAhead); 2 every step
// taken ahead, taken back (rollbackAhead) and then taken plainly — what a call between two steps does to the host's step ahead
py::list spawnSchedule(const std::string &roadnetFile, const std::string &flowFile, double interval, int seed,
                       int threadNum, int steps, int ahead) {
    cfa::HostRoadNet net;
    net.load(roadnetFile);
    cfa::Spawner sp;
    sp.init(&net, interval, threadNum, seed);
    sp.loadFlows(flowFile);
    py::list out;
    std::vector<cfx_spawn> recs;
    for (int s = 0; s < steps; ++s) {
        if (ahead) {
            sp.beginAhead();
            sp.step((size_t) s, recs);
            if (ahead == 2) {
                sp.rollbackAhead();
                sp.step((size_t) s, recs);
            } else {
                sp.commitAhead();
            }
        } else {
            sp.step((size_t) s, recs);
        }
        py::list stepList;
        for (const cfx_spawn &r : recs)
            stepList.append(py::make_tuple(sp.vehicleId(r.vid), r.priority, net.laneId(r.lane), r.enter_time, r.templ,
                                           r.route, r.prev_wait));
        out.append(stepList);
    }
    return out;
}

// seconds spent in `steps` Spawner::step calls (host-side cost of phases 0-1, no device, no Python objects)
double spawnBenchmark(const std::string &roadnetFile, const std::string &flowFile, double interval, int seed, int skip,
                      int steps) {
    cfa::HostRoadNet net;
    net.load(roadnetFile);
    cfa::Spawner sp;
    sp.init(&net, interval, 1, seed);
    sp.loadFlows(flowFile);
    std::vector<cfx_spawn> recs;
    for (int s = 0; s < skip; ++s) sp.step((size_t) s, recs);
    auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < steps; ++s) sp.step((size_t) (skip + s), recs);
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

PYBIND11_MODULE(_cityflow, m) {
    m.doc() = "MI355X-native CityFlow step engine (drop-in for the reference `cityflow` module)";

    using cfa::DeviceCheckpoint;
    py::class_<DeviceCheckpoint, std::shared_ptr<DeviceCheckpoint>>(
        m, "DeviceCheckpoint",
        "The whole simulation state of an Engine or VectorEngine in device memory (checkpoint() / rollback()); not consumed by a "
        "rollback, freed by release() or with the object")
        .def_property_readonly("step", [](const DeviceCheckpoint &c) { return c.released() ? (int64_t) -1 : c.desc().step; })
        .def_property_readonly("num_running", [](const DeviceCheckpoint &c) { return c.desc().n_running; }, "running vehicles")
        .def_property_readonly("num_vehicle_numbers", [](const DeviceCheckpoint &c) { return c.desc().n_vehicles; },
                               "vehicle numbers handed out (rows of the device's vehicle table)")
        .def_property_readonly("device_bytes", [](const DeviceCheckpoint &c) { return c.desc().device_bytes; },
                               "device memory held (0 once released)")
        .def_property_readonly("released", &DeviceCheckpoint::released)
        .def("release", &DeviceCheckpoint::release, "free the device memory now; rollback() to it is a ValueError from here on");

    py::class_<EngineHost> engineClass(m, "Engine");
    engineClass
        .def(py::init<const std::string &, int>(), "config_file"_a, "thread_num"_a = 1)
        .def_static(
            "_with_backend",
            [](const std::string &cfg, int threads, const std::string &lib) {
                return std::unique_ptr<EngineHost>(new EngineHost(cfg, threads, lib));
            },
            "config_file"_a, "thread_num"_a, "backend_library"_a,
            "Test hook: build an engine on any shared library exporting the cfx_* C ABI.")
        // ---- reference API ----
        .def("next_step", &EngineHost::nextStep)
        .def("get_vehicle_count", &EngineHost::getVehicleCount)
        .def("get_vehicles", [](EngineHost &e, bool w) -> py::object {
                 if (e.laneChange()) return py::cast(e.getVehicles(w));  // ids change with state ("_shadow"): no id cache
                 if (w) {  // vehicles pushed since the last step have no vehicle number yet (EngineHost::getVehicles lists them)
                     std::vector<std::pair<int32_t, std::string>> pushed;
                     e.spawner().pendingPushed(pushed);
                     if (!pushed.empty()) return py::cast(e.getVehicles(w));
                 }
                 return vehicleList(e, w);
             }, "include_waiting"_a = false)
        // dict[str, int] in std::map (lexicographic) key order like the reference, built from cached key objects
        .def("get_lane_vehicle_count", [](EngineHost &e) { return laneDict(e, e.laneVehicleCountArray(), 0); })
        .def("get_lane_waiting_vehicle_count", [](EngineHost &e) { return laneDict(e, e.laneWaitingVehicleCountArray(), 1); })
        .def("get_lane_vehicles", [](EngineHost &e) -> py::object {
                 if (e.laneChange()) return py::cast(e.getLaneVehicles());
                 return laneVehiclesDict(e);
             })
        .def("get_vehicle_speed", [](EngineHost &e) -> py::object {
                 if (e.laneChange()) return py::cast(e.getVehicleSpeed());
                 return vehicleValueDict(e, true);
             })
        .def("get_vehicle_info", &EngineHost::getVehicleInfo, "vehicle_id"_a)
        .def("get_vehicle_distance", [](EngineHost &e) -> py::object {
                 if (e.laneChange()) return py::cast(e.getVehicleDistance());
                 return vehicleValueDict(e, false);
             })
        .def("get_leader", &EngineHost::getLeader, "vehicle_id"_a)
        .def("get_current_time", &EngineHost::getCurrentTime)
        .def("get_average_travel_time", &EngineHost::getAverageTravelTime)
        // (set_tl_phase: engineSetTlPhase, attached below)
        .def("set_random_seed", &EngineHost::setRandomSeed, "seed"_a)
        .def("push_vehicle", &EngineHost::pushVehicle)
        .def("reset", &EngineHost::reset, "seed"_a = false)
        .def("set_vehicle_speed", &EngineHost::setVehicleSpeed, "vehicle_id"_a, "speed"_a)
        .def("set_vehicle_route", &EngineHost::setRoute, "vehicle_id"_a, "route"_a)
        .def("add_routes", &EngineHost::addRoutes, "routes"_a,
             "routes: lists of road ids, each expanded the way a flow's `route` is (consecutive roads joined by the shortest path) "
             "and registered; returns their handles for set_vehicle_routes_tensor, equal lists sharing one.  Handles stay valid "
             "across reset(), load(), rollback() and vehicle compaction.  ValueError naming the list's index for an unknown road "
             "or a route the reference would call invalid, and then nothing is added")
        .def("load", &EngineHost::load, "archive"_a)
        .def("snapshot", &EngineHost::snapshot)
        .def("load_from_file", &EngineHost::loadFromFile, "path"_a)
        .def("set_replay_file", &EngineHost::setReplayLogFile, "replay_file"_a)
        .def("set_save_replay", &EngineHost::setSaveReplay, "open"_a)
        // ---- array API (index order == lane_ids() / intersection_ids()) ----
        .def("lane_ids", &EngineHost::laneIds)
        .def("road_ids", &EngineHost::roadIds, "the roads in roadnet-file order: what the trip log's road columns index")
        .def("intersection_ids", &EngineHost::intersectionIds)
        .def("get_lane_vehicle_count_array", [](EngineHost &e) { return toArray(e.laneVehicleCountArray()); })
        .def("get_lane_waiting_vehicle_count_array",
             [](EngineHost &e) { return toArray(e.laneWaitingVehicleCountArray()); })
        .def("set_tl_phase_indexed", &EngineHost::setTrafficLightPhaseIndexed, "intersection_index"_a, "phase_id"_a)
        .def("set_tl_phases",
             [](EngineHost &e, py::array_t<int32_t, py::array::c_style | py::array::forcecast> phases) {
                 e.setTrafficLightPhases(phases.data(), (size_t) phases.size());
             },
             "phases"_a, "int array [len(intersection_ids())]; one asynchronous call sets every signal")
        .def("sync", &EngineHost::sync)
        .def("backend_name", &EngineHost::backendName)
        .def("_tensor_shapes", [](EngineHost &e) {
            return py::make_tuple(py::make_tuple(e.net().lanes.size()), py::make_tuple(e.net().inters.size()));
        }, "(shape of an observation, shape of the signals)")
        // ---- per-lane speed and position features (index order == lane_ids()) ----
        .def("get_lane_speed_sum_array",
             [](EngineHost &e) { return laneSpeedSumArray(e, {(py::ssize_t) e.net().lanes.size()}); },
             "float64 [L]: the speeds of each lane's vehicles summed front to back (mean speed = sum / count)")
        .def("get_lane_vehicle_bins_array",
             [](EngineHost &e, const EdgesArray &edges) { return laneBinsArray(e, edges, {(py::ssize_t) e.net().lanes.size()}); },
             "edges"_a, "int32 [L, B]: vehicles with edges[l, b] <= distance < edges[l, b+1]; edges [L, B+1] or [B+1]")
        // ---- introspection used by the parity tests ----
        .def("_vehicle_state",
             [](EngineHost &e) {
                 cfa::VehicleSnapshot s;
                 e.snapshotVehicles(s);
                 py::dict d;
                 d["vid"] = toArray(s.vid);
                 d["drivable"] = toArray(s.drivable);
                 d["prev_drivable"] = toArray(s.prevDrivable);
                 d["leader"] = toArray(s.leader);
                 d["blocker"] = toArray(s.blocker);
                 d["enter_ll_time"] = toArray(s.enterLLTime);
                 d["route_pos"] = toArray(s.routePos);
                 d["dis"] = toArray(s.dis);
                 d["speed"] = toArray(s.speed);
                 d["gap"] = toArray(s.gap);
                 if (e.laneChange()) {
                     d["lc_partner"] = toArray(s.lcPartner);
                     d["lc_flags"] = toArray(s.lcFlags);
                     d["lc_offset"] = toArray(s.lcOffset);
                     d["lc_last_dir"] = toArray(s.lcLastDir);
                     d["lc_target"] = toArray(s.lcTarget);
                     d["lc_direction"] = toArray(s.lcDirection);
                     d["lc_last_change_time"] = toArray(s.lcLastChangeTime);
                 }
                 return d;
             })
        .def("_waiting",
             [](EngineHost &e) {
                 std::vector<int32_t> v, l;
                 e.waitingVehicles(v, l);
                 return py::make_tuple(toArray(v), toArray(l));
             })
        .def("_keeps_lane_history", &EngineHost::keepsLaneHistory)
        .def("_compact_vehicles", &EngineHost::compactVehicles,
             "forget the finished vehicles now (automatic once \"cfx\": {\"compactVehicles\": N} vehicles have been created; default 3.5 M)")
        .def("_vehicle_table", [](EngineHost &e) { return py::make_tuple(e.vehicleTableSize(), e.vehicleCompactions()); },
             "(vehicle numbers the host holds, compactions so far)")
        .def("_lane_history",
             [](EngineHost &e) {  // test hook: cfx_get_lane_history; arrays [L], [L, 241], [L, 241], [L], [L]
                 std::vector<int32_t> len, num, hn;
                 std::vector<double> avg, ha;
                 e.laneHistory(len, num, avg, hn, ha);
                 py::dict d;
                 d["len"] = toArray(len);
                 d["vehicle_num"] = toArray(num);
                 d["average_speed"] = toArray(avg);
                 d["history_vehicle_num"] = toArray(hn);
                 d["history_average_speed"] = toArray(ha);
                 return d;
             })
        .def("_tl_state",
             [](EngineHost &e) {
                 std::vector<int32_t> p;
                 std::vector<double> r;
                 e.trafficLightState(p, r);
                 return py::make_tuple(toArray(p), toArray(r));
             })
        .def("_scalars",
             [](EngineHost &e) {
                 cfx_scalars s = e.scalars();
                 py::dict d;
                 d["step"] = s.step;
                 d["active_vehicle_count"] = s.active_vehicle_count;
                 d["finished_vehicle_count"] = s.finished_vehicle_count;
                 d["spawned_vehicle_count"] = s.spawned_vehicle_count;
                 d["cumulative_travel_time"] = s.cumulative_travel_time;
                 d["live_enter_time_sum"] = s.live_enter_time_sum;
                 d["vehicle_steps"] = s.vehicle_steps;
                 d["tie_events"] = s.tie_events;
                 py::list td;
                 for (int i = 0; i < 8; ++i)
                     if (s.tie_drivables[i] >= 0) td.append(s.tie_drivables[i]);
                 d["tie_drivables"] = td;
                 d["diag_cross_jobs"] = s.diag_cross_jobs;
                 d["dropped_future_speeds"] = s.dropped_future_speeds;
                 return d;
             })
        .def("_layout", &EngineHost::layoutName)
        .def("_ring_info", &EngineHost::ringInfo, "(total ring slots, capacity scale) of the ring layout")
        .def("_profile_enable", &EngineHost::profileEnable, "on"_a)
        .def("_device_spin", &EngineHost::deviceSpin, "microseconds"_a)
        .def("_device_memory", &EngineHost::deviceMemory, "(free, total) bytes of the engine's device")
        .def("_profile_read", &EngineHost::profileRead)
        .def("_profile_symbols", &EngineHost::profileSymbols, "timing slot -> symbol of the kernel launched last in it")
        .def("_host_stats", [](EngineHost &e, bool reset) {
            const cfx_host_stats s = e.hostStats(reset);
            const EngineHost::SlowestStep slow = e.slowestStep(reset);
            py::dict d;
            d["slowest_next_step"] = py::make_tuple(slow.total, slow.step, py::make_tuple(slow.part[0], slow.part[1], slow.part[2],
                                                                                          slow.part[3], slow.part[4], slow.part[5]));
            d["step_calls"] = s.step_calls;
            d["step_call_us_mean"] = s.step_calls ? s.step_call_us_sum / (double) s.step_calls : 0.0;
            d["worst_step_call_us"] = s.worst_step_call_us;
            d["worst_step_call_at"] = s.worst_step_call_at;
            d["worst_step_call_cause"] = s.worst_step_call_cause;
            d["calls_over_1ms"] = s.calls_over_1ms;
            d["ring_regrows_total"] = s.ring_regrows_total;
            d["table_grows_total"] = s.table_grows_total;
            d["status_queries"] = s.status_queries;
            d["worst_status_query_us"] = py::make_tuple(s.worst_status_query_us, s.worst_status_query_settle_us,
                                                         s.worst_status_query_copy_us, s.worst_status_query_wait_us);
            cfx_cross_stats x;
            if (e.crossStats(reset, &x)) {  // (kr_cross's grids: waits for the stream)
                d["cross_multi_pass_launches"] = x.multi_pass_launches;
                d["cross_max_passes"] = x.max_passes;
                d["cross_last_jobs"] = x.last_jobs;
                d["cross_last_grid_blocks"] = x.last_grid_blocks;
                d["cross_held_jobs"] = x.held_jobs;
                d["action_multi_pass_blocks"] = x.action_multi_pass_blocks;
                d["action_lanes_per_block"] = x.action_lanes_per_block;
            }
            return d;
        }, "reset"_a = false, "host time inside cfx_step (cfx_get_host_stats)")
        .def("_vehicle_id", [](EngineHost &e, int vid) { return e.vehicleId(vid); }, "vid"_a)
        .def("_vehicle_ids",
             [](EngineHost &e, py::array_t<int32_t> vids) {
                 std::vector<std::string> out;
                 auto r = vids.unchecked<1>();
                 for (py::ssize_t i = 0; i < r.shape(0); ++i) out.push_back(e.vehicleId(r(i)));
                 return out;
             })
        .def("_id_sort_key", [](EngineHost &e, int vid) { return e.spawner().idSortKey(vid); }, "vid"_a)
        .def("_vehicle_priority", [](EngineHost &e, int vid) { return e.spawner().vehicles.at(vid).priority; })
        .def("_drivable_ids",
             [](EngineHost &e) {
                 std::vector<std::string> ids;
                 int D = (int) (e.net().lanes.size() + e.net().laneLinks.size());
                 for (int d = 0; d < D; ++d) ids.push_back(e.net().drivableId(d));
                 return ids;
             })
        .def("_flat_net", [](EngineHost &e) { return flatNetToDict(e.net()); });
    defDeviceBuffers(engineClass);
    engineClass.def("_intersection_features", [](EngineHost &e) { return intersectionFeaturesTuple(e, 1); },
                    "(phase, remain, in, in_waiting, out, inside, phase_pressure), flat");
    {
        PyObject *descr = PyDescr_NewMethod((PyTypeObject *) engineClass.ptr(), &kEngineSetTlPhaseDef);
        if (!descr) throw py::error_already_set();
        engineClass.attr("set_tl_phase") = py::reinterpret_steal<py::object>(descr);
    }

    using cfa::VectorEngineHost;
    py::class_<VectorEngineHost> vectorClass(m, "VectorEngine",
                                             "num_envs independent copies of one scenario (env e uses seed + e, or seeds[e]) advanced in "
                                             "lock-step by one device engine; observations and actions are arrays of shape "
                                             "[num_envs, ...].");
    vectorClass
        .def(py::init([](const std::string &cfg, int envs, int threads, const std::optional<std::vector<int>> &seeds,
                         const std::optional<std::vector<std::vector<std::string>>> &routes) {
                 return std::unique_ptr<VectorEngineHost>(new VectorEngineHost(
                     cfg, envs, threads, "", envSeeds(envs, seeds), routes ? *routes : std::vector<std::vector<std::string>>{}));
             }),
             "config_file"_a, "num_envs"_a, "thread_num"_a = 1, "seeds"_a = py::none(), "routes"_a = py::none(),
             "seeds: num_envs ints, one per environment, instead of seed + env index (also on reset(seed=True)); equal seeds give "
             "every environment the same demand.  routes: lists of road ids, the candidate routes of set_vehicle_routes_tensor, as "
             "Engine.add_routes takes them; added_routes() has their handles.  There is no add_routes on a VectorEngine: every "
             "environment holds its own copy of the route tables, uploaded once, here")
        .def_static(
            "_with_backend",
            [](const std::string &cfg, int envs, int threads, const std::string &lib, const std::optional<std::vector<int>> &seeds,
               const std::optional<std::vector<std::vector<std::string>>> &routes) {
                return std::unique_ptr<VectorEngineHost>(new VectorEngineHost(
                    cfg, envs, threads, lib, envSeeds(envs, seeds), routes ? *routes : std::vector<std::vector<std::string>>{}));
            },
            "config_file"_a, "num_envs"_a, "thread_num"_a, "backend_library"_a, "seeds"_a = py::none(), "routes"_a = py::none())
        .def("added_routes", &VectorEngineHost::addedRoutes,
             "the handles of the constructor's `routes`, in the order given (equal in every environment)")
        .def_property_readonly("num_envs", &VectorEngineHost::numEnvs)
        .def("_host_seconds", &VectorEngineHost::hostSeconds,
             "[spawners, record translation, cfx_step] cumulative host wall seconds since the last reset")
        .def("next_step", &VectorEngineHost::nextStep)
        .def("reset", &VectorEngineHost::reset, "seed"_a = false)
        .def("get_current_time", &VectorEngineHost::getCurrentTime)
        .def("get_vehicle_count", &VectorEngineHost::totalVehicleCount)
        .def("lane_ids", &VectorEngineHost::laneIds)
        .def("road_ids", &VectorEngineHost::roadIds, "one environment's roads in roadnet-file order: what the trip log's road columns index")
        .def("intersection_ids", &VectorEngineHost::intersectionIds)
        .def("get_lane_vehicle_count_array",
             [](VectorEngineHost &e) {
                 auto a = toArray(e.laneVehicleCounts());
                 a.resize({(py::ssize_t) e.numEnvs(), (py::ssize_t) e.numLanes()});
                 return a;
             })
        .def("get_lane_waiting_vehicle_count_array",
             [](VectorEngineHost &e) {
                 auto a = toArray(e.laneWaitingVehicleCounts());
                 a.resize({(py::ssize_t) e.numEnvs(), (py::ssize_t) e.numLanes()});
                 return a;
             })
        .def("set_tl_phases",
             [](VectorEngineHost &e, py::array_t<int32_t, py::array::c_style | py::array::forcecast> phases) {
                 std::vector<int32_t> v(phases.data(), phases.data() + phases.size());
                 e.setTrafficLightPhases(v);
             },
             "phases"_a, "int array [num_envs, num_intersections] (entries of virtual intersections are ignored)")
        .def("get_lane_vehicle_count", &VectorEngineHost::getLaneVehicleCount, "env"_a)
        .def("get_vehicle_speed", &VectorEngineHost::getVehicleSpeed, "env"_a)
        .def("sync", &VectorEngineHost::sync)
        .def("backend_name", &VectorEngineHost::backendName)
        .def("_tl_state",
             [](VectorEngineHost &e) {
                 std::vector<int32_t> p;
                 std::vector<double> r;
                 e.trafficLightState(p, r);
                 auto pa = toArray(p);
                 auto ra = toArray(r);
                 pa.resize({(py::ssize_t) e.numEnvs(), (py::ssize_t) e.numIntersections()});
                 ra.resize({(py::ssize_t) e.numEnvs(), (py::ssize_t) e.numIntersections()});
                 return py::make_tuple(pa, ra);
             },
             "(current phase, remaining time), each [num_envs, num_intersections]")
        .def("_tensor_shapes", [](VectorEngineHost &e) {
            return py::make_tuple(py::make_tuple(e.numEnvs(), e.numLanes()), py::make_tuple(e.numEnvs(), e.numIntersections()));
        })
        .def("get_lane_speed_sum_array",
             [](VectorEngineHost &e) { return laneSpeedSumArray(e, {(py::ssize_t) e.numEnvs(), (py::ssize_t) e.numLanes()}); },
             "float64 [num_envs, L]")
        .def("get_lane_vehicle_bins_array",
             [](VectorEngineHost &e, const EdgesArray &edges) {
                 return laneBinsArray(e, edges, {(py::ssize_t) e.numEnvs(), (py::ssize_t) e.numLanes()});
             },
             "edges"_a, "int32 [num_envs, L, B]; edges [L, B+1] or [B+1], the same for every environment")
        .def("_profile_enable", &VectorEngineHost::profileEnable, "on"_a)
        .def("_profile_read", &VectorEngineHost::profileRead)
        .def("_scalars", [](VectorEngineHost &e) {
            cfx_scalars s = e.scalars();
            py::dict d;
            d["step"] = s.step;
            d["active_vehicle_count"] = s.active_vehicle_count;
            d["finished_vehicle_count"] = s.finished_vehicle_count;
            d["spawned_vehicle_count"] = s.spawned_vehicle_count;
            d["vehicle_steps"] = s.vehicle_steps;
                 d["tie_events"] = s.tie_events;
            d["cumulative_travel_time"] = s.cumulative_travel_time;
            return d;
        });
    defDeviceBuffers(vectorClass);
    vectorClass
        .def("_rollback_envs", &VectorEngineHost::rollbackEnvs, "checkpoint"_a, "envs"_a,
             "_rollback with environment r taking the state of environment envs[r] (num_envs ints in [0, num_envs))")
        .def("_keeps_lane_history", &VectorEngineHost::keepsLaneHistory)
        .def("_ring_info", &VectorEngineHost::ringInfo, "(total ring slots, capacity scale) of the ring layout")
        .def("_lane_history",
             [](VectorEngineHost &e, int env) {  // test hook: cfx_get_lane_history, one environment's lanes; as Engine._lane_history
                 std::vector<int32_t> len, num, hn;
                 std::vector<double> avg, ha;
                 e.laneHistory(env, len, num, avg, hn, ha);
                 py::dict d;
                 d["len"] = toArray(len);
                 d["vehicle_num"] = toArray(num);
                 d["average_speed"] = toArray(avg);
                 d["history_vehicle_num"] = toArray(hn);
                 d["history_average_speed"] = toArray(ha);
                 return d;
             },
             "env"_a);
    vectorClass.def("_intersection_features", [](VectorEngineHost &e) { return intersectionFeaturesTuple(e, e.numEnvs()); },
                    "(phase, remain, in, in_waiting, out, inside, phase_pressure), flat, env-major");

    using cfa::TiledEngineHost;
    py::class_<TiledEngineHost>(m, "TiledEngine",
                                "One road network cut into rows x cols tiles of intersections, one device engine per tile, a "
                                "one-lane halo exchanged per step.  With local_tiles empty every tile runs in this process "
                                "(next_step does the exchange); otherwise the caller moves the halo between step_begin and "
                                "step_end (cityflow_amd.tiled.DistributedEngine does it over torch.distributed).")
        .def(py::init<const std::string &, int, int, const std::vector<int> &, const std::string &>(), "config_file"_a,
             "rows"_a, "cols"_a, "local_tiles"_a = std::vector<int>(), "backend_library"_a = "")
        .def("next_step", &TiledEngineHost::nextStep)
        .def("step_begin", &TiledEngineHost::stepBegin)
        .def("step_end", &TiledEngineHost::stepEnd)
        .def("enable_mailboxes", &TiledEngineHost::enableMailboxes, "job_id"_a,
             "Exchange the halo device to device through shared-memory mailboxes (all tiles on one node); job_id must "
             "be unique per job and equal on every process")
        .def("unlink_mailboxes", &TiledEngineHost::unlinkMailboxes)
        .def("enable_device_mailboxes", &TiledEngineHost::enableDeviceMailboxes, "job_id"_a,
             "All tiles in this process: mailboxes in the receiving tile's device memory (peer HBM); False if not possible here")
        .def("device_mailbox_phase", &TiledEngineHost::deviceMailboxPhase, "job_id"_a, "phase"_a,
             "One tile per process: phase 1 (allocate + publish), a barrier, phase 2 (open + attach); False = not possible")
        .def("halo_transport", &TiledEngineHost::haloTransport)
        .def("device_mailboxes_fine_grained", &TiledEngineHost::deviceMailboxesFineGrained,
             "False if a device mailbox fell back to a plain allocation (safe only while every tile is on the same device)")
        .def("device_identities", &TiledEngineHost::deviceIdentities,
             "Physical device of each local tile (PCI bus id; \"cpu\" on the CPU twin): equal strings = one shared device")
        .def("halo_device_buffers", [](TiledEngineHost &e, int i) { return e.haloDeviceBuffers(i); }, "i"_a,
             "(send pointer, send bytes, recv pointer, recv bytes) of local tile i's device-resident halo messages")
        .def("step_begin_device", &TiledEngineHost::stepBeginDevice, "step_begin with the halo left in the device buffers")
        .def("step_end_device", &TiledEngineHost::stepEndDevice, "step_end importing from the device buffers")
        .def_property_readonly("num_tiles", &TiledEngineHost::nTiles)
        .def_property_readonly("num_local", &TiledEngineHost::nLocal)
        .def("local_rank", &TiledEngineHost::localRank, "i"_a)
        .def("peers",
             [](TiledEngineHost &e, int i) {
                 py::list out;
                 for (const cfa::TilePeer &p : e.peers(i))
                     out.append(py::make_tuple(p.rank, p.sendOff, p.sendBytes, p.recvOff, p.recvBytes));
                 return out;
             },
             "i"_a, "[(peer tile, send offset, send bytes, recv offset, recv bytes)] of local tile i")
        // zero-copy views of the halo staging buffers of local tile i (valid while the engine lives)
        .def("send_buffer",
             [](py::object self, int i) {
                 auto &e = self.cast<TiledEngineHost &>();
                 auto &b = e.sendBuffer(i);
                 return py::array_t<uint8_t>({(py::ssize_t) b.size()}, {1}, (const uint8_t *) b.data(), self);
             },
             "i"_a)
        .def("recv_buffer",
             [](py::object self, int i) {
                 auto &e = self.cast<TiledEngineHost &>();
                 auto &b = e.recvBuffer(i);
                 return py::array_t<uint8_t>({(py::ssize_t) b.size()}, {1}, (const uint8_t *) b.data(), self);
             },
             "i"_a)
        .def("get_vehicle_count", &TiledEngineHost::getVehicleCount)
        .def("get_vehicles", &TiledEngineHost::getVehicles, "include_waiting"_a = false)
        .def("get_lane_vehicles", &TiledEngineHost::getLaneVehicles)
        .def("get_vehicle_speed", &TiledEngineHost::getVehicleSpeed)
        .def("get_vehicle_distance", &TiledEngineHost::getVehicleDistance)
        .def("get_vehicle_info", &TiledEngineHost::getVehicleInfo, "vehicle_id"_a)
        .def("get_leader", &TiledEngineHost::getLeader, "vehicle_id"_a)
        .def("get_average_travel_time", &TiledEngineHost::getAverageTravelTime)
        .def("push_vehicle", &TiledEngineHost::pushVehicle)
        .def("set_vehicle_speed", &TiledEngineHost::setVehicleSpeed, "vehicle_id"_a, "speed"_a)
        .def("set_random_seed", &TiledEngineHost::setRandomSeed, "seed"_a)
        .def("get_lane_vehicle_count", &TiledEngineHost::getLaneVehicleCount)
        .def("get_lane_waiting_vehicle_count", &TiledEngineHost::getLaneWaitingVehicleCount)
        .def("get_lane_vehicle_count_array", [](TiledEngineHost &e) { return toArray(e.laneVehicleCountArray()); })
        .def("get_lane_waiting_vehicle_count_array", [](TiledEngineHost &e) { return toArray(e.laneWaitingVehicleCountArray()); })
        .def("get_current_time", &TiledEngineHost::getCurrentTime)
        .def("set_tl_phase", &TiledEngineHost::setTrafficLightPhase, "intersection_id"_a, "phase_id"_a)
        .def("set_tl_phases",
             [](TiledEngineHost &e, py::array_t<int32_t, py::array::c_style | py::array::forcecast> phases) {
                 e.setTrafficLightPhases(std::vector<int32_t>(phases.data(), phases.data() + phases.size()));
             },
             "phases"_a)
        .def("reset", &TiledEngineHost::reset, "seed"_a = false)
        .def("sync", &TiledEngineHost::sync)
        .def("lane_ids", &TiledEngineHost::laneIds)
        .def("owner", &TiledEngineHost::owner, "owning tile of every intersection (index order of the roadnet file)")
        .def("snapshot", &TiledEngineHost::snapshot, "Archive of the whole network (every tile in this process)")
        .def("load", &TiledEngineHost::load, "archive"_a, "every process loads the same archive and keeps its tiles' part")
        .def("load_from_file", &TiledEngineHost::loadFromFile, "path"_a)
        .def("set_vehicle_route", &TiledEngineHost::setRoute, "vehicle_id"_a, "route"_a)
        .def("set_replay_file", &TiledEngineHost::setReplayLogFile, "replay_file"_a)
        .def("set_save_replay", &TiledEngineHost::setSaveReplay, "open"_a)
        .def("_pending_pushed_keyed", &TiledEngineHost::pendingPushedKeyed,
             "(priority, id) of the vehicles pushed since the last step: every rank holds the same ones")
        .def("_vehicles_keyed", &TiledEngineHost::vehiclesKeyed, "include_waiting"_a = false, "local (priority, id) pairs")
        .def("_runs_here", &TiledEngineHost::runsHere, "vehicle_id"_a)
        .def("_local_status", [](TiledEngineHost &e) { return toArray(e.localStatus()); })
        .def("_average_travel_time_from",
             [](TiledEngineHost &e, double cumulative, int64_t finished, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> st) {
                 return e.averageTravelTimeFrom(cumulative, finished, std::vector<uint8_t>(st.data(), st.data() + st.size()));
             },
             "cumulative"_a, "finished"_a, "status"_a)
        .def("_wants_replay", &TiledEngineHost::wantsReplay)
        .def("_replay_part", [](TiledEngineHost &e) { return py::bytes(e.replayPart()); })
        .def("_replay_write",
             [](TiledEngineHost &e, const std::vector<py::bytes> &parts) {
                 std::vector<std::string> blobs;
                 for (const py::bytes &b : parts) blobs.push_back((std::string) b);
                 e.replayWrite(blobs);
             },
             "parts"_a)
        .def("_compact_vehicles", &TiledEngineHost::compactVehicles,
             "forget the finished vehicles now (every tile in this process; automatic once \"cfx\": {\"compactVehicles\": N} vehicles have been created; default 3.5 M)")
        .def("_keeps_lane_history", &TiledEngineHost::keepsLaneHistory)
        .def("_wants_compaction", &TiledEngineHost::wantsCompaction, "enough vehicles created since the last time (the same answer on every rank)")
        .def("_compact_from_parts",
             [](TiledEngineHost &e, const std::vector<py::bytes> &parts) {
                 std::vector<std::string> p;
                 for (const auto &b : parts) p.push_back(std::string(b));
                 e.compactFromParts(p);
             },
             "parts"_a, "several processes: _snapshot_part() of every rank in rank order, the same call on every rank")
        .def("_vehicle_table", [](TiledEngineHost &e) { return py::make_tuple(e.vehicleTableSize(), e.vehicleCompactions()); },
             "(vehicle numbers the host holds, compactions so far)")
        .def("_snapshot_part", [](TiledEngineHost &e) { return py::bytes(e.snapshotPart()); },
             "the state of this process's tiles, for _snapshot_from_parts on every process (in rank order)")
        .def("_snapshot_from_parts",
             [](TiledEngineHost &e, const std::vector<py::bytes> &parts) {
                 std::vector<std::string> blobs;
                 for (const py::bytes &b : parts) blobs.push_back((std::string) b);
                 return e.snapshotFromParts(blobs);
             },
             "parts"_a)
        .def("_set_status_reducer", &TiledEngineHost::setStatusReducer, "fn"_a)
        .def("_host_seconds", &TiledEngineHost::hostSeconds,
             "(spawner, submit) cumulative host wall seconds of this process since the last reset")
        .def("_ahead_stats", &TiledEngineHost::aheadStats, "(batches taken from the step-ahead thread, batches made by the step itself, the thread's busy seconds)")
        .def("_profile_enable", &TiledEngineHost::profileEnable, "local_tile"_a, "on"_a)
        .def("_device_spin", &TiledEngineHost::deviceSpin, "microseconds"_a)
        .def("backend_name", &TiledEngineHost::backendName)
        .def("_layout", &TiledEngineHost::layoutName)
        .def("_profile_read", &TiledEngineHost::profileRead, "local_tile"_a)
        .def("_vehicle_state",
             [](TiledEngineHost &e) {
                 cfa::VehicleSnapshot s;
                 e.snapshotVehicles(s);
                 py::dict d;
                 d["vid"] = toArray(s.vid);
                 d["drivable"] = toArray(s.drivable);
                 d["prev_drivable"] = toArray(s.prevDrivable);
                 d["leader"] = toArray(s.leader);
                 d["blocker"] = toArray(s.blocker);
                 d["enter_ll_time"] = toArray(s.enterLLTime);
                 d["route_pos"] = toArray(s.routePos);
                 d["dis"] = toArray(s.dis);
                 d["speed"] = toArray(s.speed);
                 d["gap"] = toArray(s.gap);
                 return d;
             })
        .def("_scalars", [](TiledEngineHost &e) {
            cfx_scalars s = e.scalars();
            py::dict d;
            d["step"] = s.step;
            d["active_vehicle_count"] = s.active_vehicle_count;
            d["finished_vehicle_count"] = s.finished_vehicle_count;
            d["spawned_vehicle_count"] = s.spawned_vehicle_count;
            d["cumulative_travel_time"] = s.cumulative_travel_time;
            d["live_enter_time_sum"] = s.live_enter_time_sum;
            d["vehicle_steps"] = s.vehicle_steps;
                 d["tie_events"] = s.tie_events;
            return d;
        });

    py::class_<cfa::Archive>(m, "Archive")
        .def(py::init([](EngineHost &e) { return e.snapshot(); }), "engine"_a)
        .def("dump", &cfa::Archive::dump, "path"_a)
        .def_readonly("_last_dump_inexact", &cfa::Archive::lastDumpInexact,
                      "numbers of the last dump() the reference's JSON reader cannot be made to return exactly (written with 17 digits)");

    m.def("_load_roadnet", &loadRoadnet, "path"_a);
    m.def("_roadnet_probe", &roadnetProbe, "path"_a);
    m.def("_spawn_schedule", &spawnSchedule, "roadnet_file"_a, "flow_file"_a, "interval"_a, "seed"_a, "thread_num"_a,
          "steps"_a, "ahead"_a = 0);
    m.def("_spawn_benchmark", &spawnBenchmark, "roadnet_file"_a, "flow_file"_a, "interval"_a, "seed"_a, "skip"_a, "steps"_a);
    m.def("_default_backend_path", &cfa::defaultBackendPath);
    // test hooks: the host's number reader (the reference's: rapidjson's default, json_number.h) and Archive.dump's writer
    m.def("_parse_json_number", [](const std::string &lit) {
        cfa::Json v = cfa::Json::parseText(lit);
        if (!v.isNumber()) throw std::runtime_error("not a number");
        return py::make_tuple(v.asDouble(), v.integral);
    });
    m.def("_format_json_number", &cfa::formatJsonNumber);
    m.def("_inexact_json_numbers", &cfa::inexactJsonNumbers);
#ifdef CITYFLOW_AMD_VERSION
    m.attr("__version__") = CITYFLOW_AMD_VERSION;
#else
    m.attr("__version__") = "dev";
#endif
}
