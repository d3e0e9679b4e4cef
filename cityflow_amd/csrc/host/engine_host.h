// C++ host of the drop-in `cityflow.Engine` (reference src/engine/engine.h:114-183, bound by
// src/cityflow.cpp:11-38).  It keeps everything that involves strings, JSON and the mt19937 stream on
// the CPU and drives the device engine exclusively through the C ABI of include/cityflow_amd.h, which
// it resolves from a shared library at run time:
//   * default: <package dir>/lib/libcfx_hip.so  — the HIP/gfx950 implementation (the product);
//   * tests may name another library exporting the same ABI (the CPU twin under oracle/).
// There is no CPU fallback: if the library cannot be loaded or cfx_create fails the constructor throws.
#pragma once

#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "archive.h"
#include "cityflow_amd.h"
#include "flow.h"
#include "trackers.h"
#include "replay.h"
#include "roadnet.h"

namespace cfa {

struct Backend {
    void *handle = nullptr;
    std::string path;
#define CFX_FN(name) decltype(&::name) name = nullptr;
    CFX_FN(cfx_abi_version)
    CFX_FN(cfx_create)
    CFX_FN(cfx_destroy)
    CFX_FN(cfx_last_error)
    CFX_FN(cfx_backend_name)
    CFX_FN(cfx_add_templates)
    CFX_FN(cfx_add_routes)
    CFX_FN(cfx_step)
    CFX_FN(cfx_sync)
    CFX_FN(cfx_reset)
    CFX_FN(cfx_set_tl_phase)
    CFX_FN(cfx_set_tl_phases)
    CFX_FN(cfx_get_tl_state)
    CFX_FN(cfx_get_scalars)
    CFX_FN(cfx_get_layout)
    CFX_FN(cfx_get_ring_info)
    CFX_FN(cfx_get_lane_counts)
    CFX_FN(cfx_get_lane_waiting_counts)
    CFX_FN(cfx_get_vehicles)
    CFX_FN(cfx_get_waiting)
    CFX_FN(cfx_get_vehicle_status)
    CFX_FN(cfx_set_vehicle_speed)
    CFX_FN(cfx_set_vehicle_route)
    CFX_FN(cfx_get_vehicle)
    CFX_FN(cfx_load_state)
    CFX_FN(cfx_get_custom_speeds)
    CFX_FN(cfx_lane_change_supply)
    CFX_FN(cfx_lane_change_poll)
    CFX_FN(cfx_halo_config)
    CFX_FN(cfx_halo_export)
    CFX_FN(cfx_halo_import)
    CFX_FN(cfx_halo_attach)
    CFX_FN(cfx_halo_mailbox_alloc)
    CFX_FN(cfx_halo_mailbox_open)
    CFX_FN(cfx_halo_mailbox_fine_grained)
    CFX_FN(cfx_device_identity)
    CFX_FN(cfx_device_memory)
    CFX_FN(cfx_halo_device_buffers)
    CFX_FN(cfx_halo_post)
    CFX_FN(cfx_halo_wait)
    CFX_FN(cfx_profile_kernel_count)
    CFX_FN(cfx_profile_kernel_name)
    CFX_FN(cfx_profile_enable)
    CFX_FN(cfx_profile_read)
    CFX_FN(cfx_profile_kernel_symbol)
    CFX_FN(cfx_get_host_stats)
    CFX_FN(cfx_device_spin)
    CFX_FN(cfx_get_lane_history)
    CFX_FN(cfx_set_lane_history)
#undef CFX_FN
    // optional (looked up without requiring them): observations and signals in device memory
    cfx_stream_handle_fn cfx_stream_handle = nullptr;
    cfx_observe_lanes_device_fn cfx_observe_lanes_device = nullptr;
    cfx_set_tl_phases_device_fn cfx_set_tl_phases_device = nullptr;
    cfx_device_error_fn cfx_device_error = nullptr;
    bool hasDeviceBuffers() const {
        return cfx_stream_handle && cfx_observe_lanes_device && cfx_set_tl_phases_device && cfx_device_error;
    }
    // optional on its own: speed sums and bins into host memory (without it the host computes them from cfx_get_vehicles)
    cfx_get_lane_features_fn cfx_get_lane_features = nullptr;
    // optional, each on its own: every lane observation through one descriptor, the front vehicles among them (without the
    // first the tensor calls have no front outputs; without the second the host takes them from cfx_get_vehicles)
    cfx_observe_lane_obs_device_fn cfx_observe_lane_obs_device = nullptr;
    cfx_get_lane_obs_fn cfx_get_lane_obs = nullptr;
    // optional on its own: per-vehicle rows in device memory (without it the host fills them from cfx_get_vehicles: vehicleRowsOf)
    cfx_observe_vehicles_device_fn cfx_observe_vehicles_device = nullptr;
    // optional beside it: the drivables' polylines for that call's pose outputs (without it the host computes them: vehiclePosesOf)
    cfx_set_drivable_geometry_fn cfx_set_drivable_geometry = nullptr;
    bool hasVehiclePoses() const { return hasDeviceBuffers() && cfx_observe_vehicles_device && cfx_set_drivable_geometry; }
    // optional as a pair: speed commands for many vehicles at once (without them the host commands row by row: setVehicleSpeedsOf)
    cfx_set_vehicle_speeds_device_fn cfx_set_vehicle_speeds_device = nullptr;
    cfx_set_vehicle_speeds_fn cfx_set_vehicle_speeds = nullptr;
    cfx_get_waiting_custom_speeds_fn cfx_get_waiting_custom_speeds = nullptr;
    // optional as a set: route changes for many vehicles at once and the routes they hold (without them there is no such
    // call: cfx_set_vehicle_route restarts the cursor and cannot stand in)
    cfx_set_vehicle_routes_device_fn cfx_set_vehicle_routes_device = nullptr;
    cfx_set_vehicle_routes_fn cfx_set_vehicle_routes = nullptr;
    cfx_get_vehicle_routes_device_fn cfx_get_vehicle_routes_device = nullptr;
    cfx_get_vehicle_routes_fn cfx_get_vehicle_routes = nullptr;
    bool hasVehicleRoutes() const {
        return cfx_set_vehicle_routes_device && cfx_set_vehicle_routes && cfx_get_vehicle_routes_device && cfx_get_vehicle_routes;
    }
    // optional as a pair: per-intersection observations (without them the host computes the arrays from the getters above)
    cfx_observe_intersections_device_fn cfx_observe_intersections_device = nullptr;
    cfx_get_intersection_features_fn cfx_get_intersection_features = nullptr;
    // optional as a set: per-lane flow statistics kept by the backend (without them the host keeps them: lane_flow.h)
    cfx_lane_flow_enable_fn cfx_lane_flow_enable = nullptr;
    cfx_observe_lane_flow_device_fn cfx_observe_lane_flow_device = nullptr;
    cfx_get_lane_flow_fn cfx_get_lane_flow = nullptr;
    cfx_lane_flow_get_state_fn cfx_lane_flow_get_state = nullptr;
    cfx_lane_flow_set_state_fn cfx_lane_flow_set_state = nullptr;
    // optional as a set: per-environment trip statistics kept by the backend (without them the host keeps them: trip_stats.h)
    cfx_trip_stats_enable_fn cfx_trip_stats_enable = nullptr;
    cfx_observe_trip_stats_device_fn cfx_observe_trip_stats_device = nullptr;
    cfx_get_trip_stats_fn cfx_get_trip_stats = nullptr;
    cfx_trip_stats_get_state_fn cfx_trip_stats_get_state = nullptr;
    cfx_trip_stats_set_state_fn cfx_trip_stats_set_state = nullptr;
    // optional as a set beside them: the trip log, one row per finished vehicle (without them the host tracker keeps it too)
    cfx_trip_log_enable_fn cfx_trip_log_enable = nullptr;
    cfx_observe_trip_log_device_fn cfx_observe_trip_log_device = nullptr;
    cfx_get_trip_log_fn cfx_get_trip_log = nullptr;
    cfx_trip_log_set_state_fn cfx_trip_log_set_state = nullptr;
    // optional as a set: per-movement flow statistics kept by the backend (without them the host keeps them: movement_flow.h)
    cfx_movement_flow_enable_fn cfx_movement_flow_enable = nullptr;
    cfx_observe_movement_flow_device_fn cfx_observe_movement_flow_device = nullptr;
    cfx_get_movement_flow_fn cfx_get_movement_flow = nullptr;
    cfx_movement_flow_get_state_fn cfx_movement_flow_get_state = nullptr;
    cfx_movement_flow_set_state_fn cfx_movement_flow_set_state = nullptr;
    // optional as a set: virtual loop detectors kept by the backend (without them the host keeps them: detectors.h)
    cfx_detectors_define_fn cfx_detectors_define = nullptr;
    cfx_detectors_enable_fn cfx_detectors_enable = nullptr;
    cfx_observe_detectors_device_fn cfx_observe_detectors_device = nullptr;
    cfx_get_detectors_fn cfx_get_detectors = nullptr;
    cfx_detectors_get_state_fn cfx_detectors_get_state = nullptr;
    cfx_detectors_set_state_fn cfx_detectors_set_state = nullptr;
    // optional as a set: the fixed-time signal plan as engine state (without them there is no such call: TlPlan below)
    cfx_set_tl_plan_device_fn cfx_set_tl_plan_device = nullptr;
    cfx_set_tl_plan_fn cfx_set_tl_plan = nullptr;
    cfx_get_tl_phase_durations_device_fn cfx_get_tl_phase_durations_device = nullptr;
    cfx_get_tl_phase_durations_fn cfx_get_tl_phase_durations = nullptr;
    cfx_restore_tl_plan_fn cfx_restore_tl_plan = nullptr;
    cfx_tl_plan_error_fn cfx_tl_plan_error = nullptr;
    // optional as a set: the lanes' speed limits as engine state (without them there is no such call: LaneLimits below)
    cfx_set_lane_speed_limits_device_fn cfx_set_lane_speed_limits_device = nullptr;
    cfx_set_lane_speed_limits_fn cfx_set_lane_speed_limits = nullptr;
    cfx_get_lane_speed_limits_device_fn cfx_get_lane_speed_limits_device = nullptr;
    cfx_get_lane_speed_limits_fn cfx_get_lane_speed_limits = nullptr;
    cfx_restore_lane_speed_limits_fn cfx_restore_lane_speed_limits = nullptr;
    cfx_get_cross_stats_fn cfx_get_cross_stats = nullptr;  // (a library without it: crossStats() reports nothing)
    // optional as a set: checkpoints in device memory (without them there is no such call: DeviceCheckpoint below)
    cfx_checkpoint_create_fn cfx_checkpoint_create = nullptr;
    cfx_checkpoint_save_fn cfx_checkpoint_save = nullptr;
    cfx_checkpoint_restore_fn cfx_checkpoint_restore = nullptr;
    cfx_checkpoint_info_fn cfx_checkpoint_info = nullptr;
    cfx_checkpoint_destroy_fn cfx_checkpoint_destroy = nullptr;
    cfx_checkpoint_restore_envs_fn cfx_checkpoint_restore_envs = nullptr;  // (optional beside them: VectorEngine::rollback(ck, envs))
    bool hasCheckpoints() const {
        return cfx_checkpoint_create && cfx_checkpoint_save && cfx_checkpoint_restore && cfx_checkpoint_info && cfx_checkpoint_destroy;
    }
    bool hasTlPlan() const {
        return hasDeviceBuffers() && cfx_set_tl_plan_device && cfx_set_tl_plan && cfx_get_tl_phase_durations_device &&
               cfx_get_tl_phase_durations && cfx_restore_tl_plan && cfx_tl_plan_error;
    }
    bool hasLaneLimits() const {
        return hasDeviceBuffers() && cfx_set_lane_speed_limits_device && cfx_set_lane_speed_limits && cfx_get_lane_speed_limits_device &&
               cfx_get_lane_speed_limits && cfx_restore_lane_speed_limits;
    }
    void open(const std::string &libPath);  // throws std::runtime_error
    ~Backend();
};

// Per-vehicle state downloaded from the device, in Drivable::vehicles order.
enum SnapshotField : unsigned {  // what snapshotVehicles should fetch besides the vehicle ids
    kSnapDrivable = 1, kSnapPrev = 2, kSnapLeader = 4, kSnapBlocker = 8, kSnapEnterLL = 16, kSnapRoutePos = 32,
    kSnapDis = 64, kSnapSpeed = 128, kSnapGap = 256, kSnapAll = 511,
    kSnapLaneChange = 512  // partner / flags / offset / lastDir (always fetched when the engine runs with laneChange)
};

struct VehicleSnapshot {
    std::vector<int32_t> vid, drivable, prevDrivable, leader, blocker, enterLLTime, routePos;
    std::vector<double> dis, speed, gap;
    std::vector<int32_t> lcPartner, lcLastDir, lcTarget, lcDirection;  // lane change (empty unless kSnapLaneChange)
    std::vector<uint8_t> lcFlags;               // CFX_LC_* bits
    std::vector<double> lcOffset, lcLastChangeTime, lcWaitingTime;
    int count = 0;
    bool isShadow(int i) const { return !lcFlags.empty() && (lcFlags[i] & CFX_LC_SHADOW); }
};

// The static tables behind the per-intersection observations, of ONE environment: intersection i has nRoadLinks[i] roadLinks
// (rows padded to M) and nPhases[i] phases (-1 = virtual; rows padded to P); IN / OUT lanes of a roadLink are the distinct start /
// end lanes of its laneLinks, ascending, -1 padded to Kin / Kout.
struct InterLayout {
    int I = 0, M = 0, P = 0, Kin = 0, Kout = 0;
    std::vector<int32_t> nRoadLinks, nPhases;  // [I]
    std::vector<uint8_t> phaseAvail;           // [I * P * M]
    std::vector<int32_t> roadLinkType;         // [I * M] 0 = padding
    std::vector<int32_t> inLanes, outLanes;    // [I * M * Kin], [I * M * Kout]
    std::vector<int32_t> llRow;                // [n_lanelinks] i * M + m of the laneLink's roadLink
};
InterLayout intersectionLayoutOf(const HostRoadNet &net);
// the seven outputs of cfx_observe_intersections_device in host memory ([nEnvs * I], [nEnvs * I * M], [nEnvs * I * P]; any may be null)
struct InterFeatures {
    int32_t *phase = nullptr;
    double *remain = nullptr;
    int32_t *in = nullptr, *inWaiting = nullptr, *out = nullptr, *inside = nullptr, *pressure = nullptr;
};
// ... on any backend: cfx_get_intersection_features where it exists, otherwise from cfx_get_lane_counts,
// cfx_get_lane_waiting_counts, cfx_get_vehicles (drivable column) and cfx_get_tl_state (throws std::runtime_error with the
// backend's message).  `lay`: one environment's layout, `nLanes` / `nLaneLinks`: of one environment
void intersectionFeaturesOf(const Backend &be, cfx_engine *dev, const InterLayout &lay, int nEnvs, int nLanes, int nLaneLinks,
                            const InterFeatures &out);

// The fixed-time signal plan as engine state (cfx_set_tl_plan_device and its kin; the public calls are cityflow_amd/torch_io.py):
// what EngineHost and VectorEngineHost share.  Arrays cover every environment, env-major: durations [nEnvs * I * P] (P = the
// largest phase count of a signalised intersection), phase / remain [nEnvs * I]; any of the three may be null.  The caller
// holds whatever lock its ABI calls need.  A backend without the entry points: std::logic_error from every call.
class TlPlan {
public:
    void bind(const Backend *be, cfx_engine *dev, const HostRoadNet *net, int nEnvs, bool namesEnv);
    bool available() const { return be_ && be_->hasTlPlan(); }
    int maxPhases() const { return P_; }
    // device addresses, ordered against the caller's stream; a rejected call shows in raise() once the device has run it
    void setDevice(uintptr_t durations, uintptr_t phase, uintptr_t remain, uintptr_t producerStream);
    void durationsDevice(uintptr_t out, uintptr_t consumerStream);
    // host memory, synchronous: set() throws at once what raise() would
    void set(const double *durations, const int32_t *phase, const double *remain);
    void durations(double *out);
    void restore();
    bool unchecked() const { return unchecked_; }
    // after a call that has waited for the device: std::invalid_argument naming the entry that rejected a set call
    void raise();

private:
    void need(const char *what) const;
    void check(int32_t rc, const char *what) const;
    const Backend *be_ = nullptr;
    cfx_engine *dev_ = nullptr;
    const HostRoadNet *net_ = nullptr;
    int nEnvs_ = 1, I_ = 0, P_ = 0;
    bool namesEnv_ = false, unchecked_ = false;
};

// The lanes' speed limits as engine state (cfx_set_lane_speed_limits_device and its kin; the public calls are
// cityflow_amd/torch_io.py): what EngineHost and VectorEngineHost share.  Arrays cover every environment, env-major:
// [nEnvs * L] in lane_ids() order — the device network of a VectorEngine is nEnvs concatenated copies, so they pass straight
// through.  The caller holds whatever lock its ABI calls need.  A backend without the entry points: std::logic_error.
class LaneLimits {
public:
    void bind(const Backend *be, cfx_engine *dev, int nLanesAllEnvs) {
        be_ = be;
        dev_ = dev;
        n_ = nLanesAllEnvs;
    }
    bool available() const { return be_ && be_->hasLaneLimits(); }
    int size() const { return n_; }
    // device addresses, ordered against the caller's stream (rejected: 0 or one int32)
    void setDevice(uintptr_t limits, uintptr_t rejected, uintptr_t producerStream);
    void getDevice(uintptr_t out, uintptr_t consumerStream);
    // host memory, synchronous
    int32_t set(const double *limits);  // the number of rejected entries
    void get(double *out);
    void restore();

private:
    void need(const char *what) const;
    void check(int32_t rc, const char *what) const;
    const Backend *be_ = nullptr;
    cfx_engine *dev_ = nullptr;
    int n_ = 0;
};

// the four front-vehicle outputs in host memory ([n_lanes * k] each, of every environment; any may be null)
struct LaneFronts {
    double *distance = nullptr, *speed = nullptr;
    int32_t *laneSteps = nullptr, *waitingSteps = nullptr;
};

// The running vehicles as cfx_get_vehicles lists them (ordered by drivable, front to back inside one): the columns asked for.
struct VehicleColumns {
    std::vector<int32_t> vid, drivable;
    std::vector<double> dis, speed;
    int count = 0;
};
VehicleColumns vehicleColumnsOf(const Backend &be, cfx_engine *dev, bool vid, bool dis, bool speed);  // (drivable always)

// Every running vehicle as a row, in CSR form (cfx_observe_vehicles_device's outputs and order, include/cityflow_amd.h): the
// rows by environment, then by drivable within it (lanes, then laneLinks), front to back; start [nEnvs * (D + 1)].
struct VehicleRows {
    std::vector<int32_t> start, vehicle, drivable, env, leader;
    std::vector<double> distance, speed, gap;
    std::vector<double> x, y, dirX, dirY, length, width;  // the pose columns: empty until vehiclePosesOf fills them
    int count = 0;
};
// The polylines of ONE environment's drivables, lanes first and then laneLinks (the rows' drivable numbering): drivable d has
// the points pointStart[d] .. pointStart[d + 1] - 1 of xy ({x, y} pairs), exactly the doubles the loader computed.
struct DrivableGeometry {
    std::vector<int32_t> pointStart;  // [D + 1]
    std::vector<double> xy;           // [2 * P]
};
DrivableGeometry drivableGeometryOf(const HostRoadNet &net);
// The pose columns of `rows` from its drivable and distance columns (host/polyline.h: the replay writer's two walks) and the
// template of every row's vehicle (templateOf(vehicle number)); what the twin returns and the device's kernels are compared with.
void vehiclePosesOf(VehicleRows &rows, const HostRoadNet &net, const std::function<const cfx_vehicle_template &(int32_t)> &templateOf);
// cfx_set_drivable_geometry with the network's polylines, once per engine: the first call that gives a pose pointer
void uploadDrivableGeometryOf(const Backend &be, cfx_engine *dev, const HostRoadNet &net);
inline bool wantsPoses(const cfx_vehicle_rows &r) { return r.x || r.y || r.dir_x || r.dir_y || r.length || r.width; }
// ... on any backend, from cfx_get_vehicles (nLanes / nLaneLinks: of ONE environment; throws std::runtime_error)
VehicleRows vehicleRowsOf(const Backend &be, cfx_engine *dev, int nEnvs, int nLanes, int nLaneLinks);
// ... into device memory: every pointer of `rows` a device address (cfx_observe_vehicles_device)
void observeVehiclesDeviceOf(const Backend &be, cfx_engine *dev, const cfx_vehicle_rows &rows, uintptr_t consumerStream);

// Speed commands for n rows {vehicle number, speed} (cfx_set_vehicle_speeds_device's rules, include/cityflow_amd.h).  From device
// memory: every pointer a device address, `ignored` may be 0.  From host arrays, on any backend: over cfx_set_vehicle_speeds, or
// row by row over cfx_set_vehicle_speed with the vehicles alive taken from cfx_get_vehicles / cfx_get_waiting — and then the
// rows that commanded a vehicle still waiting are added to `waitingCommands` (may be null).  Returns the rows ignored.
void setVehicleSpeedsDeviceOf(const Backend &be, cfx_engine *dev, uintptr_t vehicle, uintptr_t speed, int n, uintptr_t ignored,
                              uintptr_t producerStream);
int setVehicleSpeedsOf(const Backend &be, cfx_engine *dev, const int32_t *vehicle, const double *speed, int n,
                       std::map<int32_t, double> *waitingCommands);

// Route changes for n rows {vehicle number, route handle} and the handles the vehicles hold (cfx_set_vehicle_routes_device's
// rules, include/cityflow_amd.h), from device memory (every pointer a device address, `status` and `ignored` may be 0) and
// from host arrays (`status` may be null; returns the rows refused; vehicle == null reads the numbers 0 .. n-1).  There is no
// row-by-row form over cfx_set_vehicle_route, which restarts a route at its first road: std::runtime_error naming the
// library on a backend without the entry points.
void setVehicleRoutesDeviceOf(const Backend &be, cfx_engine *dev, uintptr_t vehicle, uintptr_t route, int n, uintptr_t status,
                              uintptr_t ignored, uintptr_t producerStream);
int setVehicleRoutesOf(const Backend &be, cfx_engine *dev, const int32_t *vehicle, const int32_t *route, int n, int32_t *status);
void vehicleRoutesDeviceOf(const Backend &be, cfx_engine *dev, uintptr_t vehicle, int n, uintptr_t out, uintptr_t consumerStream);
void vehicleRoutesOf(const Backend &be, cfx_engine *dev, const int32_t *vehicle, int n, int32_t *out);

// A checkpoint in device memory (cfx_checkpoint_* of include/cityflow_amd.h; the public calls are checkpoint() / rollback() of
// cityflow_amd/torch_io.py), of an EngineHost or a VectorEngineHost: the backend's part, and what Engine.load() takes from an
// Archive on the host — the spawners' states (one per environment) and the step — plus what an Archive does not carry.  It
// belongs to the engine that took it and must not outlive it (the binding keeps the engine alive).
struct DeviceCheckpoint {
    const Backend *be = nullptr;
    cfx_checkpoint *ck = nullptr;  // null once released
    const void *owner = nullptr;   // the EngineHost / VectorEngineHost
    std::vector<Spawner::State> host;
    bool routesStale = false;  // the vehicles' routes in `host` were behind the device's (EngineHost::routesStale_)
    size_t step = 0;
    size_t nextCompactAt = 0;                                 // EngineHost::nextCompactAt_
    std::map<int32_t, double> waitingCustom;                  // EngineHost::waitingCustom_
    std::vector<std::vector<int32_t>> localToGlobal;          // VectorEngineHost's numbering
    std::vector<std::pair<int32_t, int32_t>> globalToLocal;
    DeviceCheckpoint() = default;
    DeviceCheckpoint(const DeviceCheckpoint &) = delete;
    DeviceCheckpoint &operator=(const DeviceCheckpoint &) = delete;
    ~DeviceCheckpoint() { release(); }
    bool released() const { return ck == nullptr; }
    void release();                     // frees the device memory; the checkpoint can no longer be rolled back to
    cfx_checkpoint_desc desc() const;   // (all zero once released)
    // what the two hosts share: argument checks (std::invalid_argument), then the backend's calls
    static void checkUsable(const DeviceCheckpoint *ck, const void *owner, const char *what);
};

class EngineHost {
public:
    EngineHost(const std::string &configFile, int threadNum, const std::string &backendLib = "");
    ~EngineHost();
    EngineHost(const EngineHost &) = delete;
    EngineHost &operator=(const EngineHost &) = delete;

    // ---- reference API (engine.h:139-182) ----
    void nextStep();
    size_t getVehicleCount();
    std::vector<std::string> getVehicles(bool includeWaiting);
    std::map<std::string, int> getLaneVehicleCount();
    std::map<std::string, int> getLaneWaitingVehicleCount();
    std::map<std::string, std::vector<std::string>> getLaneVehicles();
    std::map<std::string, double> getVehicleSpeed();
    std::map<std::string, double> getVehicleDistance();
    std::string getLeader(const std::string &vehicleId);
    std::map<std::string, std::string> getVehicleInfo(const std::string &vehicleId);
    double getCurrentTime() const { return step_ * interval_; }
    double getAverageTravelTime();
    void setTrafficLightPhase(const std::string &id, int phaseIndex);
    bool keepsLaneHistory() const { return laneHistory_; }
    void setTrafficLightPhaseOf(int inter, int phaseIndex);  // the same, the id already resolved to its index in net().inters
    void setRandomSeed(int seed) {
        dropAhead();
        settleLaneChange();  // (the pending shadow draws belong to the old stream)
        spawner_.seed(seed);
    }
    void pushVehicle(const std::map<std::string, double> &info, const std::vector<std::string> &roads);
    void reset(bool resetRnd);
    void setVehicleSpeed(const std::string &id, double speed);                        // engine.cpp:827-834
    bool setRoute(const std::string &vehicleId, const std::vector<std::string> &anchors);  // engine.cpp:852-866
    Archive snapshot() { return snapshotImpl(true); }  // engine.h:177
    // Forget the finished vehicles (archive.cpp).  Automatic, between two steps, once `compactAt_` vehicles have been created
    // since the last time ("cfx": {"compactVehicles": N}; default 3.5 M = before the device's vehicle tables would double; 0 = never).
    void compactVehicles();
    size_t vehicleTableSize() const { return spawner_.vehicles.size(); }
    int64_t vehicleCompactions() const { return vehicleCompactions_; }
    void load(const Archive &archive);         // engine.h:176
    void loadFromFile(const std::string &path);  // engine.cpp:822-825
    // ---- checkpoints in device memory (DeviceCheckpoint above; archive.cpp): as load(snapshot()), except that the vehicles
    //      keep their place in their routes and nothing per vehicle crosses the link
    bool checkpointCalls() const { return be_.hasCheckpoints(); }
    std::string checkpointUnsupported();  // why this engine has no device checkpoints ("" = it has)
    std::shared_ptr<DeviceCheckpoint> checkpoint(std::shared_ptr<DeviceCheckpoint> into);  // into: overwritten in place (may be null)
    void rollback(DeviceCheckpoint &ck);
    void setReplayLogFile(const std::string &logFile);  // engine.cpp:727-734
    void setSaveReplay(bool open);                       // engine.cpp:736-742

    // ---- array getters (no string marshalling; for large grids / RL observation tensors) ----
    std::vector<int32_t> laneVehicleCountArray();
    std::vector<int32_t> laneWaitingVehicleCountArray();
    std::vector<std::string> laneIds() const;          // index -> id for the two arrays above
    std::vector<std::string> roadIds() const;          // the roads in roadnet-file order (the trip log's road columns)
    const std::vector<int32_t> &laneIdOrder();         // lane indices in lexicographic id order (std::map order)
    std::vector<std::string> intersectionIds() const;
    void setTrafficLightPhaseIndexed(int inter, int phase);
    void setTrafficLightPhases(const std::vector<int32_t> &phases);  // [n_intersections]; virtual ones ignored
    void setTrafficLightPhases(const int32_t *phases, size_t n);
    void trafficLightState(std::vector<int32_t> &phase, std::vector<double> &remain);
    // ---- observations and signals in device memory (cfx_observe_lanes_device / cfx_set_tl_phases_device; the torch layer is
    //      cityflow_amd/torch_io.py).  Pointers are device addresses, streams hipStream_t of the engine's HIP runtime.
    bool deviceBuffers() const { return be_.hasDeviceBuffers(); }
    std::pair<uintptr_t, int> streamHandle();  // {engine's stream, its device}
    void setTrafficLightPhasesDevice(uintptr_t phases, size_t n, uintptr_t producerStream);
    bool rlTrafficLight() const { return rlTrafficLight_; }
    std::vector<int32_t> phaseCounts() const;  // [n_intersections] phases per intersection, -1 for virtual ones
    // ---- the fixed-time signal plan as engine state (TlPlan above): durations [I * P], phase / remain [I], any null
    bool tlPlanCalls() const { return plan_.available(); }
    void setTlPlanDevice(uintptr_t durations, uintptr_t phase, uintptr_t remain, uintptr_t producerStream);
    void setTlPlan(const double *durations, const int32_t *phase, const double *remain);
    void tlPhaseDurationsDevice(uintptr_t out, uintptr_t consumerStream) { plan_.durationsDevice(out, consumerStream); }
    void tlPhaseDurations(double *out);
    void restoreTlPlan() { plan_.restore(); }
    // ---- the lanes' speed limits as engine state (LaneLimits above): [L] in lane_ids() order
    bool laneLimitCalls() const { return limits_.available(); }
    int laneLimitCount() const { return limits_.size(); }
    void setLaneSpeedLimitsDevice(uintptr_t limits, uintptr_t rejected, uintptr_t producerStream) {
        limits_.setDevice(limits, rejected, producerStream);
    }
    int32_t setLaneSpeedLimits(const double *limits) { return limits_.set(limits); }
    void laneSpeedLimitsDevice(uintptr_t out, uintptr_t consumerStream) { limits_.getDevice(out, consumerStream); }
    void laneSpeedLimits(double *out) { limits_.get(out); }
    void restoreLaneSpeedLimits() { limits_.restore(); }
    // ---- per-lane speed and position features (cfx_observe_lanes_device / cfx_get_lane_features; the twin: from the vehicles)
    std::vector<double> laneLengths() const;  // [n_lanes] Lane::getLength
    // speedSum [n_lanes], bins [n_lanes * nBins] (either may be null), edges: [n_lanes][nBins + 1] or [nBins + 1]
    void laneFeatures(double *speedSum, int32_t *bins, const double *edges, int nBins, bool perLaneEdges);
    // every pointer of `obs` a device address (cfx_observe_lane_obs_device; without front outputs also cfx_observe_lanes_device)
    void observeLanesDevice(const cfx_lane_obs &obs, uintptr_t consumerStream);
    // ---- the first k vehicles of every lane from the front (cfx_get_lane_obs; the twin: from the vehicles and the host tracker).
    //      [n_lanes * k] each, any may be null; the two tracker columns need trackLaneFlow(true) (std::runtime_error)
    void laneFronts(int k, const LaneFronts &out);
    // ---- every running vehicle as a row (VehicleRows above; std::runtime_error with laneChange: shadows)
    bool vehicleRowsDevice() const { return be_.hasDeviceBuffers() && be_.cfx_observe_vehicles_device; }
    bool vehiclePosesDevice() const { return be_.hasVehiclePoses(); }  // (... its pose outputs too)
    std::pair<int, int> drivableCounts() const { return {(int) net_->lanes.size(), (int) net_->laneLinks.size()}; }
    DrivableGeometry drivableGeometry() const { return drivableGeometryOf(*net_); }
    VehicleRows vehicleRows(bool poses = false);
    void observeVehiclesDevice(const cfx_vehicle_rows &rows, uintptr_t consumerStream);
    // ---- speed commands for many vehicles at once, by the vehicle numbers of the rows above (setVehicleSpeedsOf above;
    //      std::runtime_error with laneChange).  A command the device takes for a vehicle still in its entry buffer is not
    //      in waitingCustom_: compactVehicles reads those back from the device (cfx_get_waiting_custom_speeds)
    bool vehicleSpeedsDevice() const { return be_.hasDeviceBuffers() && be_.cfx_set_vehicle_speeds_device; }
    void setVehicleSpeedsDevice(uintptr_t vehicle, uintptr_t speed, int n, uintptr_t ignored, uintptr_t producerStream);
    int setVehicleSpeeds(const int32_t *vehicle, const double *speed, int n);
    // ---- candidate routes named up front and route changes for many vehicles at once (cfx_set_vehicle_routes_device and its
    //      kin, include/cityflow_amd.h).  A handle is an index into spawner_.routes, flow routes included; the tables are
    //      never dropped, so it holds across reset, load, rollback and vehicle compaction.  addRoutes: std::invalid_argument
    //      naming the list's index for an unknown road or a route the reference calls invalid, and then nothing is added.
    //      The device calls leave spawner_.vehicles[v].route stale: routesStale_ is raised, and every reader of that record
    //      calls refreshRoutes() first (one bulk read through cfx_get_vehicle_routes).  std::runtime_error with laneChange
    //      and on a backend without the entry points
    std::vector<int> addRoutes(const std::vector<std::vector<std::string>> &routes);
    std::vector<std::string> routeRoads(int handle);
    int routeCount() { return spawner().routes.count(); }
    void setVehicleRoutesDevice(uintptr_t vehicle, uintptr_t route, int n, uintptr_t status, uintptr_t ignored, uintptr_t producerStream);
    int setVehicleRoutes(const int32_t *vehicle, const int32_t *route, int n, int32_t *status);  // returns the rows refused
    void vehicleRoutesDevice(uintptr_t vehicle, int n, uintptr_t out, uintptr_t consumerStream);
    void vehicleRoutes(const int32_t *vehicle, int n, int32_t *out);
    // ---- per-intersection movement and phase observations (cfx_observe_intersections_device / cfx_get_intersection_features;
    //      the twin: from the count getters, the vehicles and the lights).  Rows of layout().M roadLinks / layout().P phases
    const InterLayout &intersectionLayout();
    void intersectionFeatures(const InterFeatures &out);  // any pointer may be null
    void observeIntersectionsDevice(uintptr_t phase, uintptr_t remain, uintptr_t in, uintptr_t inWaiting, uintptr_t out,
                                    uintptr_t inside, uintptr_t pressure, int maxRoadLinks, int maxPhases, uintptr_t consumerStream);
    // ---- per-lane flow and waiting-time statistics across steps (lane_flow.h; the torch layer is cityflow_amd/torch_io.py).
    //      Off by default; a baseline when it is turned on and after reset / load; vehicle compaction carries it along
    // ---- per-movement flow and delay statistics across steps (movement_flow.h; the torch layer is cityflow_amd/torch_io.py):
    //      outputs [I * M], any pointer may be null
    void trackMovementFlow(bool on);
    bool movementFlowTracking() const { return trackers_.move.on(); }
    int movementFlowRows() const { return (int) trackers_.move.rows(); }
    void movementFlowFeatures(const MoveFlowOut &out, bool reset);
    void observeMovementFlowDevice(const MoveFlowOut &out, bool reset, uintptr_t consumerStream);
    void trackLaneFlow(bool on);
    bool laneFlowTracking() const { return trackers_.flow.on(); }
    void laneFlowFeatures(const LaneFlowOut &out, bool reset);  // any pointer may be null
    void observeLaneFlowDevice(const LaneFlowOut &out, bool reset, uintptr_t consumerStream);
    // ---- trip statistics and the average travel time across steps (trip_stats.h; the torch layer is cityflow_amd/torch_io.py).
    //      Off by default; a baseline when it is turned on and after reset / load; vehicle compaction carries it along
    void trackTrips(bool on);
    bool tripTracking() const { return trackers_.trip.on(); }
    void tripFeatures(const cfx_trip_stats_out &out);  // any pointer may be null; one element each
    void observeTripsDevice(const cfx_trip_stats_out &out, uintptr_t consumerStream);
    // the trip log, one row per finished vehicle (trip tracking must be on; capacity 0 drops it; outputs: columns [capacity])
    void trackTripLog(int64_t capacity);
    int32_t tripLogCapacity() const { return trackers_.trip.logCapacity(); }
    void tripLogFeatures(const cfx_trip_log_out &out, bool reset);  // any pointer may be null; host memory
    void observeTripLogDevice(const cfx_trip_log_out &out, bool reset, uintptr_t consumerStream);
    // ---- virtual loop detectors across steps (detectors.h; the torch layer is cityflow_amd/torch_io.py): `n` zones of lanes;
    //      outputs [n], any pointer may be null.  Defining turns the tracker on and takes a baseline
    void defineDetectors(const int32_t *lane, const double *start, const double *end, int n);
    void dropDetectors();
    const Detectors &detectors() const { return trackers_.det; }
    void detectorFeatures(const cfx_detectors_out &out, bool reset);
    void observeDetectorsDevice(const cfx_detectors_out &out, bool reset, uintptr_t consumerStream);
    // Lane::history as the device keeps it ("cfx": {"laneHistory": true}; cfx_get_lane_history): lane-major, oldest record first
    void laneHistory(std::vector<int32_t> &len, std::vector<int32_t> &vehicleNum, std::vector<double> &averageSpeed,
                     std::vector<int32_t> &historyVehicleNum, std::vector<double> &historyAverageSpeed);
    void snapshotVehicles(VehicleSnapshot &out, unsigned fields = kSnapAll);
    // changes whenever vehicle numbers are reassigned (reset, load): per-vehicle caches of a language binding key on it
    uint64_t vehicleEpoch() const { return vehicleEpoch_; }
    void waitingVehicles(std::vector<int32_t> &vid, std::vector<int32_t> &lane);
    cfx_scalars scalars();
    void sync();
    void profileEnable(bool on);
    void deviceSpin(long long microseconds) { check(be_.cfx_device_spin(dev_, microseconds), "cfx_device_spin"); }
    std::pair<long long, long long> deviceMemory() {  // {free, total} bytes of the engine's device
        int64_t f = 0, t = 0;
        check(be_.cfx_device_memory(dev_, &f, &t), "cfx_device_memory");
        return {(long long) f, (long long) t};
    }
    std::map<std::string, std::pair<double, int64_t>> profileRead();  // kernel -> (total ms, launches)
    std::map<std::string, std::string> profileSymbols();  // timing slot -> symbol of the kernel launched last in it
    cfx_host_stats hostStats(bool reset);
    bool crossStats(bool reset, cfx_cross_stats *out);  // kr_cross's grids (false: the library has no such entry point)
    // the slowest nextStep() since the last clearing read: total us, the step, and its parts {phases + lane-change settle, this
    // step's spawn records (taken or made), table upload + lane-change supply, cfx_step, replay log, the spawner of the step ahead}
    struct SlowestStep {
        double total = 0, part[6] = {};
        int64_t step = -1;
    };
    SlowestStep slowestStep(bool reset) {
        SlowestStep s = slowest_;
        if (reset) slowest_ = SlowestStep{};
        return s;
    }

    std::shared_ptr<void> bindingCache;  // opaque per-engine cache owned by the language binding (lane id key objects)

    const HostRoadNet &net() const { return *net_; }
    const Spawner &spawner() {  // (the state as of the last step: a step taken ahead is taken back first)
        dropAhead();
        return spawner_;
    }
    std::string backendName() const { return be_.cfx_backend_name ? be_.cfx_backend_name() : "?"; }
    std::pair<int64_t, int> ringInfo() {
        int64_t slots = 0;
        int32_t scale = 1;
        be_.cfx_get_ring_info(dev_, &slots, &scale);
        return {slots, scale};
    }
    std::string layoutName() {
        const int l = be_.cfx_get_layout(dev_);
        return l == CFX_LAYOUT_RING ? "ring" : (l == CFX_LAYOUT_DENSE ? "dense" : "n/a");
    }
    std::string vehicleId(int vid, bool shadow = false) const { return spawner_.vehicleId(vid, shadow); }
    bool laneChange() const { return laneChange_; }
    bool isPendingPushed(const std::string &id);
    int vidOf(const std::string &id);  // -1 if unknown
    double interval() const { return interval_; }
    size_t step() const { return step_; }

private:
    void check(int32_t rc, const char *what);
    void uploadNewTablesIfAny();
    // a device-side signal set was enqueued whose offender record has not been read since: every call below that has waited
    // for the device reads it (raiseDeviceError), and throws std::out_of_range naming the intersection it rejected
    bool devicePhaseUnchecked_ = false;
    void raiseDeviceError();  // (then a rejected plan: TlPlan::raise, std::invalid_argument)
    TlPlan plan_;
    LaneLimits limits_;

    std::shared_ptr<HostRoadNet> net_ = std::make_shared<HostRoadNet>();
    Spawner spawner_;
    Backend be_;
    cfx_engine *dev_ = nullptr;
    double interval_ = 1.0;
    bool rlTrafficLight_ = false, laneChange_ = false, saveReplay_ = false, saveReplayInConfig_ = false;
    Archive snapshotImpl(bool hostState);
    std::map<int32_t, double> waitingCustom_;  // set_vehicle_speed on vehicles that were waiting (or not yet numbered) then
    size_t compactAt_ = 3500000, nextCompactAt_ = 3500000;
    bool compactAuto_ = true;
    int64_t vehicleCompactions_ = 0;
    bool geometryUploaded_ = false;  // cfx_set_drivable_geometry was called (the first pose output asked for in device memory)
    bool laneHistory_ = false;  // "cfx": {"laneHistory": ...}; not said: kept on the ring layout up to 20 k lanes, not with lane change
    ReplayWriter replay_;
    void updateLog();  // Engine::updateLog engine.cpp:518-554
    int seed_ = 0, threadNum_ = 1;
    std::string dir_;
    size_t step_ = 0;
    int templatesUploaded_ = 0, routesUploaded_ = 0;
    std::vector<cfx_spawn> spawnBuf_;
    // The NEXT step's spawn records, computed right after this step was handed to the device (Spawner::beginAhead): consumed
    // by the next nextStep(), taken back (dropAhead) by every other call that could see or change the spawner's state.
    bool spawnAhead_ = true, aheadValid_ = false;
    SlowestStep slowest_;
    std::vector<cfx_spawn> aheadBuf_;
    void dropAhead();
    std::vector<int32_t> shadowPool_, shadowParents_;  // lane change: priorities offered to / parents reported by a step
    int shadowPoolSize_ = 1024;
    bool lcPollPending_ = false;
    void settleLaneChange();
    std::vector<int32_t> pendingPhaseInter_, pendingPhaseValue_;  // set_tl_phase calls since the last flush
    // rlTrafficLight: the phase the device shows at every intersection, as far as this host knows (-1: not known) — with agent
    // control nothing but these calls changes a phase (TrafficLight::passTime does not run, trafficlight.cpp:29-37), so an
    // agent that sets every signal every step uploads only the ones it actually changes; forgotten on reset / load
    std::vector<int32_t> knownPhase_;
    std::vector<int32_t> realInter_, realInterPhases_, changedInter_, changedPhase_;  // setTrafficLightPhases: the signals, scratch
    void forgetPhases() { knownPhase_.assign(knownPhase_.size(), -1); }
    // keeps of (inters, phases) what differs from knownPhase_ and records it; false: nothing left to send
    bool onlyChangedPhases(std::vector<int32_t> &inters, std::vector<int32_t> &phases);
    void flushPhases();
    std::vector<int32_t> laneIdOrder_;
    uint64_t vehicleEpoch_ = 0;
    std::unique_ptr<InterLayout> interLayout_;  // built by the first call that needs it
    Trackers trackers_;
    void tripNoteVehicles();  // (host tracker: the vehicle numbers created since the last call)
    void tripNote(int32_t vid);
    bool routesStale_ = false;  // a device-side route change since spawner_.vehicles[...].route was last read back
    void refreshRoutes();
};

struct EngineConfig {  // Engine::loadConfig engine.cpp:37-84
    double interval = 1.0;
    bool rlTrafficLight = false, laneChange = false, saveReplay = false;
    int seed = 0;
    std::string dir, roadnetFile, flowFile;
    std::string roadnetLogFile, replayLogFile;  // required with saveReplay (engine.cpp:73-77)
    // optional "cfx" object (ignored by the reference): implementation choices that never change results
    int crossMode = CFX_CROSS_AUTO, layout = CFX_LAYOUT_AUTO, debugSync = 0, device = -1, ringLanesPerWave = 0, ringCapacityPercent = 0, denseForm = 0;
    bool exactShadowPeek = false;  // host: Spawner::exactPeekOnly
    int laneHistory = -1;          // keep Lane::history on the device (cfx_config::lane_history): Archive dumps then carry it, as the
                                   // reference's do.  -1 = not said: Engine keeps it where it is nearly free (ring layout, up to 20 k
                                   // lanes, no lane change: engine_host.cpp), VectorEngine and TiledEngine (no Archive of it) do not
    int hostThreads = -1;          // VectorEngine: worker threads for the per-environment host work (-1 auto, 0 serial)
    int64_t compactVehicles = -1;  // Engine: forget the finished vehicles once this many have been created since the last time (-1: 3.5 M; 0: never)
    bool spawnAhead = true;        // Engine: run the spawner of step t+1 right after step t is handed to the device (EngineHost::nextStep)
    void apply(cfx_config &cc) const;  // interval, flags, the choices above, device (config > CITYFLOW_AMD_DEVICE > LOCAL_RANK)
};
EngineConfig readEngineConfig(const std::string &configFile);  // throws std::runtime_error("load config failed! ...")

std::string defaultBackendPath();  // <dir of this shared object>/lib/libcfx_hip.so

// Per-lane speed sum and position bins (cfx_get_lane_features's semantics) of every lane, on the host: from a vehicle view of
// `count` running vehicles ordered by drivable, front to back (cfx_get_vehicles).  Lane l's edge row: l % lanesPerEnv when
// perLaneEdges, else the one row.  Either output may be null.
void laneFeaturesFromView(int nLanes, int lanesPerEnv, int count, const int32_t *drivable, const double *dis, const double *speed,
                          double *speedSum, int32_t *bins, const double *edges, int nBins, bool perLaneEdges);
// the same on any backend: cfx_get_lane_features where it exists, otherwise cfx_get_vehicles + laneFeaturesFromView
// (throws std::runtime_error with the backend's message)
void laneFeaturesOf(const Backend &be, cfx_engine *dev, int nLanes, int lanesPerEnv, double *speedSum, int32_t *bins,
                    const double *edges, int nBins, bool perLaneEdges);

// Distance and speed of the first k vehicles of every lane from the front (cfx_get_lane_obs's semantics: rows of k slots,
// -1.0 / 0.0 behind a lane's last vehicle), from such a view.  Either output may be null.
void laneFrontsFromView(int nLanes, int k, int count, const int32_t *drivable, const double *dis, const double *speed,
                        double *frontDis, double *frontSpeed);
// the same on any backend: cfx_get_lane_obs where it exists, otherwise cfx_get_vehicles + laneFrontsFromView
void laneFrontsOf(const Backend &be, cfx_engine *dev, int nLanes, int k, double *frontDis, double *frontSpeed);
// ... over every backend's cfx_observe_lanes_device / cfx_observe_lane_obs_device (throws std::runtime_error)
void observeLanesDeviceOf(const Backend &be, cfx_engine *dev, const cfx_lane_obs &obs, uintptr_t consumerStream);

}  // namespace cfa
