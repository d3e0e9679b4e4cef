// VectorEngine: R independent copies ("environments") of one scenario advanced in lock-step by ONE device
// engine.  The device sees a single road network made of R disjoint replicas (lane r*L+l, laneLink r*K+k, ...),
// so every kernel launch of a step covers all environments: launch latency is paid once per step instead of
// once per environment, and the car-following kernel finally gets enough vehicles per launch to approach the
// HBM roofline.  Each environment has its own flows and its own std::mt19937 (seed + env index, or seeds[env])
// and evolves exactly like a standalone Engine built from the same config with that seed
// (tests/test_vector_engine.py) — with laneChange: true as well: the device takes each environment's lane-change
// schedule walk and priority stream separately (cfx_config::n_envs).
#pragma once

#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "engine_host.h"

namespace cfa {

class VectorEngineHost {
public:
    // seeds: empty = env r is seeded seed + r; otherwise numEnvs seeds, one per environment (std::invalid_argument for another
    // length) — equal ones give every environment the same demand (common random numbers)
    // routes: candidate routes for set_vehicle_routes (EngineHost::addRoutes), added to every environment's spawner BEFORE the
    // one upload of the route tables — there is no adding later: every environment has its own shifted copy of the tables,
    // and routesPerEnv_ never changes.  std::invalid_argument as EngineHost::addRoutes
    VectorEngineHost(const std::string &configFile, int numEnvs, int threadNum, const std::string &backendLib = "",
                     const std::vector<int> &seeds = {}, const std::vector<std::vector<std::string>> &routes = {});
    ~VectorEngineHost();
    VectorEngineHost(const VectorEngineHost &) = delete;
    VectorEngineHost &operator=(const VectorEngineHost &) = delete;

    int numEnvs() const { return R_; }
    int numLanes() const { return L_; }
    int numIntersections() const { return I_; }
    void nextStep();
    void reset(bool resetRnd);
    // checkpoints in device memory of every environment at once (EngineHost::checkpoint and its kin)
    bool checkpointCalls() const { return be_.hasCheckpoints(); }
    std::string checkpointUnsupported();
    std::shared_ptr<DeviceCheckpoint> checkpoint(std::shared_ptr<DeviceCheckpoint> into);
    void rollback(DeviceCheckpoint &ck) { rollbackTo(ck, nullptr); }
    // ... with environment r taking the state that environment envs[r] has in the checkpoint (repeats allowed; an environment
    // named nowhere is dropped): its vehicles, entry buffers, lights, Lane::history and its spawner's state, generator included.
    // The vehicles are numbered anew, environment by environment.
    void rollbackEnvs(DeviceCheckpoint &ck, const std::vector<int32_t> &envs) { rollbackTo(ck, &envs); }
    // Lane::history of one environment as the device keeps it ("cfx": {"laneHistory": true}; EngineHost::laneHistory)
    bool keepsLaneHistory() const { return laneHistory_; }
    std::pair<int64_t, int> ringInfo() {  // (total ring slots, capacity scale) of the ring layout, as EngineHost::ringInfo
        std::lock_guard<std::mutex> guard(queryMutex_);
        int64_t slots = 0;
        int32_t scale = 1;
        be_.cfx_get_ring_info(dev_, &slots, &scale);
        return {slots, scale};
    }
    void laneHistory(int env, std::vector<int32_t> &len, std::vector<int32_t> &vehicleNum, std::vector<double> &averageSpeed,
                     std::vector<int32_t> &historyVehicleNum, std::vector<double> &historyAverageSpeed);
    double getCurrentTime() const { return step_ * interval_; }
    std::vector<int32_t> laneVehicleCounts();         // [R * L], env-major
    std::vector<int32_t> laneWaitingVehicleCounts();  // [R * L]
    int64_t totalVehicleCount();
    // phases: [R * I] (entries of virtual intersections are ignored); requires rlTrafficLight
    void setTrafficLightPhases(const std::vector<int32_t> &phases);
    void trafficLightState(std::vector<int32_t> &phase, std::vector<double> &remain);  // [R * I]
    // observations and signals in device memory, [R * L] / [R * I] (EngineHost::observeLanesDevice and its kin)
    bool deviceBuffers() const { return be_.hasDeviceBuffers(); }
    std::pair<uintptr_t, int> streamHandle();
    void setTrafficLightPhasesDevice(uintptr_t phases, size_t n, uintptr_t producerStream);
    bool rlTrafficLight() const { return rlTrafficLight_; }
    std::vector<int32_t> phaseCounts() const;  // [I] phases per intersection of one environment, -1 for virtual ones
    // the fixed-time signal plan of every environment (EngineHost::setTlPlanDevice and its kin): durations [R * I * P], phase /
    // remain [R * I]
    bool tlPlanCalls() const { return plan_.available(); }
    void setTlPlanDevice(uintptr_t durations, uintptr_t phase, uintptr_t remain, uintptr_t producerStream);
    void setTlPlan(const double *durations, const int32_t *phase, const double *remain);
    void tlPhaseDurationsDevice(uintptr_t out, uintptr_t consumerStream);
    void tlPhaseDurations(double *out);
    void restoreTlPlan();
    // the lanes' speed limits of every environment (EngineHost::setLaneSpeedLimitsDevice and its kin): [R * L], one scheme
    // per environment over the one roadnet
    bool laneLimitCalls() const { return limits_.available(); }
    int laneLimitCount() const { return limits_.size(); }
    void setLaneSpeedLimitsDevice(uintptr_t limits, uintptr_t rejected, uintptr_t producerStream);
    int32_t setLaneSpeedLimits(const double *limits);
    void laneSpeedLimitsDevice(uintptr_t out, uintptr_t consumerStream);
    void laneSpeedLimits(double *out);
    void restoreLaneSpeedLimits();
    // per-lane speed and position features over every environment (EngineHost::laneFeatures and its kin): outputs [R * L] /
    // [R * L * nBins], edges [L][nBins + 1] or [nBins + 1], shared by the environments
    std::vector<double> laneLengths() const;  // [L] of one environment
    void laneFeatures(double *speedSum, int32_t *bins, const double *edges, int nBins, bool perLaneEdges);
    void observeLanesDevice(const cfx_lane_obs &obs, uintptr_t consumerStream);
    void laneFronts(int k, const LaneFronts &out);  // [R * L * k] each
    // every running vehicle as a row, environment-major (EngineHost::vehicleRows and its kin); {L, K} of one environment
    bool vehicleRowsDevice() const { return be_.hasDeviceBuffers() && be_.cfx_observe_vehicles_device; }
    bool vehiclePosesDevice() const { return be_.hasVehiclePoses(); }
    std::pair<int, int> drivableCounts() const { return {L_, K_}; }
    DrivableGeometry drivableGeometry() const { return drivableGeometryOf(*net_); }  // one copy: the environments share the roadnet
    bool laneChange() const { return laneChange_; }
    VehicleRows vehicleRows(bool poses = false);
    void observeVehiclesDevice(const cfx_vehicle_rows &rows, uintptr_t consumerStream);
    // speed commands by those vehicle numbers, vehicles of any environment in one call (EngineHost::setVehicleSpeeds and its kin)
    bool vehicleSpeedsDevice() const { return be_.hasDeviceBuffers() && be_.cfx_set_vehicle_speeds_device; }
    void setVehicleSpeedsDevice(uintptr_t vehicle, uintptr_t speed, int n, uintptr_t ignored, uintptr_t producerStream);
    int setVehicleSpeeds(const int32_t *vehicle, const double *speed, int n);
    // route changes by those vehicle numbers, vehicles of any environment in one call (EngineHost::setVehicleRoutes and its
    // kin).  A handle is an index into ONE environment's route tables (they are equal), never read across environments
    const std::vector<int> &addedRoutes() const { return addedRoutes_; }  // the handles of the constructor's `routes`, in order
    std::vector<std::string> routeRoads(int handle);
    int routeCount() const { return routesPerEnv_; }
    void setVehicleRoutesDevice(uintptr_t vehicle, uintptr_t route, int n, uintptr_t status, uintptr_t ignored, uintptr_t producerStream);
    int setVehicleRoutes(const int32_t *vehicle, const int32_t *route, int n, int32_t *status);
    void vehicleRoutesDevice(uintptr_t vehicle, int n, uintptr_t out, uintptr_t consumerStream);
    void vehicleRoutes(const int32_t *vehicle, int n, int32_t *out);
    // per-intersection observations over every environment (EngineHost::intersectionFeatures and its kin): outputs [R * I ...];
    // the layout is one environment's
    const InterLayout &intersectionLayout();
    void intersectionFeatures(const InterFeatures &out);
    void observeIntersectionsDevice(uintptr_t phase, uintptr_t remain, uintptr_t in, uintptr_t inWaiting, uintptr_t out,
                                    uintptr_t inside, uintptr_t pressure, int maxRoadLinks, int maxPhases, uintptr_t consumerStream);
    // per-lane flow statistics across steps over every environment (EngineHost::trackLaneFlow and its kin): outputs [R * L]
    // ---- per-movement flow and delay statistics across steps over every environment (EngineHost::trackMovementFlow and its
    //      kin): outputs [R * I * M], any pointer may be null
    void trackMovementFlow(bool on);
    bool movementFlowTracking() const { return trackers_.move.on(); }
    int movementFlowRows() const { return (int) trackers_.move.rows(); }
    void movementFlowFeatures(const MoveFlowOut &out, bool reset);
    void observeMovementFlowDevice(const MoveFlowOut &out, bool reset, uintptr_t consumerStream);
    void trackLaneFlow(bool on);
    bool laneFlowTracking() const { return trackers_.flow.on(); }
    void laneFlowFeatures(const LaneFlowOut &out, bool reset);
    void observeLaneFlowDevice(const LaneFlowOut &out, bool reset, uintptr_t consumerStream);
    // trip statistics and the average travel time per environment (EngineHost::trackTrips and its kin): outputs [R]
    void trackTrips(bool on);
    bool tripTracking() const { return trackers_.trip.on(); }
    void tripFeatures(const cfx_trip_stats_out &out);
    void observeTripsDevice(const cfx_trip_stats_out &out, uintptr_t consumerStream);
    // the trip log (EngineHost::trackTripLog and its kin): ONE log for all environments, the `env` column says which
    void trackTripLog(int64_t capacity);
    int32_t tripLogCapacity() const { return trackers_.trip.logCapacity(); }
    void tripLogFeatures(const cfx_trip_log_out &out, bool reset);
    void observeTripLogDevice(const cfx_trip_log_out &out, bool reset, uintptr_t consumerStream);
    // virtual loop detectors (EngineHost::defineDetectors and its kin): ONE environment's set, which every environment gets;
    // outputs [R * n]
    void defineDetectors(const int32_t *lane, const double *start, const double *end, int n);
    void dropDetectors();
    const Detectors &detectors() const { return trackers_.det; }
    void detectorFeatures(const cfx_detectors_out &out, bool reset);
    void observeDetectorsDevice(const cfx_detectors_out &out, bool reset, uintptr_t consumerStream);
    std::vector<std::string> laneIds() const;
    std::vector<std::string> roadIds() const;  // one environment's roads, in roadnet-file order (the trip log's road columns)
    std::vector<std::string> intersectionIds() const;
    cfx_scalars scalars();
    void sync();
    void profileEnable(bool on);
    std::map<std::string, std::pair<double, int64_t>> profileRead();
    std::string backendName() const { return be_.cfx_backend_name(); }
    // cumulative host wall seconds since the last reset, ON THE CALLER'S PATH: {spawners (with the batch prepared a step ahead:
    // the wait for it), record translation, cfx_step (launches + back-pressure)}, then the ahead thread's own busy time
    std::vector<double> hostSeconds() const {
        return {hostSpawnSec_, hostTranslateSec_, hostSubmitSec_, hostAheadSec_.load(std::memory_order_relaxed)};
    }
    // per-environment id-keyed view, for parity tests against a standalone Engine
    std::map<std::string, double> getVehicleSpeed(int env);
    std::map<std::string, int> getLaneVehicleCount(int env);

private:
    void check(int32_t rc, const char *what);
    void rollbackTo(DeviceCheckpoint &ck, const std::vector<int32_t> *envs);  // (envs null: every environment its own state)
    bool laneHistory_ = false;
    bool geometryUploaded_ = false;  // cfx_set_drivable_geometry was called (the first pose output asked for in device memory)
    std::unique_ptr<InterLayout> interLayout_;  // built by the first call that needs it
    Trackers trackers_;                  // (every call with queryMutex_ held: it asks the device)
    bool devicePhaseUnchecked_ = false;  // as EngineHost: read by every call below that has waited for the device
    void raiseDeviceError();             // (the caller holds queryMutex_)
    TlPlan plan_;                        // (every call with queryMutex_ held)
    LaneLimits limits_;                  // (likewise)

    std::shared_ptr<HostRoadNet> net_ = std::make_shared<HostRoadNet>();
    std::vector<std::unique_ptr<Spawner>> spawners_;
    std::vector<std::vector<int32_t>> localToGlobal_;  // [env][local vid] -> global vid
    std::vector<std::pair<int32_t, int32_t>> globalToLocal_;  // global vid -> (env, local vid)
    Backend be_;
    cfx_engine *dev_ = nullptr;
    int R_ = 1, L_ = 0, K_ = 0, I_ = 0, routesPerEnv_ = 0;
    std::vector<int> addedRoutes_;
    // a device-side route change since the spawners' vehicles[...].route were last read back; their one reader here, the host
    // trip tracker's tripNote, calls refreshRoutes() first (queryMutex_ held)
    bool routesStale_ = false;
    void refreshRoutes();
    int hostThreads_ = -1;  // config "cfx": {"hostThreads": n}: -1 auto, 0 serial
    int autoBatches_ = 0;          // auto: serial batches timed so far (forEachEnv)
    double autoSerialUs_ = 0.0;    //       their total time
    bool autoUsePool_ = false;     //       the verdict once enough of them were seen
    double interval_ = 1.0;
    bool rlTrafficLight_ = false;
    size_t step_ = 0;
    std::vector<cfx_spawn> recs_;       // the batch being handed to the device
    std::vector<cfx_spawn> recsNext_;   // the batch being prepared (swapped with recs_ when a step takes it)
    std::vector<std::vector<cfx_spawn>> envRecs_;  // [env] this step's records in the environment's own numbering

    // The R spawners are independent (own mt19937, own flows): phases 0-1 of all environments run on a small pool of
    // host threads, the numbering of the new vehicles is then assigned serially in environment order.
    void forEachEnv(void (VectorEngineHost::*fn)(int));  // fn(env) for every environment, on the pool from 32 envs on
    void spawnEnv(int r);
    void translateEnv(int r);
    void tripNote(int32_t vid, double enterTime, int env, int route);  // (host trip tracker; `route` in the environment's own numbering)
    void peekEnv(int r);
    // lane change (laneChange: true): as EngineHost, per environment (include/cityflow_amd.h "Lane change", n_envs)
    void settleLaneChange();
    bool laneChange_ = false, lcPollPending_ = false;
    int shadowPoolPerEnv_ = 256;
    std::vector<int32_t> shadowPool_, shadowParents_;
    std::vector<std::vector<int32_t>> envPeek_;
    void workerLoop();
    void runEnvs();
    void (VectorEngineHost::*poolFn_)(int) = nullptr;
    std::vector<int32_t> envBase_;  // [env] offset of the environment's records in this step's batch
    int32_t batchFirstVid_ = 0;
    double hostSpawnSec_ = 0, hostTranslateSec_ = 0, hostSubmitSec_ = 0;
    std::atomic<double> hostAheadSec_{0.0};  // (written by the ahead thread)
    // ---- the batch of step t+1 is prepared while step t is submitted and runs (config "cfx": {"spawnAhead": false} turns it
    //      off; not with lane change, whose shadows draw from the generators after the device has scheduled them).  The
    //      reference's Flow::nextStep / planRoute (flow.cpp:6-22, engine.cpp:450-470) depend on nothing a step computes
    //      except through the rare priority collision, which asks the device — after step t has been handed over, as always.
    //      One more host thread runs the R spawners and the translation (on the pool above when that pays); every spawner
    //      journals the step (Spawner::beginAhead), so reset() can take it back.  nextStep() only waits for the batch.
    void prepareBatch(size_t step, double *spawnSec, double *translateSec);  // spawn + number + translate into recsNext_
    void aheadLoop();
    void kickAhead(size_t step);
    void waitAhead();                 // until the ahead thread is not working (rethrows what it threw)
    void dropAhead();                 // ... and take a prepared batch back (rollback of every spawner's journal)
    bool aheadEnabled_ = false;
    bool journalling_ = false;        // the batch being prepared is one a reset may have to take back
    enum AheadState { kAheadIdle, kAheadWorking, kAheadReady, kAheadFailed };
    AheadState aheadState_ = kAheadIdle;
    size_t aheadStep_ = 0;
    std::string aheadError_;
    size_t l2gMark_ = 0;              // globalToLocal_.size() before the prepared batch
    std::vector<size_t> l2gEnvMark_;  // localToGlobal_[r].size() before it
    std::thread aheadThread_;
    std::mutex aheadMutex_;
    std::condition_variable aheadCv_;
    bool aheadStop_ = false;
    std::atomic<uint64_t> aheadKicks_{0};  // requests so far (the ahead thread polls it before it sleeps)
    uint64_t aheadSeen_ = 0;
    std::atomic<bool> aheadBusy_{false};   // a request is being worked on (the caller polls it before it sleeps)
    std::atomic<uint64_t> preparing_{0};  // the step whose batch is being prepared
    std::atomic<uint64_t> submitted_{0};  // steps handed to the device so far (a priority-collision query of step s waits for s)
    std::vector<std::thread> workers_;
    std::mutex poolMutex_, queryMutex_;
    std::condition_variable poolCv_;
    std::atomic<uint64_t> poolGeneration_{0};
    bool poolStop_ = false;
    std::atomic<int> nextEnv_{0}, envsDone_{0};
    std::string poolError_;
};

}  // namespace cfa
