// cfx C ABI (include/cityflow_amd.h) implemented on HIP for gfx950 / MI355X.
// Host-side bookkeeping of the device engine: buffer ownership and growth, launch sequencing, getters.
// The arithmetic lives in cfx_device.h / cfx_kernels.h.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>


#include "cfx_kernels.h"
#include "cfx_launch_policy.h"
#include "cfx_stage_layout.h"
#include "cfx_lc_kernels.h"
#include "cfx_ring_kernels.h"
#include "cfx_dense_kernels.h"
#include "cfx_lane_limit_kernels.h"

// k_cross2's grid on the dense layout: one block per kCross2Jobs slots of the layout's bound, at most this many (the
// kernel strides over the queue, so any grid is correct; blocks beyond the queue's length only pay the prologue)
#ifndef CFX_CROSS2_BLOCKS_PER_CU
#define CFX_CROSS2_BLOCKS_PER_CU 7  // k_cross2 on the dense layout: what its LDS lets a CU hold
#endif

using namespace cfxd;

namespace {

std::string g_createError;

#ifndef CFX_DENSE_FORM_DEFAULT
#define CFX_DENSE_FORM_DEFAULT 6  // what cfx_config::dense_form = 0 means (include/cityflow_amd.h): lanes-only admission, 1024 spawn records in its arguments
#endif
enum ProfKernel { PK_SPAWN = 0, PK_ADMIT, PK_ACTION, PK_CROSS, PK_SCAN, PK_SCATTER, PK_HALO_EXPORT, PK_HALO_IMPORT, PK_COMMIT, kNumProfKernels };
// names of the step's phases; the ring layout runs kr_admit / kr_action / k_cross<.., RingCtx> / kr_commit under the first
// four and the last name (it has no scan / scatter)
const char *const kProfNames[kNumProfKernels] = {"k_spawn_link", "k_admit", "k_action", "k_cross", "k_scan", "k_scatter",
                                                 "k_halo_export", "k_halo_import", "k_commit"};

#define HIP_TRY(call)                                                                                  \
    do {                                                                                               \
        hipError_t err__ = (call);                                                                     \
        if (err__ != hipSuccess) {                                                                     \
            fail(std::string(#call) + ": " + hipGetErrorString(err__));                                \
            return CFX_ERR_DEVICE;                                                                     \
        }                                                                                              \
    } while (0)

template <typename T> struct DBuf {
    T *p = nullptr;
    size_t cap = 0;
};

inline int gridFor(size_t n) { return (int) std::max<size_t>(1, (n + kBlock - 1) / kBlock); }
// grid-stride kernels over slots: enough blocks to fill 256 CUs x 8, never more than needed
constexpr size_t kInitialVidCap = (size_t) 1 << 22;  // vehicle numbers the tables are sized for at creation (46 B each; 100 with lane change)
inline int gridStride(size_t n) { return (int) std::min<size_t>(std::max<size_t>(1, (n + kBlock - 1) / kBlock), 2048); }

}  // namespace

// A checkpoint in device memory (cfx_checkpoint_save / _restore, include/cityflow_amd.h): ONE allocation that holds the running
// vehicles in the dense form of the getters (RingDense, with leader and gap) plus everything else cfx_load_state writes, as the
// arrays stand; and on the host what cfx_load_state recomputes from an archive's columns.
struct cfx_checkpoint {
    cfx_engine *owner = nullptr;  // null once the engine is gone
    char *arena = nullptr;
    size_t arenaCap = 0;
    bool saved = false;
    int32_t nR = 0, nV = 0;
    // ---- views into the arena
    RingDense rd{};
    int32_t *off = nullptr;  // [D + 1]
    int32_t *priority = nullptr, *templ = nullptr, *route = nullptr, *nextWait = nullptr;  // [nV] VidTable
    double *enterTime = nullptr, *customSpeed = nullptr;
    uint8_t *state = nullptr, *pendingCustom = nullptr;
    int32_t *waitHead = nullptr, *curPhase = nullptr;  // [L], [I]
    double *remain = nullptr;                          // [I]
    LaneHistDev hist{};                                // (null where the engine keeps no Lane::history)
    // ---- host part
    DevScalars sc{};
    std::vector<int32_t> cnt;  // [D] vehicles per drivable (ring capacities are checked against it)
    int64_t step = -1, finishedOffset = 0, nQueueLanes = 0;
    std::vector<uint8_t> laneQueued;
    std::map<int32_t, double> futureCustom;
    bool timesDyadic = true;
};

// the trackers (cfx_engine::tracker), in the order of their lifecycle, and their names in messages
enum Tracker { kLaneFlow, kMoveFlow, kTrips, kDetectors, kTrackers };
static const char *const kTrackerName[kTrackers] = {"lane-flow", "movement-flow", "trip", "detector"};
static const char *const kTrackerEnable[kTrackers] = {"cfx_lane_flow_enable", "cfx_movement_flow_enable", "cfx_trip_stats_enable",
                                                      "cfx_detectors_enable"};

struct cfx_engine {
    int device = 0;
    int nCU = 256;  // compute units of the device (hipDeviceProp_t::multiProcessorCount)
    hipStream_t stream = nullptr;
    cfx_config cfg{};
    int R = 0, L = 0, K = 0, D = 0, I = 0, E = 0;
    std::string err;

    // ---- static network (device) ----
    DevNet net{};
    std::vector<void *> owned;  // every device allocation, for teardown

    // ---- tables ----
    std::vector<cfx_vehicle_template> hTempl;
    std::vector<int32_t> hRouteStart{0}, hRouteRoads, hNextStart{0}, hNextLL;
    DBuf<cfx_vehicle_template> dTempl;
    DBuf<int32_t> dRouteStart, dRouteRoads, dNextStart, dNextLL;
    bool tablesDirty = false;

    // ---- vehicle table ----
    VidTable vt{};
    LaneHistDev hist{};                // Lane::history, with cfx_config::lane_history (tiles: on the ring layout only)
    size_t vidCap = 0;
    int64_t spawned = 0;

    // ---- slots (two generations) ----
    SlotArrays gen[2]{};
    DBuf<int32_t> segStart[2], cnt[2];
    size_t slotCap = 0;
    int cur = 0;
    ActionBuf ab{};
    CompactScratch cs{};
    int32_t *oldToNew = nullptr;
    int32_t *finList = nullptr, *finTicket = nullptr, *crossJobs = nullptr, *jobCount = nullptr;
    int32_t *finCount = nullptr;  // [kFinShards * 32] counters of the finisher lists (FinMap)
    // getter scratch
    int32_t *viewLeader = nullptr;
    double *viewGap = nullptr;

    // ---- per-lane / per-laneLink / per-entry / per-intersection dynamic state ----
    int32_t *waitHead = nullptr, *admitStep = nullptr, *laneTail = nullptr, *curPhase = nullptr;
    int2 *admitRec = nullptr;
    int4 *llDyn = nullptr;
    int2 *llGate = nullptr;
    unsigned long long *interMask = nullptr;
    int nMaskWords = 0;
    double *remain = nullptr;
    unsigned long long *scanGranules = nullptr;
    int32_t *scanTicket = nullptr;
    int nScanBlocks = 0;
    // per-drivable arrays k_scan reads with 16-byte loads are padded to whole scan tiles
    size_t dPadded() const { return (size_t) ((D + kScanTile - 1) / kScanTile) * kScanTile; }
    int32_t *laneOut = nullptr;
    int32_t *hLaneOut = nullptr;  // pinned landing buffer of the per-lane getters (a D2H copy into pageable memory is staged twice)
    // The observation of a control loop (Engine::getLaneVehicleCount engine.cpp:628-634 read after every step): once the
    // caller has asked for the lane counts, every step's commit writes the counts it changes straight into this pinned host
    // array (kr_commit / k_scan, a few hundred 4-byte stores over PCIe), the step no longer defers its commit to the next
    // admission, and the getter is a wait for the stream plus a host memcpy — no launch, no copy engine.  `hCntValid`: the
    // array equals the device's counts as of the last step enqueued (every commit since it was filled has published);
    // `observing` is dropped again after kObserveIdle steps without a read.
    std::map<int32_t, double> futureCustom;  // cfx_set_vehicle_speed for vehicle numbers the next spawn records will create
    int64_t droppedFutureSpeeds = 0;         // ... of which the next step's records then did not create the vehicle
    std::vector<int32_t> phaseSeen;  // cfx_set_tl_phases: the call that last named each intersection (duplicates: last one wins)
    int32_t phaseCall = 0;
    int32_t *hCnt = nullptr;
    bool hCntValid = false, observing = false;
    int observeIdle = 0;
    static constexpr int kObserveIdle = 8;
    int32_t *publishTo() const { return (observing && hCntValid && !tiled) ? hCnt : nullptr; }
    // cfx_observe_lanes_device / cfx_set_tl_phases_device (observations and signals in the caller's device buffers, ordered against
    // the caller's stream with these events).  `devObserving`: someone observes on the device after every step, so the step
    // does not defer its commit (the observation would launch it anyway); dropped after kObserveIdle steps without one.
    hipEvent_t devInEvent = nullptr, devOutEvent = nullptr;
    bool devObserving = false;
    int devObserveIdle = 0;
    void deviceObserved() {  // what a device-side observation leaves behind (never on a tile)
        devObserving = !tiled;
        devObserveIdle = 0;
    }
    int32_t *hPhaseErr = nullptr;  // pinned, host-mapped: {intersection, phase} of the first rejected device-side entry, {-1, 0}
    // cfx_set_tl_plan_device and its kin: the durations in force are net.phaseTime itself, held here non-const (every kernel that
    // reads a phase's time indexes that array on every use); the file's, for cfx_restore_tl_plan; the largest phase count of a
    // signalised intersection (the row length of the padded arrays); the record of a rejected call
    double *phaseTime = nullptr, *phaseTimeFile = nullptr;
    int nPhaseTimes = 0, planMaxPhases = 0;
    TlPlanErr *hPlanErr = nullptr;  // pinned, host-mapped; inter = -1: none
    int32_t planCalls = 0;          // set calls enqueued so far (TlPlanErr::done: the last one the device has decided)
    // cfx_set_lane_speed_limits_device and its kin: the limits in force are net.drvLM[l].y and net.drvMaxSpeed[l] themselves,
    // held here non-const (the step's kernels read drvLM once per vehicle and step; cfx_lane_limit_kernels.h writes both from one
    // value); the file's lane limits [L], for cfx_restore_lane_speed_limits
    double2 *drvLM = nullptr;
    double *drvMaxSpeed = nullptr, *laneLimitFile = nullptr;
    // The staging arena of the host forms (cfx_get_lane_obs, cfx_get_lane_features, cfx_get_intersection_features,
    // cfx_get_movement_flow, cfx_get_trip_log, cfx_set_tl_plan, cfx_get_tl_phase_durations, cfx_set_vehicle_speeds,
    // cfx_set_vehicle_routes, cfx_get_vehicle_routes, cfx_set_lane_speed_limits, cfx_get_lane_speed_limits): the device side of the
    // host arrays one call was given, laid out by cfx_stage_layout.h.  ONE allocation (in `owned`), grown to the largest request
    // seen, rounded up to a power of two so that requests that creep up (the speed commands of a filling network) regrow it a
    // logarithmic number of times.  Growing frees the old one at once, which is safe because the arena is idle at every
    // entry: it is used only by calls that end in hipStreamSynchronize(stream) (stageClose).  Nothing in it outlives a call.
    char *stage = nullptr;
    size_t stageBytes = 0;
    int32_t *rowTileSum = nullptr;  // cfx_observe_vehicles_device: the scan's tile totals [ceil(D / kRowTile)] (in `owned`)
    // cfx_set_drivable_geometry: the polylines of ONE environment's drivables for that call's pose outputs (in `owned`; null
    // until set).  Part of the network, not of the state: nothing that moves vehicles touches them
    int32_t *geoStart = nullptr;    // [D / n_envs + 1]
    GeoNode *geoNodes = nullptr;
    // cfx_set_vehicle_speeds_device / cfx_set_vehicle_speeds and cfx_set_vehicle_routes_device / cfx_set_vehicle_routes: the row
    // that commands each vehicle number [speedStampCap], all -1 between calls (in `owned`; vehicleStampEnsure)
    int32_t *speedStamp = nullptr;
    size_t speedStampCap = 0;
    // cfx_observe_intersections_device / cfx_get_intersection_features: the intersection -> roadLink -> {start lanes, end lanes,
    // laneLinks} index, built and uploaded by the first call (interTables); in `owned`
    bool interBuilt = false;
    InterFeatOut interTab{};        // the table pointers and M / P; the output pointers stay null here
    // The trackers: statistics kept across steps (cfx_lane_flow_enable, cfx_movement_flow_enable, cfx_trip_stats_enable,
    // cfx_detectors_enable; DESIGN.md "One scaffold for the trackers").  One lifecycle, always in this order.  Nothing is
    // allocated or launched for a tracker that is off.  `baselineDue`: enabling, a reset or cfx_load_state left a baseline to the next step or read (trackersSettle).
    // Each keeps a per-vehicle shadow that grows with the vehicle tables (ensureVidCap) and a tick that only ever counts up.
    struct TrackerSlot {
        bool on = false, baselineDue = false;
    } tracker[kTrackers];
    LaneFlowDev flow{};             // laneFlowTick (cfx_kernels.h)
    MoveFlowDev move{};             // moveFlowTick
    TripDev trip{};                 // k_trip_tick
    DetectorDev det{};              // detectorTick
    // cfx_detectors_define: ONE environment's set as the caller gave it (kept while the tracker is off too), and the tables
    // trackerAlloc builds from it for every environment (DetectorDev's lanes / first / order point at them)
    std::vector<int32_t> detLane;
    std::vector<double> detStart, detEnd;
    int32_t *detLanes = nullptr, *detFirst = nullptr, *detOrder = nullptr;
    int cross2 = -1;                // cross phase: 1 = k_cross2 (throughput), 0 = k_cross (latency), -1 = by size
    HostMirror *hMirror = nullptr;  // pinned; valid while the last thing that changed the scalars was a step
    bool mirrorValid = false;
    DevScalars *sc = nullptr;

    cfx_spawn *dRecs = nullptr;
    size_t recCap = 0;
    // pinned staging ring for the per-step spawn records (the caller may reuse `recs` immediately)
    static constexpr int kStages = 4;
    cfx_spawn *hStage[kStages] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t stageEvent[kStages] = {nullptr, nullptr, nullptr, nullptr};
    bool stageBusy[kStages] = {false, false, false, false};
    size_t stageCap = 0;
    int stageIdx = 0;
    // ring layout, more spawn records than kr_admit's arguments hold: the batch's columns in pinned memory (SpawnBatchMem)
    int32_t *hMemStage[kStages] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t memStageEvent[kStages] = {nullptr, nullptr, nullptr, nullptr};
    bool memStageBusy[kStages] = {false, false, false, false};
    size_t memStageWords = 0;
    int memStageIdx = 0;
    std::vector<uint8_t> memSeen;
    std::vector<int32_t> memBucket, memCursor, memOrder;
    int32_t *hPhaseStage[kStages] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t phaseStageEvent[kStages] = {nullptr, nullptr, nullptr, nullptr};
    bool phaseStageBusy[kStages] = {false, false, false, false};
    size_t phaseStageCap = 0;
    int phaseStageIdx = 0;

    // ---- tiling (cfx_halo_config) ----
    bool tiled = false;
    bool mailboxesFineGrained = true;  // cfx_halo_mailbox_alloc never had to fall back to a plain allocation
    HaloDev halo{};
    std::vector<uint8_t> hLaneSpare;   // per lane; empty when not tiled
    std::vector<uint8_t> hLaneGhost;   // per lane; empty when not tiled
    int64_t spareTotal = 0;            // sum of spare slots over lanes
    char *dHaloSend = nullptr, *dHaloRecv = nullptr;
    char *hHaloSend = nullptr, *hHaloRecv = nullptr;  // pinned staging
    int haloSendBytes = 0, haloRecvBytes = 0;
    // mailbox exchange (cfx_halo_attach): per peer, device-visible addresses of the two mailboxes
    struct MailPeer {
        int sendBytes = 0, recvBytes = 0;
        void *sendHost = nullptr, *recvHost = nullptr;  // registered with hipHostRegister
        char *sendDev = nullptr, *recvDev = nullptr;
    };
    std::vector<MailPeer> mail;
    std::vector<void *> ipcOpened;     // peers' mailboxes opened with hipIpcOpenMemHandle
    std::vector<int32_t> hGhostSendOff, hGhostRecvOff, hImportSendOff, hImportRecvOff;
    int32_t *haloTicket = nullptr;
    double *finTerm = nullptr;  // [slot] travel times of the step's finishers in summation order
    HaloDev haloMail{};                // block addressing as (peer, offset inside the peer's message)
    uint32_t generation = 1;           // bumped by cfx_reset: epochs stay monotonic
    int64_t liveUpper = 0;             // upper bound of running vehicles (refreshed from the device when it runs out)
    std::vector<uint8_t> laneQueued;   // lanes that have ever had a vehicle queued (only they can admit)
    int64_t nQueueLanes = 0, spawnedHere = 0;  // ... their number; vehicles spawned onto this engine's lanes

    // ---- lane change (cfx_config::lane_change) ----
    LcDev lc{};                        // device tables (vid-indexed ones grow with the vehicle table)
    int32_t *oldToNew2 = nullptr;      // [slot] lane change: scratch of k_lc_resolve (which items are done)
    // dense layout, cfx_config::dense_form: which organisation of the step's kernels (cfx_dense_kernels.h); results never depend on it
    int denseForm = 0;
    bool laneAdmit() const { return (denseForm & 2) != 0 && useTails() && !tiled; }
    int32_t *gatePhase = nullptr;      // [2 I] laneAdmit(): the phase each intersection's gate records stand for (-1: none), by step parity
    int32_t *hPool = nullptr;          // ... pinned staging
    int32_t *hPoll = nullptr;          // pinned: [0] shadows created by the step, [1] overflow code, [2..] their parents in walk order
    hipEvent_t pollEvent = nullptr;    // the part of the step cfx_lane_change_poll has to wait for
    int poolN = 0;                     // priorities supplied for the next / current step
    bool pollPending = false;          // a lane-change step has run and was not polled yet

    // ---- dense layout with tail records (cfx_dense_kernels.h): engines without lane change and tiling ----
    TailRec *dTail[2] = {nullptr, nullptr}, *dTailNow = nullptr;
    int4 *dGate4 = nullptr;
    bool lcSegValid = false;           // lane change: segOfSlot holds every vehicle's own segment (k_scatter / k_lc_naive)
    bool tailsValid = false;           // the records describe the current generation (false after reset / load / resize)
    bool useTails() const { return !ring && !lc.on; }  // (tiles too since round 3: the halo kernels keep the cut lanes' records up)

    // ---- ring layout (cfx_ring_kernels.h): per-drivable ring segments, committed in place ----
    bool ring = false;                 // this engine uses it (decided at cfx_create; cfx_halo_config may still switch to dense)
    bool ringBuilt = false;
    std::vector<double> hDrvLength;    // host copy of cfx_net::drv_length (ring capacities)
    std::vector<int32_t> hLaneRoad, hLaneIndex;  // host copies of cfx_net::lane_road / lane_index (firstNextOf)
    // Router::getNextDrivable(0) of a vehicle waiting on `lane` with route `route`, as VidTable::firstNext keeps it (nextOf +
    // lastRoadBit of cfx_device.h on the host copies of the tables): looked up once per spawn record
    int32_t firstNextOf(int lane, int route) const {
        if (lane < 0 || lane >= L || route < 0 || route + 1 >= (int) hRouteStart.size()) return kFirstNextUnknown;
        const int road = hLaneRoad[lane], base = hRouteStart[route], len = hRouteStart[route + 1] - base;
        int p = 0;
        while (p < len && hRouteRoads[base + p] != road) ++p;
        int next = -1;
        if (p < len) {
            const int ll = hNextLL[hNextStart[base + p] + hLaneIndex[lane]];
            next = ll < 0 ? -1 : L + ll;
        }
        if (next >= 0) return next;
        return (len > 0 && hRouteRoads[base + len - 1] == road) ? -2 : -1;
    }
    std::vector<int2> hRingGeo;        // [D] {base, cap - 1}
    size_t ringSlots = 0;
    double ringMinLen = 0.0;           // shortest vehicle template the capacities were computed for
    int ringScale = 1;                 // doubled when a ring came close to full
    int ringG = 14, ringCalm = 0, ringHold = 0;      // lanes per block of the action kernel (adapted to the traffic) and steps without a dense block
    int2 *dRingGeo = nullptr;
    int32_t *rHead = nullptr, *rCnt = nullptr, *slotOf = nullptr;
    int4 *rScratch = nullptr;
    SlotArrays rs{};                   // per-slot state that changes only when a vehicle enters a drivable
    double2 *rKin[2] = {nullptr, nullptr};  // [slot] {dis, speed}: the two generations a step alternates
    int4 *rMeta = nullptr;                  // [slot] {template, next drivable, flags, enterLaneLinkTime}
    int rcur = 0;
    int2 *rBlk[2] = {nullptr, nullptr};  // by step parity
    TailRec *rTail[2] = {nullptr, nullptr}, *rTailNow = nullptr;  // [D] per-drivable tail records (by step parity; this step's view)
    MoverRec *rMovers = nullptr;
    long long *rFinKey = nullptr;
    int32_t *rFinVid = nullptr;
    double *rFinTerm = nullptr;
    int rFinCap = 0, rJobCap = 0;
    int32_t *rJobs = nullptr;
    RingJob *rJobRecs = nullptr;
    LLAux *rLLAux = nullptr;
    int4 *rLLGate = nullptr;
    int32_t *rGatePhase = nullptr;     // [2 I] RingCtx::gatePhase
    int4 *rList = nullptr;             // the step's vehicle list (kr_index -> kl_action), grown with the running vehicles
    size_t rListCap = 0;
    int32_t *rListCount = nullptr;     // [2] {entries, kr_index's tile ticket}
    unsigned long long *rIdxGranules = nullptr;  // [tiles of 256 drivables] {epoch, vehicles}
    RingDense rd{};                    // dense staging view (getters, archive, growth)
    size_t rdCap = 0;
    int32_t *rOff = nullptr;           // [D + 1] exclusive prefix sum of rCnt

    // Are the interval, every enter time seen so far and the travel-time sum multiples of 2^-10 below 2^42?  Then the
    // finish statistics need no order (exactFinishStatistics).  Sticky false once anything else shows up.
    bool timesDyadic = true;
    static bool dyadic(double x) { return x * 1024.0 == std::nearbyint(x * 1024.0) && std::fabs(x) < 4398046511104.0; }
    bool exactTimes() const {
        if (!timesDyadic) return false;
        // the running sum: as of the last step the device has finished (pinned mirror) it must be far below the bound
        const double cum = mirrorValid ? hMirror->sc.cumulativeTravelTime : cumLoaded;
        return dyadic(cum) && cum < 1099511627776.0;
    }
    double cumLoaded = 0.0;  // cumulativeTravelTime of the last reset / cfx_load_state (valid until a step has run)

    int64_t step = 0;
    int64_t finishedKnown = 0;  // lower bound of finished vehicles (refreshed on syncs)
    int64_t finishedOffset = 0; // finished vehicles that are not in the vid table (state loaded from an archive)

    // ---- optional per-kernel timing (HIP events on this engine's stream) ----
    bool profiling = false;
    std::vector<hipEvent_t> evPool;             // pairs: [2i] before, [2i+1] after
    std::vector<int> evKernel;                  // kernel id of pair i
    size_t evUsed = 0;                          // pairs in use
    double profMs[kNumProfKernels] = {};
    int64_t profLaunches[kNumProfKernels] = {};
    const char *slotSymbol[kNumProfKernels] = {};  // the kernel launched last in each timing slot (cfx_profile_kernel_symbol)
    // ---- where the host's time inside cfx_step goes (cfx_get_host_stats) ----
    cfx_host_stats hostStats{};
    int stallCause = 0;  // CFX_STALL_* bits raised by the running cfx_step call

    // Launch `kernel`; while profiling, with the dispatch's own start / stop timestamps (hipExtLaunchKernel records the
    // events at the kernel's begin and end, the same clock readings a rocprofv3 kernel trace reports — a pair of
    // hipEventRecord calls around the launch would add the marker packets' latency, ~3 us, to every kernel).
    // The instantiation of a step kernel by where it reads the vehicle templates: the block's LDS copy up to kLdsTempl of them,
    // global memory beyond (templatesOf, cfx_kernels.h).  `...`: the kernel's other template arguments, every one of them.
    bool manyTempl() const { return hTempl.size() > (size_t) kLdsTempl; }
#define CFX_BY_TEMPL(K, ...) (manyTempl() ? K<__VA_ARGS__, true> : K<__VA_ARGS__, false>)
    template <typename K, typename... A>
    void launchNamed(int kernelId, const char *symbol, K kernel, dim3 grid, dim3 block, A... args) {
        slotSymbol[kernelId] = symbol;
        launch(kernelId, kernel, grid, block, args...);
    }
    template <typename K, typename... A>
    void launch(int kernelId, K kernel, dim3 grid, dim3 block, A... args) {
        if (profiling) {
            if (evUsed * 2 + 2 > evPool.size()) {
                for (int i = 0; i < 2; ++i) {
                    hipEvent_t ev = nullptr;
                    if (hipEventCreate(&ev) != hipSuccess) break;
                    evPool.push_back(ev);
                }
                evKernel.push_back(0);
            }
            if (evUsed * 2 + 2 <= evPool.size()) {
                const size_t pair = evUsed++;
                evKernel[pair] = kernelId;
                hipExtLaunchKernelGGL(kernel, grid, block, 0, stream, evPool[2 * pair], evPool[2 * pair + 1], 0, args...);
                return;
            }
        }
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
    }
    void profCollect() {
        (void) hipStreamSynchronize(stream);
        for (size_t i = 0; i < evUsed; ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, evPool[2 * i], evPool[2 * i + 1]) == hipSuccess) {
                profMs[evKernel[i]] += ms;
                profLaunches[evKernel[i]] += 1;
            }
        }
        evUsed = 0;
    }

    int fail(const std::string &m) {
        err = m;
        return CFX_ERR_DEVICE;
    }

    // Device buffers of a caller that works on a stream of its own (cfx_observe_lanes_device / cfx_set_tl_phases_device), around
    // the engine's kernel.  Before it: the engine's stream waits for what the caller has enqueued so far — an output may still
    // be read there (a reused tensor), an input is still being produced there.  After it: the caller's stream waits for the
    // kernel, so what is enqueued there next sees the outputs, and may free or overwrite an input the kernel has read.
    int orderAfterCaller(hipStream_t caller) {
        if (caller == stream) return CFX_OK;
        HIP_TRY(hipEventRecord(devInEvent, caller));
        HIP_TRY(hipStreamWaitEvent(stream, devInEvent, 0));
        return CFX_OK;
    }
    int orderCallerAfter(hipStream_t caller) {
        if (caller == stream) return CFX_OK;
        HIP_TRY(hipEventRecord(devOutEvent, stream));
        HIP_TRY(hipStreamWaitEvent(caller, devOutEvent, 0));
        return CFX_OK;
    }

    template <typename T> int allocRaw(T **p, size_t n) {
        void *q = nullptr;
        HIP_TRY(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
        *p = (T *) q;
        owned.push_back(q);
        return CFX_OK;
    }
    void forget(void *q) { owned.erase(std::remove(owned.begin(), owned.end(), q), owned.end()); }

    // Grow a device array preserving its first `keep` elements.
    template <typename T> int grow(T **p, size_t keep, size_t newCap) {
        T *np = nullptr;
        int rc = allocRaw(&np, newCap);
        if (rc) return rc;
        if (*p && keep) HIP_TRY(hipMemcpyAsync(np, *p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
        if (*p) {
            HIP_TRY(hipStreamSynchronize(stream));
            forget(*p);
            HIP_TRY(hipFree(*p));
        }
        *p = np;
        return CFX_OK;
    }
    // ... without draining the stream: the copy is ordered on the stream like everything else, the old array is freed later
    // (retired; hipFree waits for the device) — at the next cfx_sync / reset / destroy.  For the tables that grow with the
    // vehicles ever created: a step that doubles them does not stall (round 4: ten arrays x (malloc + drain + free) = 70 ms).
    std::vector<void *> retired;
    template <typename T> int growDeferred(T **p, size_t keep, size_t newCap) {
        T *np = nullptr;
        int rc = allocRaw(&np, newCap);
        if (rc) return rc;
        if (*p && keep) HIP_TRY(hipMemcpyAsync(np, *p, keep * sizeof(T), hipMemcpyDeviceToDevice, stream));
        if (*p) retired.push_back(*p);  // (still in `owned`: cfx_destroy frees whatever is left)
        *p = np;
        return CFX_OK;
    }
    int freeRetired() {  // only where the stream is known to be idle
        for (void *q : retired) {
            forget(q);
            HIP_TRY(hipFree(q));
        }
        retired.clear();
        return CFX_OK;
    }
    template <typename T> int upload(T **dst, const T *src, size_t n) {
        int rc = allocRaw(dst, n);
        if (rc) return rc;
        if (n) HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
        return CFX_OK;
    }

    // A caller's buffer has to be device memory of this engine's GPU (`what`: "<entry point>", `name`: the buffer's)
    int checkDevicePointer(const void *p, const char *what, const char *name) {
        hipPointerAttribute_t a{};
        const hipError_t he = hipPointerGetAttributes(&a, p);
        if (he != hipSuccess) (void) hipGetLastError();  // (not sticky: the next launch check must not see it)
        if (he != hipSuccess || a.type != hipMemoryTypeDevice || a.device != device) {
            err = std::string(what) + ": " + name + ": not device memory of this engine's GPU (device " + std::to_string(device) +
                  "; the caller's HIP runtime must be the engine's)";
            return CFX_ERR_INVALID;
        }
        return CFX_OK;
    }
    // ... each given field of a pass-through layout (a staged layout's are host arrays: nothing to check)
    int stageCheck(const cfx_stage::StageLayout &s, const char *what) {
        int rc;
        if (s.passThrough)
            for (int i = 0; i < s.nFields; ++i)
                if (s.field[i].host && (rc = checkDevicePointer(s.field[i].host, what, s.field[i].name))) return rc;
        return CFX_OK;
    }

    // One body per host / device pair of calls (cfx_stage_layout.h).  Staged, the host forms (the arena above).  stageOpen: the
    // arena holds the layout, and the copies of its `in` fields are enqueued; the caller then launches on s.dev(field).
    // stageClose: the copies of its `out` fields are enqueued and the stream is waited for — the call's one wait, after which
    // the arena is idle again.  Pass-through, the `_device` forms: s.dev(field) is the caller's buffer, and the two order the
    // engine's stream against `callerStream` (orderAfterCaller / orderCallerAfter above) without waiting for either.
    int stageOpen(cfx_stage::StageLayout &s, void *callerStream) {
        if (s.passThrough) return orderAfterCaller((hipStream_t) callerStream);
        if (s.size() > stageBytes) {
            size_t cap = cfx_stage::kStageAlign;
            while (cap < s.size()) cap *= 2;
            int rc = grow(&stage, 0, cap);
            if (rc) return rc;
            stageBytes = cap;
        }
        s.base = stage;
        for (int i = 0; i < s.nFields; ++i) {
            const auto &f = s.field[i];
            if (f.host && f.bytes && !f.out) HIP_TRY(hipMemcpyAsync(s.base + f.offset, f.host, f.bytes, hipMemcpyHostToDevice, stream));
        }
        return CFX_OK;
    }
    int stageClose(const cfx_stage::StageLayout &s, void *callerStream) {
        if (s.passThrough) return orderCallerAfter((hipStream_t) callerStream);
        for (int i = 0; i < s.nFields; ++i) {
            const auto &f = s.field[i];
            if (f.host && f.bytes && f.out) HIP_TRY(hipMemcpyAsync(f.host, s.base + f.offset, f.bytes, hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        return CFX_OK;
    }

    template <typename T> int uploadConst(const T *&field, const T *src, size_t n) {
        T *tmp = nullptr;
        int rc = upload(&tmp, src, n);
        field = tmp;
        return rc;
    }

    StepCtx ctx() const {
        StepCtx c{};
        c.n = net;
        c.t.templ = dTempl.p;
        c.t.nTempl = (int) hTempl.size();
        c.t.routeStart = dRouteStart.p;
        c.t.routeRoads = dRouteRoads.p;
        c.t.nextStart = dNextStart.p;
        c.t.nextLL = dNextLL.p;
        c.s = gen[cur];
        c.segStart = segStart[cur].p;
        c.cnt = cnt[cur].p;
        c.admitStep = admitStep;
        c.curPhase = curPhase;
        c.oldToNew = oldToNew;
        c.vPriority = vt.priority;
        c.vCustomSpeed = vt.customSpeed;
        c.vGapState = vt.gapState;
        c.llDyn = llDyn;
        c.llGate = llGate;
        c.laneTail = laneTail;
        c.admitRec = admitRec;
        c.interMask = interMask;
        c.step = (int32_t) step;
        c.interval = cfg.interval;
        c.lc = lc;
        if (dTailNow && useTails()) {
            c.tailR = dTail[(step + 1) & 1];  // written by step - 1
            c.tailW = dTail[step & 1];
            c.tailNow = dTailNow;
            c.llGate4 = dGate4;
            c.laneAdmit = laneAdmit() ? 1 : 0;
        }
        return c;
    }

    int ensureVidCap(size_t need) {
        if (need <= vidCap) return CFX_OK;
        stallCause |= CFX_STALL_VID_GROW;
        hostStats.table_grows_total += 1;
        // (cfx_config::ring_capacity_percent below 100 — the tests' "start small" knob — also starts the vehicle tables small,
        // so that their growth path runs)
        const size_t first = (cfg.ring_capacity_percent > 0 && cfg.ring_capacity_percent < 100) ? (size_t) 1 << 12 : kInitialVidCap;
        size_t nc = std::max<size_t>(need, std::max<size_t>(vidCap * 2, first));
        int rc;
        if (ring && (rc = growDeferred(&slotOf, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.priority, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.templ, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.route, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.nextWait, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.enterTime, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.state, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.customSpeed, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.gapState, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.pendingCustom, (size_t) spawned, nc))) return rc;
        if ((rc = growDeferred(&vt.firstNext, (size_t) spawned, nc))) return rc;
        if (lc.on) {
#define GROW_LC(f) if ((rc = growDeferred(&lc.f, (size_t) spawned, nc))) return rc;
            GROW_LC(ptype) GROW_LC(partner) GROW_LC(offset) GROW_LC(sigSend) GROW_LC(sendDir) GROW_LC(sendUrg) GROW_LC(lastDir)
            GROW_LC(changing) GROW_LC(lcFinished) GROW_LC(sendTarget) GROW_LC(recvFrom) GROW_LC(tLeader) GROW_LC(tFollower)
            GROW_LC(leaderGap) GROW_LC(followerGap) GROW_LC(lastChangeTime) GROW_LC(gap) GROW_LC(slotOf) GROW_LC(bSpeed)
            GROW_LC(bBlocker) GROW_LC(parkIdx) GROW_LC(candPos)
#undef GROW_LC
        }
        // nextWait of not-yet-used vids must read -1 (k_spawn_link relies on it)
        HIP_TRY(hipMemsetAsync(vt.nextWait + spawned, 0xFF, (nc - (size_t) spawned) * sizeof(int32_t), stream));
        if (ring) HIP_TRY(hipMemsetAsync(slotOf + spawned, 0xFF, (nc - (size_t) spawned) * sizeof(int32_t), stream));
        // (numbers not used yet: a record names drivable -1 at tick -1 and matches nothing; a status reads never seen)
        if (tracker[kLaneFlow].on && (rc = growShadow(&flow.rec, nc))) return rc;
        if (tracker[kMoveFlow].on && (rc = growShadow(&move.rec, nc))) return rc;
        if (tracker[kTrips].on && (rc = growShadow(&trip.seen, nc))) return rc;
        if (tracker[kDetectors].on && (rc = growShadow(&det.rec, nc))) return rc;
        vidCap = nc;
        return CFX_OK;
    }
    // a tracker's per-vehicle shadow follows the vehicle tables: the numbers in use kept, the new tail all 0xFF
    template <typename T> int growShadow(T **p, size_t nc) {
        int rc;
        if ((rc = growDeferred(p, (size_t) spawned, nc))) return rc;
        HIP_TRY(hipMemsetAsync(*p + spawned, 0xFF, (nc - (size_t) spawned) * sizeof(T), stream));
        return CFX_OK;
    }

    int ensureSlotCap(size_t need) {
        if (need <= slotCap) return CFX_OK;
        stallCause |= CFX_STALL_SLOT_GROW;
        hostStats.table_grows_total += 1;
        // refresh the live bound first: maybe no growth is needed
        size_t nc = std::max<size_t>(need + need / 2, 1 << 14);
        // the current generation must be preserved; everything else is scratch
        SlotArrays &g = gen[cur];
        size_t keep = slotCap;
        int rc;
#define GROW_KEEP(f) if ((rc = grow(&g.f, keep, nc))) return rc;
        GROW_KEEP(vid) GROW_KEEP(drv) GROW_KEEP(prevDrv) GROW_KEEP(next) GROW_KEEP(blocker) GROW_KEEP(enterLLT) GROW_KEEP(routePos)
        GROW_KEEP(templ) GROW_KEEP(route) GROW_KEEP(flags) GROW_KEEP(dis) GROW_KEEP(speed)
#undef GROW_KEEP
        SlotArrays &o = gen[cur ^ 1];
#define GROW_SCRATCH(ptr) if ((rc = grow(&ptr, 0, nc))) return rc;
        GROW_SCRATCH(o.vid) GROW_SCRATCH(o.drv) GROW_SCRATCH(o.prevDrv) GROW_SCRATCH(o.next) GROW_SCRATCH(o.blocker) GROW_SCRATCH(o.enterLLT)
        GROW_SCRATCH(o.routePos) GROW_SCRATCH(o.templ) GROW_SCRATCH(o.route) GROW_SCRATCH(o.flags) GROW_SCRATCH(o.dis) GROW_SCRATCH(o.speed)
        GROW_SCRATCH(ab.dis) GROW_SCRATCH(ab.speed) GROW_SCRATCH(ab.drv) GROW_SCRATCH(ab.blocker)
        GROW_SCRATCH(cs.inNext) GROW_SCRATCH(finList) GROW_SCRATCH(finTerm) GROW_SCRATCH(viewLeader) GROW_SCRATCH(viewGap)
        if ((rc = grow(&crossJobs, 0, nc * kJobShards))) return rc;
#undef GROW_SCRATCH
        if ((rc = grow(&oldToNew, keep, nc))) return rc;  // committed blockers point through it
        if (lc.on && (rc = grow(&oldToNew2, 0, nc))) return rc;
        if (lc.on && (rc = grow(&lc.newToOld, keep, nc))) return rc;
        if (lc.on && (rc = grow(&lc.parkList, 0, nc))) return rc;
        if (lc.on && (rc = grow(&lc.parkDep, 0, nc))) return rc;
        if (lc.on && (rc = grow(&lc.candAll, 0, nc))) return rc;
        if (lc.on && (rc = grow(&lc.candAllEnv, 0, nc))) return rc;
        if (lc.on && (rc = grow(&lc.segOfSlot, keep, nc))) return rc;  // (k_scatter leaves the next step's input in it)
        slotCap = nc;
        return CFX_OK;
    }

    int syncTables() {
        if (!tablesDirty) return CFX_OK;
        auto up = [this](auto &dbuf, const auto &h) -> int {
            using T = typename std::remove_reference<decltype(*dbuf.p)>::type;
            if (h.size() > dbuf.cap) {
                size_t nc = std::max<size_t>(h.size() * 2, 64);
                int rc = grow(&dbuf.p, 0, nc);
                if (rc) return rc;
                dbuf.cap = nc;
            }
            if (!h.empty()) HIP_TRY(hipMemcpyAsync(dbuf.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
            return CFX_OK;
        };
        // kernels in flight may still read the old buffers: drain before (re)uploading
        stallCause |= CFX_STALL_TABLES;
        HIP_TRY(hipStreamSynchronize(stream));
        int rc;
        if ((rc = up(dTempl, hTempl))) return rc;
        if ((rc = up(dRouteStart, hRouteStart))) return rc;
        if ((rc = up(dRouteRoads, hRouteRoads))) return rc;
        if ((rc = up(dNextStart, hNextStart))) return rc;
        if ((rc = up(dNextLL, hNextLL))) return rc;
        HIP_TRY(hipStreamSynchronize(stream));  // sources are pageable host vectors
        tablesDirty = false;
        return CFX_OK;
    }

    int readScalars(DevScalars &out) {
        stallCause |= CFX_STALL_SCALARS;
        if (mirrorValid) {
            HIP_TRY(hipStreamSynchronize(stream));
            out = hMirror->sc;
        } else {
            HIP_TRY(hipMemcpyAsync(&out, sc, sizeof(DevScalars), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        finishedKnown = out.finishedCnt;
        if (out.overflow == 4) return fail("halo: a neighbour tile did not publish its step in time (cfx_halo_wait)");
        if (out.overflow == 3) return fail("halo: more vehicles crossed one cut lane in one step than CFX_HALO_MAX_MIGRANTS");
        if (out.overflow == 5) return fail("lane change: more shadows in one step than priorities supplied (cfx_lane_change_supply)");
        if (out.overflow == 6) return fail("lane change: more shadows on one road in one step than the schedule walk tracks");
        if (out.overflow == 7) return fail("lane change: inconsistent pair state (k_lc_resolve did not converge)");
        if (out.overflow == 8) return fail("ring layout: a drivable's ring of slots is full");
        if (out.overflow == 9) return fail("cross phase: job queue capacity exceeded");
        if (out.overflow == 10) return fail("action phase: more slots in use than the host's bound (internal error)");
        if (out.overflow == 11) return fail("lane change: no room behind the layout for the lanes that got shadows in one step");
        if (out.overflow == 12) return fail("lane change: more shadows on one lane in one step than k_lc_insert places (kLcRoadInserts)");
        if (out.overflow) return fail("device capacity overflow (finish list)");
        return CFX_OK;
    }


    // ------------------------------------------------------------------------------------------ ring layout
    // `atStep` / `atRcur`: the context of an EARLIER step (the deferred commit of step - 1, see settle)
    RingCtx rctx(bool stepping = false, int64_t atStep = -1, int atRcur = -1) const {
        const int64_t step = atStep >= 0 ? atStep : this->step;
        const int rcur = atRcur >= 0 ? atRcur : this->rcur;
        RingCtx c{};
        c.tailR = rTail[(step + 1) & 1];
        c.tailW = rTail[step & 1];
        c.tailNow = rTailNow;
        c.betweenSteps = stepping ? 0 : 1;
        c.n = net;
        c.t.templ = dTempl.p;
        c.t.nTempl = (int) hTempl.size();
        c.t.routeStart = dRouteStart.p;
        c.t.routeRoads = dRouteRoads.p;
        c.t.nextStart = dNextStart.p;
        c.t.nextLL = dNextLL.p;
        c.s = rs;
        c.kin = rKin[rcur];
        c.kinN = rKin[rcur ^ 1];
        c.meta = rMeta;
        c.blkR = rBlk[(step + 1) & 1];  // written by step - 1
        c.blkW = rBlk[step & 1];
        c.slotOf = slotOf;
        c.vState = vt.state;
        c.ringGeo = dRingGeo;
        c.head = rHead;
        c.cnt = rCnt;
        c.admitStep = admitStep;
        c.curPhase = curPhase;
        c.vPriority = vt.priority;
        c.vCustomSpeed = vt.customSpeed;
        c.vGapState = vt.gapState;
        c.llDyn = llDyn;
        c.interMask = interMask;
        c.llGate = rLLGate;
        c.gatePhase = rGatePhase;
        c.llAux = rLLAux;
        c.laneTail = laneTail;
        c.admitRec = admitRec;
        c.step = (int32_t) step;
        c.interval = cfg.interval;
        return c;
    }
    template <typename T> int freeRaw(T **p) {
        if (*p) {
            forget(*p);
            HIP_TRY(hipFree(*p));
            *p = nullptr;
        }
        return CFX_OK;
    }
    int ringFree() {
        int rc = 0;
        rc |= freeRaw(&rs.vid) | freeRaw(&rs.drv) | freeRaw(&rs.prevDrv) | freeRaw(&rs.routePos) | freeRaw(&rs.route) |
              freeRaw(&rBlk[0]) | freeRaw(&rBlk[1]) | freeRaw(&rKin[0]) | freeRaw(&rKin[1]) | freeRaw(&rMeta) | freeRaw(&rMovers) |
              freeRaw(&dRingGeo) | freeRaw(&rJobs) | freeRaw(&rJobRecs);
        return rc ? CFX_ERR_DEVICE : CFX_OK;
    }
    // Ring capacities: a drivable of length len holds at most ~len / (shortest vehicle) vehicles bumper to bumper; a few
    // more for the transient overlaps the reference allows (Lane::canEnter lets a vehicle in behind a moving tail,
    // roadnet.cpp:437-445), rounded up to a power of two.  kr_commit raises a flag well before a ring is full and the next
    // cfx_step doubles every capacity; a full ring is an error (DevScalars::overflow = 8), never silent.
    int ringAllocate(double minLen) {
        hRingGeo.resize((size_t) D);
        size_t run = 0;
        for (int d = 0; d < D; ++d) {
            double want = std::ceil(hDrvLength[d] / minLen) + 6.0;
            if (cfg.ring_capacity_percent > 0) want = std::max(2.0, want * cfg.ring_capacity_percent / 100.0);
            want *= ringScale;
            size_t cap = 8;
            while ((double) cap < want && cap < (1u << (kRingIdxBits - 1))) cap <<= 1;
            run = (run + cap - 1) & ~(cap - 1);
            hRingGeo[d] = make_int2((int) run, (int) cap - 1);
            run += cap;
            if (run > 0x7fff0000u) return fail("ring layout: more than 2^31 slots");
        }
        ringSlots = run;
        ringMinLen = minLen;
        int rc;
#define RALLOC(ptr) if ((rc = allocRaw(&ptr, ringSlots))) return rc;
        RALLOC(rs.vid) RALLOC(rs.drv) RALLOC(rs.prevDrv) RALLOC(rs.routePos) RALLOC(rs.route)
        RALLOC(rBlk[0]) RALLOC(rBlk[1]) RALLOC(rKin[0]) RALLOC(rKin[1]) RALLOC(rMeta) RALLOC(rMovers)
#undef RALLOC
        HIP_TRY(hipMemsetAsync(rBlk[0], 0xFF, ringSlots * sizeof(int2), stream));
        HIP_TRY(hipMemsetAsync(rBlk[1], 0xFF, ringSlots * sizeof(int2), stream));
        HIP_TRY(hipMemsetAsync(rMeta, 0, ringSlots * sizeof(int4), stream));
        if ((rc = upload(&dRingGeo, hRingGeo.data(), hRingGeo.size()))) return rc;
        rJobCap = (int) std::max<size_t>(4096, ringSlots / 8);
        if ((rc = allocRaw(&rJobs, (size_t) rJobCap * kJobShards))) return rc;
        if ((rc = allocRaw(&rJobRecs, (size_t) rJobCap * kJobShards))) return rc;
        if (!rHead) {
            if ((rc = allocRaw(&rHead, (size_t) D + 1))) return rc;
            if ((rc = allocRaw(&rCnt, (size_t) D + 1))) return rc;
            if ((rc = allocRaw(&rOff, (size_t) D + 2))) return rc;
            if ((rc = allocRaw(&rScratch, (size_t) D))) return rc;
            if ((rc = allocRaw(&rTail[0], (size_t) D))) return rc;
            if ((rc = allocRaw(&rTail[1], (size_t) D))) return rc;
            if ((rc = allocRaw(&rTailNow, (size_t) D))) return rc;
            if ((rc = allocRaw(&rLLAux, (size_t) K))) return rc;
            if ((rc = allocRaw(&rLLGate, (size_t) K))) return rc;
            if ((rc = allocRaw(&rGatePhase, (size_t) 2 * std::max(I, 1)))) return rc;
            HIP_TRY(hipMemsetAsync(rGatePhase, 0xFF, (size_t) 2 * std::max(I, 1) * sizeof(int32_t), stream));
            rFinCap = std::max(1 << 16, L * 8);
            if ((rc = allocRaw(&rFinKey, (size_t) rFinCap))) return rc;
            if ((rc = allocRaw(&rFinVid, (size_t) rFinCap))) return rc;
            if ((rc = allocRaw(&rFinTerm, (size_t) rFinCap))) return rc;
            HIP_TRY(hipMemsetAsync(rCnt, 0, ((size_t) D + 1) * sizeof(int32_t), stream));
        }
        return CFX_OK;
    }
    int ensureDense(size_t n) {
        if (n <= rdCap) return CFX_OK;
        const size_t nc = std::max<size_t>(n + n / 4, 1 << 14);
        int rc;
        HIP_TRY(hipStreamSynchronize(stream));
#define DGROW(ptr) if ((rc = freeRaw(&ptr)) || (rc = allocRaw(&ptr, nc))) return rc;
        DGROW(rd.vid) DGROW(rd.drv) DGROW(rd.prevDrv) DGROW(rd.blockerVid) DGROW(rd.enterLLT) DGROW(rd.routePos) DGROW(rd.leaderVid)
        DGROW(rd.flags) DGROW(rd.dis) DGROW(rd.speed) DGROW(rd.gap)
#undef DGROW
        rdCap = nc;
        return CFX_OK;
    }
    // ring order -> dense staging arrays (Drivable::vehicles order); returns the number of running vehicles
    int ringGather(bool wantLeader, int32_t *totalOut) {
        int rc = ringOffsets(totalOut);
        if (rc || (rc = ensureDense((size_t) *totalOut))) return rc;
        return ringGatherInto(rd, *totalOut, wantLeader);
    }
    // ... its two halves, for a caller that brings the arrays (cfx_checkpoint_save): the offsets into rOff and the number of
    // running vehicles (waits for the stream), then the gather
    int ringOffsets(int32_t *totalOut) {
        hipLaunchKernelGGL(kr_offsets, dim3(1), dim3(kOffBlock), 0, stream, (const int32_t *) rCnt, rOff, D + 1);
        int32_t total = 0;
        HIP_TRY(hipMemcpyAsync(&total, rOff + D, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *totalOut = total;
        return CFX_OK;
    }
    int ringGatherInto(const RingDense &out, int32_t total, bool wantLeader) {
        if (total) hipLaunchKernelGGL(kr_gather, dim3(gridFor(D)), dim3(kBlock), 0, stream, rctx(), (const int32_t *) rOff, out, wantLeader ? 1 : 0);
        HIP_TRY(hipGetLastError());
        return CFX_OK;
    }
    // cfx_load_state and cfx_checkpoint_restore, after the reset: rings that are too small for the state's vehicles (`cnt`: per
    // drivable) — capacities from a fraction of the bound, or a state denser than this engine has seen — double every capacity
    // until it fits: the growth path of a running engine.  `what` names the caller in the error.
    int ringFit(const int32_t *cnt, const char *what) {
        for (;;) {
            bool fits = true;
            for (int d = 0; d < D && fits; ++d) fits = cnt[d] + std::min(8, (hRingGeo[d].y + 1) / 2) <= hRingGeo[d].y;
            if (fits) break;
            if (ringScale >= 4096) return fail(std::string(what) + ": more vehicles on one drivable than its ring can hold");
            ringGrowRequested = true;
            const int rc = ringEnsure();
            if (rc) return rc;
        }
        for (int d = 0; d < D; ++d)
            if (cnt[d] > hRingGeo[d].y) return fail(std::string(what) + ": more vehicles on one drivable than its ring holds");
        return CFX_OK;
    }
    // ... at their end: the dense arrays (rd, rOff) onto the rings, once the vehicle table and the step counter are in place
    // (the blockers' validity tag is "set in the previous step")
    int ringFromDense() {
        if (spawned) HIP_TRY(hipMemsetAsync(slotOf, 0xFF, (size_t) spawned * sizeof(int32_t), stream));
        const int rc = ringClearStepTags();
        if (rc) return rc;
        hipLaunchKernelGGL(kr_scatter_in, dim3(gridFor(D)), dim3(kBlock), 0, stream, rctx(), (const int32_t *) rOff, rd, vt);
        HIP_TRY(hipGetLastError());
        return CFX_OK;
    }
    // Device checkpoints of this engine that are still alive (cfx_checkpoint_create / _destroy): cfx_destroy takes their memory
    std::vector<cfx_checkpoint *> checkpoints;
    DBuf<int32_t> envGather;  // cfx_checkpoint_restore_envs: the tables of the last call (kept: a search loop calls it every round)
    // Records that are valid "for the step in their tag" must not survive a change of the step counter (reset, load) or of
    // the slots they name (rebuilt rings); the occupancy bits are rebuilt by kr_scatter_in.
    int ringClearStepTags() {
        HIP_TRY(hipMemsetAsync(rTailNow, 0xFF, (size_t) D * sizeof(TailRec), stream));
        HIP_TRY(hipMemsetAsync(interMask, 0, (size_t) std::max(nMaskWords, 1) * sizeof(unsigned long long), stream));
        return CFX_OK;
    }
    // ---- the commit of a step may ride with the NEXT step's admission (kr_admit<true>: one launch less per step).  Until
    //      then it is pending; anything else that looks at the state launches it on its own first.
    bool ringMerge = true;       // cfx_config::ring_lanes_per_wave / 10000 == 4 turns the deferral off (developer knob)
    bool commitPending = false;  // the commit of step - 1 has not been launched yet (its lights were advanced by kr_cross)
    // kr_cross's grid: the peak of the reported job counts (cfx_launch_policy.h); cfx_config::ring_lanes_per_wave / 100000 > 0
    // forces its blocks instead (developer knob, for the tests: results never depend on the grid); the blocks of the last launch
    cfx_policy::CrossGridPolicy crossPolicy;
    int crossForceBlocks = 0, lastCrossBlocks = 0;
    size_t activeEstimate() const {
        const unsigned long long pr = __atomic_load_n(&hMirror->progress, __ATOMIC_RELAXED);
        return (size_t) (pr & 0xFFFFFFFFu) + (size_t) nQueueLanes * 4;
    }
    RingCommit commitArgs(size_t activeEst, bool lightsDone, int *nStatOut) {
        const int nStat = (int) std::min<size_t>(std::max<size_t>(1, activeEst >> 16), 64);
        *nStatOut = nStat;
        return RingCommit{rScratch, rMovers, waitHead, curPhase, remain, (int) cfg.rl_traffic_light, (int) nMaskWords,
                          sc, rFinKey, rFinVid, rFinTerm, rFinCap, jobCount,
                          // (a tile's `active` is final only after the halo import; its mirror serves as the stale estimate that
                          // sizes the next steps' grids — mirrorValid stays false, nothing else reads it)
                          hMirror, finTicket, nStat, vt.state, slotOf, exactTimes() ? 1 : 0,
                          lightsDone ? 1 : 0, publishTo(), finCount};
    }
    // tiling on the rings, mailbox transports: cfx_halo_wait leaves the import to the next step's admission launch (one launch
    // less per tile-step); anything else that looks at the state first sends it out as a kernel of its own
    bool haloImportPending = false;
    RingHaloIn pendingImport{};
    // Lane::history on the rings: the record of a step is taken by trailing blocks of the NEXT step's action launch (RingHist,
    // cfx_ring_kernels.h); `histPending`: the last submitted step's has not been.  settle() sends it out as a launch of its own —
    // except for the callers that only read what the history does not touch (the per-step getters of an agent's loop).
    bool histPending = false;
    RingHist takeHist(int firstBlock) {
        RingHist rh{};
        rh.firstBlock = 0x7fffffff;
        if (hist.num && ring && histPending) {  // (tiles too: the step's halo import runs in front of this launch)
            rh.h = hist;
            rh.firstBlock = firstBlock;
            histPending = false;
        }
        return rh;
    }
    // cfx_lane_flow_enable: one tick (or baseline) on the committed state, after everything enqueued so far
    int flowTick(bool baseline) {
        flow.tick += 1;
        flow.step = (int32_t) step;
        flow.baseline = baseline ? 1 : 0;
        flow.vidCap = (int) vidCap;
        if (L <= 0) return CFX_OK;
        const size_t threads = (size_t) L * kFeatGroup;
        if (ring) hipLaunchKernelGGL(kr_lane_flow, dim3(gridFor(threads)), dim3(kBlock), 0, stream, rctx(), flow);
        else hipLaunchKernelGGL(kd_lane_flow, dim3(gridFor(threads)), dim3(kBlock), 0, stream, ctx(), flow);
        HIP_TRY(hipGetLastError());
        return CFX_OK;
    }
    // cfx_movement_flow_enable: one tick (or baseline) over every drivable, on the committed state, after everything enqueued so far
    int moveTick(bool baseline) {
        move.tick += 1;
        move.step = (int32_t) step;
        move.baseline = baseline ? 1 : 0;
        move.vidCap = (int) vidCap;
        if (baseline && K > 0) {
            HIP_TRY(hipMemsetAsync(move.link, 0, (size_t) K * sizeof(cfx_movement_flow_link), stream));
            HIP_TRY(hipMemsetAsync(move.skip, 0, (size_t) K * 3 * sizeof(unsigned long long), stream));
        }
        if (D <= 0) return CFX_OK;
        const size_t threads = (size_t) D * kFeatGroup;
        if (ring) hipLaunchKernelGGL(kr_movement_flow, dim3(gridFor(threads)), dim3(kBlock), 0, stream, rctx(), move);
        else hipLaunchKernelGGL(kd_movement_flow, dim3(gridFor(threads)), dim3(kBlock), 0, stream, ctx(), move);
        HIP_TRY(hipGetLastError());
        return CFX_OK;
    }
    // cfx_trip_stats_enable: one tick (or baseline) over the vehicle numbers, on the committed state, after everything enqueued so far
    int tripTick(bool baseline) {
        if (baseline) {
            HIP_TRY(hipMemsetAsync(trip.seen, 0xFF, std::max<size_t>(vidCap, 1), stream));
            HIP_TRY(hipMemsetAsync(trip.env, 0, (size_t) trip.nEnvs * sizeof(cfx_trip_stats_env), stream));
            if (trip.log) HIP_TRY(hipMemsetAsync(trip.logHead, 0, 2 * sizeof(int), stream));  // (a baseline empties the log)
        }
        if (spawned <= 0) return CFX_OK;
        trip.state = vt.state;
        trip.enterTime = vt.enterTime;
        trip.route = vt.route;
        trip.routeStart = dRouteStart.p;
        trip.routeRoads = dRouteRoads.p;
        trip.interval = cfg.interval;
        trip.spawned = (int) spawned;
        trip.vidCap = (int) vidCap;
        trip.step = (int32_t) step;
        trip.baseline = baseline ? 1 : 0;
        hipLaunchKernelGGL(k_trip_tick, dim3(gridFor(((size_t) spawned + 15) / 16)), dim3(kBlock), 0, stream, trip);
        HIP_TRY(hipGetLastError());
        return CFX_OK;
    }
    // cfx_detectors_enable: one tick (or baseline) over the lanes that have a detector, on the committed state, after everything
    // enqueued so far
    int detectorTick(bool baseline) {
        det.tick += 1;
        det.baseline = baseline ? 1 : 0;
        det.vidCap = (int) vidCap;
        if (det.nLanes <= 0) return CFX_OK;
        const size_t threads = (size_t) det.nLanes * kFeatGroup;
        if (ring) hipLaunchKernelGGL(kr_detectors, dim3(gridFor(threads)), dim3(kBlock), 0, stream, rctx(), det);
        else hipLaunchKernelGGL(kd_detectors, dim3(gridFor(threads)), dim3(kBlock), 0, stream, ctx(), det);
        HIP_TRY(hipGetLastError());
        return CFX_OK;
    }
    // the detector records of every environment from the set cfx_detectors_define keeps, and the index of the lanes that have
    // one: lanes[g], and order[first[g] .. first[g + 1]) = the records on that lane in the caller's order
    int detectorTables() {
        const int nEnvs = cfg.n_envs > 1 ? cfg.n_envs : 1, lanesPerEnv = L / nEnvs, n = (int) detLane.size();
        std::vector<cfx_detector> recs((size_t) nEnvs * n);
        std::vector<int32_t> perLane((size_t) L + 1, 0), lanes, first{0}, order((size_t) nEnvs * n);
        for (int r = 0; r < nEnvs; ++r)
            for (int i = 0; i < n; ++i) {
                cfx_detector &a = recs[(size_t) r * n + i];
                a = cfx_detector{};
                a.start = detStart[(size_t) i];
                a.end = detEnd[(size_t) i];
                a.lane = r * lanesPerEnv + detLane[(size_t) i];
                perLane[(size_t) a.lane + 1] += 1;
            }
        for (int l = 0; l < L; ++l) {
            if (perLane[(size_t) l + 1]) {
                lanes.push_back(l);
                first.push_back(first.back() + perLane[(size_t) l + 1]);
            }
            perLane[(size_t) l + 1] += perLane[(size_t) l];  // (now: where lane l + 1's run starts)
        }
        for (size_t d = 0; d < recs.size(); ++d) order[(size_t) perLane[(size_t) recs[d].lane]++] = (int32_t) d;
        int rc;
        if ((rc = allocRaw(&det.det, recs.size())) || (rc = allocRaw(&detLanes, lanes.size())) ||
            (rc = allocRaw(&detFirst, first.size())) || (rc = allocRaw(&detOrder, order.size())))
            return rc;
        HIP_TRY(hipMemcpyAsync(det.det, recs.data(), recs.size() * sizeof(cfx_detector), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(detLanes, lanes.data(), lanes.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(detFirst, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(detOrder, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));  // (the vectors live on this frame)
        det.lanes = detLanes;
        det.first = detFirst;
        det.order = detOrder;
        det.nLanes = (int) lanes.size();
        det.nDet = (int) recs.size();
        return CFX_OK;
    }
    int detectorTablesFree() {
        const int rc = freeRaw(&det.det) | freeRaw(&detLanes) | freeRaw(&detFirst) | freeRaw(&detOrder);
        det.lanes = det.first = det.order = nullptr;
        det.nLanes = det.nDet = 0;
        return rc;
    }
    // what enabling a tracker allocates (a shadow starts all 0xFF; what the first baseline fills is left to it) ...
    int trackerAlloc(int which) {
        int rc;
        if (which == kLaneFlow) {
            if ((rc = allocRaw(&flow.rec, vidCap)) || (rc = allocRaw(&flow.lane, (size_t) L))) return rc;
            HIP_TRY(hipMemsetAsync(flow.rec, 0xFF, std::max<size_t>(vidCap, 1) * sizeof(int4), stream));
            HIP_TRY(hipMemsetAsync(flow.lane, 0, std::max<size_t>((size_t) L, 1) * sizeof(cfx_lane_flow_lane), stream));
        } else if (which == kMoveFlow) {
            if ((rc = allocRaw(&move.rec, vidCap)) || (rc = allocRaw(&move.link, (size_t) K)) || (rc = allocRaw(&move.skip, (size_t) K * 3))) return rc;
            HIP_TRY(hipMemsetAsync(move.rec, 0xFF, std::max<size_t>(vidCap, 1) * sizeof(int4), stream));
        } else if (which == kDetectors) {
            if (detLane.empty()) {
                err = "cfx_detectors_enable: no detectors are defined (cfx_detectors_define)";
                return CFX_ERR_STATE;
            }
            if ((rc = allocRaw(&det.rec, vidCap))) return rc;
            HIP_TRY(hipMemsetAsync(det.rec, 0xFF, std::max<size_t>(vidCap, 1) * sizeof(int4), stream));
            if ((rc = detectorTables())) return rc;
        } else {
            const int nEnvs = cfg.n_envs > 1 ? cfg.n_envs : 1;
            if (R % nEnvs != 0) {
                err = "cfx_trip_stats_enable: n_envs does not divide the number of roads";
                return CFX_ERR_STATE;
            }
            if ((rc = allocRaw(&trip.seen, vidCap)) || (rc = allocRaw(&trip.env, (size_t) nEnvs))) return rc;
            trip.nEnvs = nEnvs;
            trip.roadsPerEnv = std::max(R / nEnvs, 1);
        }
        return CFX_OK;
    }
    // ... and disabling frees
    int trackerFree(int which) {
        int rc;
        if (which == kLaneFlow) {
            rc = freeRaw(&flow.rec) | freeRaw(&flow.lane);
            flow = LaneFlowDev{};
        } else if (which == kMoveFlow) {
            rc = freeRaw(&move.rec) | freeRaw(&move.link) | freeRaw(&move.skip);
            move = MoveFlowDev{};
        } else if (which == kDetectors) {
            rc = freeRaw(&det.rec) | detectorTablesFree();
            det = DetectorDev{};
            detLane.clear();
            detStart.clear();
            detEnd.clear();
        } else {
            rc = freeRaw(&trip.seen) | freeRaw(&trip.env) | freeRaw(&trip.log) | freeRaw(&trip.logHead);
            trip = TripDev{};
        }
        return rc ? CFX_ERR_DEVICE : CFX_OK;
    }
    // ---- the trackers' lifecycle, always lane, movement, trips, detectors
    int trackerTick(int which, bool baseline) {
        return which == kLaneFlow ? flowTick(baseline) : which == kMoveFlow ? moveTick(baseline) : which == kTrips ? tripTick(baseline) : detectorTick(baseline);
    }
    bool anyTracker() const { return tracker[kLaneFlow].on || tracker[kMoveFlow].on || tracker[kTrips].on || tracker[kDetectors].on; }
    // the baseline that enabling, a reset or a load left to the next step or read (the caller has settled the step and the rings)
    int trackerSettle(int which) {
        if (!tracker[which].on || !tracker[which].baselineDue) return CFX_OK;
        tracker[which].baselineDue = false;
        return trackerTick(which, true);
    }
    int trackersSettle() {
        int rc = CFX_OK;
        for (int t = 0; t < kTrackers && !rc; ++t) rc = trackerSettle(t);
        return rc;
    }
    int trackersTick() {  // after a step, on the committed state
        int rc = CFX_OK;
        for (int t = 0; t < kTrackers && !rc; ++t)
            if (tracker[t].on) rc = trackerTick(t, false);
        return rc;
    }
    void trackersRebaseline() {  // a reset or a load: taken on the state the caller sets up, before the next step or read
        for (TrackerSlot &t : tracker) t.baselineDue = t.on;
    }
    // cfx_*_enable: on takes the first baseline at once
    int trackerEnable(int which, int32_t on) {
        HIP_TRY(hipSetDevice(device));
        TrackerSlot &t = tracker[which];
        if (!on) {
            if (!t.on) return CFX_OK;
            HIP_TRY(hipStreamSynchronize(stream));  // (a tick may still be running; a shadow a growth retired stays with `retired`)
            t = TrackerSlot{};
            return trackerFree(which);
        }
        if (lc.on || tiled) {
            err = std::string(kTrackerEnable[which]) + ": not with lane change and not on a tile";
            return CFX_ERR_STATE;
        }
        if (t.on) return CFX_OK;
        int rc;
        if ((rc = settle(false))) return rc;
        if (ring && (rc = ringEnsure())) return rc;
        if ((rc = trackerAlloc(which))) return rc;
        t.on = t.baselineDue = true;
        return trackerSettle(which);
    }
    int settle(bool withHistory = true) {
        if (haloImportPending) {
            haloImportPending = false;
            const int n = pendingImport.h.nGhost + pendingImport.h.nImport;
            launchNamed(PK_HALO_IMPORT, "kr_halo_import", kr_halo_import, dim3(gridFor(n)), dim3(kBlock), rctx(), pendingImport.h, pendingImport.io, vt,
                        sc, dHaloActiveOut);
            HIP_TRY(hipGetLastError());
        }
        if (commitPending) {
            commitPending = false;
            int nStat = 1;
            const RingCommit rk = commitArgs(activeEstimate(), true, &nStat);
            launchNamed(PK_COMMIT, "kr_commit", kr_commit, dim3(gridStride((size_t) std::max(D, std::max(I, nMaskWords))) + nStat), dim3(kBlock),
                   rctx(true, step - 1, rcur ^ 1), rk, vt, RingHalo{});
            HIP_TRY(hipGetLastError());
        }
        if (withHistory && histPending) {
            const RingHist rh = takeHist(0);
            if (rh.h.num) {
                hipLaunchKernelGGL(kr_lane_history, dim3(gridFor(L)), dim3(kBlock), 0, stream, rctx(), rh.h);
                HIP_TRY(hipGetLastError());
            }
            histPending = false;
        }
        return CFX_OK;
    }

    // ================================================================================= the parts of cfx_step (stepImpl)
    // cfx_config::debug_sync (developer aid): wait for what the step has launched so far and name the kernel that faulted
    int debugCheck(bool ringStep, const char *name) {
        if (!cfg.debug_sync) return CFX_OK;
        if (ringStep) fprintf(stderr, "[cfx ring] step %lld: %s\n", (long long) step, name);
        const hipError_t er = hipStreamSynchronize(stream);
        if (er != hipSuccess) return fail(std::string(ringStep ? "ring step: " : "lane change: ") + name + ": " + hipGetErrorString(er));
        return CFX_OK;
    }

    // What has to hold before a step touches anything: tables uploaded, no overflow pending, the host not too far ahead, rings
    // built, baselines of the statistics taken, the lane-change protocol kept (`n`: the step's spawn records)
    int stepPreamble(int32_t n) {
        HIP_TRY(hipSetDevice(device));
        int rc;
        if ((rc = syncTables())) return rc;
        // Fail at the step that failed (or the one after): every step leaves its scalars in pinned host memory, so an
        // overflow code raised by a step the device has already finished is seen here without waiting for anything.
        if (mirrorValid && __atomic_load_n(&hMirror->sc.overflow, __ATOMIC_RELAXED) != 0) {
            DevScalars s;
            if ((rc = readScalars(s))) return rc == CFX_ERR_DEVICE ? CFX_ERR_CAPACITY : rc;
        }
        // ---- the host's lead over the device is bounded.  A free-running caller submits a 30x30 step in ~20 us and the device takes
        //      ~40: unbounded, the stream's backlog grows by half a step per step, and the next call that has to wait for the device
        //      (a getter, the spawner's priority-collision query) pays for all of it — 4.5 ms behind a 200-step window, 2 ms with 48 steps in flight.  The step's
        //      commit publishes the number of completed steps in pinned host memory: wait (yielding) while more than kMaxLead steps
        //      are in flight.  The device is never idle for it — kMaxLead steps of work are queued behind the one it is executing —
        //      and a caller that synchronises every step never waits here.  (Built while looking for the 45-80 ms "stall" of the
        //      sustained windows of rounds 4-6, which it did NOT cure: that was the container's CPU quota — bench.py's header.)
        if (mirrorValid && !tiled) {
            constexpr int64_t kMaxLead = 16;  // (16 steps of a 30x30 network = 0.65 ms of queued work: what the next waiting call pays at most)
            const auto t0 = std::chrono::steady_clock::now();
            for (unsigned spins = 0;; ++spins) {
                const int64_t done = (int64_t) (__atomic_load_n(&hMirror->progress, __ATOMIC_RELAXED) >> 32);
                if (done <= 0 || done > step || step - done <= kMaxLead) break;
                if ((spins & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;  // (never hang on it)
                std::this_thread::yield();
            }
        }
        if (ring) {
            if (mirrorValid && __atomic_load_n(&hMirror->sc.ringNearFull, __ATOMIC_RELAXED) != 0) ringGrowRequested = true;
            if ((rc = ringEnsure())) return rc;
        }
        if ((rc = trackersSettle())) return rc;  // (a baseline that is due is taken on the state this step starts from)
        if (observing && ++observeIdle > kObserveIdle) {  // nobody has read the lane counts for a while
            observing = false;
            hCntValid = false;
        }
        if (devObserving && ++devObserveIdle > kObserveIdle) devObserving = false;

        if (lc.on) {
            if (pollPending) return fail("cfx_step: the previous lane-change step was not polled (cfx_lane_change_poll)");
            if (!hPoll) return fail("cfx_step: cfx_lane_change_supply must be called before a step with lane change");
            if ((rc = ensureVidCap((size_t) spawned + (size_t) n + (size_t) poolN))) return rc;
        }
        return CFX_OK;
    }

    // ---- phase 0/1 tail: how a step's spawn records reach the device (stageSpawns fills it, the admission launches read it)
    struct SpawnPlan {
        SpawnBatchBig batch;    // the records go with the admission kernel's arguments: up to kAdmitRecs, kd_admit / kr_admit up to kAdmitRecsBig
        SpawnBatchMem mem{};    // ... or, more of them on the ring layout, in pinned memory
        bool inMem = false;     // (neither: k_spawn_link has linked them, the admission takes an empty batch)
        int memStageUsed = -1;  // the pinned buffer `mem` points into: free again when the admission launch is through
        SpawnBatch smallBatch() const {  // (the kernels that take at most kAdmitRecs records)
            SpawnBatch b;
            b.n = batch.n;
            b.firstNewVid = batch.firstNewVid;
            b.enterTime = batch.enterTime;
            for (int i = 0; i < batch.n && i < kAdmitRecs; ++i) {
                b.lane[i] = batch.lane[i];
                b.prevWait[i] = batch.prevWait[i];
                b.route[i] = batch.route[i];
                b.priority[i] = batch.priority[i];
                b.firstNext[i] = batch.firstNext[i];
                b.templ[i] = batch.templ[i];
                b.vidOff[i] = batch.vidOff[i];
            }
            return b;
        }
    };

    // the records as kernel arguments (kr_admit / kd_admit / k_admit take the batch): sorted by lane; false if they do not qualify
    bool spawnsInArgs(const cfx_spawn *recs, int32_t n, SpawnBatchBig &batch) const {
        batch.n = (int) n;
        batch.firstNewVid = (int) spawned;
        batch.enterTime = recs[0].enter_time;
        int order[kAdmitRecsBig];
        bool seen[kAdmitRecsBig] = {};
        bool inArgs = true;
        for (int i = 0; inArgs && i < n; ++i) {
            const int64_t off = (int64_t) recs[i].vid - spawned;
            inArgs = off >= 0 && off < n && !seen[off] && recs[i].lane >= -1 && recs[i].enter_time == batch.enterTime &&
                     recs[i].templ < 32768;
            if (inArgs) seen[off] = true;
            order[i] = i;
        }
        if (!inArgs) {
            batch.n = 0;
            return false;
        }
        std::sort(order, order + n, [recs](int x, int y) {
            return recs[x].lane != recs[y].lane ? recs[x].lane < recs[y].lane : recs[x].vid < recs[y].vid;
        });
        for (int j = 0; j < n; ++j) {
            const cfx_spawn &r = recs[order[j]];
            batch.lane[j] = r.lane;
            batch.prevWait[j] = r.prev_wait;
            batch.route[j] = r.route;
            batch.priority[j] = r.priority;
            batch.firstNext[j] = firstNextOf(r.lane, r.route);
            batch.templ[j] = (int16_t) r.templ;
            batch.vidOff[j] = (int16_t) (r.vid - spawned);
        }
        return true;
    }

    // ring layout, more records than the arguments hold (batched environments): the columns go into pinned memory, sorted
    // by lane, with the offsets of every block of lanes — kr_admit reads its own lanes' records from there (SpawnBatchMem).
    // `p.inMem` says whether they qualified.
    int spawnsInMem(const cfx_spawn *recs, int32_t n, SpawnPlan &p) {
        const int nLaneBlocks = (L + kBlock - 1) / kBlock;
        bool inMem = true;
        const int64_t base = spawned;
        const double t0 = recs[0].enter_time;
        // a counting sort by block of lanes (bucket 0: the records without a lane here), then each block's few records by
        // lane — the kernel looks a lane's records up by bisection; a lane's own records may come in any order
        memSeen.assign((size_t) n, 0);
        memBucket.assign((size_t) nLaneBlocks + 2, 0);
        for (int i = 0; inMem && i < n; ++i) {
            const int64_t off = (int64_t) recs[i].vid - base;
            inMem = off >= 0 && off < n && !memSeen[(size_t) off] && recs[i].lane >= -1 && recs[i].lane < L &&
                    recs[i].enter_time == t0;
            if (inMem) {
                memSeen[(size_t) off] = 1;  // (every vehicle number once)
                memBucket[(size_t) (recs[i].lane < 0 ? 0 : 1 + recs[i].lane / kBlock) + 1] += 1;
            }
        }
        if (!inMem) return CFX_OK;
        for (int q = 0; q <= nLaneBlocks; ++q) memBucket[(size_t) q + 1] += memBucket[(size_t) q];  // bucket q starts at [q]
        memOrder.resize((size_t) n);
        memCursor.assign(memBucket.begin(), memBucket.end() - 1);
        for (int i = 0; i < n; ++i) memOrder[(size_t) memCursor[(size_t) (recs[i].lane < 0 ? 0 : 1 + recs[i].lane / kBlock)]++] = i;
        for (int q = 1; q <= nLaneBlocks; ++q) {
            int32_t *const o = memOrder.data();
            const int from = memBucket[(size_t) q], to = memBucket[(size_t) q + 1];
            if (to - from > 24) {
                std::stable_sort(o + from, o + to, [recs](int x, int y) { return recs[x].lane < recs[y].lane; });
            } else {
                for (int j = from + 1; j < to; ++j) {
                    const int x = o[j], lx = recs[x].lane;
                    int i = j;
                    for (; i > from && recs[o[i - 1]].lane > lx; --i) o[i] = o[i - 1];
                    o[i] = x;
                }
            }
        }
        const size_t words = (size_t) 7 * (size_t) n + (size_t) nLaneBlocks + 1;
        if (words > memStageWords) {
            stallCause |= CFX_STALL_STAGE_GROW;
            HIP_TRY(hipStreamSynchronize(stream));
            const size_t nc = std::max<size_t>(words * 2, 4096);
            for (int i = 0; i < kStages; ++i) {
                if (hMemStage[i]) HIP_TRY(hipHostFree(hMemStage[i]));
                hMemStage[i] = nullptr;
                HIP_TRY(hipHostMalloc((void **) &hMemStage[i], nc * sizeof(int32_t), hipHostMallocDefault));
                if (!memStageEvent[i]) HIP_TRY(hipEventCreateWithFlags(&memStageEvent[i], hipEventDisableTiming));
                memStageBusy[i] = false;
            }
            memStageWords = nc;
        }
        const int si = memStageIdx;
        memStageIdx = (si + 1) % kStages;
        if (memStageBusy[si]) HIP_TRY(hipEventSynchronize(memStageEvent[si]));
        int32_t *const w = hMemStage[si];
        int32_t *const cLane = w, *const cPrev = w + n, *const cRoute = w + 2 * (size_t) n, *const cPrio = w + 3 * (size_t) n,
                       *const cNext = w + 4 * (size_t) n, *const cTempl = w + 5 * (size_t) n, *const cOff = w + 6 * (size_t) n,
                       *const cBlock = w + 7 * (size_t) n;
        for (int j = 0; j < n; ++j) {
            const cfx_spawn &r = recs[memOrder[(size_t) j]];
            cLane[j] = r.lane;
            cPrev[j] = r.prev_wait;
            cRoute[j] = r.route;
            cPrio[j] = r.priority;
            cNext[j] = firstNextOf(r.lane, r.route);
            cTempl[j] = r.templ;
            cOff[j] = (int32_t) (r.vid - spawned);
        }
        for (int q = 0; q <= nLaneBlocks; ++q) cBlock[q] = memBucket[(size_t) q + 1];  // block q's records: bucket q + 1
        p.mem.n = (int) n;
        p.mem.firstNewVid = (int) spawned;
        p.mem.enterTime = recs[0].enter_time;
        p.mem.lane = cLane;
        p.mem.prevWait = cPrev;
        p.mem.route = cRoute;
        p.mem.priority = cPrio;
        p.mem.firstNext = cNext;
        p.mem.templ = cTempl;
        p.mem.vidOff = cOff;
        p.mem.blockOff = cBlock;
        p.mem.nLaneBlocks = nLaneBlocks;
        p.inMem = true;
        p.memStageUsed = si;
        return CFX_OK;
    }

    // ... and whatever fits neither: a pinned copy of the records and a launch of k_spawn_link, with the custom speeds that
    // wait for one of these vehicles behind it on the stream
    int spawnsByKernel(const cfx_spawn *recs, int32_t n, const std::vector<std::pair<int32_t, double>> &customNow) {
        int rc;
        if ((rc = settle(false))) return rc;  // (k_spawn_link looks at what the previous step's commit leaves)
        if ((size_t) n > recCap) {
            size_t nc = std::max<size_t>((size_t) n * 2, 1024);
            if ((rc = grow(&dRecs, 0, nc))) return rc;
            recCap = nc;
        }
        if ((size_t) n > stageCap) {
            stallCause |= CFX_STALL_STAGE_GROW;
            HIP_TRY(hipStreamSynchronize(stream));
            size_t nc = std::max<size_t>((size_t) n * 2, 1024);
            for (int i = 0; i < kStages; ++i) {
                if (hStage[i]) HIP_TRY(hipHostFree(hStage[i]));
                HIP_TRY(hipHostMalloc((void **) &hStage[i], nc * sizeof(cfx_spawn), hipHostMallocDefault));
                if (!stageEvent[i]) HIP_TRY(hipEventCreateWithFlags(&stageEvent[i], hipEventDisableTiming));
                stageBusy[i] = false;
            }
            stageCap = nc;
        }
        const int si = stageIdx;
        stageIdx = (si + 1) % kStages;
        if (stageBusy[si]) HIP_TRY(hipEventSynchronize(stageEvent[si]));
        memcpy(hStage[si], recs, (size_t) n * sizeof(cfx_spawn));
        // the kernel reads the pinned (device-visible) staging buffer itself: no separate copy launch
        launchNamed(PK_SPAWN, "k_spawn_link", k_spawn_link, dim3(gridFor(n)), dim3(kBlock), (const cfx_spawn *) hStage[si], (int) n,
                    (int) spawned, vt, waitHead, lc);
        HIP_TRY(hipEventRecord(stageEvent[si], stream));
        stageBusy[si] = true;
        if (!customNow.empty()) {  // Vehicle::setCustomSpeed on a vehicle still in its waiting buffer (cfx_set_vehicle_speed)
            const uint8_t one = 1;
            for (const auto &fc : customNow) {
                HIP_TRY(hipMemcpyAsync(vt.customSpeed + fc.first, &fc.second, sizeof(double), hipMemcpyHostToDevice, stream));
                HIP_TRY(hipMemcpyAsync(vt.pendingCustom + fc.first, &one, 1, hipMemcpyHostToDevice, stream));
            }
            HIP_TRY(hipStreamSynchronize(stream));  // (the sources live on this frame)
        }
        return CFX_OK;
    }

    // Hand the spawn records to the device, by the cheapest route they qualify for
    int stageSpawns(const cfx_spawn *recs, int32_t n, SpawnPlan &p) {
        p.batch.n = 0;
        p.batch.firstNewVid = 0;
        if (n <= 0) return CFX_OK;
        int rc;
        // (the ring layout too: more records than the small batch holds kept the step from riding its commit with the next
        // admission, and cost a launch of their own; a step with up to kAdmitRecs records runs the small instantiation as before)
        const int batchRoom = ((useTails() && (denseForm & 4)) || ring) ? kAdmitRecsBig : kAdmitRecs;
        // the batch carries the next n vehicle numbers, each once, in any order (checked in full by the CPU twin)
        if (recs[0].vid < spawned || recs[0].vid >= spawned + n)
            return fail("cfx_step: spawn records must continue the dense vid sequence");
        if ((rc = ensureVidCap((size_t) spawned + n))) return rc;
        // a custom speed waiting for one of these vehicles has to be in the vehicle table before the admission looks at it:
        // the records then take the k_spawn_link path and the speeds follow it on the stream (rare: push_vehicle + set_vehicle_speed)
        std::vector<std::pair<int32_t, double>> customNow;
        for (const auto &fc : futureCustom)
            if (fc.first < spawned + n) customNow.push_back(fc);
        // ring layout: a step's few records go with kr_admit's arguments (each lane's thread links its own): no launch.  They
        // fit if they are few, all for lanes of this engine, and all enter at the same time (what a host spawner produces:
        // Engine::getCurrentTime); record i of the batch is vehicle spawned + i, whatever order they came in
        const bool inArgs = n <= batchRoom && customNow.empty() && spawnsInArgs(recs, n, p.batch);
        if (!inArgs && ring && n > batchRoom && customNow.empty() && !cfg.debug_sync && (rc = spawnsInMem(recs, n, p))) return rc;
        if (!inArgs && !p.inMem && (rc = spawnsByKernel(recs, n, customNow))) return rc;
        spawned += n;
        return CFX_OK;
    }

    // What the step's records mean for the host's bookkeeping: custom speeds that found no vehicle, and the slot capacity.
    // Two host-side upper bounds of the vehicles that can be running after this step:
    //   (a) spawned - finished (as of the last read)           — tight while nobody queues for long;
    //   (b) running (as of the last read) + what can have been admitted since: at most one vehicle per step on every
    //       lane that has ever had a vehicle queued, plus halo migrants — stays small when entry lanes saturate and the
    //       waiting queues grow without bound (they hold vehicle-table entries, not slots).
    // When the smaller of the two outgrows the buffers, the true count is read back and the buffers grow only if needed.
    void accountSpawns(const cfx_spawn *recs, int32_t n) {
        for (const auto &fc : futureCustom)  // (what this batch did not create was not a vehicle of this step: counted, not silent)
            if (fc.first >= spawned) droppedFutureSpeeds += 1;
        futureCustom.clear();
        for (int i = 0; i < n; ++i) {
            if (!dyadic(recs[i].enter_time)) timesDyadic = false;
            const int lane = recs[i].lane;
            if (lane >= 0 && !laneQueued[lane]) {
                laneQueued[lane] = 1;
                nQueueLanes += 1;
            }
            spawnedHere += lane >= 0;
        }
        liveUpper += nQueueLanes;
    }

    // ---- ring layout
    // kr_admit<COMMIT, N, Batch>: with or without the previous step's commit, for the records as the plan holds them
    template <bool COMMIT>
    void launchRingAdmit(const SpawnPlan &p, int blocks, const RingCtx &c, const RingCommit &rk, const RingHaloIn &hin) {
        if (p.inMem)
            launchNamed(PK_ADMIT, COMMIT ? "kr_admit<true, kBlock, SpawnBatchMem>" : "kr_admit<false, kBlock, SpawnBatchMem>",
                        CFX_BY_TEMPL(kr_admit, COMMIT, kBlock, SpawnBatchMem), dim3(blocks), dim3(kBlock), c, admitStep, waitHead, vt, sc, p.mem, rk, hin);
        else if (p.batch.n > kAdmitRecs)
            launchNamed(PK_ADMIT, COMMIT ? "kr_admit<true, kAdmitRecsBig>" : "kr_admit<false, kAdmitRecsBig>", CFX_BY_TEMPL(kr_admit, COMMIT, kAdmitRecsBig, SpawnBatchT<kAdmitRecsBig>),
                        dim3(blocks), dim3(kBlock), c, admitStep, waitHead, vt, sc, p.batch, rk, hin);
        else
            launchNamed(PK_ADMIT, COMMIT ? "kr_admit<true>" : "kr_admit<false>", CFX_BY_TEMPL(kr_admit, COMMIT, kAdmitRecs, SpawnBatchT<kAdmitRecs>), dim3(blocks), dim3(kBlock), c, admitStep,
                        waitHead, vt, sc, p.smallBatch(), rk, hin);
    }
    // kr_action<B, GHOST>: a tile's ghost lanes take the instantiations that know about frozen proxies
    template <int B>
    void launchRingLanes(dim3 grid, const RingCtx &c, const RingOut &ro, const JobQueue &jq, RingJob *jobRecs, int G, int nLaneBlocks,
                         int nLLBlocks, const RingHist &rh) {
        static_assert(B == 256 || B == 512, "the block sizes kr_action is launched with");
        if (tiled)
            launchNamed(PK_ACTION, B == 256 ? "kr_action<256, true>" : "kr_action<512, true>", CFX_BY_TEMPL(kr_action, B, true), grid, dim3(B), c, ro, jq,
                        jobRecs, G, nLaneBlocks, nLLBlocks, rh);
        else
            launchNamed(PK_ACTION, B == 256 ? "kr_action<256>" : "kr_action<512>", CFX_BY_TEMPL(kr_action, B, false), grid, dim3(B), c, ro, jq, jobRecs, G,
                        nLaneBlocks, nLLBlocks, rh);
    }

    // The action phase's organisation.  Lane walking (kr_action): one workgroup = B threads over G lanes (or B laneLinks).
    // G is picked so that a block's vehicles fit one pass (B - 1) with room for uneven lanes; small networks take small blocks
    // (every block resident at once, the step is bound by the slowest block's chain), large ones full blocks (throughput).
    // The list form (kr_index + kl_action) is the default where the cross phase runs k_cross2, and on large networks: lane
    // walking costs per lane, the list per vehicle plus 8 to 12 us for the list — 30x30, 10.8 k lanes, 90 k vehicles: 41.0 us
    // per step lane-walking, 49.0 with the list; 100x100, 120 k lanes, 72 k vehicles: 97.1 and 54.7.
    // cfx_config::ring_lanes_per_wave = G + 1000 * (B / 256) overrides G and B (developer knob; B = 256 or 512); + 20000
    // forces lane walking, + 30000 the list (+ 60000: with its tiles handed out by ticket).
    struct RingShape {
        int G, B;
        bool list;
    };
    RingShape pickRingShape(size_t activeEst, bool useBig) {
        int G = ringG, Bsel = 256;
        const int form = (cfg.ring_lanes_per_wave / 10000) % 10;
        const int want = cfg.ring_lanes_per_wave % 10000;
        if (want > 0) {
            G = std::max(1, want % 1000);
            Bsel = want >= 2000 ? 512 : 256;
        } else if (useBig || activeEst > 240000) {
            G = 28;  // many rounds of blocks anyway: full blocks, a second chunk where the lanes are dense (throughput)
        } else if (mirrorValid) {
            // adapt to the traffic: the densest block of a recent step (pinned mirror, possibly a few steps old) should
            // fit one pass with some room; results do not depend on G
            const int maxT = __atomic_load_n(&hMirror->sc.actionMaxT, __ATOMIC_RELAXED);
            if (ringHold > 0) {
                ringHold -= 1;  // (the mirror lags a few steps behind: let a change show before the next one)
            } else if (maxT > Bsel - 1) {
                ringG = std::max(4, ringG - 1);
                ringCalm = 0;
                ringHold = 8;
            } else if (maxT == 0 && ringG < 16) {  // no block above 3/4 of a pass for a while: fuller blocks
                if (++ringCalm >= 256) {
                    ringG += 1;
                    ringCalm = 0;
                }
            } else {
                ringCalm = 0;
            }
            G = ringG;
        }
        const bool list = form == 3 || form == 6 || (form == 0 && (useBig || activeEst > 240000 || L > 20000));
        return RingShape{std::min(G, Bsel), Bsel, list};
    }

    // The list form: a TRUE bound of the vehicles this step can list (the list and the launch are sized by it) — what the
    // device reported after the last step it has completed (`pr`) plus one admission per queueing lane and step since — and
    // the list grown to it.  Returns the blocks of kListBlock entries the action launch covers.
    int ringListEnsure(unsigned long long pr, int *nVehBlocksOut) {
        const int64_t done = (int64_t) (pr >> 32);
        // (a tile: plus what the halo can have brought in since — its count is as of the commit, before that step's import)
        if (done > 0 && done <= step)
            liveUpper = std::min(liveUpper, (int64_t) (pr & 0xFFFFFFFFu) + nQueueLanes * (step + 1 - done) +
                                                (tiled ? (int64_t) halo.nImport * CFX_HALO_MAX_MIGRANTS * (step + 2 - done) +
                                                             2 * (int64_t) halo.nGhost : 0));
        const size_t listBound = (size_t) std::min<int64_t>(liveUpper, (int64_t) ringSlots);
        const size_t needList = (listBound + kListBlock - 1) / kListBlock * kListBlock + kListBlock;
        if (needList > rListCap) {
            stallCause |= CFX_STALL_LIST_GROW;
            hostStats.table_grows_total += 1;
            const size_t nc = std::max(needList + needList / 4, rListCap * 2) / kListBlock * kListBlock;
            int rc = growDeferred(&rList, 0, nc);  // (rebuilt every step: nothing to keep)
            if (rc) return rc;
            rListCap = nc;
            if (!rListCount) {
                if ((rc = allocRaw(&rListCount, 2)) || (rc = allocRaw(&rIdxGranules, (size_t) gridFor(D)))) return rc;
                HIP_TRY(hipMemsetAsync(rIdxGranules, 0, (size_t) gridFor(D) * sizeof(unsigned long long), stream));
                HIP_TRY(hipMemsetAsync(rListCount, 0, 2 * sizeof(int32_t), stream));
            }
        }
        *nVehBlocksOut = (int) (needList / kListBlock);  // (every entry a block of the launch reads exists)
        return CFX_OK;
    }

    // The action phase (+ the laneLinks' notify sources, + the last step's Lane::history) in the form `shape` names
    int launchRingAction(const RingShape &shape, unsigned long long pr, const RingCtx &c, const RingOut &ro, const JobQueue &jq, RingJob *jobRecs) {
        int rc;
        if (shape.list) {
            int nVehBlocks = 0;
            if ((rc = ringListEnsure(pr, &nVehBlocks))) return rc;
            const int nLL = (K + kListBlock - 1) / kListBlock;
            const int nIdxTiles = (int) ((D + kIndexTile - 1) / kIndexTile);
            // (1024 threads: two blocks per CU.  Form 6 hands the tiles out by ticket whatever their number: the path of networks
            //  above half a million drivables, for the tests)
            const bool ticketForm = (cfg.ring_lanes_per_wave / 10000) % 10 == 6;
            int32_t *const idxTicket = (nIdxTiles > kScanResidentTiles || ticketForm) ? rListCount + 1 : nullptr;
            launchNamed(PK_SCAN, "kr_index", kr_index, dim3(nIdxTiles), dim3(kIndexBlock), c, rIdxGranules, idxTicket, (unsigned) (step + 1),
                        // (the capacity the kernel checks is what THIS step's action launch covers, not the allocation — which has
                        //  25 % of headroom and never shrinks: entries beyond the launch would never take their step, unflagged)
                        rList, (int) std::min<size_t>(rListCap, (size_t) nVehBlocks * kListBlock), rListCount, sc);
            if ((rc = debugCheck(true, "kr_index"))) return rc;
            const RingHist rh = takeHist(nVehBlocks + nLL);  // (the last step's Lane::history: trailing blocks of this launch)
            const int nHist = rh.h.num ? (L + kListBlock - 1) / kListBlock : 0;
            launchNamed(PK_ACTION, tiled ? "kl_action<true>" : "kl_action", tiled ? CFX_BY_TEMPL(kl_action, true) : CFX_BY_TEMPL(kl_action, false), dim3(nVehBlocks + nLL + nHist),
                        dim3(kListBlock), c, ro, jq, jobRecs, (const int4 *) rList, (const int32_t *) rListCount, nVehBlocks, idxTicket, rh);
            return CFX_OK;
        }
        const int G = shape.G, Bsel = shape.B;
        const int nLaneBlocks = (L + G - 1) / G, nLLBlocks = (K + Bsel - 1) / Bsel;
        // (as many blocks again at the end of the grid compute the laneLinks' notify sources)
        const RingHist rh = takeHist(nLaneBlocks + 2 * nLLBlocks);  // (the last step's Lane::history: trailing blocks of this launch)
        const dim3 grid(nLaneBlocks + 2 * nLLBlocks + (rh.h.num ? (L + Bsel - 1) / Bsel : 0));
        if (Bsel == 256) launchRingLanes<256>(grid, c, ro, jq, jobRecs, G, nLaneBlocks, nLLBlocks, rh);
        else launchRingLanes<512>(grid, c, ro, jq, jobRecs, G, nLaneBlocks, nLLBlocks, rh);
        return CFX_OK;
    }

    // The cross phase in its form for throughput (k_cross2, from the slots) or for latency (kr_cross, from the job records);
    // `lightsToo`: the kernel advances the lights, because the step's commit is deferred
    void launchRingCross(bool useBig, size_t activeEst, const RingCtx &c, const RingOut &ro, const JobQueue &jq, bool lightsToo) {
        if (useBig) {
            launchNamed(PK_CROSS, "k_cross2<false, RingCtx, RingOut>", CFX_BY_TEMPL(k_cross2, false, RingCtx, RingOut),
                        dim3((int) std::min<size_t>(std::max<size_t>(64, (activeEst / 4 + 15) / 16), (size_t) CFX_RING_CROSS2_WAVES * nCU)),  // (5 blocks per CU: 96 registers)
                        dim3(kCross2Block), c, ro, jq, RingLights{curPhase, remain, lightsToo ? 1 : 0});
            return;
        }
        // one 16-lane group per queued vehicle; sized by the decayed peak of the job counts the device has reported (every
        // block of the grid pays the prologue, so not simply by the running vehicles; the last report alone is about
        // kMaxLead + 2 steps old and follows the queue down into every all-red phase: cfx_launch_policy.h)
        static_assert(cfx_policy::kCrossLanes == kCrossGroup && cfx_policy::kCrossThreads == kCrossBlock && cfx_policy::kCrossShards == kJobShards,
                      "cfx_launch_policy.h counts in kr_cross's groups, blocks and shards");
        if (mirrorValid) {
            const int jobs = __atomic_load_n(&hMirror->sc.nCrossJobs, __ATOMIC_RELAXED);
            const int at = __atomic_load_n(&hMirror->sc.crossJobsStep, __ATOMIC_RELAXED);
            if (jobs > 0 || crossPolicy.lastStep >= 0) crossPolicy.report(at, jobs);
        } else {
            crossPolicy.reset();
        }
#ifdef CFX_CROSS_GRID_LAST_REPORT  // (measurement aid: the sizing this policy replaced, from the last report alone)
        const size_t groups = cfx_policy::crossGroups(activeEst, crossPolicy.lastStep >= 0 ? (size_t) std::max(0, __atomic_load_n(&hMirror->sc.nCrossJobs, __ATOMIC_RELAXED)) : 0);
#else
        const size_t groups = crossPolicy.groups(activeEst);
#endif
        lastCrossBlocks = cfx_policy::crossBlocks(groups, crossForceBlocks);
        launchNamed(PK_CROSS, "kr_cross", manyTempl() ? kr_cross<true> : kr_cross<false>, dim3(lastCrossBlocks), dim3(kCrossBlock), c, ro, jq, (const RingJob *) rJobRecs,
                    RingLights{curPhase, remain, lightsToo ? 1 : 0});
    }

    // debug_sync: the rings' invariants after the action phase (kr_validate)
    int ringValidate(const RingCtx &c, const JobQueue &jq) {
        HIP_TRY(hipMemsetAsync(laneOut, 0, 8 * sizeof(int32_t), stream));
        hipLaunchKernelGGL(kr_validate, dim3(gridFor(std::max(D, 16))), dim3(kBlock), 0, stream, c, jq, (int) spawned,
                           (int) hRouteStart.size() - 1, (int) ringSlots, laneOut);
        int32_t rep[5] = {0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(rep, laneOut, sizeof rep, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (rep[0]) {
            char buf[160];
            snprintf(buf, sizeof buf, "ring invariant %d violated at step %lld: %d %d %d %d", rep[0], (long long) step, rep[1], rep[2], rep[3], rep[4]);
            return fail(buf);
        }
        return CFX_OK;
    }

    // ring layout: admit, action (+ notify sources), cross, commit — no scan, no scatter
    int stepRing(const SpawnPlan &p) {
        int rc;
        RingCtx c = rctx(true);
        const bool dbg = cfg.debug_sync != 0;  // developer aid: name the kernel that faults
        if ((rc = debugCheck(true, "before the step"))) return rc;
        const unsigned long long pr = __atomic_load_n(&hMirror->progress, __ATOMIC_RELAXED);
        // running vehicles as of the last step the device has completed (stale by the few steps the host runs ahead):
        // only sizes the cross phase's grid and picks its organisation
        const size_t activeEst = (size_t) (pr & 0xFFFFFFFFu) + (size_t) nQueueLanes * 4;
        const bool useBig = cross2 >= 0 ? cross2 == 1 : activeEst > 240000;  // which form of the cross phase (§4)
        // This step's commit rides with the next step's admission (one launch less per step) where the step runs kr_cross,
        // which then advances the lights; the previous step's, if it is still pending, goes with this step's admission.
        const bool deferCommit = ringMerge && !dbg && !tiled && !observing && !devObserving && !anyTracker();  // (a caller that reads the lane counts after every step wants the commit now; so do the trackers' ticks)
        // tiling: the previous step's halo import, if cfx_halo_wait left it to this launch
        const RingHaloIn hin = haloImportPending ? pendingImport : RingHaloIn{};
        haloImportPending = false;
        if (commitPending) {
            commitPending = false;
            int nStatPrev = 1;
            const RingCommit rkPrev = commitArgs(activeEst, true, &nStatPrev);
            launchRingAdmit<true>(p, gridFor(D) + nStatPrev, rctx(true, step - 1, rcur ^ 1), rkPrev, RingHaloIn{});
        } else {
            launchRingAdmit<false>(p, gridFor(D), c, RingCommit{}, hin);
        }
        if (p.memStageUsed >= 0) {  // (the kernel reads the pinned buffer itself: free again when this launch is through)
            HIP_TRY(hipEventRecord(memStageEvent[p.memStageUsed], stream));
            memStageBusy[p.memStageUsed] = true;
        }
        if ((rc = debugCheck(true, "kr_admit"))) return rc;
        RingJob *const jobRecs = useBig ? nullptr : rJobRecs;  // k_cross2 starts from the slots: no job records then
        RingOut ro{c.kinN, c.blkW, rScratch, rMovers, sc, rFinKey, rFinVid, rFinCap, finCount};
        JobQueue jq{jobCount, rJobs, rJobCap, &sc->overflow};
        if ((rc = launchRingAction(pickRingShape(activeEst, useBig), pr, c, ro, jq, jobRecs))) return rc;
        if ((rc = debugCheck(true, "kr_action"))) return rc;
        if (dbg && (rc = ringValidate(c, jq))) return rc;
        launchRingCross(useBig, activeEst, c, ro, jq, deferCommit && !cfg.rl_traffic_light);
        if ((rc = debugCheck(true, "k_cross"))) return rc;
        if (deferCommit) {
            commitPending = true;  // launched by the next cfx_step (with its admission) or by settle()
        } else {
            int nStat = 1;
            const RingCommit rk = commitArgs(activeEst, false, &nStat);
            launchNamed(PK_COMMIT, "kr_commit", kr_commit, dim3(gridStride((size_t) std::max(D, std::max(I, nMaskWords))) + nStat), dim3(kBlock), c, rk, vt,
                        ringHalo());
            if ((rc = debugCheck(true, "kr_commit"))) return rc;
        }
        HIP_TRY(hipGetLastError());
        rcur ^= 1;
        step += 1;
        mirrorValid = !tiled;
        histPending = hist.num != 0;  // (this step's Lane::history: with the next action launch, or settle() — on a tile behind the step's halo import)
        return trackersTick();
    }

    // ---- dense layout (and lane change, which runs on it)
    // a host-side upper bound of the vehicles that can be running after this step (accountSpawns has the story)
    int64_t denseBound() const {
        const int64_t a = spawnedHere - (finishedKnown - finishedOffset);
        return tiled ? liveUpper : std::min(a, liveUpper);
    }
    int64_t shadowRoom() const { return lc.on ? poolN : 0; }  // this step's shadows
    // ... and the lanes that get them move behind the layout's end (k_lc_insert), each at most once per step, with the shadows
    // they receive: all running vehicles plus the step's shadows is a true bound of what can move (round 3 reserved a heuristic
    // quarter of the vehicles, which a dense jam in which every lane gets a shadow could exceed: ADVICE round 3)
    int64_t moveRoom() const { return lc.on ? denseBound() + shadowRoom() + 64 : (int64_t) 0; }

    // the slots the step can need, with the buffers grown to them
    int denseEnsureSlots(size_t *needOut) {
        int rc;
        const int64_t spare = tiled ? spareTotal : (int64_t) L;
        size_t need = (size_t) (denseBound() + spare + shadowRoom() + moveRoom()) + 1;
        if (need > slotCap && !tiled) {
            // the device's own count as of the last step it has completed, read without waiting for it
            const unsigned long long pr = __atomic_load_n(&hMirror->progress, __ATOMIC_RELAXED);
            const int64_t done = (int64_t) (pr >> 32);
            if (done > 0 && done <= step) {
                // since then: at most one admission per queueing lane and step, and (lane change) that step's shadows
                liveUpper = std::min(liveUpper, (int64_t) (pr & 0xFFFFFFFFu) + (nQueueLanes + shadowRoom()) * (step + 1 - done));
                need = (size_t) (denseBound() + spare + shadowRoom() + moveRoom()) + 1;
            }
        }
        if (need > slotCap) {
            DevScalars s;
            if ((rc = readScalars(s))) return rc;  // refreshes finishedKnown too
            liveUpper = s.active + 2 * (int64_t) halo.nGhost + nQueueLanes;
            need = (size_t) (denseBound() + spare + shadowRoom() + moveRoom()) + 1;
            if ((rc = ensureSlotCap(need))) return rc;
        }
        *needOut = need;
        return CFX_OK;
    }

    // kd_admit<LANES, N> over the lanes only or over every drivable, k_admit with lane change
    template <bool LANES>
    void launchDenseAdmit(const SpawnPlan &p, const StepCtx &c) {
        if (p.batch.n > kAdmitRecs)
            launchNamed(PK_ADMIT, LANES ? "kd_admit<true, kAdmitRecsBig>" : "kd_admit<false, kAdmitRecsBig>", CFX_BY_TEMPL(kd_admit, LANES, kAdmitRecsBig),
                        dim3(gridFor(LANES ? L : D)), dim3(kBlock), c, admitStep, waitHead, vt, cs, p.batch, LANES ? gatePhase : (int32_t *) nullptr);
        else
            launchNamed(PK_ADMIT, LANES ? "kd_admit<true, kAdmitRecs>" : "kd_admit<false, kAdmitRecs>", CFX_BY_TEMPL(kd_admit, LANES, kAdmitRecs),
                        dim3(gridFor(LANES ? L : D)), dim3(kBlock), c, admitStep, waitHead, vt, cs, p.smallBatch(), LANES ? gatePhase : (int32_t *) nullptr);
    }

    // Engine::nextStep engine.cpp:571-575: initSegments, planLaneChange (+ scheduleLaneChange), and the order rebuilt
    // with the step's shadows in place (cfx_lc_kernels.h)
    int stepLaneChange(StepCtx &c, size_t slotBound) {
        int rc;
        hipLaunchKernelGGL(k_lc_plan, dim3(gridStride(slotBound)), dim3(kBlock), 0, stream, c);
        if ((rc = debugCheck(false, "k_lc_plan"))) return rc;
        hipLaunchKernelGGL(k_lc_schedule, dim3(R), dim3(64), 0, stream, c, sc, (const int32_t *) vt.priority);
        if ((rc = debugCheck(false, "k_lc_schedule"))) return rc;
        hipLaunchKernelGGL(k_lc_insert, dim3(256), dim3(64), 0, stream, c, vt, sc, hPoll, oldToNew, segStart[cur].p, cnt[cur].p,
                           (int) slotCap);
        if ((rc = debugCheck(false, "k_lc_insert"))) return rc;
        HIP_TRY(hipEventRecord(pollEvent, stream));  // cfx_lane_change_poll waits for this, not for the whole step
        pollPending = true;
        HIP_TRY(hipGetLastError());
        c.admissionsVisible = 1;
        // the leader / gap pass between planLaneChange and getAction takes a history record too (engine.cpp:571-575, 429-442);
        // k_lc_insert has moved the lanes that got shadows: the context is taken anew
        if (hist.num && !tiled) hipLaunchKernelGGL(k_lane_history, dim3(gridFor(L)), dim3(kBlock), 0, stream, ctx(), hist);
        return CFX_OK;
    }

    // dense layout: admit, (lane change,) action, cross, (lane change's resolution,) scan, scatter
    int stepDense(const SpawnPlan &p) {
        int rc;
        size_t need = 0;
        if ((rc = denseEnsureSlots(&need))) return rc;
        if (lc.on) {  // per-step fields of the lane-change context
            lc.firstShadowVid = (int) spawned;
            lc.pool = hPool;  // pinned: k_lc_insert reads the few priorities it hands out straight from the host's buffer
            lc.insCap = poolN;
        }
        const bool tails = useTails();
        if (tails && !dTailNow) {
            if ((rc = allocRaw(&dTail[0], (size_t) D))) return rc;
            if ((rc = allocRaw(&dTail[1], (size_t) D))) return rc;
            if ((rc = allocRaw(&dTailNow, (size_t) D))) return rc;
            if ((rc = allocRaw(&dGate4, (size_t) std::max(K, 1)))) return rc;
        }
        StepCtx c = ctx();
        if (tails && !tailsValid) {  // after a reset / cfx_load_state: the records of the generation the step starts from
            hipLaunchKernelGGL(kd_init_tails, dim3(gridFor(D)), dim3(kBlock), 0, stream, c, dTail[0], dTail[1]);
            tailsValid = true;
        }
        // grids: the slots the layout can hold; with lane change the room reserved for moving lanes lies behind them and is
        // covered by the kernels' stride loops in the (rare) step that uses much of it
        const size_t slotBound = std::min(need - (size_t) moveRoom() + (lc.on ? (size_t) 4096 : 0), slotCap);
        // Two organisations of the cross walk: for latency (fewest dependent rounds per vehicle) and, for large networks, for
        // throughput (far fewer wave-rounds per vehicle).  They break even at ~220 k slots on the MI355X.
        const bool useBig = cross2 >= 0 ? cross2 == 1 : slotBound > 240000;
        if (lc.on && !lcSegValid) {  // after a reset / cfx_load_state
            hipLaunchKernelGGL(k_lc_naive, dim3(gridStride(slotBound)), dim3(kBlock), 0, stream, c);
            lcSegValid = true;
        }
        if (tails && c.laneAdmit) {
            if (!gatePhase) {
                if ((rc = allocRaw(&gatePhase, (size_t) 2 * std::max(I, 1)))) return rc;
                HIP_TRY(hipMemsetAsync(gatePhase, 0xFF, (size_t) 2 * std::max(I, 1) * sizeof(int32_t), stream));
            }
            launchDenseAdmit<true>(p, c);
        } else if (tails) {
            launchDenseAdmit<false>(p, c);
        } else {
            launchNamed(PK_ADMIT, "k_admit", k_admit, dim3(gridFor(D)), dim3(kBlock), c, admitStep, waitHead, vt, cs, p.smallBatch());
        }
        ActionOut ao{ab, cs, vt, sc, finList, (int) slotCap, finCount};
        if (lc.on && (rc = stepLaneChange(c, slotBound))) return rc;
        const int nxt = cur ^ 1;
        JobQueue jq{jobCount, crossJobs, (int) slotCap, &sc->overflow};
        if (tails) {
            const int nv = (int) ((slotBound + kDenseActBlock - 1) / kDenseActBlock), nl = (K + kDenseActBlock - 1) / kDenseActBlock;
            launchNamed(PK_ACTION, "kd_action", manyTempl() ? kd_action<true> : kd_action<false>, dim3(nv + nl), dim3(kDenseActBlock), c, ao, jq, nv);
        } else {  // (lane change)
            const int nVehBlocks = (int) std::min<size_t>(std::max<size_t>(1, (slotBound + kActBlock - 1) / kActBlock), 8192);
            const int nLLBlocks = (K + kActBlock - 1) / kActBlock;
            launchNamed(PK_ACTION, "k_action<true>", manyTempl() ? k_action<true> : k_action<false>, dim3(nVehBlocks + nLLBlocks), dim3(kActBlock), c, ao, jq, nVehBlocks);
        }
        if (useBig)
            // (the blocks the chip holds at once — 7 per CU: the kernel's LDS — or fewer for a short queue: the kernel sizes its batches)
            launchNamed(PK_CROSS, lc.on ? "k_cross2<true>" : "k_cross2<false>", lc.on ? CFX_BY_TEMPL(k_cross2, true, StepCtx, ActionOut) : CFX_BY_TEMPL(k_cross2, false, StepCtx, ActionOut), dim3((int) std::min<size_t>(std::max<size_t>(1, (slotBound + 15) / 16), (size_t) CFX_CROSS2_BLOCKS_PER_CU * nCU)),
                        dim3(kCross2Block), c, ao, jq, RingLights{nullptr, nullptr, 0});
        else
            launchNamed(PK_CROSS, lc.on ? "k_cross<true>" : "k_cross<false>", lc.on ? CFX_BY_TEMPL(k_cross, true, StepCtx, ActionOut) : CFX_BY_TEMPL(k_cross, false, StepCtx, ActionOut),
                        dim3((int) std::min<size_t>(std::max<size_t>(1, (slotBound * 16 + kCrossBlock - 1) / kCrossBlock), 32768)),
                        dim3(kCrossBlock), c, ao, jq);
        if (lc.on) {
            hipLaunchKernelGGL(k_lc_resolve, dim3((int) std::min<size_t>(std::max<size_t>(1, (slotBound / 8 + kBlock - 1) / kBlock), 1024)),
                               dim3(kBlock), 0, stream, c, ao, oldToNew2);
            hipLaunchKernelGGL(k_lc_resolve_rest, dim3(1), dim3(kBlock), 0, stream, c, ao, oldToNew2);
        }
        int32_t *const ticket = nScanBlocks > kScanResidentTiles ? scanTicket : nullptr;
        launchNamed(PK_SCAN, "k_scan", k_scan, dim3(nScanBlocks), dim3(kBlock), (int) D, (int) L, (const int32_t *) cnt[cur].p, cs,
                    scanGranules, ticket, (unsigned) (step + 1), segStart[nxt].p, cnt[nxt].p, gen[nxt].vid,
                    gen[nxt].drv, sc, net.laneSpare, (const int32_t *) admitStep, (int) step, waitHead, vt,
                    net.laneGhost, (const int2 *) admitRec, publishTo(), lc.on ? 1 : 0);
        // finish statistics: one extra block per 64 k slots (a rank sort of the step's finishers, see finishStatistics)
        const int nStat = (int) std::min<size_t>(std::max<size_t>(1, slotBound >> 16), 64);
        launchNamed(PK_SCATTER, lc.on ? "k_scatter<true>" : "k_scatter<false>", lc.on ? k_scatter<true> : k_scatter<false>,
                    dim3(gridStride(std::max<size_t>(slotBound, (size_t) std::max(I, nMaskWords))) + nStat), dim3(kBlock), c, ab,
                    cs, gen[nxt], (const int32_t *) segStart[nxt].p, oldToNew, curPhase, remain,
                    (int) cfg.rl_traffic_light, (int) nMaskWords, ticket, vt, sc, (const int32_t *) finList,
                    finTerm, (int) slotCap, jobCount, tiled ? (HostMirror *) nullptr : hMirror, finTicket, nStat,
                    exactTimes() ? 1 : 0, (const int32_t *) cnt[nxt].p, finCount);
        HIP_TRY(hipGetLastError());
        cur = nxt;
        step += 1;
        mirrorValid = !tiled;
        if (hist.num && !tiled) {  // Lane::updateHistory, on the committed state
            hipLaunchKernelGGL(k_lane_history, dim3(gridFor(L)), dim3(kBlock), 0, stream, ctx(), hist);
            HIP_TRY(hipGetLastError());
        }
        return trackersTick();
    }

    // (Re)build the rings: first use, a shorter vehicle template than the capacities were computed for, or growth.
    // ---- tiling on the rings: the export is part of the step's commit (RingHalo), the import a kernel of its own
    int32_t *dCutIndex = nullptr;     // [L] -1 / ghost lane i / nGhost + import lane j
    long long *dHaloActiveOut = nullptr;
    // the halo argument of the commit launched by the step that is being submitted (epoch = the step's number + 1: what
    // cfx_halo_post / cfx_halo_wait, called after cfx_step has returned, compute from the advanced step counter)
    RingHalo ringHalo() const {
        RingHalo rh{};
        if (!tiled || !ring) return rh;
        rh.on = 1;
        rh.cutIndex = dCutIndex;
        rh.activeOut = dHaloActiveOut;
        const unsigned long long epoch = ((unsigned long long) generation << 32) | (unsigned long long) (uint32_t) (step + 1);
        if (!mail.empty()) {
            rh.h = haloMail;
            const int par = (int) (epoch & 1ULL);
            for (size_t p = 0; p < mail.size(); ++p) {
                rh.io.send[p] = mail[p].sendDev + CFX_HALO_MAILBOX_HEADER + (size_t) par * mail[p].sendBytes;
                rh.io.signalFlag[p] = (unsigned long long *) mail[p].sendDev;
            }
            rh.io.nSignal = (int) mail.size();
            rh.io.ticket = haloTicket;
        } else {
            rh.h = halo;
            rh.io.send[0] = dHaloSend;  // the staged path: cfx_halo_export copies it out
        }
        rh.io.epoch = epoch;
        return rh;
    }
    bool ringGrowRequested = false;
    int ringEnsure() {
        double minLen = 1e300;
        for (const auto &t : hTempl) minLen = std::min(minLen, t.len);
        if (hTempl.empty()) minLen = 5.0;
        minLen = std::max(minLen, 0.25);
        if (ringBuilt && !(minLen < ringMinLen) && !ringGrowRequested) return CFX_OK;
        int rc;
        if ((rc = settle())) return rc;
        int32_t total = 0;
        if (ringBuilt) {  // carry the running vehicles over
            stallCause |= CFX_STALL_RING_REGROW;
            hostStats.ring_regrows_total += 1;
            if ((rc = ringGather(false, &total))) return rc;
            HIP_TRY(hipStreamSynchronize(stream));
            if ((rc = ringFree())) return rc;
            if (ringGrowRequested) ringScale *= 2;
            minLen = std::min(minLen, ringMinLen);
        }
        ringGrowRequested = false;
        if ((rc = ringAllocate(minLen))) return rc;
        ringBuilt = true;
        hipLaunchKernelGGL(kr_reset, dim3(gridFor(D)), dim3(kBlock), 0, stream, D, rHead, rCnt, rScratch);
        HIP_TRY(hipMemsetAsync(rTail[0], 0xFF, (size_t) D * sizeof(TailRec), stream));  // slot -1: empty
        HIP_TRY(hipMemsetAsync(rTail[1], 0xFF, (size_t) D * sizeof(TailRec), stream));
        if ((rc = ringClearStepTags())) return rc;
        if (total) {
            hipLaunchKernelGGL(kr_scatter_in, dim3(gridFor(D)), dim3(kBlock), 0, stream, rctx(), (const int32_t *) rOff, rd, vt);
            const int zero = 0;
            HIP_TRY(hipMemcpyAsync(&sc->ringNearFull, &zero, sizeof(int), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        return CFX_OK;
    }

    int resetState() {
        // Lane::history outlives Engine::reset (Lane::reset roadnet.cpp:832-835) and a load that does not carry it: the last
        // step's record — and the commit it reads — first
        if (histPending && ringBuilt) {
            const int rc = settle();
            if (rc) return rc;
        }
        commitPending = false;  // (whatever a deferred commit would have written is overwritten below)
        haloImportPending = false;
        histPending = false;
        HIP_TRY(hipStreamSynchronize(stream));
        if (!retired.empty() && freeRetired()) return CFX_ERR_DEVICE;
        mirrorValid = false;
        hCntValid = false;
        futureCustom.clear();
        tailsValid = false;
        if (gatePhase) HIP_TRY(hipMemsetAsync(gatePhase, 0xFF, (size_t) 2 * std::max(I, 1) * sizeof(int32_t), stream));
        if (rGatePhase) HIP_TRY(hipMemsetAsync(rGatePhase, 0xFF, (size_t) 2 * std::max(I, 1) * sizeof(int32_t), stream));
        lcSegValid = false;
        if (hMirror) hMirror->progress = 0;  // the stream is idle: nothing is writing it
        pollPending = false;
        poolN = 0;
        if (lc.on) {
            HIP_TRY(hipMemsetAsync(lc.roadCand, 0, (size_t) std::max(R, 1) * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(lc.insHead, 0xFF, (size_t) std::max(L, 1) * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(lc.parkCount, 0, 4 * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(lc.fixCount, 0, sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(lc.insCount, 0, sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(lc.candAllCount, 0, sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(lc.insLaneCount, 0, sizeof(int32_t), stream));
        }
        timesDyadic = dyadic(cfg.interval);
        cumLoaded = 0.0;
        laneQueued.assign((size_t) L, 0);
        nQueueLanes = 0;
        spawnedHere = 0;
        liveUpper = 0;
        generation += 1;
        cur = 0;
        step = 0;
        spawned = 0;
        finishedKnown = 0;
        finishedOffset = 0;
        if (!tiled) {
            hipLaunchKernelGGL(k_init_layout, dim3(gridFor(D + 1)), dim3(kBlock), 0, stream, D, L, segStart[0].p, cnt[0].p,
                               gen[0].vid, gen[0].drv);
        } else {  // lanes own laneSpare[l] empty slots each
            std::vector<int32_t> ss((size_t) D + 1);
            int32_t run = 0;
            for (int d = 0; d <= D; ++d) {
                ss[d] = run;
                if (d < L) run += hLaneSpare[d];
            }
            HIP_TRY(hipMemcpyAsync(segStart[0].p, ss.data(), ss.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemsetAsync(cnt[0].p, 0, (size_t) D * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(gen[0].vid, 0xFF, (size_t) run * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(gen[0].drv, 0xFF, (size_t) run * sizeof(int32_t), stream));
            HIP_TRY(hipMemsetAsync(gen[0].blocker, 0xFF, (size_t) run * sizeof(int32_t), stream));
            HIP_TRY(hipStreamSynchronize(stream));  // ss lives on this frame
            liveUpper = 2 * (int64_t) halo.nGhost;
        }
        if (ring && ringBuilt) {
            hipLaunchKernelGGL(kr_reset, dim3(gridFor(D)), dim3(kBlock), 0, stream, D, rHead, rCnt, rScratch);
            HIP_TRY(hipMemsetAsync(rTail[0], 0xFF, (size_t) D * sizeof(TailRec), stream));
            HIP_TRY(hipMemsetAsync(rTail[1], 0xFF, (size_t) D * sizeof(TailRec), stream));
            {
                const int rcClear = ringClearStepTags();
                if (rcClear) return rcClear;
            }
            // blocker records carry step numbers, which start over
            HIP_TRY(hipMemsetAsync(rBlk[0], 0xFF, ringSlots * sizeof(int2), stream));
            HIP_TRY(hipMemsetAsync(rBlk[1], 0xFF, ringSlots * sizeof(int2), stream));
            rcur = 0;
        }
        hipLaunchKernelGGL(k_init_lights, dim3(gridFor(I)), dim3(kBlock), 0, stream, net, curPhase, remain);
        HIP_TRY(hipMemsetAsync(waitHead, 0xFF, L * sizeof(int32_t), stream));
        HIP_TRY(hipMemsetAsync(admitStep, 0xFF, dPadded() * sizeof(int32_t), stream));
        HIP_TRY(hipMemsetAsync(interMask, 0, std::max(nMaskWords, 1) * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(sc, 0, sizeof(DevScalars), stream));
        HIP_TRY(hipMemsetAsync(scanGranules, 0, (size_t) nScanBlocks * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(scanTicket, 0, sizeof(int32_t), stream));
        if (rIdxGranules) {  // (the epochs are step numbers, which start over)
            HIP_TRY(hipMemsetAsync(rIdxGranules, 0, (size_t) gridFor(D) * sizeof(unsigned long long), stream));
            HIP_TRY(hipMemsetAsync(rListCount, 0, 2 * sizeof(int32_t), stream));
        }
        HIP_TRY(hipMemsetAsync(jobCount, 0, (size_t) kJobShards * kJobShardStride * sizeof(int32_t), stream));
        if (finCount) HIP_TRY(hipMemsetAsync(finCount, 0, (size_t) kFinShards * 32 * sizeof(int32_t), stream));
        if (finTicket) HIP_TRY(hipMemsetAsync(finTicket, 0, 4 * sizeof(int32_t), stream));
        if (dHaloActiveOut) HIP_TRY(hipMemsetAsync(dHaloActiveOut, 0, sizeof(long long), stream));
        HIP_TRY(hipMemsetAsync(oldToNew, 0xFF, slotCap * sizeof(int32_t), stream));
        if (vidCap) HIP_TRY(hipMemsetAsync(vt.nextWait, 0xFF, vidCap * sizeof(int32_t), stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        trackersRebaseline();
        return CFX_OK;
    }
};

// =============================================================================================== C ABI
extern "C" {

int32_t cfx_abi_version(void) { return CFX_ABI_VERSION; }
const char *cfx_backend_name(void) { return "hip-gfx950"; }
const char *cfx_last_error(const cfx_engine *e) { return e ? e->err.c_str() : g_createError.c_str(); }

void cfx_destroy(cfx_engine *e) {
    if (!e) return;
    (void) hipSetDevice(e->device);
    if (e->stream) (void) hipStreamSynchronize(e->stream);
    for (cfx_checkpoint *ck : e->checkpoints) {  // (they outlive the engine as empty shells: cfx_checkpoint_destroy)
        if (ck->arena) (void) hipFree(ck->arena);
        ck->arena = nullptr;
        ck->arenaCap = 0;
        ck->saved = false;
        ck->owner = nullptr;
    }
    for (void *p : e->owned) (void) hipFree(p);
    for (hipEvent_t ev : e->evPool) (void) hipEventDestroy(ev);
    for (int i = 0; i < cfx_engine::kStages; ++i) {
        if (e->hStage[i]) (void) hipHostFree(e->hStage[i]);
        if (e->hMemStage[i]) (void) hipHostFree(e->hMemStage[i]);
        if (e->memStageEvent[i]) (void) hipEventDestroy(e->memStageEvent[i]);
        if (e->stageEvent[i]) (void) hipEventDestroy(e->stageEvent[i]);
        if (e->hPhaseStage[i]) (void) hipHostFree(e->hPhaseStage[i]);
        if (e->phaseStageEvent[i]) (void) hipEventDestroy(e->phaseStageEvent[i]);
    }
    for (auto &m : e->mail) {
        if (m.sendHost) (void) hipHostUnregister(m.sendHost);
        if (m.recvHost) (void) hipHostUnregister(m.recvHost);
    }
    for (void *p : e->ipcOpened) (void) hipIpcCloseMemHandle(p);
    if (e->hLaneOut) (void) hipHostFree(e->hLaneOut);
    if (e->hCnt) (void) hipHostFree(e->hCnt);
    if (e->hMirror) (void) hipHostFree(e->hMirror);
    if (e->hHaloSend) (void) hipHostFree(e->hHaloSend);
    if (e->hHaloRecv) (void) hipHostFree(e->hHaloRecv);
    if (e->hPool) (void) hipHostFree(e->hPool);
    if (e->hPoll) (void) hipHostFree(e->hPoll);
    if (e->pollEvent) (void) hipEventDestroy(e->pollEvent);
    if (e->devInEvent) (void) hipEventDestroy(e->devInEvent);
    if (e->devOutEvent) (void) hipEventDestroy(e->devOutEvent);
    if (e->hPhaseErr) (void) hipHostFree(e->hPhaseErr);
    if (e->hPlanErr) (void) hipHostFree(e->hPlanErr);
    if (e->stream) (void) hipStreamDestroy(e->stream);
    delete e;
}

static int32_t createImpl(cfx_engine *e, const cfx_net *n, const cfx_config *cfg) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    {  // the form digit of the developer knob names a form of the step, or nothing (include/cityflow_amd.h)
        const int form = (cfg->ring_lanes_per_wave / 10000) % 10;
        if (form == 1 || form == 5 || form == 8 || form == 9) {
            e->fail("cfx_create: ringLanesPerWave = " + std::to_string(cfg->ring_lanes_per_wave) + " names no form of the step (digit " +
                    std::to_string(form) + " of cfx_config::ring_lanes_per_wave / 10000; the forms are 0, 2, 3, 4, 6, 7)");
            return CFX_ERR_INVALID;
        }
    }
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return e->fail("no HIP device visible");
    e->device = cfg->device % ndev;
    HIP_TRY(hipSetDevice(e->device));
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->device) == hipSuccess && cus > 0) e->nCU = cus;
    }
    HIP_TRY(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->cfg = *cfg;
    e->cross2 = cfg->cross_mode == CFX_CROSS_THROUGHPUT ? 1 : cfg->cross_mode == CFX_CROSS_LATENCY ? 0 : -1;
    if (cfg->layout == CFX_LAYOUT_RING && cfg->lane_change)
        return e->fail("cfx_create: layout ring does not run lane change (its mid-lane insertions use the dense layout)");
    // auto: the ring layout wherever it runs (not lane change; a tiled engine goes back to the dense layout in
    // cfx_halo_config).  It commits a step with a fraction of the dense layout's data movement; until round 5 its action
    // phase walked the lanes, which a large, sparsely filled network made slower than the dense layout (100x100: 227 vs 191
    // us) — with the list form of the action phase (kr_index + kl_action) it is ahead at every size measured: 100x100 with
    // 72 k / 277 k / 970 k running vehicles 54.7 / 86 / 141 us per step against 69.4 / 100 / 157.6 on the dense layout.
    e->ring = cfg->layout == CFX_LAYOUT_RING || (cfg->layout == CFX_LAYOUT_AUTO && !cfg->lane_change);
    e->ringMerge = (cfg->ring_lanes_per_wave / 10000) % 10 != 4;
    e->crossForceBlocks = std::max(0, cfg->ring_lanes_per_wave / 100000);
    e->denseForm = cfg->dense_form ? (cfg->dense_form & 255) : CFX_DENSE_FORM_DEFAULT;
    e->hDrvLength.assign(n->drv_length, n->drv_length + n->n_lanes + n->n_lanelinks);
    e->hLaneRoad.assign(n->lane_road, n->lane_road + n->n_lanes);
    e->hLaneIndex.assign(n->lane_index, n->lane_index + n->n_lanes);
    e->timesDyadic = cfx_engine::dyadic(cfg->interval);
    e->R = n->n_roads;
    e->L = n->n_lanes;
    e->K = n->n_lanelinks;
    e->D = e->L + e->K;
    e->I = n->n_inters;
    e->E = n->n_xentries;
    DevNet &d = e->net;
    d.R = e->R;
    d.L = e->L;
    d.K = e->K;
    d.I = e->I;
    d.E = e->E;
    int rc;
#define UP(field, src, count) \
    if ((rc = e->uploadConst(d.field, src, (size_t) (count)))) return rc;
    UP(drvLength, n->drv_length, e->D)
    if ((rc = e->upload(&e->drvMaxSpeed, n->drv_max_speed, (size_t) e->D))) return rc;  // (lanes written by cfx_set_lane_speed_limits*)
    d.drvMaxSpeed = e->drvMaxSpeed;
    if ((rc = e->upload(&e->laneLimitFile, n->drv_max_speed, (size_t) e->L))) return rc;
    UP(laneRoad, n->lane_road, e->L)
    UP(laneIndex, n->lane_index, e->L)
    UP(laneLLStart, n->lane_ll_start, e->L + 1)
    UP(laneLL, n->lane_ll, e->K)
    UP(llStartLane, n->ll_start_lane, e->K)
    UP(llEndLane, n->ll_end_lane, e->K)
    UP(llInter, n->ll_inter, e->K)
    UP(llRoadLink, n->ll_roadlink, e->K)
    UP(llType, n->ll_type, e->K)
    UP(llXStart, n->ll_x_start, e->K + 1)
    UP(xDist, n->x_dist, e->E)
    UP(xPeer, n->x_peer, e->E)
    UP(xLL, n->x_ll, e->E)
    UP(interVirtual, n->inter_virtual, e->I)
    UP(interNRL, n->inter_n_roadlinks, e->I)
    UP(interPhaseStart, n->inter_phase_start, e->I + 1)
    UP(interAvailStart, n->inter_avail_start, e->I)
    if ((rc = e->upload(&e->phaseTime, n->phase_time, (size_t) n->n_phases))) return rc;  // (written by cfx_set_tl_plan*)
    d.phaseTime = e->phaseTime;
    if ((rc = e->upload(&e->phaseTimeFile, n->phase_time, (size_t) n->n_phases))) return rc;
    e->nPhaseTimes = n->n_phases;
    for (int i = 0; i < e->I; ++i)
        if (!n->inter_virtual[i]) e->planMaxPhases = std::max(e->planMaxPhases, n->inter_phase_start[i + 1] - n->inter_phase_start[i]);
    UP(phaseAvail, n->phase_avail, n->n_avail)
#undef UP
    const size_t dPad = e->dPadded();
    for (int g = 0; g < 2; ++g) {
        if ((rc = e->allocRaw(&e->segStart[g].p, dPad + 8))) return rc;  // k_scan writes whole 8-entry groups
        if ((rc = e->allocRaw(&e->cnt[g].p, dPad))) return rc;
        HIP_TRY(hipMemset(e->cnt[g].p, 0, dPad * sizeof(int32_t)));
    }
    if ((rc = e->allocRaw(&e->cs.leaveCnt, dPad))) return rc;
    HIP_TRY(hipMemset(e->cs.leaveCnt, 0, dPad * sizeof(int32_t)));
    if ((rc = e->allocRaw(&e->cs.maxLeaveIdx, (size_t) e->D))) return rc;
    if ((rc = e->allocRaw(&e->cs.inCnt, dPad))) return rc;
    HIP_TRY(hipMemset(e->cs.inCnt, 0, dPad * sizeof(int32_t)));
    if ((rc = e->allocRaw(&e->cs.inHead, (size_t) e->D))) return rc;
    if ((rc = e->allocRaw(&e->waitHead, (size_t) e->L))) return rc;
    if ((rc = e->allocRaw(&e->admitStep, dPad))) return rc;  // lanes only are ever set; the rest stays -1 (k_scan reads 8 at a time)
    if ((rc = e->allocRaw(&e->laneOut, (size_t) e->L))) return rc;
    HIP_TRY(hipHostMalloc((void **) &e->hMirror, sizeof(HostMirror), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **) &e->hLaneOut, std::max<size_t>((size_t) e->L, 2) * sizeof(int32_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **) &e->hCnt, std::max<size_t>((size_t) e->L, 2) * sizeof(int32_t), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **) &e->hPhaseErr, 2 * sizeof(int32_t), hipHostMallocDefault));
    e->hPhaseErr[0] = -1;
    e->hPhaseErr[1] = 0;
    HIP_TRY(hipHostMalloc((void **) &e->hPlanErr, sizeof(TlPlanErr), hipHostMallocDefault));
    *e->hPlanErr = TlPlanErr{-1, 0, -1, 0, 0.0};
    HIP_TRY(hipEventCreateWithFlags(&e->devInEvent, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->devOutEvent, hipEventDisableTiming));
    if ((rc = e->allocRaw(&e->finTicket, 4))) return rc;  // [0] ticket, [2..3] 64-bit total of exactFinishStatistics
    HIP_TRY(hipMemset(e->finTicket, 0, 4 * sizeof(int32_t)));
    if ((rc = e->allocRaw(&e->finCount, (size_t) kFinShards * 32))) return rc;
    HIP_TRY(hipMemset(e->finCount, 0, (size_t) kFinShards * 32 * sizeof(int32_t)));
    if ((rc = e->allocRaw(&e->llDyn, (size_t) e->K))) return rc;
    if ((rc = e->allocRaw(&e->llGate, (size_t) e->K))) return rc;
    if ((rc = e->allocRaw(&e->laneTail, (size_t) e->L))) return rc;
    if ((rc = e->allocRaw(&e->admitRec, dPad))) return rc;
    {
        // derived tables: index of each laneLink inside its intersection (laneLinks of one intersection are
        // contiguous in RoadNet::getLaneLinks() order), the peer's bit for every cross entry, mask offsets
        std::vector<int32_t> llLocal(e->K), xPeerBit(e->E), maskStart(e->I + 1, 0), nLL(e->I, 0), first(e->I, -1);
        for (int k = 0; k < e->K; ++k) {
            int in = n->ll_inter[k];
            if (first[in] < 0) first[in] = k;
            llLocal[k] = k - first[in];
            nLL[in] = std::max(nLL[in], llLocal[k] + 1);
        }
        for (int i = 0; i < e->I; ++i) maskStart[i + 1] = maskStart[i] + (nLL[i] + 63) / 64;
        for (int x = 0; x < e->E; ++x) xPeerBit[x] = llLocal[n->x_ll[n->x_peer[x]]];
        e->nMaskWords = maskStart[e->I];
        std::vector<double2> lm((size_t) e->D), xdd((size_t) e->E);
        std::vector<int4> xpack((size_t) e->E);
        for (int dv = 0; dv < e->D; ++dv) lm[dv] = make_double2(n->drv_length[dv], n->drv_max_speed[dv]);
        for (int x = 0; x < e->E; ++x) {
            int pe = n->x_peer[x], pll = n->x_ll[pe];
            xdd[x] = make_double2(n->x_dist[x], n->x_dist[pe]);
            xpack[x] = make_int4(pll, llLocal[pll], n->ll_type[pll], n->ll_roadlink[pll]);
        }
        if ((rc = e->upload(&e->drvLM, lm.data(), lm.size()))) return rc;  // (.y of the lanes written with drvMaxSpeed)
        d.drvLM = e->drvLM;
        if ((rc = e->uploadConst(d.xDD, xdd.data(), xdd.size()))) return rc;
        if ((rc = e->uploadConst(d.xPack, xpack.data(), xpack.size()))) return rc;
        std::vector<int4> llpack((size_t) e->K);
        for (int k = 0; k < e->K; ++k)
            llpack[k] = make_int4(n->ll_x_start[k], n->ll_x_start[k + 1], maskStart[n->ll_inter[k]], n->ll_type[k]);
        if ((rc = e->uploadConst(d.llPack, llpack.data(), llpack.size()))) return rc;
        std::vector<int4> ll4((size_t) e->L), le4((size_t) e->L);
        for (int l = 0; l < e->L; ++l) {
            const int b = n->lane_ll_start[l], cnt = n->lane_ll_start[l + 1] - b;
            int v[4] = {-1, -1, -1, -1}, en[4] = {-1, -1, -1, -1};
            for (int q = 0; q < cnt && q < 4; ++q) {
                v[q] = n->lane_ll[b + q];
                en[q] = n->ll_end_lane[v[q]];
            }
            ll4[l] = cnt > 4 ? make_int4(-2, -2, -2, -2) : make_int4(v[0], v[1], v[2], v[3]);
            le4[l] = cnt > 4 ? make_int4(-1, -1, -1, -1) : make_int4(en[0], en[1], en[2], en[3]);
        }
        if ((rc = e->uploadConst(d.laneLL4, ll4.data(), ll4.size()))) return rc;
        if ((rc = e->uploadConst(d.laneEnd4, le4.data(), le4.size()))) return rc;
        if ((rc = e->uploadConst(d.llLocal, llLocal.data(), llLocal.size()))) return rc;
        if ((rc = e->uploadConst(d.xPeerBit, xPeerBit.data(), xPeerBit.size()))) return rc;
        if ((rc = e->uploadConst(d.interMaskStart, maskStart.data(), maskStart.size()))) return rc;
        if ((rc = e->allocRaw(&e->interMask, (size_t) std::max(e->nMaskWords, 1)))) return rc;
    }
    if ((rc = e->allocRaw(&e->curPhase, (size_t) e->I))) return rc;
    if ((rc = e->allocRaw(&e->remain, (size_t) e->I))) return rc;
    e->nScanBlocks = (e->D + kScanTile - 1) / kScanTile;
    if ((rc = e->allocRaw(&e->scanGranules, (size_t) e->nScanBlocks))) return rc;
    if ((rc = e->allocRaw(&e->scanTicket, 1))) return rc;
    if ((rc = e->allocRaw(&e->jobCount, (size_t) kJobShards * kJobShardStride))) return rc;
    if ((rc = e->allocRaw(&e->sc, 1))) return rc;
    if (cfg->lane_history) {
        LaneHistDev &h = e->hist;
        const size_t nL = (size_t) std::max(e->L, 1);
        h.L = e->L;
        if ((rc = e->allocRaw(&h.num, nL * kLaneHistoryMax))) return rc;
        if ((rc = e->allocRaw(&h.avg, nL * kLaneHistoryMax))) return rc;
        if ((rc = e->allocRaw(&h.head, nL))) return rc;
        if ((rc = e->allocRaw(&h.len, nL))) return rc;
        if ((rc = e->allocRaw(&h.hNum, nL))) return rc;
        if ((rc = e->allocRaw(&h.hAvg, nL))) return rc;
        HIP_TRY(hipMemset(h.num, 0, nL * kLaneHistoryMax * sizeof(int32_t)));
        HIP_TRY(hipMemset(h.avg, 0, nL * kLaneHistoryMax * sizeof(double)));
        HIP_TRY(hipMemset(h.head, 0, nL * sizeof(int32_t)));
        HIP_TRY(hipMemset(h.len, 0, nL * sizeof(int32_t)));
        HIP_TRY(hipMemset(h.hNum, 0, nL * sizeof(int32_t)));
        HIP_TRY(hipMemset(h.hAvg, 0, nL * sizeof(double)));
    }
    if (cfg->lane_change) {
        LcDev &lc = e->lc;
        lc.on = 1;
        // batched environments (cfx_config::n_envs): E disjoint copies of one network, index spaces concatenated copy by copy
        const int nEnvs = cfg->n_envs > 1 ? cfg->n_envs : 1;
        if (e->R % nEnvs != 0 || nEnvs >= (1 << (31 - kLcEnvShift))) {
            e->err = "cfx_create: n_envs does not divide the number of roads (or is too large)";
            return CFX_ERR_INVALID;
        }
        lc.roadsPerEnv = std::max(e->R / nEnvs, 1);
        lc.poolPerEnv = 0;
        if ((rc = e->uploadConst(lc.laneWidth, n->lane_width, (size_t) e->L))) return rc;
        if ((rc = e->uploadConst(lc.roadLaneStart, n->road_lane_start, (size_t) e->R + 1))) return rc;
        if ((rc = e->uploadConst(lc.laneNumSegs, n->lane_n_segments, (size_t) e->L))) return rc;
        if ((rc = e->allocRaw(&lc.roadCand, (size_t) e->R))) return rc;
        HIP_TRY(hipMemset(lc.roadCand, 0, (size_t) std::max(e->R, 1) * sizeof(int32_t)));
        if ((rc = e->allocRaw(&lc.insHead, (size_t) e->L))) return rc;
        HIP_TRY(hipMemset(lc.insHead, 0xFF, (size_t) std::max(e->L, 1) * sizeof(int32_t)));
        if ((rc = e->allocRaw(&lc.insCount, 1))) return rc;
        HIP_TRY(hipMemset(lc.insCount, 0, sizeof(int32_t)));
        if ((rc = e->allocRaw(&lc.parkCount, 4))) return rc;
        HIP_TRY(hipMemset(lc.parkCount, 0, 4 * sizeof(int32_t)));
        if ((rc = e->allocRaw(&lc.roadCandList, (size_t) std::max(e->R, 1) * kLcRoadCand))) return rc;
        if ((rc = e->allocRaw(&lc.insLanes, (size_t) e->L))) return rc;
        if ((rc = e->allocRaw(&lc.insLaneCount, 1))) return rc;
        HIP_TRY(hipMemset(lc.insLaneCount, 0, sizeof(int32_t)));
        if ((rc = e->allocRaw(&lc.fixCount, 1))) return rc;
        HIP_TRY(hipMemset(lc.fixCount, 0, sizeof(int32_t)));
        if ((rc = e->allocRaw(&lc.candAllCount, 1))) return rc;
        HIP_TRY(hipMemset(lc.candAllCount, 0, sizeof(int32_t)));
        HIP_TRY(hipEventCreateWithFlags(&e->pollEvent, hipEventDisableTiming));
    }
    // Capacities for the run, taken once: slots for half of what the network holds bumper to bumper (5 m per vehicle; the
    // dense layout only — the ring layout has its own rings), vehicle numbers for kInitialVidCap vehicles between two resets.
    // Both still grow when a run outgrows them, the vehicle tables without draining the stream (growDeferred) — but a step of
    // an ordinary run never allocates (round 4's 70 ms hiccup in the 200-step windows was the vehicle table doubling from 64 k).
    {
        size_t slots = (size_t) e->L + 4096;
        if (!e->ring) {
            double jam = 0;
            for (int d = 0; d < e->D; ++d) jam += std::ceil(e->hDrvLength[d] / 5.0);
            slots = std::max(slots, std::min<size_t>((size_t) (jam / 2) + (size_t) e->L + 4096, (size_t) 1 << 24));
        }
        if ((rc = e->ensureSlotCap(slots))) return rc;
    }
    if ((rc = e->ensureVidCap(1))) return rc;
    return e->resetState();
}

int32_t cfx_create(const cfx_net *n, const cfx_config *cfg, cfx_engine **out) {
    if (!n || !cfg || !out) {
        g_createError = "cfx_create: null argument";
        return CFX_ERR_INVALID;
    }
    if (cfg->lane_change && (!n->lane_width || !n->road_lane_start || !n->lane_n_segments)) {
        g_createError = "cfx_create: lane_change needs cfx_net::lane_width, lane_n_segments and road_lane_start";
        return CFX_ERR_INVALID;
    }
    cfx_engine *e = new cfx_engine();
    int32_t rc = createImpl(e, n, cfg);
    if (rc != CFX_OK) {
        g_createError = e->err;
        cfx_destroy(e);
        *out = nullptr;
        return rc;
    }
    *out = e;
    return CFX_OK;
}

int32_t cfx_add_templates(cfx_engine *e, int32_t n, const cfx_vehicle_template *t) {
    if (!e || n < 0 || (n && !t)) return CFX_ERR_INVALID;
    e->hTempl.insert(e->hTempl.end(), t, t + n);
    e->tablesDirty = true;
    return CFX_OK;
}

int32_t cfx_add_routes(cfx_engine *e, int32_t nRoutes, const int32_t *routeStart, const int32_t *roads,
                       const int32_t *nextStart, const int32_t *nextLL) {
    if (!e || nRoutes < 0) return CFX_ERR_INVALID;
    int roadBase = (int) e->hRouteRoads.size();
    int nextBase = (int) e->hNextLL.size();
    int nPos = routeStart[nRoutes];
    for (int r = 1; r <= nRoutes; ++r) e->hRouteStart.push_back(roadBase + routeStart[r]);
    e->hRouteRoads.insert(e->hRouteRoads.end(), roads, roads + nPos);
    for (int p = 1; p <= nPos; ++p) e->hNextStart.push_back(nextBase + nextStart[p]);
    e->hNextLL.insert(e->hNextLL.end(), nextLL, nextLL + nextStart[nPos]);
    e->tablesDirty = true;
    return CFX_OK;
}

}  // extern "C"
// One step: the parts are members of cfx_engine, in this order
static int32_t stepImpl(cfx_engine *e, const cfx_spawn *recs, int32_t n) {
    int rc;
    if ((rc = e->stepPreamble(n))) return rc;
    cfx_engine::SpawnPlan plan;
    if ((rc = e->stageSpawns(recs, n, plan))) return rc;
    e->accountSpawns(recs, n);
    return e->ring ? e->stepRing(plan) : e->stepDense(plan);
}
// A descriptor with a leading struct_size (cfx_lane_obs, cfx_vehicle_rows, cfx_movement_flow_out) as this library knows it:
// the members the caller's header did not have yet are zero in `*copy`.  CFX_ERR_INVALID otherwise, with a message where the
// caller's header is the newer one.  (A template: outside the C linkage of the entry points that use it.)
template <typename T> static int takeDescriptor(cfx_engine *e, const T *in, T *copy, const char *what) {
    if (!e || !in || in->struct_size < (int32_t) sizeof(int32_t)) return CFX_ERR_INVALID;
    if ((size_t) in->struct_size > sizeof(T)) {
        e->err = std::string(what) + ": struct_size names members this library does not know";
        return CFX_ERR_INVALID;
    }
    *copy = T{};
    memcpy(copy, in, (size_t) in->struct_size);
    return CFX_OK;
}
extern "C" {

int32_t cfx_step(cfx_engine *e, const cfx_spawn *recs, int32_t n) {
    if (!e || n < 0 || (n && !recs)) return CFX_ERR_INVALID;
    // (the host's own time in here is accounted: cfx_get_host_stats)
    e->stallCause = 0;
    const int64_t at = e->step;
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t rc = stepImpl(e, recs, n);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    cfx_host_stats &hs = e->hostStats;
    hs.step_calls += 1;
    hs.step_call_us_sum += us;
    if (us > 1000.0) hs.calls_over_1ms += 1;
    if (us > hs.worst_step_call_us) {
        hs.worst_step_call_us = us;
        hs.worst_step_call_at = at;
        hs.worst_step_call_cause = e->stallCause;
    }
    return rc;
}

int32_t cfx_get_host_stats(cfx_engine *e, cfx_host_stats *out, int32_t reset) {
    if (!e || !out) return CFX_ERR_INVALID;
    *out = e->hostStats;
    if (reset) {
        const int64_t rr = e->hostStats.ring_regrows_total, tg = e->hostStats.table_grows_total;
        e->hostStats = cfx_host_stats{};
        e->hostStats.ring_regrows_total = rr;
        e->hostStats.table_grows_total = tg;
    }
    return CFX_OK;
}

// what kr_cross's grids did (optional entry point of include/cityflow_amd.h)
int32_t cfx_get_cross_stats(cfx_engine *e, cfx_cross_stats *out, int32_t reset) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;
    DevScalars s;
    if (int rc = e->readScalars(s)) return rc;
    out->multi_pass_launches = s.crossMultiPass;
    out->max_passes = s.crossMaxPasses;
    out->last_jobs = s.nCrossJobs;
    out->last_grid_blocks = e->lastCrossBlocks;
    out->held_jobs = (int32_t) std::min<int64_t>(e->crossPolicy.held, INT32_MAX);
    out->action_multi_pass_blocks = s.actionMultiPass;
    out->action_lanes_per_block = e->ringG;
    if (reset) {  // (the stream is idle: the three counters sit side by side, here and in the pinned copy)
        static_assert(offsetof(DevScalars, actionMultiPass) == offsetof(DevScalars, crossMultiPass) + 2 * sizeof(int), "cleared together");
        HIP_TRY(hipMemsetAsync(&e->sc->crossMultiPass, 0, 3 * sizeof(int), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (e->hMirror) e->hMirror->sc.crossMultiPass = e->hMirror->sc.crossMaxPasses = e->hMirror->sc.actionMultiPass = 0;
    }
    return CFX_OK;
}

const char *cfx_profile_kernel_symbol(cfx_engine *e, int32_t k) {
    return (e && k >= 0 && k < kNumProfKernels && e->slotSymbol[k]) ? e->slotSymbol[k] : "";
}

// Lane::history as the ABI shows it: lane-major, oldest record first (the device keeps a ring per lane, record-major)
int32_t cfx_get_lane_history(cfx_engine *e, cfx_lane_history *out) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (!e->hist.num) return e->fail("cfx_get_lane_history: the engine was created without cfx_config::lane_history"), CFX_ERR_STATE;
    if (out->n_lanes != e->L) return e->fail("cfx_get_lane_history: n_lanes"), CFX_ERR_INVALID;
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle()) return rcSettle;
    // (the rings are turned into the ABI's arrays on the device: 42 MB at 30x30, which a strided loop on the host took 20 ms over)
    const size_t L = (size_t) e->L, M = (size_t) kLaneHistoryMax;
    int32_t *dNum = nullptr;
    double *dAvg = nullptr;
    if (hipMalloc((void **) &dNum, M * L * sizeof(int32_t)) != hipSuccess || hipMalloc((void **) &dAvg, M * L * sizeof(double)) != hipSuccess) {
        (void) hipFree(dNum);
        return e->fail("cfx_get_lane_history: no device memory for the staging arrays"), CFX_ERR_DEVICE;
    }
    hipLaunchKernelGGL(k_hist_export, dim3((unsigned) ((M * L + kBlock - 1) / kBlock)), dim3(kBlock), 0, e->stream, e->hist, dNum, dAvg);
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(out->vehicle_num, dNum, M * L * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(out->average_speed, dAvg, M * L * sizeof(double), hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(out->len, e->hist.len, L * 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(out->history_vehicle_num, e->hist.hNum, L * 4, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(out->history_average_speed, e->hist.hAvg, L * 8, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    (void) hipFree(dNum);
    (void) hipFree(dAvg);
    HIP_TRY(he);
    return CFX_OK;
}

int32_t cfx_set_lane_history(cfx_engine *e, const cfx_lane_history *in) {
    if (!e || !in) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (!e->hist.num) return e->fail("cfx_set_lane_history: the engine was created without cfx_config::lane_history"), CFX_ERR_STATE;
    if (in->n_lanes != e->L) return e->fail("cfx_set_lane_history: n_lanes"), CFX_ERR_INVALID;
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle()) return rcSettle;
    const size_t L = (size_t) e->L, M = (size_t) kLaneHistoryMax;
    for (size_t l = 0; l < L; ++l)
        if (in->len[l] < 0 || in->len[l] > kLaneHistoryMax) return e->fail("cfx_set_lane_history: len out of range"), CFX_ERR_INVALID;
    int32_t *dNum = nullptr;
    double *dAvg = nullptr;
    if (hipMalloc((void **) &dNum, M * L * sizeof(int32_t)) != hipSuccess || hipMalloc((void **) &dAvg, M * L * sizeof(double)) != hipSuccess) {
        (void) hipFree(dNum);
        return e->fail("cfx_set_lane_history: no device memory for the staging arrays"), CFX_ERR_DEVICE;
    }
    hipError_t he = hipMemcpyAsync(dNum, in->vehicle_num, M * L * sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(dAvg, in->average_speed, M * L * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(e->hist.len, in->len, L * 4, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(e->hist.hNum, in->history_vehicle_num, L * 4, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(e->hist.hAvg, in->history_average_speed, L * 8, hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) {
        hipLaunchKernelGGL(k_hist_import, dim3((unsigned) ((M * L + kBlock - 1) / kBlock)), dim3(kBlock), 0, e->stream, e->hist, (const int32_t *) dNum,
                           (const double *) dAvg);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    (void) hipFree(dNum);
    (void) hipFree(dAvg);
    HIP_TRY(he);
    return CFX_OK;
}

int32_t cfx_sync(cfx_engine *e) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (!e->retired.empty()) return e->freeRetired();  // (arrays a growing vehicle table left behind: the stream is idle now)
    return CFX_OK;
}

int32_t cfx_reset(cfx_engine *e) {
    if (!e) return CFX_ERR_INVALID;
    (void) hipSetDevice(e->device);
    return e->resetState();
}

int32_t cfx_set_tl_phase(cfx_engine *e, int32_t inter, int32_t phase) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (inter < 0 || inter >= e->I) {
        e->err = "cfx_set_tl_phase: intersection index out of range";
        return CFX_ERR_INVALID;
    }
    // range check against the host copy is the caller's job for speed; here only non-negativity
    if (phase < 0) {
        e->err = "cfx_set_tl_phase: negative phase";
        return CFX_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    // TrafficLight::setPhase trafficlight.cpp:39-41 (remainDuration untouched); ordered on the stream
    HIP_TRY(hipMemcpyAsync(e->curPhase + inter, &phase, sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

int32_t cfx_set_tl_phases(cfx_engine *e, int32_t n, const int32_t *inters, const int32_t *phases) {
    if (!e || n < 0 || (n && (!inters || !phases))) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    for (int i = 0; i < n; ++i)
        if (inters[i] < 0 || inters[i] >= e->I || phases[i] < 0) {
            e->err = "cfx_set_tl_phases: index out of range";
            return CFX_ERR_INVALID;
        }
    // One pinned staging buffer per call slot (ring of kStages), uploaded asynchronously on the engine's stream and
    // scattered by a tiny kernel: no synchronisation, the RL loop keeps running ahead of the device.
    const size_t need = (size_t) n * 2;
    if (need > e->phaseStageCap) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        size_t nc = std::max<size_t>(need * 2, 4096);
        for (int i = 0; i < cfx_engine::kStages; ++i) {
            if (e->hPhaseStage[i]) HIP_TRY(hipHostFree(e->hPhaseStage[i]));
            HIP_TRY(hipHostMalloc((void **) &e->hPhaseStage[i], nc * sizeof(int32_t), hipHostMallocDefault));
            if (!e->phaseStageEvent[i]) HIP_TRY(hipEventCreateWithFlags(&e->phaseStageEvent[i], hipEventDisableTiming));
            e->phaseStageBusy[i] = false;
        }
        e->phaseStageCap = nc;
    }
    const int si = e->phaseStageIdx;
    e->phaseStageIdx = (si + 1) % cfx_engine::kStages;
    if (e->phaseStageBusy[si]) HIP_TRY(hipEventSynchronize(e->phaseStageEvent[si]));
    // An intersection named more than once keeps the LAST phase, as successive TrafficLight::setPhase calls would
    // (trafficlight.cpp:39-41; a host that collects set_tl_phase calls between two steps hands them over in one call): each
    // intersection goes to the device once — k_set_phases writes one thread per pair, and two threads writing one
    // intersection's phase would leave whichever came last in time, not in the list.
    if (e->phaseSeen.size() != (size_t) e->I) e->phaseSeen.assign((size_t) e->I, 0);
    e->phaseCall += 1;
    if (e->phaseCall == INT32_MAX) {
        e->phaseSeen.assign((size_t) e->I, 0);
        e->phaseCall = 1;
    }
    {
        int32_t *outI = e->hPhaseStage[si], *outP = e->hPhaseStage[si] + n;
        int m = 0;
        for (int i = n - 1; i >= 0; --i) {  // from the back: the first one seen is the one that wins
            if (e->phaseSeen[(size_t) inters[i]] == e->phaseCall) continue;
            e->phaseSeen[(size_t) inters[i]] = e->phaseCall;
            outI[m] = inters[i];
            outP[m] = phases[i];
            ++m;
        }
        if (m < n) memmove(outI + m, outP, (size_t) m * sizeof(int32_t));  // (the kernel reads pairs[i] and pairs[m + i])
        n = m;
    }
    if (n) hipLaunchKernelGGL(k_set_phases, dim3(gridFor(n)), dim3(kBlock), 0, e->stream, e->hPhaseStage[si], n, e->curPhase);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(e->phaseStageEvent[si], e->stream));
    e->phaseStageBusy[si] = true;
    return CFX_OK;
}

int32_t cfx_get_tl_state(cfx_engine *e, int32_t *phase, double *remain) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    if (phase) HIP_TRY(hipMemcpyAsync(phase, e->curPhase, e->I * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (remain) HIP_TRY(hipMemcpyAsync(remain, e->remain, e->I * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

int32_t cfx_get_scalars(cfx_engine *e, cfx_scalars *out) {
    if (!e || !out) return CFX_ERR_INVALID;
    (void) hipSetDevice(e->device);
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    DevScalars s;
    int rc = e->readScalars(s);
    if (rc) return rc;
    out->step = e->step;
    out->active_vehicle_count = s.active;
    out->finished_vehicle_count = s.finishedCnt;
    out->spawned_vehicle_count = e->spawned;
    out->cumulative_travel_time = s.cumulativeTravelTime;
    out->live_enter_time_sum = 0.0;  // not maintained on the device path
    out->vehicle_steps = s.vehicleSteps;
    out->tie_events = s.tieEvents;
    for (int i = 0; i < 8; ++i) out->tie_drivables[i] = s.tieEvents > i ? s.tieDrv[i] : -1;
    out->diag_cross_jobs = s.nCrossJobs;
    out->dropped_future_speeds = (int32_t) std::min<int64_t>(e->droppedFutureSpeeds, INT32_MAX);
    return CFX_OK;
}

int32_t cfx_get_layout(cfx_engine *e) { return !e ? CFX_ERR_INVALID : (e->ring ? CFX_LAYOUT_RING : CFX_LAYOUT_DENSE); }
int32_t cfx_get_ring_info(cfx_engine *e, int64_t *slots, int32_t *scale) {
    if (!e) return CFX_ERR_INVALID;
    if (slots) *slots = e->ring ? (int64_t) e->ringSlots : 0;
    if (scale) *scale = e->ringScale;
    return CFX_OK;
}

int32_t cfx_get_lane_counts(cfx_engine *e, int32_t *out) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    if (e->ring && !e->ringBuilt) {  // nothing has run yet
        memset(out, 0, e->L * sizeof(int32_t));
        return CFX_OK;
    }
    e->observeIdle = 0;
    if (!(e->hCntValid && e->observing)) {  // first read (or first after a load / reset / pause): fetch, and have the steps publish from now on
        HIP_TRY(hipMemcpyAsync(e->hCnt, e->ring ? e->rCnt : e->cnt[e->cur].p, e->L * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        e->hCntValid = !e->tiled;
        e->observing = !e->tiled;
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    memcpy(out, e->hCnt, e->L * sizeof(int32_t));
    return CFX_OK;
}

// the one walk over a lane's vehicles (laneFeatures, cfx_kernels.h): a group of kFeatGroup threads per lane
static void launchLaneFeatures(cfx_engine *e, const LaneFeatOut &o) {
    const size_t threads = (size_t) e->L * kFeatGroup;
    if (e->ring) hipLaunchKernelGGL(kr_lane_features, dim3(gridFor(threads)), dim3(kBlock), 0, e->stream, e->rctx(), o);
    else hipLaunchKernelGGL(kd_lane_features, dim3(gridFor(threads)), dim3(kBlock), 0, e->stream, e->ctx(), o);
}

int32_t cfx_get_lane_waiting_counts(cfx_engine *e, int32_t *out) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    int rc;
    if ((rc = e->syncTables())) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    LaneFeatOut o{};
    o.waiting = e->laneOut;
    launchLaneFeatures(e, o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e->hLaneOut, e->laneOut, e->L * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    memcpy(out, e->hLaneOut, e->L * sizeof(int32_t));
    return CFX_OK;
}

int32_t cfx_get_vehicles(cfx_engine *e, cfx_vehicle_view *view) {
    if (!e || !view) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    int rc;
    if ((rc = e->syncTables())) return rc;
    if (e->ring) {
        // the ring order as dense arrays (kr_gather), then only the columns the caller asked for
        if ((rc = e->ringEnsure())) return rc;
        int32_t n = 0;
        if ((rc = e->ringGather(view->leader_vid || view->gap, &n))) return rc;
        view->count = n;
        if (n > view->capacity) {
            e->err = "cfx_get_vehicles: capacity too small";
            return CFX_ERR_CAPACITY;
        }
        auto dl = [&](void *dst, const void *src, size_t bytes) {
            return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream) : hipSuccess;
        };
        const size_t sn = (size_t) n;
        HIP_TRY(dl(view->vid, e->rd.vid, sn * 4));
        HIP_TRY(dl(view->drivable, e->rd.drv, sn * 4));
        HIP_TRY(dl(view->prev_drivable, e->rd.prevDrv, sn * 4));
        HIP_TRY(dl(view->leader_vid, e->rd.leaderVid, sn * 4));
        HIP_TRY(dl(view->blocker_vid, e->rd.blockerVid, sn * 4));
        HIP_TRY(dl(view->enter_ll_time, e->rd.enterLLT, sn * 4));
        HIP_TRY(dl(view->route_pos, e->rd.routePos, sn * 4));
        HIP_TRY(dl(view->dis, e->rd.dis, sn * 8));
        HIP_TRY(dl(view->speed, e->rd.speed, sn * 8));
        HIP_TRY(dl(view->gap, e->rd.gap, sn * 8));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (int i = 0; i < n; ++i) {  // no lane change on this layout
            if (view->lc_partner_vid) view->lc_partner_vid[i] = -1;
            if (view->lc_flags) view->lc_flags[i] = 0;
            if (view->lc_offset) view->lc_offset[i] = 0.0;
            if (view->lc_last_dir) view->lc_last_dir[i] = 0;
            if (view->lc_target_lane) view->lc_target_lane[i] = -1;
            if (view->lc_direction) view->lc_direction[i] = 0;
            if (view->lc_last_change_time) view->lc_last_change_time[i] = 0.0;
            if (view->lc_waiting_time) view->lc_waiting_time[i] = 0.0;
        }
        return CFX_OK;
    }
    // number of slots of the current generation
    int32_t S = 0;
    if (e->mirrorValid) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        S = e->hMirror->slots;
    } else {
        HIP_TRY(hipMemcpyAsync(&S, e->segStart[e->cur].p + e->D, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    // only what the caller asked for is computed and copied (the string getters want vid + one column)
    const bool wantLeader = view->leader_vid || view->gap, wantBlocker = view->blocker_vid != nullptr;
    if (wantLeader) {
        StepCtx c = e->ctx();
        hipLaunchKernelGGL(k_leader_view, dim3(gridStride(S)), dim3(kBlock), 0, e->stream, c, e->viewLeader, e->viewGap);
        HIP_TRY(hipGetLastError());
    }
    const SlotArrays &g = e->gen[e->cur];
    std::vector<int32_t> vid(S), drv, prev, blk, ellt, rpos, lead, o2n;
    std::vector<double> dis, speed, gap;
    auto dl = [&](void *dst, const void *src, size_t bytes) {
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream);
    };
    if (S) {
        HIP_TRY(dl(vid.data(), g.vid, S * 4));
#define WANT(field, vec, src, bytes) \
    if (field) {                      \
        vec.resize(S);                \
        HIP_TRY(dl(vec.data(), src, (size_t) S * bytes)); \
    }
        WANT(view->drivable, drv, g.drv, 4)
        WANT(view->prev_drivable, prev, g.prevDrv, 4)
        WANT(wantBlocker, blk, g.blocker, 4)
        WANT(view->enter_ll_time, ellt, g.enterLLT, 4)
        WANT(view->route_pos, rpos, g.routePos, 4)
        WANT(view->leader_vid, lead, e->viewLeader, 4)
        WANT(view->dis, dis, g.dis, 8)
        WANT(view->speed, speed, g.speed, 8)
        WANT(view->gap, gap, e->viewGap, 8)
#undef WANT
        if (wantBlocker) {
            o2n.resize(e->slotCap);
            HIP_TRY(dl(o2n.data(), e->oldToNew, e->slotCap * 4));
        }
    }
    // lane change: per-vehicle state lives in vid-indexed tables
    const bool wantLc = e->lc.on && (view->lc_partner_vid || view->lc_flags || view->lc_offset || view->lc_last_dir ||
                                     view->lc_target_lane || view->lc_direction || view->lc_last_change_time || view->gap);
    std::vector<int8_t> lcType, lcChanging, lcLastDir, lcSendDir;
    std::vector<int32_t> lcPartner, lcTarget;
    std::vector<double> lcOffset, lcLastTime, lcGap;
    if (wantLc) {
        const size_t nv = (size_t) e->spawned;
        lcType.resize(nv); lcChanging.resize(nv); lcLastDir.resize(nv); lcSendDir.resize(nv);
        lcPartner.resize(nv); lcTarget.resize(nv); lcOffset.resize(nv); lcLastTime.resize(nv); lcGap.resize(nv);
        if (nv) {
            HIP_TRY(dl(lcType.data(), e->lc.ptype, nv));
            HIP_TRY(dl(lcChanging.data(), e->lc.changing, nv));
            HIP_TRY(dl(lcLastDir.data(), e->lc.lastDir, nv));
            HIP_TRY(dl(lcSendDir.data(), e->lc.sendDir, nv));
            HIP_TRY(dl(lcPartner.data(), e->lc.partner, nv * 4));
            HIP_TRY(dl(lcTarget.data(), e->lc.sendTarget, nv * 4));
            HIP_TRY(dl(lcOffset.data(), e->lc.offset, nv * 8));
            HIP_TRY(dl(lcLastTime.data(), e->lc.lastChangeTime, nv * 8));
            HIP_TRY(dl(lcGap.data(), e->lc.gap, nv * 8));
        }
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    int n = 0;
    for (int s = 0; s < S; ++s) n += vid[s] >= 0;
    view->count = n;
    if (n > view->capacity) {
        e->err = "cfx_get_vehicles: capacity too small";
        return CFX_ERR_CAPACITY;
    }
    int i = 0;
    for (int s = 0; s < S; ++s) {
        if (vid[s] < 0) continue;
        if (view->vid) view->vid[i] = vid[s];
        if (view->drivable) view->drivable[i] = drv[s];
        if (view->prev_drivable) view->prev_drivable[i] = prev[s];
        if (view->leader_vid) view->leader_vid[i] = lead[s] >= 0 ? vid[lead[s]] : -1;
        if (view->blocker_vid) {
            if (blk[s] <= -2) {  // kept by vehicle id (a proxy on a ghost lane, see k_cross)
                view->blocker_vid[i] = -blk[s] - 2;
            } else {
                int b = blk[s] >= 0 ? o2n[blk[s]] : -1;
                int bv = b >= 0 ? vid[b] : -1;
                view->blocker_vid[i] = bv <= -2 ? -bv - 2 : bv;  // tombstone of a vehicle that migrated to a neighbour
            }
        }
        if (view->enter_ll_time) view->enter_ll_time[i] = ellt[s];
        if (view->route_pos) view->route_pos[i] = rpos[s];
        if (view->dis) view->dis[i] = dis[s];
        if (view->speed) view->speed[i] = speed[s];
        if (view->gap) view->gap[i] = gap[s];
        const int v = vid[s];
        if (wantLc && view->gap && lead[s] < 0) view->gap[i] = lcGap[v];  // ControllerInfo::gap keeps its last value
        const bool chg = wantLc && lcChanging[v];
        if (view->lc_partner_vid) view->lc_partner_vid[i] = wantLc ? lcPartner[v] : -1;
        if (view->lc_flags)
            view->lc_flags[i] = wantLc ? (uint8_t) ((lcType[v] == 2 ? CFX_LC_SHADOW : 0) | (lcType[v] == 1 ? CFX_LC_PARENT : 0) |
                                                   (chg ? CFX_LC_CHANGING : 0))
                                       : 0;
        if (view->lc_offset) view->lc_offset[i] = wantLc ? lcOffset[v] : 0.0;
        if (view->lc_last_dir) view->lc_last_dir[i] = wantLc ? lcLastDir[v] : 0;
        if (view->lc_target_lane) view->lc_target_lane[i] = chg ? lcTarget[v] : -1;
        if (view->lc_direction) view->lc_direction[i] = chg ? lcSendDir[v] : 0;
        if (view->lc_last_change_time) view->lc_last_change_time[i] = wantLc ? lcLastTime[v] : 0.0;
        if (view->lc_waiting_time) view->lc_waiting_time[i] = 0.0;  // LaneChange::waitingTime is write-only in the reference; not kept
        ++i;
    }
    return CFX_OK;
}

int32_t cfx_get_vehicle_status(cfx_engine *e, int32_t first, int32_t n, uint8_t *out) {
    if (!e || !out || first < 0 || n < 0 || (int64_t) first + n > e->spawned) {
        if (e) e->err = "cfx_get_vehicle_status: range out of bounds";
        return CFX_ERR_INVALID;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    const auto q0 = std::chrono::steady_clock::now();
    auto qus = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::micro>(b - a).count();
    };
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    const auto q1 = std::chrono::steady_clock::now();
    // A few bytes (the spawner's priority-collision query asks for ONE vehicle, in the middle of a run): through the engine's
    // pinned scratch — a device-to-host copy into the caller's pageable memory makes the runtime stage or pin it per call.
    // The call is timed (cfx_get_host_stats): behind a free-running host its cost is the wait for the stream's backlog.
    const size_t scratchBytes = std::max<size_t>((size_t) e->L, 2) * sizeof(int32_t);
    if (n && (size_t) n <= scratchBytes) {
        HIP_TRY(hipMemcpyAsync(e->hLaneOut, e->vt.state + first, (size_t) n, hipMemcpyDeviceToHost, e->stream));
        const auto q2 = std::chrono::steady_clock::now();
        HIP_TRY(hipStreamSynchronize(e->stream));
        const auto q3 = std::chrono::steady_clock::now();
        memcpy(out, e->hLaneOut, (size_t) n);
        cfx_host_stats &hs = e->hostStats;
        hs.status_queries += 1;
        if (qus(q0, q3) > hs.worst_status_query_us) {
            hs.worst_status_query_us = qus(q0, q3);
            hs.worst_status_query_settle_us = qus(q0, q1);
            hs.worst_status_query_copy_us = qus(q1, q2);
            hs.worst_status_query_wait_us = qus(q2, q3);
        }
        return CFX_OK;
    }
    if (n) HIP_TRY(hipMemcpyAsync(out, e->vt.state + first, (size_t) n, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

int32_t cfx_get_waiting(cfx_engine *e, int32_t capacity, int32_t *vid, int32_t *lane, int32_t *nOut) {
    if (!e || !nOut) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    // The waiting FIFOs are linked lists through the vid table; walk them on the host (debug / API path).
    std::vector<int32_t> head(e->L), next((size_t) e->spawned);
    HIP_TRY(hipMemcpyAsync(head.data(), e->waitHead, e->L * 4, hipMemcpyDeviceToHost, e->stream));
    if (e->spawned)
        HIP_TRY(hipMemcpyAsync(next.data(), e->vt.nextWait, (size_t) e->spawned * 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    int i = 0;
    for (int l = 0; l < e->L; ++l)
        for (int v = head[l]; v >= 0; v = next[v]) {
            if (i >= capacity) {
                e->err = "cfx_get_waiting: capacity too small";
                return CFX_ERR_CAPACITY;
            }
            if (vid) vid[i] = v;
            if (lane) lane[i] = l;
            ++i;
        }
    *nOut = i;
    return CFX_OK;
}

int32_t cfx_set_vehicle_speed(cfx_engine *e, int32_t vid, double speed) {
    if (!e) return CFX_ERR_INVALID;
    if (vid < 0 || vid >= e->spawned + CFX_FUTURE_SPEED_WINDOW) {
        e->err = "cfx_set_vehicle_speed: no such vehicle";
        return CFX_ERR_INVALID;
    }
    if (vid >= e->spawned) {
        // a vehicle the next spawn records will create (pushed since the last step): kept until then, see cfx_step — which
        // counts the speeds whose vehicle its records did not create (cfx_scalars::dropped_future_speeds)
        e->futureCustom[vid] = speed;
        return CFX_OK;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    uint8_t st = 0;
    HIP_TRY(hipMemcpyAsync(&st, e->vt.state + vid, 1, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (st == 2) {
        e->err = "cfx_set_vehicle_speed: vehicle already finished";
        return CFX_ERR_INVALID;
    }
    HIP_TRY(hipMemcpyAsync(e->vt.customSpeed + vid, &speed, sizeof(double), hipMemcpyHostToDevice, e->stream));
    if (st == 0) {
        uint8_t one = 1;
        HIP_TRY(hipMemcpyAsync(e->vt.pendingCustom + vid, &one, 1, hipMemcpyHostToDevice, e->stream));
    } else {
        int rc = e->syncTables();
        if (rc) return rc;
        if (e->ring && (rc = e->ringEnsure())) return rc;
        if (e->ring) hipLaunchKernelGGL(kr_set_speed, dim3(1), dim3(1), 0, e->stream, e->rctx(), vid);
        else hipLaunchKernelGGL(k_set_speed, dim3(gridStride(e->slotCap)), dim3(kBlock), 0, e->stream, e->ctx(), vid);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(e->stream));  // the two sources above live on this stack frame
    return CFX_OK;
}

int32_t cfx_set_vehicle_route(cfx_engine *e, int32_t vid, int32_t route) {
    if (!e || vid < 0 || vid >= e->spawned || route < 0 || route + 1 >= (int32_t) e->hRouteStart.size()) {
        if (e) e->err = "cfx_set_vehicle_route: bad vehicle or route";
        return CFX_ERR_INVALID;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    int rc = e->syncTables();
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(e->vt.route + vid, &route, sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) (e->vt.firstNext + vid), kFirstNextUnknown, 1, e->stream));  // (a waiting vehicle: its admission walks the new route)
    if (e->ring) {
        if ((rc = e->ringEnsure())) return rc;
        uint8_t st = 0;
        HIP_TRY(hipMemcpyAsync(&st, e->vt.state + vid, 1, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (st == 1) hipLaunchKernelGGL(kr_set_route, dim3(1), dim3(1), 0, e->stream, e->rctx(), vid, route);
    } else {
        hipLaunchKernelGGL(k_set_route, dim3(gridStride(e->slotCap)), dim3(kBlock), 0, e->stream, e->ctx(), vid, route);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

int32_t cfx_get_vehicle(cfx_engine *e, int32_t vid, int32_t *state, int32_t *drivable, int32_t *routePos, int32_t *route) {
    if (!e || vid < 0 || vid >= e->spawned) {
        if (e) e->err = "cfx_get_vehicle: vid out of range";
        return CFX_ERR_INVALID;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    int rc = e->syncTables();
    if (rc) return rc;
    uint8_t st = 0;
    int32_t r = -1, found[2] = {-1, -1};
    HIP_TRY(hipMemcpyAsync(&st, e->vt.state + vid, 1, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&r, e->vt.route + vid, 4, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemsetAsync(e->laneOut, 0xFF, 8, e->stream));
    if (e->ring) {
        if ((rc = e->ringEnsure())) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (st == 1) hipLaunchKernelGGL(kr_find_vehicle, dim3(1), dim3(1), 0, e->stream, e->rctx(), vid, e->laneOut);
    } else {
        hipLaunchKernelGGL(k_find_vehicle, dim3(gridStride(e->slotCap)), dim3(kBlock), 0, e->stream, e->ctx(), vid, e->laneOut);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(found, e->laneOut, 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (state) *state = st;
    if (drivable) *drivable = st == 1 ? found[0] : -1;
    if (routePos) *routePos = st == 1 ? found[1] : -1;
    if (route) *route = r;
    return CFX_OK;
}

// Lane change: the priorities the step's shadows will get, and who got one (include/cityflow_amd.h "Lane change")
int32_t cfx_lane_change_supply(cfx_engine *e, int32_t n, const int32_t *priorities) {
    if (!e || n < 0 || (n && !priorities)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (!e->lc.on) return e->fail("cfx_lane_change_supply: this engine was created without lane change"), CFX_ERR_STATE;
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if (e->pollPending) return e->fail("cfx_lane_change_supply: the previous lane-change step was not polled"), CFX_ERR_STATE;
    const int nEnvs = e->cfg.n_envs > 1 ? e->cfg.n_envs : 1;
    if (n % nEnvs != 0) return e->fail("cfx_lane_change_supply: n must be a multiple of cfx_config::n_envs"), CFX_ERR_INVALID;
    e->lc.poolPerEnv = n / nEnvs;
    if (n > e->lc.insCap || !e->hPool) {  // (re)allocate pool, records and the landing buffer of the poll
        HIP_TRY(hipStreamSynchronize(e->stream));
        const size_t cap = std::max<size_t>((size_t) n, 1024);
        if ((rc = e->grow(&e->lc.ins, 0, cap))) return rc;
        if ((rc = e->grow(&e->lc.insNext, 0, cap))) return rc;
        if ((rc = e->grow(&e->lc.insKey, 0, cap))) return rc;
        if ((rc = e->grow(&e->lc.fixList, 0, 3 * 8 * cap))) return rc;
        e->lc.fixCap = (int) (8 * cap);
        if (e->hPool) HIP_TRY(hipHostFree(e->hPool));
        if (e->hPoll) HIP_TRY(hipHostFree(e->hPoll));
        HIP_TRY(hipHostMalloc((void **) &e->hPool, cap * sizeof(int32_t), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **) &e->hPoll, (cap + 2) * sizeof(int32_t), hipHostMallocDefault));
        e->lc.insCap = (int) cap;
    }
    // (the previous step was polled, so the device is done with the pinned staging buffer)
    memcpy(e->hPool, priorities, (size_t) n * sizeof(int32_t));
    e->poolN = n;
    return CFX_OK;
}

int32_t cfx_lane_change_poll(cfx_engine *e, int32_t capacity, int32_t *parent_vid, int32_t *n) {
    if (!e || !n || capacity < 0 || (capacity && !parent_vid)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (!e->lc.on) return e->fail("cfx_lane_change_poll: this engine was created without lane change"), CFX_ERR_STATE;
    *n = 0;
    if (!e->pollPending) return CFX_OK;
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipEventSynchronize(e->pollEvent));  // plan + schedule + assign of the step; the rest keeps running
    e->pollPending = false;
    const int k = e->hPoll[0];
    if (e->hPoll[1] == 6) {
        e->err = "lane change: a capacity of the schedule walk was exceeded (shadows per road / members of a segment / "
                 "provisional neighbours in one step)";
        return CFX_ERR_CAPACITY;
    }
    if (k > e->poolN) {
        e->err = "lane change: more shadows in one step than priorities supplied (cfx_lane_change_supply)";
        return CFX_ERR_CAPACITY;
    }
    if (k > capacity) {
        e->err = "cfx_lane_change_poll: capacity too small";
        return CFX_ERR_CAPACITY;
    }
    for (int i = 0; i < k; ++i) parent_vid[i] = e->hPoll[2 + i];
    *n = k;
    e->spawned += k;  // shadows are vehicles: the next step's spawn records are numbered after them
    e->spawnedHere += k;
    e->liveUpper += k;
    return CFX_OK;
}

int32_t cfx_get_custom_speeds(cfx_engine *e, int32_t capacity, double *out) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (int rcSettle = e->settle(false)) return rcSettle;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    if (e->ring) {
        int rc;
        if ((rc = e->syncTables()) || (rc = e->ringEnsure())) return rc;
        int32_t n = 0;
        if ((rc = e->ringGather(false, &n))) return rc;
        if (n > capacity) return CFX_ERR_CAPACITY;
        std::vector<int32_t> vid((size_t) n);
        std::vector<uint8_t> flags((size_t) n);
        std::vector<double> cs((size_t) e->spawned);
        if (n) {
            HIP_TRY(hipMemcpyAsync(vid.data(), e->rd.vid, (size_t) n * 4, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipMemcpyAsync(flags.data(), e->rd.flags, (size_t) n, hipMemcpyDeviceToHost, e->stream));
        }
        if (e->spawned) HIP_TRY(hipMemcpyAsync(cs.data(), e->vt.customSpeed, (size_t) e->spawned * 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        for (int i = 0; i < n; ++i) out[i] = (flags[i] & 1) ? cs[vid[i]] : __builtin_nan("");
        return CFX_OK;
    }
    int32_t S = 0;
    HIP_TRY(hipMemcpyAsync(&S, e->segStart[e->cur].p + e->D, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::vector<int32_t> vid(S);
    std::vector<uint8_t> flags(S);
    std::vector<double> cs((size_t) e->spawned);
    if (S) {
        HIP_TRY(hipMemcpyAsync(vid.data(), e->gen[e->cur].vid, S * 4, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(flags.data(), e->gen[e->cur].flags, S, hipMemcpyDeviceToHost, e->stream));
    }
    if (e->spawned) HIP_TRY(hipMemcpyAsync(cs.data(), e->vt.customSpeed, (size_t) e->spawned * 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    int i = 0;
    for (int s = 0; s < S; ++s) {
        if (vid[s] < 0) continue;
        if (i >= capacity) return CFX_ERR_CAPACITY;
        out[i++] = (flags[s] & 1) ? cs[vid[s]] : __builtin_nan("");
    }
    return CFX_OK;
}

// Archive::resume (archive.cpp:73-126): replace the whole dynamic state.
int32_t cfx_load_state(cfx_engine *e, const cfx_state *s) {
    if (!e || !s) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->syncTables())) return rc;
    if ((rc = e->resetState())) return rc;
    const int L = e->L, D = e->D, nV = s->n_vehicles, nR = s->n_running;
    if ((rc = e->ensureVidCap((size_t) nV + 1))) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    if (!e->ring && (rc = e->ensureSlotCap((size_t) nR + (e->tiled ? (size_t) e->spareTotal : (size_t) L) + 1))) return rc;
    // ---- layout: vehicles of drivable d, then one spare slot for lanes
    std::vector<int32_t> cnt(D, 0), segStart(D + 1, 0);
    for (int i = 0; i < nR; ++i) {
        int d = s->r_drivable[i];
        if (d < 0 || d >= D || (i && d < s->r_drivable[i - 1])) return e->fail("cfx_load_state: running vehicles must be grouped by drivable, ascending");
        cnt[d]++;
    }
    auto up = [&](void *dst, const void *src, size_t bytes) {
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream) : hipSuccess;
    };
    std::vector<double> customR(std::max(nV, 1), 0.0);
    // ControllerInfo::gap as the state carries it: used instead of the derived gap in the first step (kFlagStateGap, cfx_device.h)
    std::vector<double> gapState(std::max(nV, 1), 0.0);
    auto stateGapOf = [&](int i, int v) {
        if (!s->r_gap || !(s->r_gap[i] == s->r_gap[i])) return 0;
        gapState[v] = s->r_gap[i];
        return kFlagStateGap;
    };
    if (e->ring) {
        // the caller's arrays ARE the dense staging view (Drivable::vehicles order); kr_scatter_in (below, once the vehicle
        // table is on the device) puts them on the rings
        // (rings that are too small for the archive grow first)
        if ((rc = e->ringFit(cnt.data(), "cfx_load_state"))) return rc;
        for (int d = 0; d < D; ++d) segStart[d + 1] = segStart[d] + cnt[d];
        if ((rc = e->ensureDense((size_t) nR))) return rc;
        std::vector<int32_t> blk((size_t) std::max(nR, 1), -1);
        std::vector<uint8_t> flags((size_t) std::max(nR, 1), 0);
        for (int i = 0; i < nR; ++i) {
            const int v = s->r_vid[i];
            if (v < 0 || v >= nV) return e->fail("cfx_load_state: running vid out of range");
            const int b = s->r_blocker_vid[i];
            blk[i] = (b >= 0 && b < nV) ? b : -1;
            if (s->r_custom_speed && s->r_custom_speed[i] == s->r_custom_speed[i]) {
                flags[i] = 1;
                customR[v] = s->r_custom_speed[i];
            }
            flags[i] |= (uint8_t) stateGapOf(i, v);
        }
        HIP_TRY(up(e->rOff, segStart.data(), ((size_t) D + 1) * 4));
        HIP_TRY(up(e->rd.vid, s->r_vid, (size_t) nR * 4));
        HIP_TRY(up(e->rd.prevDrv, s->r_prev_drivable, (size_t) nR * 4));
        HIP_TRY(up(e->rd.blockerVid, blk.data(), (size_t) nR * 4));
        HIP_TRY(up(e->rd.enterLLT, s->r_enter_ll_time, (size_t) nR * 4));
        HIP_TRY(up(e->rd.routePos, s->r_route_pos, (size_t) nR * 4));
        HIP_TRY(up(e->rd.flags, flags.data(), (size_t) nR));
        HIP_TRY(up(e->rd.dis, s->r_dis, (size_t) nR * 8));
        HIP_TRY(up(e->rd.speed, s->r_speed, (size_t) nR * 8));
        HIP_TRY(hipStreamSynchronize(e->stream));  // blk / flags die with this scope
    }
    // (a tile's lanes own laneSpare[l] empty slots each: room for a step's migrants on import lanes)
    for (int d = 0; d < D && !e->ring; ++d) segStart[d + 1] = segStart[d] + cnt[d] + (d < L ? (e->tiled ? (int) e->hLaneSpare[d] : 1) : 0);
    const int S = e->ring ? 0 : segStart[D];
    std::vector<int32_t> vid(S, -1), drv(S, -1), prev(S, -1), next(S, -1), blk(S, -1), ellt(S, CFX_INT_MAX), rpos(S, 0),
        templ(S, 0), route(S, 0), slotOfVid(std::max(nV, 1), -1);
    std::vector<uint8_t> flags(S, 0);
    std::vector<double> dis(S, 0.0), speed(S, 0.0), custom(std::max(nV, 1), 0.0);
    if (!e->ring) {
        std::vector<int32_t> fill(D, 0);
        for (int i = 0; i < nR; ++i) {
            int d = s->r_drivable[i];
            int sl = segStart[d] + fill[d]++;
            int v = s->r_vid[i];
            if (v < 0 || v >= nV) return e->fail("cfx_load_state: running vid out of range");
            slotOfVid[v] = sl;
            vid[sl] = v;
            drv[sl] = d;
            prev[sl] = s->r_prev_drivable[i];
            ellt[sl] = s->r_enter_ll_time[i];
            rpos[sl] = s->r_route_pos[i];
            templ[sl] = s->v_templ[v];
            route[sl] = s->v_route[v];
            dis[sl] = s->r_dis[i];
            speed[sl] = s->r_speed[i];
            if (s->r_custom_speed && s->r_custom_speed[i] == s->r_custom_speed[i]) {
                flags[sl] = 1;
                custom[v] = s->r_custom_speed[i];
            }
            flags[sl] |= (uint8_t) stateGapOf(i, v);
        }
        for (int i = 0; i < nR; ++i) {  // blockers: vid -> slot (oldToNew is reset to identity below)
            int b = s->r_blocker_vid[i];
            int bs = (b >= 0 && b < nV) ? slotOfVid[b] : -1;
            // tiling: a blocker that is the proxy on a ghost lane is kept by vehicle id (keepBlocker, cfx_kernels.h)
            if (bs >= 0 && e->tiled && drv[bs] < L && e->hLaneGhost[drv[bs]]) bs = -(b + 2);
            blk[slotOfVid[s->r_vid[i]]] = bs;
        }
    }
    // ---- uploads
    SlotArrays &g = e->gen[e->cur];
    if (e->ring) custom = customR;
    if (!e->ring) {
    HIP_TRY(up(e->segStart[e->cur].p, segStart.data(), (D + 1) * 4));
    HIP_TRY(up(e->cnt[e->cur].p, cnt.data(), D * 4));
    HIP_TRY(up(g.vid, vid.data(), S * 4));
    HIP_TRY(up(g.drv, drv.data(), S * 4));
    HIP_TRY(up(g.prevDrv, prev.data(), S * 4));
    HIP_TRY(up(g.blocker, blk.data(), S * 4));
    HIP_TRY(up(g.enterLLT, ellt.data(), S * 4));
    HIP_TRY(up(g.routePos, rpos.data(), S * 4));
    HIP_TRY(up(g.templ, templ.data(), S * 4));
    HIP_TRY(up(g.route, route.data(), S * 4));
    HIP_TRY(up(g.flags, flags.data(), S));
    HIP_TRY(up(g.dis, dis.data(), S * 8));
    HIP_TRY(up(g.speed, speed.data(), S * 8));
    std::vector<int32_t> ident(S);
    for (int i = 0; i < S; ++i) ident[i] = i;
    HIP_TRY(up(e->oldToNew, ident.data(), S * 4));
    if (e->lc.on) HIP_TRY(up(e->lc.newToOld, ident.data(), S * 4));
    HIP_TRY(hipStreamSynchronize(e->stream));
    }
    // vehicle table + waiting FIFOs
    std::vector<int32_t> nextWait(std::max(nV, 1), -1), waitHead(L, -1);
    for (int i = 0; i < s->n_waiting; ++i) {
        int v = s->w_vid[i], lane = s->w_lane[i];
        if (v < 0 || v >= nV || lane < 0 || lane >= L) return e->fail("cfx_load_state: waiting entry out of range");
        if (i > 0 && s->w_lane[i - 1] == lane) nextWait[s->w_vid[i - 1]] = v;
        else waitHead[lane] = v;
    }
    HIP_TRY(up(e->vt.priority, s->v_priority, (size_t) nV * 4));
    HIP_TRY(up(e->vt.templ, s->v_templ, (size_t) nV * 4));
    HIP_TRY(up(e->vt.route, s->v_route, (size_t) nV * 4));
    HIP_TRY(up(e->vt.enterTime, s->v_enter_time, (size_t) nV * 8));
    HIP_TRY(up(e->vt.state, s->v_state, (size_t) nV));
    HIP_TRY(up(e->vt.customSpeed, custom.data(), (size_t) nV * 8));
    HIP_TRY(up(e->vt.gapState, gapState.data(), (size_t) nV * 8));
    HIP_TRY(hipMemsetAsync(e->vt.pendingCustom, 0, std::max(nV, 1), e->stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) e->vt.firstNext, kFirstNextUnknown, (size_t) std::max(nV, 1), e->stream));  // (waiting vehicles: the walk)
    HIP_TRY(up(e->vt.nextWait, nextWait.data(), (size_t) nV * 4));
    HIP_TRY(up(e->waitHead, waitHead.data(), (size_t) L * 4));
    HIP_TRY(up(e->curPhase, s->tl_phase, (size_t) e->I * 4));
    HIP_TRY(up(e->remain, s->tl_remain, (size_t) e->I * 8));
    DevScalars sc{};
    sc.active = nR;
    if (e->tiled)  // the vehicle on a ghost lane is the frozen proxy of the owner's tail: not one of this tile's vehicles
        for (int i = 0; i < nR; ++i) sc.active -= s->r_drivable[i] < L && e->hLaneGhost[s->r_drivable[i]];
    sc.finishedCnt = s->finished_vehicle_count;
    sc.cumulativeTravelTime = s->cumulative_travel_time;
    sc.vehicleSteps = s->vehicle_steps;
    e->cumLoaded = s->cumulative_travel_time;
    for (int v = 0; v < nV; ++v)
        if (s->v_state[v] != 2 && !cfx_engine::dyadic(s->v_enter_time[v])) e->timesDyadic = false;
    HIP_TRY(up(e->sc, &sc, sizeof sc));
    e->step = s->step;
    e->spawned = nV;
    e->spawnedHere = nV;
    e->liveUpper = nR + 2 * (int64_t) e->halo.nGhost;
    for (int i = 0; i < s->n_waiting; ++i)
        if (!e->laneQueued[s->w_lane[i]]) {
            e->laneQueued[s->w_lane[i]] = 1;
            e->nQueueLanes += 1;
        }
    e->finishedKnown = s->finished_vehicle_count;
    {
        int64_t inTable = 0;
        for (int v = 0; v < nV; ++v) inTable += s->v_state[v] == 2;
        e->finishedOffset = s->finished_vehicle_count - inTable;
    }
    if (e->lc.on) {
        // lane-change tables: defaults for every vehicle number, then what the archive carries for the running ones (the
        // part of LaneChange / LaneChangeInfo that outlives a step, include/cityflow_amd.h cfx_state)
        const size_t nv = (size_t) std::max(nV, 1);
        std::vector<int8_t> ptype(nv, 0), sig(nv, 0), sdir(nv, 0), surg(nv, 0), ldir(nv, 0), chg(nv, 0), fin(nv, 0);
        std::vector<int32_t> partner(nv, -1), target(nv, -1), none(nv, -1);
        std::vector<double> offset(nv, 0.0), lastTime(nv, 0.0), gapv(nv, 0.0), zero(nv, 0.0);
        for (int i = 0; i < nR; ++i) {
            const int v = s->r_vid[i];
            if (s->r_gap) gapv[v] = s->r_gap[i];
            if (s->r_lc_flags) {
                const uint8_t f = s->r_lc_flags[i];
                ptype[v] = (f & CFX_LC_SHADOW) ? 2 : ((f & CFX_LC_PARENT) ? 1 : 0);
                chg[v] = (f & CFX_LC_CHANGING) ? 1 : 0;
            }
            if (s->r_lc_partner_vid) partner[v] = s->r_lc_partner_vid[i];
            if (s->r_lc_offset) offset[v] = s->r_lc_offset[i];
            if (s->r_lc_last_dir) ldir[v] = (int8_t) s->r_lc_last_dir[i];
            if (s->r_lc_last_change_time) lastTime[v] = s->r_lc_last_change_time[i];
            if (chg[v] && s->r_lc_target_lane && s->r_lc_direction) {  // the signal of a change in progress
                sig[v] = 1;
                surg[v] = 1;
                target[v] = s->r_lc_target_lane[i];
                sdir[v] = (int8_t) s->r_lc_direction[i];
            }
        }
        const LcDev &lc = e->lc;
        HIP_TRY(up(lc.ptype, ptype.data(), nv));
        HIP_TRY(up(lc.sigSend, sig.data(), nv));
        HIP_TRY(up(lc.sendDir, sdir.data(), nv));
        HIP_TRY(up(lc.sendUrg, surg.data(), nv));
        HIP_TRY(up(lc.lastDir, ldir.data(), nv));
        HIP_TRY(up(lc.changing, chg.data(), nv));
        HIP_TRY(up(lc.lcFinished, fin.data(), nv));
        HIP_TRY(up(lc.partner, partner.data(), nv * 4));
        HIP_TRY(up(lc.sendTarget, target.data(), nv * 4));
        HIP_TRY(up(lc.recvFrom, none.data(), nv * 4));
        HIP_TRY(up(lc.tLeader, none.data(), nv * 4));
        HIP_TRY(up(lc.tFollower, none.data(), nv * 4));
        HIP_TRY(up(lc.slotOf, slotOfVid.data(), nv * 4));
        HIP_TRY(up(lc.offset, offset.data(), nv * 8));
        HIP_TRY(up(lc.lastChangeTime, lastTime.data(), nv * 8));
        HIP_TRY(up(lc.gap, gapv.data(), nv * 8));
        HIP_TRY(up(lc.leaderGap, zero.data(), nv * 8));
        HIP_TRY(up(lc.followerGap, zero.data(), nv * 8));
        HIP_TRY(hipStreamSynchronize(e->stream));  // the staging vectors die with this scope
    }
    if (e->ring) {
        if ((rc = e->ringFromDense())) return rc;
    } else
    // cached next drivable of every slot (uses the device copies of the route tables)
    hipLaunchKernelGGL(k_refresh_next, dim3(gridStride(std::max(S, 1))), dim3(kBlock), 0, e->stream, e->ctx());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

// ---------------------------------------------------------------------------------------------- device checkpoints
// (optional entry points of include/cityflow_amd.h)

// Where a checkpoint of nR running vehicles and nV vehicle numbers keeps its arrays: one after the other from `base`, each on
// a 256-byte boundary (so that the pack kernel moves 16 bytes per lane).  Returns the bytes needed; base may be null (sizing).
static size_t checkpointLayout(cfx_checkpoint *ck, char *base, const cfx_engine *e, size_t nR, size_t nV) {
    size_t at = 0;
    auto take = [&](auto *&ptr, size_t n) {
        using T = typename std::remove_reference<decltype(*ptr)>::type;
        ptr = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at += (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t) 255;
    };
    take(ck->rd.vid, nR); take(ck->rd.drv, nR); take(ck->rd.prevDrv, nR); take(ck->rd.blockerVid, nR); take(ck->rd.enterLLT, nR);
    take(ck->rd.routePos, nR); take(ck->rd.leaderVid, nR); take(ck->rd.flags, nR); take(ck->rd.dis, nR); take(ck->rd.speed, nR);
    take(ck->rd.gap, nR);
    take(ck->off, (size_t) e->D + 1);
    take(ck->priority, nV); take(ck->templ, nV); take(ck->route, nV); take(ck->nextWait, nV); take(ck->enterTime, nV);
    take(ck->customSpeed, nV); take(ck->state, nV); take(ck->pendingCustom, nV);
    take(ck->waitHead, (size_t) e->L); take(ck->curPhase, (size_t) e->I); take(ck->remain, (size_t) e->I);
    ck->hist = LaneHistDev{};
    if (e->hist.num) {
        const size_t L = (size_t) e->L, M = (size_t) kLaneHistoryMax;
        take(ck->hist.num, M * L); take(ck->hist.avg, M * L); take(ck->hist.head, L); take(ck->hist.len, L); take(ck->hist.hNum, L);
        take(ck->hist.hAvg, L);
        ck->hist.L = e->hist.L;
    }
    return at;
}

// The segments of a save (toCheckpoint) or a restore: every array that is kept as it stands; a restore also brings the dense
// form back into the engine's staging arrays, from where the rings are rebuilt
static int checkpointPack(cfx_engine *e, cfx_checkpoint *ck, bool toCheckpoint) {
    PackTable t{};
    unsigned chunks = 0;
    bool full = false;
    auto seg = [&](auto *engineSide, auto *checkpointSide, size_t n) {
        const unsigned long long bytes = (unsigned long long) n * sizeof(*engineSide);
        static_assert(sizeof(*engineSide) == sizeof(*checkpointSide), "one element type on both sides");
        if (!bytes) return;
        if (t.n >= kPackSegs) {
            full = true;
            return;
        }
        t.src[t.n] = toCheckpoint ? (const char *) engineSide : (const char *) checkpointSide;
        t.dst[t.n] = toCheckpoint ? (char *) checkpointSide : (char *) engineSide;
        t.bytes[t.n] = bytes;
        chunks += (unsigned) ((bytes + kPackChunk - 1) / kPackChunk);
        t.chunkEnd[t.n] = chunks;
        t.n += 1;
    };
    const size_t nR = (size_t) ck->nR, nV = (size_t) ck->nV, L = (size_t) e->L, I = (size_t) e->I;
    if (!toCheckpoint) {  // (a save's dense form is written by the gather itself)
        seg(e->rd.vid, ck->rd.vid, nR); seg(e->rd.prevDrv, ck->rd.prevDrv, nR); seg(e->rd.blockerVid, ck->rd.blockerVid, nR);
        seg(e->rd.enterLLT, ck->rd.enterLLT, nR); seg(e->rd.routePos, ck->rd.routePos, nR); seg(e->rd.flags, ck->rd.flags, nR);
        seg(e->rd.dis, ck->rd.dis, nR); seg(e->rd.speed, ck->rd.speed, nR); seg(e->rd.gap, ck->rd.gap, nR);
    }
    seg(e->rOff, ck->off, (size_t) e->D + 1);
    seg(e->vt.priority, ck->priority, nV); seg(e->vt.templ, ck->templ, nV); seg(e->vt.route, ck->route, nV);
    seg(e->vt.nextWait, ck->nextWait, nV); seg(e->vt.enterTime, ck->enterTime, nV); seg(e->vt.customSpeed, ck->customSpeed, nV);
    seg(e->vt.state, ck->state, nV); seg(e->vt.pendingCustom, ck->pendingCustom, nV);
    seg(e->waitHead, ck->waitHead, L); seg(e->curPhase, ck->curPhase, I); seg(e->remain, ck->remain, I);
    if (e->hist.num && ck->hist.num) {
        const size_t M = (size_t) kLaneHistoryMax;
        seg(e->hist.num, ck->hist.num, M * L); seg(e->hist.avg, ck->hist.avg, M * L); seg(e->hist.head, ck->hist.head, L);
        seg(e->hist.len, ck->hist.len, L); seg(e->hist.hNum, ck->hist.hNum, L); seg(e->hist.hAvg, ck->hist.hAvg, L);
    }
    if (full) return e->fail("device checkpoint: more segments than the pack kernel's table holds (internal error)");
    if (!chunks) return CFX_OK;
    t.chunks = chunks;
    hipLaunchKernelGGL(k_pack_segments, dim3(std::min(chunks, 2048u)), dim3(kPackBlock), 0, e->stream, t);
    if (hipGetLastError() != hipSuccess) return e->fail("device checkpoint: the pack launch failed");
    return CFX_OK;
}

int32_t cfx_checkpoint_create(cfx_engine *e, cfx_checkpoint **out) {
    if (!e || !out) return CFX_ERR_INVALID;
    *out = nullptr;
    if (!e->ring || e->lc.on || e->tiled) {
        e->err = std::string("cfx_checkpoint_create: device checkpoints exist on the ring layout only; this engine ") +
                 (e->lc.on ? "runs with lane_change" : (e->tiled ? "is a tile" : "uses the dense layout"));
        return CFX_ERR_STATE;
    }
    cfx_checkpoint *ck = new cfx_checkpoint();
    ck->owner = e;
    e->checkpoints.push_back(ck);
    *out = ck;
    return CFX_OK;
}

int32_t cfx_checkpoint_save(cfx_engine *e, cfx_checkpoint *ck) {
    if (!e || !ck) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (ck->owner != e) {
        e->err = "cfx_checkpoint_save: the checkpoint belongs to another engine";
        return CFX_ERR_INVALID;
    }
    if (!e->ring || e->lc.on || e->tiled) return e->fail("cfx_checkpoint_save: the engine has left the ring layout"), CFX_ERR_STATE;
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->settle())) return rc;  // (a deferred commit, the last step's Lane::history record)
    if ((rc = e->syncTables()) || (rc = e->ringEnsure())) return rc;
    ck->saved = false;
    // the scalars and the per-drivable counts ride with the wait for the number of running vehicles
    ck->cnt.assign((size_t) e->D, 0);
    HIP_TRY(hipMemcpyAsync(&ck->sc, e->sc, sizeof(DevScalars), hipMemcpyDeviceToHost, e->stream));
    if (e->D) HIP_TRY(hipMemcpyAsync(ck->cnt.data(), e->rCnt, (size_t) e->D * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    int32_t total = 0;
    if ((rc = e->ringOffsets(&total))) return rc;
    e->finishedKnown = ck->sc.finishedCnt;
    if (ck->sc.overflow) {
        DevScalars s;
        return (rc = e->readScalars(s)) ? rc : e->fail("cfx_checkpoint_save: the device reported a capacity overflow");
    }
    const size_t need = checkpointLayout(ck, nullptr, e, (size_t) total, (size_t) e->spawned);
    if (need > ck->arenaCap) {
        if (ck->arena) HIP_TRY(hipFree(ck->arena));  // (waits for the device: nothing reads it any more)
        ck->arena = nullptr;
        ck->arenaCap = 0;
        const size_t cap = need + need / 8;  // (a checkpoint that is overwritten as the traffic grows does not reallocate every time)
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, cap));
        ck->arena = (char *) p;
        ck->arenaCap = cap;
    }
    checkpointLayout(ck, ck->arena, e, (size_t) total, (size_t) e->spawned);
    ck->nR = total;
    ck->nV = (int32_t) e->spawned;
    if ((rc = e->ringGatherInto(ck->rd, total, true))) return rc;
    if ((rc = checkpointPack(e, ck, true))) return rc;
    ck->step = e->step;
    ck->finishedOffset = e->finishedOffset;
    ck->laneQueued = e->laneQueued;
    ck->nQueueLanes = e->nQueueLanes;
    ck->futureCustom = e->futureCustom;
    ck->timesDyadic = e->timesDyadic;
    ck->saved = true;
    return CFX_OK;
}

// cfx_load_state's ring branch with the checkpoint's arrays as the sources
int32_t cfx_checkpoint_restore(cfx_engine *e, cfx_checkpoint *ck) {
    if (!e || !ck) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (ck->owner != e || !ck->saved) {
        e->err = ck->owner != e ? "cfx_checkpoint_restore: the checkpoint belongs to another engine" : "cfx_checkpoint_restore: nothing was saved into the checkpoint";
        return CFX_ERR_INVALID;
    }
    if (!e->ring || e->lc.on || e->tiled) return e->fail("cfx_checkpoint_restore: the engine has left the ring layout"), CFX_ERR_STATE;
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->syncTables())) return rc;
    if ((rc = e->resetState())) return rc;
    const int nV = ck->nV, nR = ck->nR;
    if ((rc = e->ensureVidCap((size_t) nV + 1))) return rc;
    if ((rc = e->ringEnsure())) return rc;
    if ((rc = e->ringFit(ck->cnt.data(), "cfx_checkpoint_restore"))) return rc;
    if ((rc = e->ensureDense((size_t) nR))) return rc;
    if ((rc = checkpointPack(e, ck, false))) return rc;
    if (nR) hipLaunchKernelGGL(k_checkpoint_state_gap, dim3(gridFor((size_t) nR)), dim3(kBlock), 0, e->stream, nR, (const int32_t *) e->rd.vid,
                               (const double *) e->rd.gap, e->rd.flags, e->vt.gapState, nV);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) e->vt.firstNext, kFirstNextUnknown, (size_t) std::max(nV, 1), e->stream));  // (waiting vehicles: the walk)
    DevScalars sc{};
    sc.active = nR;
    sc.finishedCnt = ck->sc.finishedCnt;
    sc.cumulativeTravelTime = ck->sc.cumulativeTravelTime;
    sc.vehicleSteps = ck->sc.vehicleSteps;
    HIP_TRY(hipMemcpyAsync(e->sc, &sc, sizeof sc, hipMemcpyHostToDevice, e->stream));
    e->cumLoaded = sc.cumulativeTravelTime;
    e->timesDyadic = ck->timesDyadic;
    e->step = ck->step;
    e->spawned = nV;
    e->spawnedHere = nV;
    e->liveUpper = nR;
    e->laneQueued = ck->laneQueued;
    e->nQueueLanes = ck->nQueueLanes;
    e->futureCustom = ck->futureCustom;
    e->finishedKnown = sc.finishedCnt;
    e->finishedOffset = ck->finishedOffset;
    if ((rc = e->ringFromDense())) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (`sc` lives on this frame)
    return CFX_OK;
}

// cfx_checkpoint_restore with every environment taking another's state: the same reset, capacity checks, ring growth and
// rebuild; the checkpoint's arrays come through the three k_env_gather_* kernels instead of the pack, and what the restore
// takes from the checkpoint's host part is put together from the environments taken
int32_t cfx_checkpoint_restore_envs(cfx_engine *e, cfx_checkpoint *ck, const cfx_env_gather *g) {
    if (!e || !ck || !g) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (ck->owner != e || !ck->saved) {
        e->err = ck->owner != e ? "cfx_checkpoint_restore_envs: the checkpoint belongs to another engine" : "cfx_checkpoint_restore_envs: nothing was saved into the checkpoint";
        return CFX_ERR_INVALID;
    }
    if (!e->ring || e->lc.on || e->tiled) return e->fail("cfx_checkpoint_restore_envs: the engine has left the ring layout"), CFX_ERR_STATE;
    auto invalid = [e](const std::string &m) {
        e->err = "cfx_checkpoint_restore_envs: " + m;
        return CFX_ERR_INVALID;
    };
    // ---- the tables: nothing that is not checked here indexes device memory below
    const int nE = e->cfg.n_envs > 1 ? e->cfg.n_envs : 1, nOld = ck->nV, nNew = g->n_new;
    const int nRoutes = (int) e->hRouteStart.size() - 1;
    if (g->n_envs != nE) return invalid("n_envs is not the engine's");
    if (e->L % nE || e->K % nE || e->I % nE || nRoutes % nE) return invalid("the environments do not divide the network or the routes evenly");
    if (g->n_old != nOld) return invalid("n_old is not the checkpoint's number of vehicle numbers");
    if (nNew < 0 || !g->src_env || !g->env_first || (nOld && (!g->old_env || !g->old_local)) || (nNew && !g->new_src)) return invalid("a table is missing");
    if (ck->finishedOffset != 0) {
        e->err = "cfx_checkpoint_restore_envs: the checkpoint counts finished vehicles that are not in its vehicle table (a state loaded from an archive)";
        return CFX_ERR_STATE;
    }
    const int Lpe = e->L / nE, Kpe = e->K / nE, Ipe = e->I / nE, L = e->L, D = e->D;
    std::vector<int32_t> perEnv((size_t) nE, 0);
    for (int o = 0; o < nOld; ++o) {
        if (g->old_env[o] < 0 || g->old_env[o] >= nE || g->old_local[o] < 0) return invalid("old_env / old_local: entry out of range");
        perEnv[(size_t) g->old_env[o]] += 1;
    }
    if (g->env_first[0] != 0 || g->env_first[nE] != nNew) return invalid("env_first does not span the new numbers");
    for (int r = 0; r < nE; ++r) {
        const int s = g->src_env[r];
        if (s < 0 || s >= nE) return invalid("src_env: entry out of range");
        if (g->env_first[r + 1] - g->env_first[r] != perEnv[(size_t) s]) return invalid("env_first: an environment's numbers are not its source's");
        for (int v = g->env_first[r]; v < g->env_first[r + 1]; ++v) {
            const int o = g->new_src[v];
            if (o < 0 || o >= nOld || g->old_env[o] != s || g->old_local[o] != v - g->env_first[r]) return invalid("new_src does not match old_env / old_local");
        }
    }
    // ---- per drivable: the vehicles after the call, where they start, and the two runs of every environment
    auto srcDrv = [&](int d) { return d < L ? d + (g->src_env[d / Lpe] - d / Lpe) * Lpe : d + (g->src_env[(d - L) / Kpe] - (d - L) / Kpe) * Kpe; };
    std::vector<int32_t> srcOff((size_t) D + 1, 0), cnt((size_t) D, 0), off((size_t) D + 1, 0);
    for (int d = 0; d < D; ++d) srcOff[(size_t) d + 1] = srcOff[(size_t) d] + ck->cnt[(size_t) d];
    if (srcOff[(size_t) D] != ck->nR) return e->fail("cfx_checkpoint_restore_envs: the checkpoint's counts do not add up (internal error)");
    for (int d = 0; d < D; ++d) {
        cnt[(size_t) d] = ck->cnt[(size_t) srcDrv(d)];
        if ((int64_t) off[(size_t) d] + cnt[(size_t) d] > INT32_MAX) return e->fail("cfx_checkpoint_restore_envs: more than 2^31 running vehicles");
        off[(size_t) d + 1] = off[(size_t) d] + cnt[(size_t) d];
    }
    const int nR = off[(size_t) D];
    // one upload: srcEnv, envFirst, runDst, runSrc, oldLocal, newSrc, newEnv, then the counter of finished vehicles (8 bytes, aligned)
    const size_t aSrcEnv = 0, aEnvFirst = aSrcEnv + nE, aRunDst = aEnvFirst + nE, aRunSrc = aRunDst + 2 * (size_t) nE + 1,
                 aOldLocal = aRunSrc + 2 * (size_t) nE, aNewSrc = aOldLocal + (size_t) nOld, aNewEnv = aNewSrc + (size_t) nNew,
                 aFinished = (aNewEnv + (size_t) nNew + 1) & ~(size_t) 1, nWords = aFinished + 2;
    std::vector<int32_t> h(nWords, 0);
    for (int r = 0; r < nE; ++r) {
        const int s = g->src_env[r];
        h[aSrcEnv + r] = s;
        h[aEnvFirst + r] = g->env_first[r];
        h[aRunDst + r] = off[(size_t) r * Lpe];
        h[aRunDst + nE + r] = off[(size_t) L + (size_t) r * Kpe];
        h[aRunSrc + r] = srcOff[(size_t) s * Lpe];
        h[aRunSrc + nE + r] = srcOff[(size_t) L + (size_t) s * Kpe];
        std::fill(h.begin() + aNewEnv + g->env_first[r], h.begin() + aNewEnv + g->env_first[r + 1], r);
    }
    h[aRunDst + 2 * (size_t) nE] = nR;
    if (nOld) std::copy(g->old_local, g->old_local + nOld, h.begin() + aOldLocal);
    if (nNew) std::copy(g->new_src, g->new_src + nNew, h.begin() + aNewSrc);

    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->syncTables())) return rc;
    if ((rc = e->resetState())) return rc;
    if ((rc = e->ensureVidCap((size_t) nNew + 1))) return rc;
    if ((rc = e->ringEnsure())) return rc;
    if ((rc = e->ringFit(cnt.data(), "cfx_checkpoint_restore_envs"))) return rc;
    if ((rc = e->ensureDense((size_t) nR))) return rc;
    if (nWords > e->envGather.cap) {
        const size_t nc = nWords + nWords / 4;
        if ((rc = e->freeRaw(&e->envGather.p)) || (rc = e->allocRaw(&e->envGather.p, nc))) return rc;
        e->envGather.cap = nc;
    }
    int32_t *t = e->envGather.p;
    HIP_TRY(hipMemcpyAsync(t, h.data(), nWords * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->rOff, off.data(), ((size_t) D + 1) * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    EnvGather eg{};
    eg.nEnvs = nE, eg.lanesPerEnv = Lpe, eg.linksPerEnv = Kpe, eg.intersPerEnv = Ipe, eg.routesPerEnv = nRoutes / nE;
    eg.nOld = nOld, eg.nNew = nNew;
    eg.srcEnv = t + aSrcEnv, eg.envFirst = t + aEnvFirst, eg.oldLocal = t + aOldLocal, eg.newSrc = t + aNewSrc, eg.newEnv = t + aNewEnv;
    eg.runDst = t + aRunDst, eg.runSrc = t + aRunSrc;
    unsigned long long *dFinished = reinterpret_cast<unsigned long long *>(t + aFinished);
    if (nR) hipLaunchKernelGGL(k_env_gather_running, dim3(gridFor((size_t) nR)), dim3(kBlock), 0, e->stream, eg, nR, ck->rd, e->rd, e->vt.gapState);
    if (nNew) {
        const EnvGatherTable src{ck->priority, ck->templ, ck->route, ck->nextWait, ck->enterTime, ck->customSpeed, ck->state, ck->pendingCustom};
        hipLaunchKernelGGL(k_env_gather_table, dim3(gridFor((size_t) nNew)), dim3(kBlock), 0, e->stream, eg, src, e->vt, dFinished);
    }
    {
        EnvGatherNet src{ck->waitHead, ck->curPhase, ck->remain, ck->hist};
        LaneHistDev hist = e->hist;
        if (!ck->hist.num) hist.num = nullptr;
        hipLaunchKernelGGL(k_env_gather_net, dim3(gridFor((size_t) std::max(e->L, e->I))), dim3(kBlock), 0, e->stream, eg, src, e->waitHead, e->curPhase,
                           e->remain, hist);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t) e->vt.firstNext, kFirstNextUnknown, (size_t) std::max(nNew, 1), e->stream));  // (waiting vehicles: the walk)
    unsigned long long finished = 0;
    HIP_TRY(hipMemcpyAsync(&finished, dFinished, sizeof finished, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (`h`, `off` and `finished` live on this frame)
    DevScalars sc{};
    sc.active = nR;
    sc.finishedCnt = (long long) finished;
    // (the travel-time sum and the vehicle steps are kept per engine, not per environment: the checkpoint's totals stand)
    sc.cumulativeTravelTime = ck->sc.cumulativeTravelTime;
    sc.vehicleSteps = ck->sc.vehicleSteps;
    HIP_TRY(hipMemcpyAsync(e->sc, &sc, sizeof sc, hipMemcpyHostToDevice, e->stream));
    e->cumLoaded = sc.cumulativeTravelTime;
    e->timesDyadic = ck->timesDyadic;
    e->step = ck->step;
    e->spawned = nNew;
    e->spawnedHere = nNew;
    e->liveUpper = nR;
    e->nQueueLanes = 0;
    for (int l = 0; l < L; ++l) {
        e->laneQueued[(size_t) l] = ck->laneQueued[(size_t) srcDrv(l)];
        e->nQueueLanes += e->laneQueued[(size_t) l] ? 1 : 0;
    }
    e->finishedKnown = sc.finishedCnt;
    e->finishedOffset = 0;
    if ((rc = e->ringFromDense())) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (`sc` lives on this frame)
    return CFX_OK;
}

int32_t cfx_checkpoint_info(const cfx_checkpoint *ck, cfx_checkpoint_desc *out) {
    if (!ck || !out) return CFX_ERR_INVALID;
    out->step = ck->saved ? ck->step : -1;
    out->device_bytes = (int64_t) ck->arenaCap;
    out->n_running = ck->saved ? ck->nR : 0;
    out->n_vehicles = ck->saved ? ck->nV : 0;
    return CFX_OK;
}

void cfx_checkpoint_destroy(cfx_checkpoint *ck) {
    if (!ck) return;
    if (cfx_engine *e = ck->owner) {
        (void) hipSetDevice(e->device);
        if (ck->arena) (void) hipFree(ck->arena);  // (waits for the device: a pack launch may still be reading it)
        e->checkpoints.erase(std::remove(e->checkpoints.begin(), e->checkpoints.end(), ck), e->checkpoints.end());
    }
    delete ck;
}

// ---------------------------------------------------------------------------------------------- tiling
int32_t cfx_halo_config(cfx_engine *e, const cfx_halo_layout *h) {
    if (!e || !h || h->n_ghost < 0 || h->n_import < 0) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (e->tiled || e->step != 0 || e->spawned != 0) {
        e->err = "cfx_halo_config: must be called once, right after cfx_create";
        return CFX_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(e->device));
    // Tiles run on either layout.  On the rings (round 6; `layout: ring`, and what `auto` resolves to unless the developer knob
    // cfx_config::ring_lanes_per_wave / 10000 == 7 asks for the dense tiles of rounds 2-5) the halo export is part of the step's
    // commit and the import one small kernel: 5 launches per tile-step instead of 7.
    if (e->ring && e->cfg.layout == CFX_LAYOUT_AUTO && (e->cfg.ring_lanes_per_wave / 10000) % 10 == 7) e->ring = false;
    std::vector<uint8_t> ghost((size_t) e->L, 0);
    e->hLaneSpare.assign((size_t) e->L, 1);
    for (int i = 0; i < h->n_ghost; ++i) {
        if (h->ghost_lane[i] < 0 || h->ghost_lane[i] >= e->L) return CFX_ERR_INVALID;
        ghost[h->ghost_lane[i]] = 1;
    }
    for (int i = 0; i < h->n_import; ++i) {
        if (h->import_lane[i] < 0 || h->import_lane[i] >= e->L) return CFX_ERR_INVALID;
        e->hLaneSpare[h->import_lane[i]] = 1 + CFX_HALO_MAX_MIGRANTS;
    }
    e->hLaneGhost = ghost;
    e->spareTotal = 0;
    for (uint8_t v : e->hLaneSpare) e->spareTotal += v;
    int rc;
    if ((rc = e->uploadConst(e->net.laneGhost, ghost.data(), ghost.size()))) return rc;
    if (e->ring) {
        std::vector<int32_t> cut((size_t) e->L, -1);
        for (int i = 0; i < h->n_ghost; ++i) cut[(size_t) h->ghost_lane[i]] = i;
        for (int j = 0; j < h->n_import; ++j) {
            if (cut[(size_t) h->import_lane[j]] >= 0) return e->fail("cfx_halo_config: a lane is both a ghost and an import lane");
            cut[(size_t) h->import_lane[j]] = h->n_ghost + j;
        }
        if ((rc = e->upload(&e->dCutIndex, cut.data(), cut.size()))) return rc;
        if ((rc = e->allocRaw(&e->dHaloActiveOut, 1))) return rc;
        HIP_TRY(hipMemset(e->dHaloActiveOut, 0, sizeof(long long)));
    }
    if ((rc = e->uploadConst(e->net.laneSpare, e->hLaneSpare.data(), e->hLaneSpare.size()))) return rc;
    HaloDev &d = e->halo;
    d.nGhost = h->n_ghost;
    d.nImport = h->n_import;
    if ((rc = e->uploadConst(d.ghostLane, h->ghost_lane, (size_t) h->n_ghost))) return rc;
    if ((rc = e->uploadConst(d.ghostSendOff, h->ghost_send_off, (size_t) h->n_ghost))) return rc;
    if ((rc = e->uploadConst(d.ghostRecvOff, h->ghost_recv_off, (size_t) h->n_ghost))) return rc;
    if ((rc = e->uploadConst(d.importLane, h->import_lane, (size_t) h->n_import))) return rc;
    if ((rc = e->uploadConst(d.importRecvOff, h->import_recv_off, (size_t) h->n_import))) return rc;
    if ((rc = e->uploadConst(d.importSendOff, h->import_send_off, (size_t) h->n_import))) return rc;
    if ((rc = e->uploadConst(d.llGlobal, h->lanelink_global, (size_t) e->K))) return rc;
    if ((rc = e->uploadConst(d.llLocalOfGlobal, h->lanelink_local, (size_t) h->n_global_lanelinks))) return rc;
    if ((rc = e->allocRaw(&d.ghostHadEntrants, (size_t) h->n_ghost))) return rc;
    {
        std::vector<int32_t> zeros((size_t) std::max(h->n_ghost, h->n_import) + 1, 0);
        if ((rc = e->uploadConst(d.ghostPeer, zeros.data(), (size_t) h->n_ghost))) return rc;
        if ((rc = e->uploadConst(d.importPeer, zeros.data(), (size_t) h->n_import))) return rc;
    }
    e->hGhostSendOff.assign(h->ghost_send_off, h->ghost_send_off + h->n_ghost);
    e->hGhostRecvOff.assign(h->ghost_recv_off, h->ghost_recv_off + h->n_ghost);
    e->hImportSendOff.assign(h->import_send_off, h->import_send_off + h->n_import);
    e->hImportRecvOff.assign(h->import_recv_off, h->import_recv_off + h->n_import);
    e->haloSendBytes = h->send_bytes;
    e->haloRecvBytes = h->recv_bytes;
    if ((rc = e->allocRaw(&e->dHaloSend, (size_t) h->send_bytes))) return rc;
    if ((rc = e->allocRaw(&e->dHaloRecv, (size_t) h->recv_bytes))) return rc;
    HIP_TRY(hipHostMalloc((void **) &e->hHaloSend, std::max(h->send_bytes, 1), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **) &e->hHaloRecv, std::max(h->recv_bytes, 1), hipHostMallocDefault));
    e->tiled = true;
    if ((rc = e->ensureSlotCap((size_t) e->spareTotal + 4096))) return rc;
    return e->resetState();
}

int32_t cfx_halo_export(cfx_engine *e, void *sendHost) {
    if (!e || !e->tiled) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    const int n = e->halo.nGhost + e->halo.nImport;
    HaloIO io{};
    io.send[0] = e->dHaloSend;
    // (ring layout: the step's commit has written the messages already — RingHalo)
    if (n && !e->ring) hipLaunchKernelGGL(k_halo_export, dim3(gridFor(n)), dim3(kBlock), 0, e->stream, e->ctx(), e->cnt[e->cur].p, e->halo,
                                          e->cs.inCnt, io, e->sc);
    HIP_TRY(hipGetLastError());
    if (e->haloSendBytes && sendHost) HIP_TRY(hipMemcpyAsync(e->hHaloSend, e->dHaloSend, (size_t) e->haloSendBytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (device-to-device transports run on another stream: the message is complete)
    if (e->haloSendBytes && sendHost) memcpy(sendHost, e->hHaloSend, (size_t) e->haloSendBytes);
    return CFX_OK;
}

int32_t cfx_halo_import(cfx_engine *e, const void *recvHost) {
    if (!e || !e->tiled) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipStreamSynchronize(e->stream));  // the pinned staging buffer of the previous import may still be read
    if (e->haloRecvBytes && recvHost) {
        memcpy(e->hHaloRecv, recvHost, (size_t) e->haloRecvBytes);
        HIP_TRY(hipMemcpyAsync(e->dHaloRecv, e->hHaloRecv, (size_t) e->haloRecvBytes, hipMemcpyHostToDevice, e->stream));
    }
    const int n = e->halo.nGhost + e->halo.nImport;
    HaloIO io{};
    io.recv[0] = e->dHaloRecv;
    if (n && e->ring) {
        hipLaunchKernelGGL(kr_halo_import, dim3(gridFor(n)), dim3(kBlock), 0, e->stream, e->rctx(), e->halo, io, e->vt, e->sc, e->dHaloActiveOut);
        e->hCntValid = false;
    } else if (n) hipLaunchKernelGGL(k_halo_import, dim3(gridFor(n)), dim3(kBlock), 0, e->stream, e->ctx(), e->cnt[e->cur].p, e->halo,
                              io, e->vt, e->sc);
    HIP_TRY(hipGetLastError());
    e->liveUpper += (int64_t) e->halo.nImport * CFX_HALO_MAX_MIGRANTS;
    return CFX_OK;
}

int32_t cfx_halo_attach(cfx_engine *e, int32_t nPeers, const cfx_halo_peer *peers) {
    if (!e || !e->tiled || nPeers < 0 || (nPeers && !peers)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (nPeers > CFX_HALO_MAX_PEERS) {
        e->err = "cfx_halo_attach: more neighbour tiles than CFX_HALO_MAX_PEERS";
        return CFX_ERR_CAPACITY;
    }
    if (!e->mail.empty()) {
        e->err = "cfx_halo_attach: already attached";
        return CFX_ERR_STATE;
    }
    HIP_TRY(hipSetDevice(e->device));
    e->mail.resize((size_t) nPeers);
    for (int p = 0; p < nPeers; ++p) {
        cfx_engine::MailPeer &m = e->mail[p];
        m.sendBytes = peers[p].send_bytes;
        m.recvBytes = peers[p].recv_bytes;
        if (!peers[p].send_mailbox || !peers[p].recv_mailbox) return CFX_ERR_INVALID;
        if (peers[p].device_memory) {
            // mailboxes in HBM: mine (recv) on this GPU, the peer's (send) on its GPU — opened through IPC by the caller, or a
            // plain pointer of another GPU of this process, which needs peer access
            m.sendDev = (char *) peers[p].send_mailbox;
            m.recvDev = (char *) peers[p].recv_mailbox;
            hipPointerAttribute_t attr{};
            if (hipPointerGetAttributes(&attr, m.sendDev) == hipSuccess && attr.device != e->device) {
                hipError_t pe = hipDeviceEnablePeerAccess(attr.device, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) return e->fail("cfx_halo_attach: no peer access to the neighbour tile's GPU");
                (void) hipGetLastError();
            }
            continue;
        }
        m.sendHost = peers[p].send_mailbox;
        m.recvHost = peers[p].recv_mailbox;
        HIP_TRY(hipHostRegister(m.sendHost, CFX_HALO_MAILBOX_BYTES(m.sendBytes), hipHostRegisterMapped | hipHostRegisterPortable));
        HIP_TRY(hipHostRegister(m.recvHost, CFX_HALO_MAILBOX_BYTES(m.recvBytes), hipHostRegisterMapped | hipHostRegisterPortable));
        HIP_TRY(hipHostGetDevicePointer((void **) &m.sendDev, m.sendHost, 0));
        HIP_TRY(hipHostGetDevicePointer((void **) &m.recvDev, m.recvHost, 0));
    }
    // address every block as (peer, offset inside that peer's message)
    auto split = [&](const std::vector<int32_t> &off, bool send, std::vector<int32_t> &peer, std::vector<int32_t> &rel) {
        peer.resize(off.size());
        rel.resize(off.size());
        for (size_t i = 0; i < off.size(); ++i) {
            int found = -1;
            for (int p = 0; p < nPeers; ++p) {
                const int lo = send ? peers[p].send_off : peers[p].recv_off;
                const int n = send ? peers[p].send_bytes : peers[p].recv_bytes;
                if (off[i] >= lo && off[i] < lo + n) {
                    found = p;
                    rel[i] = off[i] - lo;
                }
            }
            if (found < 0) return false;
            peer[i] = found;
        }
        return true;
    };
    std::vector<int32_t> gp, gs, gp2, gr, ip, is, ip2, ir;
    if (!split(e->hGhostSendOff, true, gp, gs) || !split(e->hGhostRecvOff, false, gp2, gr) ||
        !split(e->hImportSendOff, true, ip, is) || !split(e->hImportRecvOff, false, ip2, ir) || gp != gp2 || ip != ip2) {
        e->err = "cfx_halo_attach: peer slices do not cover the halo layout";
        return CFX_ERR_INVALID;
    }
    HaloDev &d = e->haloMail;
    d = e->halo;  // lanes, maps, ghostHadEntrants are shared with the staged path
    int rc;
    if ((rc = e->uploadConst(d.ghostPeer, gp.data(), gp.size()))) return rc;
    if ((rc = e->uploadConst(d.ghostSendOff, gs.data(), gs.size()))) return rc;
    if ((rc = e->uploadConst(d.ghostRecvOff, gr.data(), gr.size()))) return rc;
    if ((rc = e->uploadConst(d.importPeer, ip.data(), ip.size()))) return rc;
    if ((rc = e->uploadConst(d.importSendOff, is.data(), is.size()))) return rc;
    if ((rc = e->uploadConst(d.importRecvOff, ir.data(), ir.size()))) return rc;
    if ((rc = e->allocRaw(&e->haloTicket, 1))) return rc;
    HIP_TRY(hipMemset(e->haloTicket, 0, sizeof(int32_t)));
    return CFX_OK;
}

int32_t cfx_halo_mailbox_alloc(cfx_engine *e, int32_t messageBytes, void **devicePtr, uint8_t *handle) {
    if (!e || !e->tiled || messageBytes < 0 || !devicePtr || !handle) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    static_assert(sizeof(hipIpcMemHandle_t) <= CFX_IPC_HANDLE_BYTES, "IPC handle size");
    const size_t bytes = CFX_HALO_MAILBOX_BYTES(messageBytes);
    void *p = nullptr;
    // fine-grained device memory first (stores of a kernel on ANOTHER GPU become visible while both kernels run); a plain
    // allocation if the platform cannot export that
    hipIpcMemHandle_t h;
    bool ok = hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) == hipSuccess && hipIpcGetMemHandle(&h, p) == hipSuccess;
    if (!ok) {
        (void) hipGetLastError();
        if (p) (void) hipFree(p);
        p = nullptr;
        e->mailboxesFineGrained = false;
        if (hipMalloc(&p, bytes) != hipSuccess || hipIpcGetMemHandle(&h, p) != hipSuccess) {
            (void) hipGetLastError();
            if (p) (void) hipFree(p);
            e->err = "cfx_halo_mailbox_alloc: device memory cannot be shared with other processes on this platform";
            return CFX_ERR_STATE;
        }
    }
    e->owned.push_back(p);
    HIP_TRY(hipMemset(p, 0, bytes));  // epoch 0 = nothing published
    memset(handle, 0, CFX_IPC_HANDLE_BYTES);
    memcpy(handle, &h, sizeof h);
    *devicePtr = p;
    return CFX_OK;
}

int32_t cfx_halo_mailbox_fine_grained(cfx_engine *e) { return e && e->mailboxesFineGrained ? 1 : 0; }

int32_t cfx_device_memory(cfx_engine *e, int64_t *free_bytes, int64_t *total_bytes) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    size_t f = 0, t = 0;
    HIP_TRY(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t) f;
    if (total_bytes) *total_bytes = (int64_t) t;
    return CFX_OK;
}

int32_t cfx_device_identity(cfx_engine *e, char *buf, int32_t capacity) {
    if (!e || !buf || capacity < 2) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipDeviceGetPCIBusId(buf, capacity, e->device));
    buf[capacity - 1] = 0;
    return CFX_OK;
}

int32_t cfx_halo_mailbox_open(cfx_engine *e, const uint8_t *handle, void **devicePtr) {
    if (!e || !e->tiled || !handle || !devicePtr) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof h);
    void *p = nullptr;
    if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        (void) hipGetLastError();
        e->err = "cfx_halo_mailbox_open: hipIpcOpenMemHandle failed";
        return CFX_ERR_STATE;
    }
    e->ipcOpened.push_back(p);
    *devicePtr = p;
    return CFX_OK;
}

int32_t cfx_halo_device_buffers(cfx_engine *e, void **sendDev, void **recvDev) {
    if (!e || !e->tiled) return CFX_ERR_INVALID;
    if (sendDev) *sendDev = e->dHaloSend;
    if (recvDev) *recvDev = e->dHaloRecv;
    return CFX_OK;
}

// epoch of the step that has just been launched: (generation, step) packed, monotonic over resets
static inline unsigned long long haloEpoch(const cfx_engine *e) {
    return ((unsigned long long) e->generation << 32) | (unsigned long long) (uint32_t) e->step;
}

int32_t cfx_halo_post(cfx_engine *e) {
    if (!e || !e->tiled) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    const unsigned long long epoch = haloEpoch(e);
    const int par = (int) (epoch & 1ULL);
    HaloIO io{};
    const int nPeers = (int) e->mail.size();
    for (int p = 0; p < nPeers; ++p) {
        io.send[p] = e->mail[p].sendDev + CFX_HALO_MAILBOX_HEADER + (size_t) par * e->mail[p].sendBytes;
        io.signalFlag[p] = (unsigned long long *) e->mail[p].sendDev;
    }
    io.nSignal = nPeers;
    io.ticket = e->haloTicket;
    io.epoch = epoch;
    const int n = e->halo.nGhost + e->halo.nImport;  // every peer implies at least one cut lane, so n > 0 with peers
    if (n && !e->ring) {  // (ring layout: the step's commit wrote the messages and published the epoch — RingHalo)
        e->launchNamed(PK_HALO_EXPORT, "k_halo_export", k_halo_export, dim3(gridFor(n)), dim3(kBlock), e->ctx(), e->cnt[e->cur].p, e->haloMail,
                  (const int32_t *) e->cs.inCnt, io, e->sc);
    }
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

int32_t cfx_halo_wait(cfx_engine *e) {
    if (!e || !e->tiled) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    const unsigned long long epoch = haloEpoch(e);
    const int par = (int) (epoch & 1ULL);
    HaloIO io{};
    const int nPeers = (int) e->mail.size();
    for (int p = 0; p < nPeers; ++p) {
        io.recv[p] = e->mail[p].recvDev + CFX_HALO_MAILBOX_HEADER + (size_t) par * e->mail[p].recvBytes;
        io.waitFlag[p] = (const unsigned long long *) e->mail[p].recvDev;
    }
    io.nWait = nPeers;
    io.epoch = epoch;
    const int n = e->halo.nGhost + e->halo.nImport;
    if (n && e->ring) {
        // (left to the next step's admission launch — kr_admit, RingHaloIn; a getter in between sends it out itself: settle())
        e->pendingImport = RingHaloIn{1, e->dCutIndex, e->haloMail, io, e->dHaloActiveOut};
        e->haloImportPending = true;
    } else if (n) {  // includes the wait for the neighbours' epochs
        e->launchNamed(PK_HALO_IMPORT, "k_halo_import", k_halo_import, dim3(gridFor(n)), dim3(kBlock), e->ctx(), e->cnt[e->cur].p, e->haloMail, io,
                  e->vt, e->sc);
    }
    HIP_TRY(hipGetLastError());
    e->liveUpper += (int64_t) e->halo.nImport * CFX_HALO_MAX_MIGRANTS;
    return CFX_OK;
}

#ifdef CFX_TRACE
// developer build: dump the action kernel's per-block phase stamps of the LAST step to a file (raw int64[blocks][8])
int32_t cfx_trace_dump(const char *path, int32_t blocks) {
    static long long *buf = nullptr;
    if (!buf) {
        (void) hipMalloc((void **) &buf, (size_t) 65536 * 8 * sizeof(long long));
        (void) hipMemset(buf, 0, (size_t) 65536 * 8 * sizeof(long long));
        (void) hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof buf);
        return 0;
    }
    (void) hipDeviceSynchronize();
    if (blocks < 0) {  // clear the stamps (a kernel whose blocks do not all stamp in every step)
        (void) hipMemset(buf, 0, (size_t) 65536 * 8 * sizeof(long long));
        return 0;
    }
    std::vector<long long> h((size_t) blocks * 8);
    (void) hipMemcpy(h.data(), buf, h.size() * sizeof(long long), hipMemcpyDeviceToHost);
    FILE *f = fopen(path, "wb");
    if (!f) return -1;
    fwrite(h.data(), sizeof(long long), h.size(), f);
    fclose(f);
    return 0;
}
#endif

__global__ void k_device_spin(long long ticks, double *sink) {  // wall_clock64: 100 MHz on gfx950
    const long long t0 = (long long) wall_clock64();
    double x = 1.0 + threadIdx.x * 1e-9;
    while ((long long) wall_clock64() - t0 < ticks)
        for (int i = 0; i < 64; ++i) x = x * 1.0000001 + 1e-12;
    if (x == 0.12345) *sink = x;
}

int32_t cfx_device_spin(cfx_engine *e, int64_t microseconds) {
    if (!e || microseconds < 0) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (microseconds > 2000000) microseconds = 2000000;
    hipLaunchKernelGGL(k_device_spin, dim3(1024), dim3(256), 0, e->stream, (long long) microseconds * 100LL, (double *) e->sc);
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

// ---- observations and signals in device memory (torch tensors), ordered against the caller's stream (the optional entry
// points of include/cityflow_amd.h: declared there as the types of the symbols, which the asserts at the end of this file hold
// the definitions to)
int32_t cfx_stream_handle(cfx_engine *e, void **stream, int32_t *device) {
    if (!e) return CFX_ERR_INVALID;
    if (stream) *stream = (void *) e->stream;
    if (device) *device = e->device;
    return CFX_OK;
}

int32_t cfx_set_tl_phases_device(cfx_engine *e, const int32_t *phases, int32_t n, void *producerStream) {
    if (!e || !phases || n != e->I) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->checkDevicePointer(phases, "cfx_set_tl_phases_device", "phases"))) return rc;
    if ((rc = e->settle(false))) return rc;  // (as cfx_set_tl_phases: the deferred commit advances the lights of the last step first)
    if ((rc = e->orderAfterCaller((hipStream_t) producerStream))) return rc;
    hipLaunchKernelGGL(k_set_phases_dense, dim3(1), dim3(1024), 0, e->stream, phases, n, e->net.interPhaseStart,
                       e->net.interVirtual, e->curPhase, e->hPhaseErr);
    HIP_TRY(hipGetLastError());
    return e->orderCallerAfter((hipStream_t) producerStream);
}

int32_t cfx_device_error(cfx_engine *e, int32_t *inter, int32_t *phase) {
    if (!e) return CFX_ERR_INVALID;
    volatile int32_t *rec = e->hPhaseErr;
    const int32_t i = rec[0];
    if (i < 0) return 0;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (inter) *inter = i;
    if (phase) *phase = rec[1];
    rec[0] = -1;
    return 1;
}

// ---- the fixed-time signal plan as engine state (optional entry points of include/cityflow_amd.h, as above)

// what every plan call checks first: not on a tile (its lights are another tile's too), the caller's row length
static int tlPlanArgs(cfx_engine *e, int32_t maxPhases, const char *what) {
    if (e->tiled) {
        e->err = std::string(what) + ": not on a tile";
        return CFX_ERR_STATE;
    }
    if (maxPhases != e->planMaxPhases) {
        e->err = std::string(what) + ": max_phases must be the network's " + std::to_string(e->planMaxPhases) + ", not " +
                 std::to_string(maxPhases);
        return CFX_ERR_INVALID;
    }
    return CFX_OK;
}

static void launchSetTlPlan(cfx_engine *e, const double *durations, const int32_t *phase, const double *remain) {
    const TlPlanIn in{durations, phase, remain, e->I, e->planMaxPhases, e->cfg.interval, ++e->planCalls};
    hipLaunchKernelGGL(k_set_tl_plan, dim3(1), dim3(1024), 0, e->stream, in, e->net.interPhaseStart, e->net.interVirtual, e->phaseTime,
                       e->curPhase, e->remain, e->hPlanErr);
}

// Both forms of a call, here and below, are one body.  toHost: the arrays are host memory, staged through the engine's arena
// and waited for; otherwise device memory, ordered against the caller's `stream`.  `what` names the entry point in messages.
static int setTlPlan(cfx_engine *e, const double *durations, const int32_t *phase, const double *remain, int32_t n, int32_t maxPhases,
                     bool toHost, void *stream, const char *what) {
    if (!e || (!durations && !phase && !remain) || n != e->I) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = tlPlanArgs(e, maxPhases, what))) return rc;
    const size_t nI = (size_t) e->I, nD = nI * (size_t) e->planMaxPhases;
    cfx_stage::StageLayout s(!toHost);
    const auto fDurations = s.in(durations, "durations", nD);
    const auto fPhase = s.in(phase, "phase", nI);
    const auto fRemain = s.in(remain, "remain", nI);
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = e->settle(false))) return rc;  // (as cfx_set_tl_phases_device: the deferred commit advances the lights of the last step first)
    if ((rc = e->stageOpen(s, stream))) return rc;
    launchSetTlPlan(e, s.dev(fDurations), s.dev(fPhase), s.dev(fRemain));
    HIP_TRY(hipGetLastError());
    return e->stageClose(s, stream);
}
int32_t cfx_set_tl_plan_device(cfx_engine *e, const double *durations, const int32_t *phase, const double *remain, int32_t n,
                               int32_t maxPhases, void *producerStream) {
    return setTlPlan(e, durations, phase, remain, n, maxPhases, false, producerStream, "cfx_set_tl_plan_device");
}
int32_t cfx_set_tl_plan(cfx_engine *e, const double *durations, const int32_t *phase, const double *remain, int32_t n, int32_t maxPhases) {
    return setTlPlan(e, durations, phase, remain, n, maxPhases, true, nullptr, "cfx_set_tl_plan");
}

static void launchGetPhaseDurations(cfx_engine *e, double *out) {
    const size_t total = (size_t) e->I * (size_t) e->planMaxPhases;
    if (!total) return;
    hipLaunchKernelGGL(k_get_phase_durations, dim3(gridFor((int) std::min<size_t>(total, 1u << 20))), dim3(kBlock), 0, e->stream, e->I,
                       e->planMaxPhases, e->net.interPhaseStart, e->net.interVirtual, e->phaseTime, out);
}

// (no settle: the durations are written by the calls above and by nothing a step launches)
static int getTlPhaseDurations(cfx_engine *e, double *out, int32_t maxPhases, bool toHost, void *stream, const char *what) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = tlPlanArgs(e, maxPhases, what))) return rc;
    cfx_stage::StageLayout s(!toHost);
    const auto fOut = s.out(out, "out", (size_t) e->I * (size_t) e->planMaxPhases);
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = e->stageOpen(s, stream))) return rc;
    launchGetPhaseDurations(e, s.dev(fOut));
    HIP_TRY(hipGetLastError());
    return e->stageClose(s, stream);
}
int32_t cfx_get_tl_phase_durations_device(cfx_engine *e, double *out, int32_t maxPhases, void *consumerStream) {
    return getTlPhaseDurations(e, out, maxPhases, false, consumerStream, "cfx_get_tl_phase_durations_device");
}
int32_t cfx_get_tl_phase_durations(cfx_engine *e, double *out, int32_t maxPhases) {
    return getTlPhaseDurations(e, out, maxPhases, true, nullptr, "cfx_get_tl_phase_durations");
}

int32_t cfx_restore_tl_plan(cfx_engine *e) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = tlPlanArgs(e, e->planMaxPhases, "cfx_restore_tl_plan"))) return rc;
    if ((rc = e->settle(false))) return rc;  // (the last step's lights advance on the durations that were in force for it)
    if (e->nPhaseTimes)
        HIP_TRY(hipMemcpyAsync(e->phaseTime, e->phaseTimeFile, (size_t) e->nPhaseTimes * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    return CFX_OK;
}

int32_t cfx_tl_plan_error(cfx_engine *e, int32_t *what, int32_t *inter, int32_t *phase, double *value) {
    if (!e) return CFX_ERR_INVALID;
    volatile TlPlanErr *rec = e->hPlanErr;
    const bool decided = rec->done - e->planCalls >= 0;  // (every set call enqueued so far has validated)
    std::atomic_thread_fence(std::memory_order_acquire);
    const int32_t i = rec->inter;
    if (i < 0) return decided ? 0 : 2;
    std::atomic_thread_fence(std::memory_order_acquire);
    if (what) *what = rec->what;
    if (inter) *inter = i;
    if (phase) *phase = rec->phase;
    if (value) *value = rec->value;
    rec->inter = -1;
    return 1;
}

// ---- the lanes' speed limits as engine state (optional entry points of include/cityflow_amd.h, as above)

// what every limit call checks first: not on a tile (a cut lane's limit would be another tile's too), the caller's length
static int laneLimitArgs(cfx_engine *e, int32_t n, const char *what) {
    if (e->tiled) {
        e->err = std::string(what) + ": not on a tile";
        return CFX_ERR_STATE;
    }
    if (n != e->L) {
        e->err = std::string(what) + ": n must be the network's " + std::to_string(e->L) + " lanes, not " + std::to_string(n);
        return CFX_ERR_INVALID;
    }
    return CFX_OK;
}

// (no settle in these calls: a deferred commit reads no limit — the action phase of the step it belongs to has run)
static int launchSetLaneLimits(cfx_engine *e, const double *limits, int32_t *rejected) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (rejected) HIP_TRY(hipMemsetAsync(rejected, 0, sizeof(int32_t), e->stream));
    if (e->L)
        hipLaunchKernelGGL(k_set_lane_limits, dim3(gridStride((size_t) e->L)), dim3(kBlock), 0, e->stream, limits, e->L, e->drvLM,
                           e->drvMaxSpeed, rejected);
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

static int setLaneSpeedLimits(cfx_engine *e, const double *limits, int32_t n, int32_t *rejected, bool toHost, void *stream, const char *what) {
    if (!e || !limits) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = laneLimitArgs(e, n, what))) return rc;
    cfx_stage::StageLayout s(!toHost);
    const auto fLimits = s.in(limits, "limits", (size_t) e->L);
    const auto fRejected = s.out(rejected, "rejected", 1);
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = e->stageOpen(s, stream))) return rc;
    if ((rc = launchSetLaneLimits(e, s.dev(fLimits), s.dev(fRejected)))) return rc;
    return e->stageClose(s, stream);
}
int32_t cfx_set_lane_speed_limits_device(cfx_engine *e, const double *limits, int32_t n, int32_t *rejected, void *producerStream) {
    return setLaneSpeedLimits(e, limits, n, rejected, false, producerStream, "cfx_set_lane_speed_limits_device");
}
int32_t cfx_set_lane_speed_limits(cfx_engine *e, const double *limits, int32_t n, int32_t *rejected) {
    return setLaneSpeedLimits(e, limits, n, rejected, true, nullptr, "cfx_set_lane_speed_limits");
}

static void launchGetLaneLimits(cfx_engine *e, double *out) {
    if (e->L) hipLaunchKernelGGL(k_get_lane_limits, dim3(gridStride((size_t) e->L)), dim3(kBlock), 0, e->stream, e->L, e->drvMaxSpeed, out);
}

static int getLaneSpeedLimits(cfx_engine *e, double *out, int32_t n, bool toHost, void *stream, const char *what) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = laneLimitArgs(e, n, what))) return rc;
    cfx_stage::StageLayout s(!toHost);
    const auto fOut = s.out(out, "out", (size_t) e->L);
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = e->stageOpen(s, stream))) return rc;
    launchGetLaneLimits(e, s.dev(fOut));
    HIP_TRY(hipGetLastError());
    return e->stageClose(s, stream);
}
int32_t cfx_get_lane_speed_limits_device(cfx_engine *e, double *out, int32_t n, void *consumerStream) {
    return getLaneSpeedLimits(e, out, n, false, consumerStream, "cfx_get_lane_speed_limits_device");
}
int32_t cfx_get_lane_speed_limits(cfx_engine *e, double *out, int32_t n) {
    return getLaneSpeedLimits(e, out, n, true, nullptr, "cfx_get_lane_speed_limits");
}

int32_t cfx_restore_lane_speed_limits(cfx_engine *e) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = laneLimitArgs(e, e->L, "cfx_restore_lane_speed_limits"))) return rc;
    if (e->L)
        hipLaunchKernelGGL(k_restore_lane_limits, dim3(gridStride((size_t) e->L)), dim3(kBlock), 0, e->stream, e->L, e->laneLimitFile,
                           e->drvLM, e->drvMaxSpeed);
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

// ---- per-lane speed and position features (optional entry points of include/cityflow_amd.h, as above)

static bool laneFeatureArgs(cfx_engine *e, const int32_t *bins, const double *edges, int32_t nBins, const char *what) {
    if (!bins) return true;
    if (!edges || nBins < 1 || nBins > CFX_MAX_LANE_BINS) {
        e->err = std::string(what) + ": bins need edges and 1 <= n_bins <= " + std::to_string(CFX_MAX_LANE_BINS);
        return false;
    }
    return true;
}

// ---- every lane observation through one descriptor (optional entry points of include/cityflow_amd.h, as above); the three
// entry points above it in the header are forwards onto laneObs

// The one path of the lane observations.  toHost: the outputs and edges are host memory (the launch writes the staging arena,
// and what was asked for is copied back); otherwise device memory, ordered against the caller's stream.  `what` names the
// entry point in messages.
static int laneObs(cfx_engine *e, const cfx_lane_obs *obs, bool toHost, void *consumerStream, const char *what) {
    cfx_lane_obs a{};
    int rc;
    if ((rc = takeDescriptor(e, obs, &a, what))) return rc;
    const bool tracker = a.front_lane_steps || a.front_waiting_steps, front = a.front_distance || a.front_speed || tracker;
    if (!a.counts && !a.waiting && !a.speed_sum && !a.bins && !front) return CFX_ERR_INVALID;
    if (!laneFeatureArgs(e, a.bins, a.edges, a.n_bins, what)) return CFX_ERR_INVALID;
    if (front && (a.n_front < 1 || a.n_front > CFX_MAX_LANE_FRONT)) {
        e->err = std::string(what) + ": front outputs need 1 <= n_front <= " + std::to_string(CFX_MAX_LANE_FRONT);
        return CFX_ERR_INVALID;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    const int lanesPerEnv = std::max(e->L / (e->cfg.n_envs > 1 ? e->cfg.n_envs : 1), 1);
    const size_t nL = (size_t) e->L, nB = a.bins ? nL * a.n_bins : 0, nF = front ? nL * a.n_front : 0,
                 nEdges = a.bins ? (a.per_lane_edges ? (size_t) lanesPerEnv : 1) * (a.n_bins + 1) : 0;
    cfx_stage::StageLayout s(!toHost);
    const auto fCounts = s.out(a.counts, "counts", nL), fWaiting = s.out(a.waiting, "waiting", nL);
    const auto fSum = s.out(a.speed_sum, "speed_sum", nL);
    const auto fBins = s.out(a.bins, "bins", nB);
    const auto fEdges = s.in(a.bins ? a.edges : nullptr, "edges", nEdges);  // (edges without bins: not given)
    const auto fDis = s.out(a.front_distance, "front_distance", nF), fSpeed = s.out(a.front_speed, "front_speed", nF);
    const auto fSteps = s.out(a.front_lane_steps, "front_lane_steps", nF), fWait = s.out(a.front_waiting_steps, "front_waiting_steps", nF);
    if ((rc = e->stageCheck(s, what))) return rc;
    if (tracker && !e->tracker[kLaneFlow].on) {
        e->err = std::string(what) + ": front_lane_steps / front_waiting_steps need lane-flow tracking (cfx_lane_flow_enable)";
        return CFX_ERR_STATE;
    }
    if ((rc = e->settle(false))) return rc;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    if ((rc = e->syncTables())) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    if ((rc = e->stageOpen(s, consumerStream))) return rc;
    LaneFeatOut o{s.dev(fCounts), s.dev(fWaiting), s.dev(fSum), s.dev(fBins), s.dev(fEdges), a.bins ? a.n_bins : 0,
                  (a.bins && a.per_lane_edges) ? a.n_bins + 1 : 0, lanesPerEnv,
                  front ? a.n_front : 0, s.dev(fDis), s.dev(fSpeed), s.dev(fSteps), s.dev(fWait)};
    if (tracker) {
        o.flowRec = e->flow.rec;
        o.flowVidCap = (int) e->vidCap;
        o.flowTick = e->flow.tick + (e->tracker[kLaneFlow].baselineDue ? 1 : 0);  // (a baseline that is due: no record carries the tick it will take)
        o.flowStep = e->flow.step;
    }
    launchLaneFeatures(e, o);
    HIP_TRY(hipGetLastError());
    if ((rc = e->stageClose(s, consumerStream))) return rc;
    if (!toHost) e->deviceObserved();
    return CFX_OK;
}

int32_t cfx_observe_lane_obs_device(cfx_engine *e, const cfx_lane_obs *obs, void *consumerStream) {
    return laneObs(e, obs, false, consumerStream, "cfx_observe_lane_obs_device");
}
int32_t cfx_get_lane_obs(cfx_engine *e, const cfx_lane_obs *obs) { return laneObs(e, obs, true, nullptr, "cfx_get_lane_obs"); }

static cfx_lane_obs laneObsOf(int32_t *counts, int32_t *waiting, double *speedSum, int32_t *bins, const double *edges, int32_t nBins,
                              int32_t perLaneEdges) {
    cfx_lane_obs a{};
    a.struct_size = (int32_t) sizeof a;
    a.counts = counts;
    a.waiting = waiting;
    a.speed_sum = speedSum;
    a.bins = bins;
    a.edges = edges;
    a.n_bins = nBins;
    a.per_lane_edges = perLaneEdges;
    return a;
}

int32_t cfx_observe_lanes_device(cfx_engine *e, int32_t *counts, int32_t *waiting, double *speedSum, int32_t *bins,
                                 const double *edges, int32_t nBins, int32_t perLaneEdges, void *consumerStream) {
    const cfx_lane_obs a = laneObsOf(counts, waiting, speedSum, bins, edges, nBins, perLaneEdges);
    return laneObs(e, &a, false, consumerStream, "cfx_observe_lanes_device");
}

// (the two counts alone: cfx_observe_lanes_device with the other outputs null)
int32_t cfx_observe_device(cfx_engine *e, int32_t *counts, int32_t *waiting, void *consumerStream) {
    if (!e || (!counts && !waiting)) return CFX_ERR_INVALID;
    return cfx_observe_lanes_device(e, counts, waiting, nullptr, nullptr, nullptr, 0, 0, consumerStream);
}

int32_t cfx_get_lane_features(cfx_engine *e, double *speedSum, int32_t *bins, const double *edges, int32_t nBins,
                              int32_t perLaneEdges) {
    const cfx_lane_obs a = laneObsOf(nullptr, nullptr, speedSum, bins, edges, nBins, perLaneEdges);
    return laneObs(e, &a, true, nullptr, "cfx_get_lane_features");
}

// ---- per-vehicle observations (an optional entry point of include/cityflow_amd.h, as above): k_vehicle_tile_sums, then
// kr_vehicle_rows / kd_vehicle_rows (cfx_kernels.h has the scheme)

int32_t cfx_observe_vehicles_device(cfx_engine *e, const cfx_vehicle_rows *rows, void *consumerStream) {
    const char *what = "cfx_observe_vehicles_device";
    cfx_vehicle_rows a{};
    int rc;
    if ((rc = takeDescriptor(e, rows, &a, what))) return rc;
    if (a.n_rows < 0) {
        e->err = std::string(what) + ": n_rows must not be negative";
        return CFX_ERR_INVALID;
    }
    if (a.n_rows == 0) {
        a.vehicle = a.drivable = a.env = a.leader = nullptr, a.distance = a.speed = a.gap = nullptr;
        a.x = a.y = a.dir_x = a.dir_y = a.length = a.width = nullptr;
    }
    const bool poses = a.x || a.y || a.dir_x || a.dir_y || a.length || a.width;
    const bool anyRow = poses || a.vehicle || a.drivable || a.env || a.distance || a.speed || a.leader || a.gap;
    if (!a.start && !a.count && !anyRow) return CFX_ERR_INVALID;
    if (e->lc.on || e->tiled) {
        e->err = std::string(what) + ": not with lane change (shadows) and not on a tile";
        return CFX_ERR_STATE;
    }
    if (poses && !e->geoNodes) {
        e->err = std::string(what) + ": x, y, dir_x, dir_y, length and width need the drivables' polylines: call cfx_set_drivable_geometry first";
        return CFX_ERR_STATE;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    cfx_stage::StageLayout s(true);  // (no host form: the layout is the list of buffers to validate)
    s.out(a.start, "start"), s.out(a.count, "count"), s.out(a.vehicle, "vehicle"), s.out(a.drivable, "drivable"), s.out(a.env, "env");
    s.out(a.distance, "distance"), s.out(a.speed, "speed"), s.out(a.leader, "leader"), s.out(a.gap, "gap");
    s.out(a.x, "x"), s.out(a.y, "y"), s.out(a.dir_x, "dir_x"), s.out(a.dir_y, "dir_y"), s.out(a.length, "length"), s.out(a.width, "width");
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = e->settle(false))) return rc;  // (ring layout: a commit deferred to the next step's admission)
    if ((rc = e->syncTables())) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    const int nEnvs = e->cfg.n_envs > 1 ? e->cfg.n_envs : 1;
    VehRowsOut o{};
    o.start = a.start, o.count = a.count;
    o.vehicle = a.vehicle, o.drivable = a.drivable, o.env = a.env, o.leader = a.leader;
    o.distance = a.distance, o.speed = a.speed, o.gap = a.gap;
    o.nRows = a.n_rows;
    o.nEnvs = nEnvs, o.lanesPerEnv = e->L / nEnvs, o.linksPerEnv = e->K / nEnvs;
    o.nTiles = (int) std::max<size_t>(1, ((size_t) e->D + kRowTile - 1) / kRowTile);
    if (!e->rowTileSum && (rc = e->allocRaw(&e->rowTileSum, (size_t) o.nTiles))) return rc;
    o.tileSum = e->rowTileSum;
    const int padBlocks = anyRow ? (int) (((size_t) a.n_rows + kRowPadRows - 1) / kRowPadRows) : 0;
    const VehPoseOut g{a.x, a.y, a.dir_x, a.dir_y, a.length, a.width, e->geoStart, e->geoNodes};
    if ((rc = e->orderAfterCaller((hipStream_t) consumerStream))) return rc;
    if (e->ring) {
        const RingCtx c = e->rctx();
        hipLaunchKernelGGL(k_vehicle_tile_sums, dim3(o.nTiles), dim3(kBlock), 0, e->stream, (const int32_t *) c.cnt, c.n.L, o);
        if (poses) hipLaunchKernelGGL(kr_vehicle_poses, dim3(o.nTiles + padBlocks), dim3(kBlock), 0, e->stream, c, o, g);
        else hipLaunchKernelGGL(kr_vehicle_rows, dim3(o.nTiles + padBlocks), dim3(kBlock), 0, e->stream, c, o);
    } else {
        const StepCtx c = e->ctx();
        hipLaunchKernelGGL(k_vehicle_tile_sums, dim3(o.nTiles), dim3(kBlock), 0, e->stream, (const int32_t *) c.cnt, c.n.L, o);
        if (poses) hipLaunchKernelGGL(kd_vehicle_poses, dim3(o.nTiles + padBlocks), dim3(kBlock), 0, e->stream, c, o, g);
        else hipLaunchKernelGGL(kd_vehicle_rows, dim3(o.nTiles + padBlocks), dim3(kBlock), 0, e->stream, c, o);
    }
    HIP_TRY(hipGetLastError());
    if ((rc = e->orderCallerAfter((hipStream_t) consumerStream))) return rc;
    e->deviceObserved();  // (tiles were refused above)
    return CFX_OK;
}

// ---- the drivables' polylines for the pose outputs above (an optional entry point of include/cityflow_amd.h): the table is
// checked, turned into GeoNode records — segment lengths, their left-to-right sum and the unit vectors, in the reference's
// expressions and order (this file is compiled without contraction, and the host's sqrt and division round correctly) — and
// uploaded.  The kernels trust point_start, so nothing is uploaded that has not passed the checks

int32_t cfx_set_drivable_geometry(cfx_engine *e, const cfx_drivable_geometry *geometry) {
    const char *what = "cfx_set_drivable_geometry";
    cfx_drivable_geometry a{};
    int rc;
    if ((rc = takeDescriptor(e, geometry, &a, what))) return rc;
    auto invalid = [&](const std::string &m) {
        e->err = std::string(what) + ": " + m;
        return CFX_ERR_INVALID;
    };
    if (e->tiled) {
        e->err = std::string(what) + ": not on a tile";
        return CFX_ERR_STATE;
    }
    const int nEnvs = e->cfg.n_envs > 1 ? e->cfg.n_envs : 1;
    const int D = e->D / nEnvs;
    if (!a.point_start || !a.xy) return invalid("point_start and xy must be given");
    if (a.n_drivables != D) return invalid("n_drivables must be the " + std::to_string(D) + " drivables of one environment");
    if (a.point_start[0] != 0 || a.point_start[D] != a.n_points) return invalid("point_start must run from 0 to n_points");
    for (int d = 0; d < D; ++d)
        if (a.point_start[d + 1] - (int64_t) a.point_start[d] < 2 || a.point_start[d + 1] > a.n_points)
            return invalid("drivable " + std::to_string(d) + " needs at least two points inside the table");
    std::vector<GeoNode> nodes((size_t) a.n_points);
    for (int d = 0; d < D; ++d) {
        const int p0 = a.point_start[d], p1 = a.point_start[d + 1];
        double total = 0.0;
        for (int p = p0; p < p1; ++p) {
            GeoNode &n = nodes[(size_t) p];
            n = GeoNode{};
            n.x = a.xy[2 * (size_t) p], n.y = a.xy[2 * (size_t) p + 1];
            if (p + 1 == p1) break;
            const double dx = a.xy[2 * (size_t) p + 2] - n.x, dy = a.xy[2 * (size_t) p + 3] - n.y;
            n.len = sqrt(dx * dx + dy * dy);
            n.ux = dx / n.len, n.uy = dy / n.len;
            total += n.len;
        }
        nodes[(size_t) p1 - 1].len = total;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    if (e->geoNodes) {  // a second call: the kernels of the first may still read the old table
        HIP_TRY(hipStreamSynchronize(e->stream));
        if ((rc = e->freeRaw(&e->geoStart)) || (rc = e->freeRaw(&e->geoNodes))) return rc;
    }
    if ((rc = e->upload(&e->geoStart, a.point_start, (size_t) D + 1))) return rc;
    return e->upload(&e->geoNodes, nodes.data(), nodes.size());
}

// ---- speed commands for many vehicles at once (optional entry points of include/cityflow_amd.h, as above): k_speeds_claim,
// k_speeds_apply and, on the dense layout, k_speeds_flag_dense (cfx_kernels.h has the scheme)

// what both forms check first
static int vehicleSpeedsArgs(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n, const char *what) {
    if (n < 0 || (n > 0 && (!vehicle || !speed))) {
        e->err = std::string(what) + ": n must not be negative, and vehicle and speed are needed for n > 0";
        return CFX_ERR_INVALID;
    }
    if (e->lc.on || e->tiled) {
        e->err = std::string(what) + ": not with lane change (the vehicle numbers are cfx_observe_vehicles_device's) and not on a tile";
        return CFX_ERR_STATE;
    }
    return CFX_OK;
}

// the stamp table of the speed and the route commands holds every vehicle number issued
static int vehicleStampEnsure(cfx_engine *e) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (e->speedStampCap >= (size_t) e->spawned) return CFX_OK;  // (idle: nothing to keep, the new one starts out all -1)
    const size_t cap = std::max<size_t>(e->vidCap, (size_t) e->spawned);
    int32_t *stamp = nullptr;
    int rc;
    if ((rc = e->allocRaw(&stamp, cap))) return rc;
    HIP_TRY(hipMemsetAsync(stamp, 0xFF, std::max<size_t>(cap, 1) * sizeof(int32_t), e->stream));
    if (e->speedStamp) e->retired.push_back(e->speedStamp);
    e->speedStamp = stamp;
    e->speedStampCap = cap;
    return CFX_OK;
}

// the kernels of one call on the engine's stream; every pointer device memory, `ignored` may be null.  The caller has settled.
static int launchVehicleSpeeds(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n, int32_t *ignored) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (ignored) HIP_TRY(hipMemsetAsync(ignored, 0, sizeof(int32_t), e->stream));
    if (n == 0) return CFX_OK;
    int rc;
    if ((rc = e->syncTables())) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    if ((rc = vehicleStampEnsure(e))) return rc;
    const VehSpeedsIn in{vehicle, speed, n, (int) e->spawned, e->speedStamp, ignored};
    const dim3 grid((unsigned) (((size_t) n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_speeds_claim, grid, dim3(kBlock), 0, e->stream, in, (const uint8_t *) e->vt.state);
    if (e->ring) {
        const RingCtx c = e->rctx();
        hipLaunchKernelGGL(k_speeds_apply, grid, dim3(kBlock), 0, e->stream, in, e->vt, (const int32_t *) c.slotOf, c.meta);
    } else {
        hipLaunchKernelGGL(k_speeds_apply, grid, dim3(kBlock), 0, e->stream, in, e->vt, (const int32_t *) nullptr, (int4 *) nullptr);
        hipLaunchKernelGGL(k_speeds_flag_dense, dim3(gridStride(e->slotCap)), dim3(kBlock), 0, e->stream, e->ctx(), e->speedStamp, in.nVid);
    }
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

static int setVehicleSpeeds(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n, int32_t *ignored, bool toHost,
                            void *stream, const char *what) {
    if (!e) return CFX_ERR_INVALID;
    int rc;
    if ((rc = vehicleSpeedsArgs(e, vehicle, speed, n, what))) return rc;
    if (toHost) {  // (no rows: the host form is done without touching the device)
        if (ignored) *ignored = 0;
        if (n == 0) return CFX_OK;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int32_t count = 0;  // (the host form's kernels always count, into a cell of the arena)
    cfx_stage::StageLayout s(!toHost);
    const auto fVehicle = s.in(n ? vehicle : nullptr, "vehicle", (size_t) n);  // (no rows: the arrays are not looked at)
    const auto fSpeed = s.in(n ? speed : nullptr, "speed", (size_t) n);
    const auto fIgnored = s.out(toHost ? &count : ignored, "ignored", 1);
    if ((rc = e->stageCheck(s, what))) return rc;
    if (n == 0 && !ignored) return CFX_OK;  // (the device form with nothing to do)
    if ((rc = e->settle(false))) return rc;  // (ring layout: a commit deferred to the next step's admission)
    if ((rc = e->stageOpen(s, stream))) return rc;
    if ((rc = launchVehicleSpeeds(e, s.dev(fVehicle), s.dev(fSpeed), n, s.dev(fIgnored)))) return rc;
    if ((rc = e->stageClose(s, stream))) return rc;  // (the count is there; a device form's rows may be overwritten)
    if (toHost && ignored) *ignored = count;
    return CFX_OK;
}
int32_t cfx_set_vehicle_speeds_device(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n, int32_t *ignored,
                                      void *producerStream) {
    return setVehicleSpeeds(e, vehicle, speed, n, ignored, false, producerStream, "cfx_set_vehicle_speeds_device");
}
int32_t cfx_set_vehicle_speeds(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n, int32_t *ignored) {
    return setVehicleSpeeds(e, vehicle, speed, n, ignored, true, nullptr, "cfx_set_vehicle_speeds");
}

// The custom speeds of the vehicles still in an entry buffer (state 0 with pendingCustom): three copies of the vehicle tables
// and a walk on the host - its one caller is a vehicle compaction, which reads the whole state anyway.
int32_t cfx_get_waiting_custom_speeds(cfx_engine *e, int32_t capacity, int32_t *vid, double *speed, int32_t *n) {
    if (!e || !n || capacity < 0 || (capacity > 0 && (!vid || !speed))) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->settle(false))) return rc;
    if ((rc = e->syncTables())) return rc;
    *n = 0;
    const size_t nV = (size_t) e->spawned;
    if (!nV) return CFX_OK;
    std::vector<uint8_t> state(nV), pending(nV);
    std::vector<double> cs(nV);
    HIP_TRY(hipMemcpyAsync(state.data(), e->vt.state, nV, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(pending.data(), e->vt.pendingCustom, nV, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(cs.data(), e->vt.customSpeed, nV * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    int32_t k = 0;
    for (size_t v = 0; v < nV; ++v)
        if (state[v] == 0 && pending[v]) {
            if (k == capacity) {
                e->err = "cfx_get_waiting_custom_speeds: capacity too small";
                return CFX_ERR_CAPACITY;
            }
            vid[k] = (int32_t) v;
            speed[k] = cs[v];
            ++k;
        }
    *n = k;
    return CFX_OK;
}

// ---- route changes for many vehicles at once, and the routes they hold (optional entry points of include/cityflow_amd.h, as
// above): k_routes_claim and kr_routes_apply, or k_routes_superseded and k_routes_apply_dense (cfx_kernels.h has the scheme)

// what the four forms check first (`second`: the route handles, or the output of the read)
static int vehicleRoutesArgs(cfx_engine *e, const void *vehicle, const void *second, bool vehicleNeeded, int32_t n, const char *what) {
    if (n < 0 || (n > 0 && ((vehicleNeeded && !vehicle) || !second))) {
        e->err = std::string(what) + ": n must not be negative, and the arrays are needed for n > 0";
        return CFX_ERR_INVALID;
    }
    if (e->lc.on || e->tiled) {
        e->err = std::string(what) + ": not with lane change (the vehicle numbers are cfx_observe_vehicles_device's) and not on a tile";
        return CFX_ERR_STATE;
    }
    return CFX_OK;
}
// the routes of one environment (a handle's range) and its lanes
static void vehicleRoutesEnv(const cfx_engine *e, int *routesPerEnv, int *lanesPerEnv) {
    const int nEnvs = e->cfg.n_envs > 1 ? e->cfg.n_envs : 1;
    *routesPerEnv = ((int) e->hRouteStart.size() - 1) / nEnvs;
    *lanesPerEnv = std::max(e->L / nEnvs, 1);
}

// the kernels of one call on the engine's stream; every pointer device memory, `status` and `ignored` may be null.  The caller has settled.
static int launchVehicleRoutes(cfx_engine *e, const int32_t *vehicle, const int32_t *route, int32_t n, int32_t *status, int32_t *ignored) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (ignored) HIP_TRY(hipMemsetAsync(ignored, 0, sizeof(int32_t), e->stream));
    if (n == 0) return CFX_OK;
    int rc;
    if ((rc = e->syncTables())) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    if ((rc = vehicleStampEnsure(e))) return rc;
    VehRoutesIn in{vehicle, route, n, (int) e->spawned, 0, 1, e->speedStamp, status, ignored};
    vehicleRoutesEnv(e, &in.routesPerEnv, &in.lanesPerEnv);
    const dim3 grid((unsigned) (((size_t) n + kBlock - 1) / kBlock));
    hipLaunchKernelGGL(k_routes_claim, grid, dim3(kBlock), 0, e->stream, in, (const uint8_t *) e->vt.state);
    if (e->ring) {
        hipLaunchKernelGGL(kr_routes_apply, grid, dim3(kBlock), 0, e->stream, e->rctx(), in, e->vt);
    } else {
        hipLaunchKernelGGL(k_routes_superseded, grid, dim3(kBlock), 0, e->stream, in, (const uint8_t *) e->vt.state);
        hipLaunchKernelGGL(k_routes_apply_dense, dim3(gridStride(e->slotCap)), dim3(kBlock), 0, e->stream, e->ctx(), in, e->vt);
    }
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

// (the shape of setVehicleSpeeds above, comment by comment)
static int setVehicleRoutes(cfx_engine *e, const int32_t *vehicle, const int32_t *route, int32_t n, int32_t *status, int32_t *ignored,
                            bool toHost, void *stream, const char *what) {
    if (!e) return CFX_ERR_INVALID;
    int rc;
    if ((rc = vehicleRoutesArgs(e, vehicle, route, true, n, what))) return rc;
    if (toHost) {
        if (ignored) *ignored = 0;
        if (n == 0) return CFX_OK;
    }
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int32_t count = 0;
    cfx_stage::StageLayout s(!toHost);
    const auto fVehicle = s.in(n ? vehicle : nullptr, "vehicle", (size_t) n);
    const auto fRoute = s.in(n ? route : nullptr, "route", (size_t) n);
    const auto fStatus = s.out(n ? status : nullptr, "status", (size_t) n);
    const auto fIgnored = s.out(toHost ? &count : ignored, "ignored", 1);
    if ((rc = e->stageCheck(s, what))) return rc;
    if (n == 0 && !ignored) return CFX_OK;
    if ((rc = e->settle(false))) return rc;  // (ring layout: a commit deferred to the next step's admission)
    if ((rc = e->stageOpen(s, stream))) return rc;
    if ((rc = launchVehicleRoutes(e, s.dev(fVehicle), s.dev(fRoute), n, s.dev(fStatus), s.dev(fIgnored)))) return rc;
    if ((rc = e->stageClose(s, stream))) return rc;  // (status and the count are there; a device form's rows may be overwritten)
    if (toHost && ignored) *ignored = count;
    return CFX_OK;
}
int32_t cfx_set_vehicle_routes_device(cfx_engine *e, const int32_t *vehicle, const int32_t *route, int32_t n, int32_t *status,
                                      int32_t *ignored, void *producerStream) {
    return setVehicleRoutes(e, vehicle, route, n, status, ignored, false, producerStream, "cfx_set_vehicle_routes_device");
}
int32_t cfx_set_vehicle_routes(cfx_engine *e, const int32_t *vehicle, const int32_t *route, int32_t n, int32_t *status, int32_t *ignored) {
    return setVehicleRoutes(e, vehicle, route, n, status, ignored, true, nullptr, "cfx_set_vehicle_routes");
}

// the kernel of one read on the engine's stream; vehicle may be null (the numbers 0 .. n-1).  The caller has settled; n > 0.
static int launchGetVehicleRoutes(cfx_engine *e, const int32_t *vehicle, int32_t n, int32_t *routeOut) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    int routesPerEnv = 0, lanesPerEnv = 1;
    vehicleRoutesEnv(e, &routesPerEnv, &lanesPerEnv);
    hipLaunchKernelGGL(k_get_routes, dim3((unsigned) (((size_t) n + kBlock - 1) / kBlock)), dim3(kBlock), 0, e->stream, vehicle, (int) n,
                       (int) e->spawned, (const int32_t *) e->vt.route, (const uint8_t *) e->vt.state, std::max(routesPerEnv, 1), routeOut);
    HIP_TRY(hipGetLastError());
    return CFX_OK;
}

static int getVehicleRoutes(cfx_engine *e, const int32_t *vehicle, int32_t n, int32_t *routeOut, bool toHost, void *stream, const char *what) {
    if (!e) return CFX_ERR_INVALID;
    int rc;
    // (the host form alone reads the numbers 0 .. n-1 for a null `vehicle`)
    if ((rc = vehicleRoutesArgs(e, vehicle, routeOut, !toHost, n, what))) return rc;
    if (toHost && n == 0) return CFX_OK;  // (as the setters': done without touching the device)
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    cfx_stage::StageLayout s(!toHost);
    const auto fVehicle = s.in(n ? vehicle : nullptr, "vehicle", (size_t) n);
    const auto fOut = s.out(n ? routeOut : nullptr, "route_out", (size_t) n);
    if ((rc = e->stageCheck(s, what))) return rc;
    if (n == 0) return CFX_OK;
    if ((rc = e->settle(false))) return rc;
    if ((rc = e->stageOpen(s, stream))) return rc;
    if ((rc = launchGetVehicleRoutes(e, s.dev(fVehicle), n, s.dev(fOut)))) return rc;
    return e->stageClose(s, stream);
}
int32_t cfx_get_vehicle_routes_device(cfx_engine *e, const int32_t *vehicle, int32_t n, int32_t *routeOut, void *consumerStream) {
    return getVehicleRoutes(e, vehicle, n, routeOut, false, consumerStream, "cfx_get_vehicle_routes_device");
}
int32_t cfx_get_vehicle_routes(cfx_engine *e, const int32_t *vehicle, int32_t n, int32_t *routeOut) {
    return getVehicleRoutes(e, vehicle, n, routeOut, true, nullptr, "cfx_get_vehicle_routes");
}

// ---- per-intersection movement and phase observations (optional entry points of include/cityflow_amd.h, as above)

// The static index of InterFeatOut from the network tables the device holds (read back once: the engine keeps no host copy of
// them).  Device memory: 16 (I M + 1) bytes of rows, 4 bytes per in-lane, out-lane and laneLink entry, 4 I P ceil(M / 32) of masks.
static int interTables(cfx_engine *e) {
    if (e->interBuilt) return CFX_OK;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    const int K = e->K, I = e->I;
    std::vector<int32_t> llStart((size_t) K), llEnd((size_t) K), llInter((size_t) K), llRL((size_t) K), nRL((size_t) I),
        phStart((size_t) I + 1), virt((size_t) I), availStart((size_t) I);
    auto down = [&](std::vector<int32_t> &h, const int32_t *d) {
        return h.empty() ? hipSuccess : hipMemcpy(h.data(), d, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    };
    HIP_TRY(down(llStart, e->net.llStartLane));
    HIP_TRY(down(llEnd, e->net.llEndLane));
    HIP_TRY(down(llInter, e->net.llInter));
    HIP_TRY(down(llRL, e->net.llRoadLink));
    HIP_TRY(down(nRL, e->net.interNRL));
    HIP_TRY(down(phStart, e->net.interPhaseStart));
    HIP_TRY(down(virt, e->net.interVirtual));
    HIP_TRY(down(availStart, e->net.interAvailStart));
    int M = 0, P = 0;
    size_t availEnd = 0;
    for (int i = 0; i < I; ++i) {
        M = std::max(M, nRL[(size_t) i]);
        if (virt[(size_t) i]) continue;
        const int nPh = phStart[(size_t) i + 1] - phStart[(size_t) i];
        P = std::max(P, nPh);
        availEnd = std::max(availEnd, (size_t) availStart[(size_t) i] + (size_t) nPh * nRL[(size_t) i]);
    }
    if ((size_t) M * sizeof(int32_t) > 32768) {  // (the kernel keeps M words of LDS per block)
        e->err = "intersection features: an intersection with " + std::to_string(M) + " roadLinks is beyond the kernel's LDS row";
        return CFX_ERR_INVALID;
    }
    std::vector<uint8_t> avail(availEnd);
    if (availEnd) HIP_TRY(hipMemcpy(avail.data(), e->net.phaseAvail, availEnd, hipMemcpyDeviceToHost));
    const size_t rows = (size_t) I * M;
    std::vector<std::vector<int32_t>> inOf(rows), outOf(rows), llOf(rows);
    for (int k = 0; k < K; ++k) {
        const int i = llInter[(size_t) k], m = llRL[(size_t) k];
        if (i < 0 || i >= I || m < 0 || m >= nRL[(size_t) i] || llStart[(size_t) k] < 0 || llStart[(size_t) k] >= e->L ||
            llEnd[(size_t) k] < 0 || llEnd[(size_t) k] >= e->L) {
            e->err = "intersection features: laneLink " + std::to_string(k) + " names no roadLink / lane of the network";
            return CFX_ERR_INVALID;
        }
        const size_t row = (size_t) i * M + m;
        inOf[row].push_back(llStart[(size_t) k]);
        outOf[row].push_back(llEnd[(size_t) k]);
        llOf[row].push_back(k);
    }
    std::vector<int4> off(rows + 1);
    std::vector<int32_t> inL, outL, links;
    auto distinct = [](std::vector<int32_t> &v) {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    };
    for (size_t row = 0; row < rows; ++row) {
        off[row] = make_int4((int) inL.size(), (int) outL.size(), (int) links.size(), 0);
        distinct(inOf[row]);
        distinct(outOf[row]);
        inL.insert(inL.end(), inOf[row].begin(), inOf[row].end());
        outL.insert(outL.end(), outOf[row].begin(), outOf[row].end());
        links.insert(links.end(), llOf[row].begin(), llOf[row].end());
    }
    off[rows] = make_int4((int) inL.size(), (int) outL.size(), (int) links.size(), 0);
    const int W = (M + 31) / 32;
    std::vector<uint32_t> mask((size_t) I * P * W, 0u);
    for (int i = 0; i < I; ++i) {
        if (virt[(size_t) i]) continue;
        const int nPh = phStart[(size_t) i + 1] - phStart[(size_t) i], nr = nRL[(size_t) i];
        for (int p = 0; p < nPh; ++p)
            for (int m = 0; m < nr; ++m)
                if (avail[(size_t) availStart[(size_t) i] + (size_t) p * nr + m]) mask[((size_t) i * P + p) * W + m / 32] |= 1u << (m % 32);
    }
    InterFeatOut &t = e->interTab;
    int rc;
    if ((rc = e->uploadConst(t.rlOff, off.data(), off.size()))) return rc;
    if ((rc = e->uploadConst(t.inLanes, inL.data(), inL.size()))) return rc;
    if ((rc = e->uploadConst(t.outLanes, outL.data(), outL.size()))) return rc;
    if ((rc = e->uploadConst(t.rlLinks, links.data(), links.size()))) return rc;
    if ((rc = e->uploadConst(t.phaseMask, mask.data(), mask.size()))) return rc;
    t.M = M;
    t.P = P;
    t.maskWords = W;
    e->interBuilt = true;
    return CFX_OK;
}

// one block per intersection (interFeatures, cfx_kernels.h)
static void launchInterFeatures(cfx_engine *e, int32_t *phase, double *remain, int32_t *in, int32_t *inWaiting, int32_t *out,
                                int32_t *inside, int32_t *pressure) {
    if (e->I <= 0) return;
    InterFeatOut o = e->interTab;
    o.phase = phase;
    o.remain = remain;
    o.in = in;
    o.inWaiting = inWaiting;
    o.out = out;
    o.inside = inside;
    o.pressure = pressure;
    o.remainSrc = e->remain;
    const size_t lds = (size_t) o.M * sizeof(int32_t);
    if (e->ring) hipLaunchKernelGGL(kr_intersection_features, dim3((unsigned) e->I), dim3(kBlock), lds, e->stream, e->rctx(), o);
    else hipLaunchKernelGGL(kd_intersection_features, dim3((unsigned) e->I), dim3(kBlock), lds, e->stream, e->ctx(), o);
}

// what both entry points do before their launch: the deferred commit, tables, rings, the index, the caller's row lengths
static int interPrepare(cfx_engine *e, int32_t maxRoadLinks, int32_t maxPhases, const char *what) {
    int rc;
    if ((rc = e->settle(false))) return rc;  // (ring layout: a commit deferred to the next step's admission; Lane::history is not read here)
    if ((rc = e->syncTables())) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    if ((rc = interTables(e))) return rc;
    if (maxRoadLinks != e->interTab.M || maxPhases != e->interTab.P) {
        e->err = std::string(what) + ": max_roadlinks / max_phases must be the network's " + std::to_string(e->interTab.M) + " / " +
                 std::to_string(e->interTab.P) + ", not " + std::to_string(maxRoadLinks) + " / " + std::to_string(maxPhases);
        return CFX_ERR_INVALID;
    }
    return CFX_OK;
}

static int interFeatures(cfx_engine *e, int32_t *phase, double *remain, int32_t *in, int32_t *inWaiting, int32_t *out, int32_t *inside,
                         int32_t *pressure, int32_t maxRoadLinks, int32_t maxPhases, bool toHost, void *stream, const char *what) {
    if (!e || (!phase && !remain && !in && !inWaiting && !out && !inside && !pressure)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    const size_t nI = (size_t) e->I;
    cfx_stage::StageLayout s(!toHost);
    const auto fPhase = s.out(phase, "phase", nI);
    const auto fRemain = s.out(remain, "remain", nI);
    const auto fIn = s.out(in, "in"), fWait = s.out(inWaiting, "in_waiting"), fOut = s.out(out, "out"), fInside = s.out(inside, "inside"),
               fPressure = s.out(pressure, "phase_pressure");
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = interPrepare(e, maxRoadLinks, maxPhases, what))) return rc;
    const size_t nM = nI * e->interTab.M, nP = nI * e->interTab.P;  // (the row lengths: known once the index is built)
    s.count(fIn, nM), s.count(fWait, nM), s.count(fOut, nM), s.count(fInside, nM), s.count(fPressure, nP);
    if ((rc = e->stageOpen(s, stream))) return rc;
    launchInterFeatures(e, s.dev(fPhase), s.dev(fRemain), s.dev(fIn), s.dev(fWait), s.dev(fOut), s.dev(fInside), s.dev(fPressure));
    HIP_TRY(hipGetLastError());
    if ((rc = e->stageClose(s, stream))) return rc;
    if (!toHost) e->deviceObserved();
    return CFX_OK;
}
int32_t cfx_observe_intersections_device(cfx_engine *e, int32_t *phase, double *remain, int32_t *in, int32_t *inWaiting, int32_t *out,
                                         int32_t *inside, int32_t *pressure, int32_t maxRoadLinks, int32_t maxPhases,
                                         void *consumerStream) {
    return interFeatures(e, phase, remain, in, inWaiting, out, inside, pressure, maxRoadLinks, maxPhases, false, consumerStream,
                         "cfx_observe_intersections_device");
}
int32_t cfx_get_intersection_features(cfx_engine *e, int32_t *phase, double *remain, int32_t *in, int32_t *inWaiting, int32_t *out,
                                      int32_t *inside, int32_t *pressure, int32_t maxRoadLinks, int32_t maxPhases) {
    return interFeatures(e, phase, remain, in, inWaiting, out, inside, pressure, maxRoadLinks, maxPhases, true, nullptr,
                         "cfx_get_intersection_features");
}

// ---- per-lane flow and waiting-time statistics across steps (optional entry points of include/cityflow_amd.h, as above)

// ---- what the entry points of the three trackers share
static int trackerRequire(cfx_engine *e, int which, const char *what) {
    if (e->tracker[which].on) return CFX_OK;
    e->err = std::string(what) + ": " + kTrackerName[which] + " tracking is off (" + kTrackerEnable[which] + ")";
    return CFX_ERR_STATE;
}

// what every reader does first: the step's commit, the rings, a baseline that is due
static int trackerPrepare(cfx_engine *e, int which, const char *what) {
    int rc;
    if ((rc = trackerRequire(e, which, what))) return rc;
    if ((rc = e->settle(false))) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    return e->trackerSettle(which);
}

// the per-vehicle records of a flow tracker (`rec`: LaneFlowDev::rec, MoveFlowDev::rec), copied out for cfx_*_get_state ...
static int recordsOut(cfx_engine *e, const char *what, const int4 *rec, int32_t *records, int32_t nVehicles) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if ((size_t) nVehicles > e->vidCap) return e->fail(std::string(what) + ": n_vehicles beyond the vehicle tables"), CFX_ERR_INVALID;
    if (nVehicles) HIP_TRY(hipMemcpyAsync(records, rec, (size_t) nVehicles * sizeof(int4), hipMemcpyDeviceToHost, e->stream));
    return CFX_OK;
}
// ... and in for cfx_*_set_state, behind the step's commit: the numbers past `nVehicles` read unused (0xFF) again
static int recordsIn(cfx_engine *e, const char *what, int4 *rec, const int32_t *records, int32_t nVehicles) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if ((size_t) nVehicles > e->vidCap) return e->fail(std::string(what) + ": n_vehicles beyond the vehicle tables"), CFX_ERR_INVALID;
    int rc;
    if ((rc = e->settle(false))) return rc;
    HIP_TRY(hipMemsetAsync(rec, 0xFF, std::max<size_t>(e->vidCap, 1) * sizeof(int4), e->stream));
    if (nVehicles) HIP_TRY(hipMemcpyAsync(rec, records, (size_t) nVehicles * sizeof(int4), hipMemcpyHostToDevice, e->stream));
    return CFX_OK;
}

int32_t cfx_lane_flow_enable(cfx_engine *e, int32_t on) { return e ? e->trackerEnable(kLaneFlow, on) : CFX_ERR_INVALID; }

static void launchLaneFlowDrain(cfx_engine *e, const LaneFlowOut &o, int32_t reset) {
    if (e->L <= 0) return;
    hipLaunchKernelGGL(k_lane_flow_drain, dim3(gridFor((size_t) e->L)), dim3(kBlock), 0, e->stream, e->flow.lane, e->L, o, reset ? 1 : 0);
}

int32_t cfx_observe_lane_flow_device(cfx_engine *e, int32_t *entered, int32_t *left, int64_t *leftSteps, int64_t *leftWaitingSteps,
                                     int64_t *waitingSteps, int32_t *maxWaitingSteps, int32_t reset, void *consumerStream) {
    if (!e || (!entered && !left && !leftSteps && !leftWaitingSteps && !waitingSteps && !maxWaitingSteps && !reset)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    cfx_stage::StageLayout s(true);  // (the host form decodes records on the host: the layout is the list of buffers to validate)
    s.out(entered, "entered"), s.out(left, "left"), s.out(leftSteps, "left_steps"), s.out(leftWaitingSteps, "left_waiting_steps");
    s.out(waitingSteps, "waiting_steps"), s.out(maxWaitingSteps, "max_waiting_steps");
    if ((rc = e->stageCheck(s, "cfx_observe_lane_flow_device"))) return rc;
    if ((rc = trackerPrepare(e, kLaneFlow, "cfx_observe_lane_flow_device"))) return rc;
    if ((rc = e->orderAfterCaller((hipStream_t) consumerStream))) return rc;
    launchLaneFlowDrain(e, LaneFlowOut{entered, left, leftSteps, leftWaitingSteps, waitingSteps, maxWaitingSteps}, reset);
    HIP_TRY(hipGetLastError());
    return e->orderCallerAfter((hipStream_t) consumerStream);
}

int32_t cfx_get_lane_flow(cfx_engine *e, int32_t *entered, int32_t *left, int64_t *leftSteps, int64_t *leftWaitingSteps,
                          int64_t *waitingSteps, int32_t *maxWaitingSteps, int32_t reset) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kLaneFlow, "cfx_get_lane_flow"))) return rc;
    // (the records themselves come back, 48 bytes per lane: no device scratch, and the kernel only has to zero)
    std::vector<cfx_lane_flow_lane> lanes((size_t) e->L);
    if (e->L > 0) HIP_TRY(hipMemcpyAsync(lanes.data(), e->flow.lane, lanes.size() * sizeof(cfx_lane_flow_lane), hipMemcpyDeviceToHost, e->stream));
    if (reset) {
        launchLaneFlowDrain(e, LaneFlowOut{}, 1);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t l = 0; l < lanes.size(); ++l) {
        if (entered) entered[l] = lanes[l].entered;
        if (left) left[l] = lanes[l].left;
        if (leftSteps) leftSteps[l] = lanes[l].left_steps;
        if (leftWaitingSteps) leftWaitingSteps[l] = lanes[l].left_waiting_steps;
        if (waitingSteps) waitingSteps[l] = lanes[l].waiting_steps;
        if (maxWaitingSteps) maxWaitingSteps[l] = lanes[l].max_waiting_steps;
    }
    return CFX_OK;
}

int32_t cfx_lane_flow_get_state(cfx_engine *e, int32_t *records, int32_t nVehicles, cfx_lane_flow_lane *lanes, int32_t *tick) {
    if (!e || !lanes || !tick || nVehicles < 0 || (nVehicles > 0 && !records)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kLaneFlow, "cfx_lane_flow_get_state"))) return rc;
    if ((rc = recordsOut(e, "cfx_lane_flow_get_state", e->flow.rec, records, nVehicles))) return rc;
    if (e->L > 0) HIP_TRY(hipMemcpyAsync(lanes, e->flow.lane, (size_t) e->L * sizeof(cfx_lane_flow_lane), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *tick = e->flow.tick;
    return CFX_OK;
}

int32_t cfx_lane_flow_set_state(cfx_engine *e, const int32_t *records, int32_t nVehicles, const cfx_lane_flow_lane *lanes, int32_t tick) {
    if (!e || !lanes || nVehicles < 0 || (nVehicles > 0 && !records)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerRequire(e, kLaneFlow, "cfx_lane_flow_set_state"))) return rc;
    if ((rc = recordsIn(e, "cfx_lane_flow_set_state", e->flow.rec, records, nVehicles))) return rc;
    if (e->L > 0) HIP_TRY(hipMemcpyAsync(e->flow.lane, lanes, (size_t) e->L * sizeof(cfx_lane_flow_lane), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->flow.tick = tick;
    e->tracker[kLaneFlow].baselineDue = false;
    return CFX_OK;
}

// ---- virtual loop detectors (optional entry points of include/cityflow_amd.h, as above)

int32_t cfx_detectors_define(cfx_engine *e, const int32_t *lane, const double *start, const double *end, int32_t n) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (!lane || !start || !end || n < 1) return e->fail("cfx_detectors_define: lane, start and end of n >= 1 detectors"), CFX_ERR_INVALID;
    if (e->lc.on || e->tiled) {
        e->err = "cfx_detectors_define: not with lane change and not on a tile";
        return CFX_ERR_STATE;
    }
    const int lanesPerEnv = e->L / (e->cfg.n_envs > 1 ? e->cfg.n_envs : 1);
    for (int32_t i = 0; i < n; ++i) {  // (every entry before anything changes)
        const char *bad = (lane[i] < 0 || lane[i] >= lanesPerEnv) ? "lane is not a lane of one environment"
                          : !(std::isfinite(start[i]) && start[i] >= 0.0) ? "start is not finite and >= 0"
                          : !(end[i] > start[i]) ? "end is not beyond start" : nullptr;
        if (bad) return e->fail("cfx_detectors_define: position " + std::to_string(i) + ": " + bad), CFX_ERR_INVALID;
    }
    e->detLane.assign(lane, lane + n);
    e->detStart.assign(start, start + n);
    e->detEnd.assign(end, end + n);
    if (!e->tracker[kDetectors].on) return CFX_OK;
    // the set in force is replaced: new records and lane index (the vehicle records stay: a baseline overwrites what it uses)
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = e->settle(false))) return rc;
    if (e->ring && (rc = e->ringEnsure())) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (a tick may still be reading the tables)
    if (e->detectorTablesFree()) return CFX_ERR_DEVICE;
    if ((rc = e->detectorTables())) return rc;
    e->tracker[kDetectors].baselineDue = true;
    return e->trackerSettle(kDetectors);
}

int32_t cfx_detectors_enable(cfx_engine *e, int32_t on) { return e ? e->trackerEnable(kDetectors, on) : CFX_ERR_INVALID; }

static void launchDetectorsDrain(cfx_engine *e, const cfx_detectors_out &o, int32_t reset) {
    if (e->det.nDet <= 0) return;
    hipLaunchKernelGGL(k_detectors_drain, dim3(gridFor((size_t) e->det.nDet)), dim3(kBlock), 0, e->stream, e->det.det, e->det.nDet, o, reset ? 1 : 0);
}

int32_t cfx_observe_detectors_device(cfx_engine *e, const cfx_detectors_out *out, int32_t reset, void *consumerStream) {
    if (!e || !out) return CFX_ERR_INVALID;
    const cfx_detectors_out o = *out;
    if (!o.passed && !o.occupied_steps && !o.vehicle_steps && !o.waiting_vehicle_steps && !o.speed_sum && !o.count && !reset) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    cfx_stage::StageLayout s(true);  // (as cfx_observe_lane_flow_device)
    s.out(o.passed, "passed"), s.out(o.occupied_steps, "occupied_steps"), s.out(o.vehicle_steps, "vehicle_steps");
    s.out(o.waiting_vehicle_steps, "waiting_vehicle_steps"), s.out(o.speed_sum, "speed_sum"), s.out(o.count, "count");
    if ((rc = e->stageCheck(s, "cfx_observe_detectors_device"))) return rc;
    if ((rc = trackerPrepare(e, kDetectors, "cfx_observe_detectors_device"))) return rc;
    if ((rc = e->orderAfterCaller((hipStream_t) consumerStream))) return rc;
    launchDetectorsDrain(e, o, reset);
    HIP_TRY(hipGetLastError());
    return e->orderCallerAfter((hipStream_t) consumerStream);
}

int32_t cfx_get_detectors(cfx_engine *e, const cfx_detectors_out *out, int32_t reset) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kDetectors, "cfx_get_detectors"))) return rc;
    // (the records themselves come back, 64 bytes per detector: no device scratch, and the kernel only has to zero)
    std::vector<cfx_detector> recs((size_t) e->det.nDet);
    if (!recs.empty()) HIP_TRY(hipMemcpyAsync(recs.data(), e->det.det, recs.size() * sizeof(cfx_detector), hipMemcpyDeviceToHost, e->stream));
    if (reset) {
        launchDetectorsDrain(e, cfx_detectors_out{}, 1);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t d = 0; d < recs.size(); ++d) {
        if (out->passed) out->passed[d] = recs[d].passed;
        if (out->occupied_steps) out->occupied_steps[d] = recs[d].occupied_steps;
        if (out->vehicle_steps) out->vehicle_steps[d] = recs[d].vehicle_steps;
        if (out->waiting_vehicle_steps) out->waiting_vehicle_steps[d] = recs[d].waiting_vehicle_steps;
        if (out->speed_sum) out->speed_sum[d] = recs[d].speed_sum;
        if (out->count) out->count[d] = recs[d].count;
    }
    return CFX_OK;
}

int32_t cfx_detectors_get_state(cfx_engine *e, int32_t *records, int32_t nVehicles, cfx_detector *detectors, int32_t nDetectors, int32_t *tick) {
    if (!e || !detectors || !tick || nVehicles < 0 || (nVehicles > 0 && !records)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kDetectors, "cfx_detectors_get_state"))) return rc;
    if (nDetectors != e->det.nDet) return e->fail("cfx_detectors_get_state: n_detectors is not the number of detectors"), CFX_ERR_INVALID;
    if ((rc = recordsOut(e, "cfx_detectors_get_state", e->det.rec, records, nVehicles))) return rc;
    HIP_TRY(hipMemcpyAsync(detectors, e->det.det, (size_t) nDetectors * sizeof(cfx_detector), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    *tick = e->det.tick;
    return CFX_OK;
}

int32_t cfx_detectors_set_state(cfx_engine *e, const int32_t *records, int32_t nVehicles, const cfx_detector *detectors, int32_t nDetectors,
                                int32_t tick) {
    if (!e || !detectors || nVehicles < 0 || (nVehicles > 0 && !records)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerRequire(e, kDetectors, "cfx_detectors_set_state"))) return rc;
    if (nDetectors != e->det.nDet) return e->fail("cfx_detectors_set_state: n_detectors is not the number of detectors"), CFX_ERR_INVALID;
    if ((rc = recordsIn(e, "cfx_detectors_set_state", e->det.rec, records, nVehicles))) return rc;
    HIP_TRY(hipMemcpyAsync(e->det.det, detectors, (size_t) nDetectors * sizeof(cfx_detector), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->det.tick = tick;
    e->tracker[kDetectors].baselineDue = false;
    return CFX_OK;
}

// ---- per-environment trip statistics across steps (optional entry points of include/cityflow_amd.h, as above)

int32_t cfx_trip_stats_enable(cfx_engine *e, int32_t on) { return e ? e->trackerEnable(kTrips, on) : CFX_ERR_INVALID; }

static void launchTripDrain(cfx_engine *e, const cfx_trip_stats_out &o) {
    hipLaunchKernelGGL(k_trip_drain, dim3(gridFor((size_t) e->trip.nEnvs)), dim3(kBlock), 0, e->stream, e->trip.env, e->trip.nEnvs,
                       (long long) e->step, e->cfg.interval, o);
}

int32_t cfx_observe_trip_stats_device(cfx_engine *e, const cfx_trip_stats_out *out, void *consumerStream) {
    if (!e || !out) return CFX_ERR_INVALID;
    const cfx_trip_stats_out &o = *out;
    if (!o.entered && !o.admitted && !o.admitted_buffer_steps && !o.finished && !o.finished_travel_steps && !o.in_system && !o.buffered &&
        !o.in_system_travel_steps && !o.average_travel_time)
        return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    cfx_stage::StageLayout s(true);  // (as cfx_observe_lane_flow_device)
    s.out(o.entered, "entered"), s.out(o.admitted, "admitted"), s.out(o.admitted_buffer_steps, "admitted_buffer_steps");
    s.out(o.finished, "finished"), s.out(o.finished_travel_steps, "finished_travel_steps"), s.out(o.in_system, "in_system");
    s.out(o.buffered, "buffered"), s.out(o.in_system_travel_steps, "in_system_travel_steps");
    s.out(o.average_travel_time, "average_travel_time");
    if ((rc = e->stageCheck(s, "cfx_observe_trip_stats_device"))) return rc;
    if ((rc = trackerPrepare(e, kTrips, "cfx_observe_trip_stats_device"))) return rc;
    if ((rc = e->orderAfterCaller((hipStream_t) consumerStream))) return rc;
    launchTripDrain(e, o);
    HIP_TRY(hipGetLastError());
    return e->orderCallerAfter((hipStream_t) consumerStream);
}

// (the records themselves come back, 56 bytes per environment, and the host does the drain's few lines: no device scratch)
int32_t cfx_get_trip_stats(cfx_engine *e, const cfx_trip_stats_out *out) {
    if (!e || !out) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kTrips, "cfx_get_trip_stats"))) return rc;
    std::vector<cfx_trip_stats_env> envs((size_t) e->trip.nEnvs);
    HIP_TRY(hipMemcpyAsync(envs.data(), e->trip.env, envs.size() * sizeof(cfx_trip_stats_env), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    const cfx_trip_stats_out &o = *out;
    for (size_t r = 0; r < envs.size(); ++r) {
        const cfx_trip_stats_env &a = envs[r];
        const int32_t inSystem = a.base_in_system + a.entered - a.finished;
        const int64_t inSteps = (int64_t) inSystem * e->step - (a.enter_sum_created - a.enter_sum_finished);
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
            o.average_travel_time[r] = n == 0 ? 0.0 : (double) (a.finished_travel_steps + inSteps) * e->cfg.interval / (double) n;
    }
    return CFX_OK;
}

int32_t cfx_trip_stats_get_state(cfx_engine *e, cfx_trip_stats_env *envs, int32_t nEnvs) {
    if (!e || !envs) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kTrips, "cfx_trip_stats_get_state"))) return rc;
    if (nEnvs != e->trip.nEnvs) return e->fail("cfx_trip_stats_get_state: n_envs is not the engine's"), CFX_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(envs, e->trip.env, (size_t) nEnvs * sizeof(cfx_trip_stats_env), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

int32_t cfx_trip_stats_set_state(cfx_engine *e, const cfx_trip_stats_env *envs, int32_t nEnvs) {
    if (!e || !envs) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kTrips, "cfx_trip_stats_set_state"))) return rc;  // (the load's baseline builds the shadow; then the records)
    if (nEnvs != e->trip.nEnvs) return e->fail("cfx_trip_stats_set_state: n_envs is not the engine's"), CFX_ERR_INVALID;
    HIP_TRY(hipMemcpyAsync(e->trip.env, envs, (size_t) nEnvs * sizeof(cfx_trip_stats_env), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return CFX_OK;
}

// ---- the trip log: one row per finished vehicle, kept by the trip tracker (optional entry points of include/cityflow_amd.h)

int32_t cfx_trip_log_enable(cfx_engine *e, int32_t capacity) {
    if (!e) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    if (capacity < 0 || capacity > CFX_TRIP_LOG_MAX_CAPACITY) return e->err = "cfx_trip_log_enable: capacity outside [0, 1 << 26]", CFX_ERR_INVALID;
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerRequire(e, kTrips, "cfx_trip_log_enable"))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (a tick or a drain may still be running on the log that goes)
    if (e->freeRaw(&e->trip.log) | e->freeRaw(&e->trip.logHead)) return CFX_ERR_DEVICE;
    e->trip.logCap = 0;
    if (capacity == 0) return CFX_OK;
    if ((rc = e->allocRaw(&e->trip.logHead, 2))) return rc;
    if ((rc = e->allocRaw(&e->trip.log, 2 * (size_t) capacity))) {
        (void) e->freeRaw(&e->trip.logHead);
        return rc;
    }
    HIP_TRY(hipMemsetAsync(e->trip.logHead, 0, 2 * sizeof(int), e->stream));
    e->trip.logCap = capacity;
    return CFX_OK;
}

// trip tracking on, a log there, and what every reader does first (trackerPrepare)
static int tripLogPrepare(cfx_engine *e, const char *what) {
    int rc;
    if ((rc = trackerRequire(e, kTrips, what))) return rc;
    if (!e->trip.log) {
        e->err = std::string(what) + ": there is no trip log (cfx_trip_log_enable)";
        return CFX_ERR_STATE;
    }
    return trackerPrepare(e, kTrips, what);
}

static int launchTripLogDrain(cfx_engine *e, const cfx_trip_log_out &o, int32_t reset) {
    auto fail = [e](const std::string &m) { return e->fail(m); };
    hipLaunchKernelGGL(k_trip_log_drain, dim3(gridFor((size_t) e->trip.logCap)), dim3(kBlock), 0, e->stream, (const int4 *) e->trip.log,
                       (const int *) e->trip.logHead, e->trip.logCap, o);
    HIP_TRY(hipGetLastError());
    // (behind the kernel, not inside it: no block of the drain reads a count another has cleared)
    if (reset) HIP_TRY(hipMemsetAsync(e->trip.logHead, 0, 2 * sizeof(int), e->stream));
    return CFX_OK;
}

static bool tripLogNoneGiven(const cfx_trip_log_out &o) {
    return !o.count && !o.dropped && !o.env && !o.vehicle && !o.origin_road && !o.destination_road && !o.enter_step && !o.finish_step &&
           !o.travel_steps;
}

static int tripLog(cfx_engine *e, const cfx_trip_log_out *out, int32_t reset, bool toHost, void *stream, const char *what) {
    if (!e || !out || tripLogNoneGiven(*out)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    const size_t cap = (size_t) e->trip.logCap;  // (0 without a log: refused below)
    cfx_stage::StageLayout s(!toHost);
    const auto fCount = s.out(out->count, "count", 1), fDropped = s.out(out->dropped, "dropped", 1), fEnv = s.out(out->env, "env", cap),
               fVehicle = s.out(out->vehicle, "vehicle", cap), fOrigin = s.out(out->origin_road, "origin_road", cap),
               fDest = s.out(out->destination_road, "destination_road", cap), fEnter = s.out(out->enter_step, "enter_step", cap),
               fFinish = s.out(out->finish_step, "finish_step", cap), fTravel = s.out(out->travel_steps, "travel_steps", cap);
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = tripLogPrepare(e, what))) return rc;
    if ((rc = e->stageOpen(s, stream))) return rc;
    const cfx_trip_log_out o{s.dev(fCount), s.dev(fDropped), s.dev(fEnv),   s.dev(fVehicle), s.dev(fOrigin),
                             s.dev(fDest),  s.dev(fEnter),   s.dev(fFinish), s.dev(fTravel)};
    if ((rc = launchTripLogDrain(e, o, reset))) return rc;
    return e->stageClose(s, stream);
}
int32_t cfx_observe_trip_log_device(cfx_engine *e, const cfx_trip_log_out *out, int32_t reset, void *consumerStream) {
    return tripLog(e, out, reset, false, consumerStream, "cfx_observe_trip_log_device");
}
int32_t cfx_get_trip_log(cfx_engine *e, const cfx_trip_log_out *out, int32_t reset) {
    return tripLog(e, out, reset, true, nullptr, "cfx_get_trip_log");
}

int32_t cfx_trip_log_set_state(cfx_engine *e, const cfx_trip_log_out *rows, int32_t n, int32_t dropped) {
    if (!e || n < 0 || dropped < 0 ||
        (n > 0 && (!rows || !rows->env || !rows->vehicle || !rows->origin_road || !rows->destination_road || !rows->enter_step ||
                   !rows->finish_step || !rows->travel_steps)))
        return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = tripLogPrepare(e, "cfx_trip_log_set_state"))) return rc;  // (the load's baseline empties the log; then the rows)
    if (n > e->trip.logCap) return e->err = "cfx_trip_log_set_state: n beyond the log's capacity", CFX_ERR_INVALID;
    std::vector<int32_t> packed((size_t) n * 8);
    for (size_t i = 0; i < (size_t) n; ++i) {
        int32_t *row = &packed[8 * i];
        row[0] = rows->env[i], row[1] = rows->vehicle[i], row[2] = rows->origin_road[i], row[3] = rows->destination_road[i];
        row[4] = rows->enter_step[i], row[5] = rows->finish_step[i], row[6] = rows->travel_steps[i], row[7] = 0;
    }
    const int head[2] = {n, dropped};
    if (n) HIP_TRY(hipMemcpyAsync(e->trip.log, packed.data(), packed.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(e->trip.logHead, head, sizeof head, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // (the vectors live on this frame)
    return CFX_OK;
}

// ---- per-movement flow and delay statistics across steps (optional entry points of include/cityflow_amd.h, as above)

int32_t cfx_movement_flow_enable(cfx_engine *e, int32_t on) { return e ? e->trackerEnable(kMoveFlow, on) : CFX_ERR_INVALID; }

// the descriptor as this library knows it; CFX_ERR_INVALID with a message otherwise
static int moveFlowArgs(cfx_engine *e, const cfx_movement_flow_out *out, cfx_movement_flow_out *a, const char *what) {
    int rc;
    if ((rc = takeDescriptor(e, out, a, what))) return rc;
    if (!a->entered && !a->entered_lane_steps && !a->entered_lane_waiting_steps && !a->left && !a->left_steps && !a->left_waiting_steps &&
        !a->waiting_steps && !a->max_waiting_steps && !a->reset)
        return CFX_ERR_INVALID;
    return CFX_OK;
}

// ... the roadLink index and the caller's row length
static int moveFlowRows(cfx_engine *e, const cfx_movement_flow_out &a, const char *what) {
    int rc;
    if ((rc = interTables(e))) return rc;
    if (a.max_roadlinks != e->interTab.M) {
        e->err = std::string(what) + ": max_roadlinks must be the network's " + std::to_string(e->interTab.M) + ", not " +
                 std::to_string(a.max_roadlinks);
        return CFX_ERR_INVALID;
    }
    return CFX_OK;
}

// a group per roadLink row (k_movement_flow_drain, cfx_kernels.h)
static void launchMoveFlowDrain(cfx_engine *e, const MoveFlowOut &o, int32_t reset) {
    const size_t rows = (size_t) e->I * e->interTab.M;
    if (rows == 0) return;
    hipLaunchKernelGGL(k_movement_flow_drain, dim3(gridFor(rows * kFeatGroup)), dim3(kBlock), 0, e->stream, e->move.link, e->move.skip,
                       e->interTab.rlOff, e->interTab.rlLinks, e->net.interVirtual, (int) rows, e->interTab.M, o, reset ? 1 : 0);
}

static int moveFlow(cfx_engine *e, const cfx_movement_flow_out *out, bool toHost, void *stream, const char *what) {
    cfx_movement_flow_out a{};
    int rc;
    if ((rc = moveFlowArgs(e, out, &a, what))) return rc;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    cfx_stage::StageLayout s(!toHost);
    const auto fEntered = s.out(a.entered, "entered");
    const auto fELS = s.out(a.entered_lane_steps, "entered_lane_steps"), fELW = s.out(a.entered_lane_waiting_steps, "entered_lane_waiting_steps");
    const auto fLeft = s.out(a.left, "left");
    const auto fLS = s.out(a.left_steps, "left_steps"), fLW = s.out(a.left_waiting_steps, "left_waiting_steps"),
               fW = s.out(a.waiting_steps, "waiting_steps");
    const auto fMax = s.out(a.max_waiting_steps, "max_waiting_steps");
    if ((rc = e->stageCheck(s, what))) return rc;
    if ((rc = trackerPrepare(e, kMoveFlow, what))) return rc;
    if ((rc = moveFlowRows(e, a, what))) return rc;
    const size_t rows = (size_t) e->I * e->interTab.M;  // (known once the index is built)
    s.count(fEntered, rows), s.count(fELS, rows), s.count(fELW, rows), s.count(fLeft, rows);
    s.count(fLS, rows), s.count(fLW, rows), s.count(fW, rows), s.count(fMax, rows);
    if ((rc = e->stageOpen(s, stream))) return rc;
    launchMoveFlowDrain(e, MoveFlowOut{s.dev(fEntered), s.dev(fELS), s.dev(fELW), s.dev(fLeft), s.dev(fLS), s.dev(fLW), s.dev(fW),
                                       s.dev(fMax)}, a.reset);
    HIP_TRY(hipGetLastError());
    return e->stageClose(s, stream);
}
int32_t cfx_observe_movement_flow_device(cfx_engine *e, const cfx_movement_flow_out *out, void *consumerStream) {
    return moveFlow(e, out, false, consumerStream, "cfx_observe_movement_flow_device");
}
int32_t cfx_get_movement_flow(cfx_engine *e, const cfx_movement_flow_out *out) {
    return moveFlow(e, out, true, nullptr, "cfx_get_movement_flow");
}

int32_t cfx_movement_flow_get_state(cfx_engine *e, int32_t *records, int32_t nVehicles, cfx_movement_flow_link *links, int32_t *tick) {
    if (!e || !tick || nVehicles < 0 || (nVehicles > 0 && !records) || (e->K > 0 && !links)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerPrepare(e, kMoveFlow, "cfx_movement_flow_get_state"))) return rc;
    if ((rc = recordsOut(e, "cfx_movement_flow_get_state", e->move.rec, records, nVehicles))) return rc;
    std::vector<unsigned long long> skip((size_t) e->K * 3);
    if (e->K > 0) {
        HIP_TRY(hipMemcpyAsync(links, e->move.link, (size_t) e->K * sizeof(cfx_movement_flow_link), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(skip.data(), e->move.skip, skip.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (size_t k = 0; k < (size_t) e->K; ++k) {  // (what crossings of whole laneLinks added, folded in as the drain does)
        links[k].entered += (int32_t) skip[3 * k];
        links[k].left += (int32_t) skip[3 * k];
        links[k].entered_lane_steps += (int64_t) skip[3 * k + 1];
        links[k].entered_lane_waiting_steps += (int64_t) skip[3 * k + 2];
    }
    *tick = e->move.tick;
    return CFX_OK;
}

int32_t cfx_movement_flow_set_state(cfx_engine *e, const int32_t *records, int32_t nVehicles, const cfx_movement_flow_link *links,
                                    int32_t tick) {
    if (!e || nVehicles < 0 || (nVehicles > 0 && !records) || (e->K > 0 && !links)) return CFX_ERR_INVALID;
    auto fail = [e](const std::string &m) { return e->fail(m); };
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = trackerRequire(e, kMoveFlow, "cfx_movement_flow_set_state"))) return rc;
    if ((rc = recordsIn(e, "cfx_movement_flow_set_state", e->move.rec, records, nVehicles))) return rc;
    if (e->K > 0) {
        HIP_TRY(hipMemcpyAsync(e->move.link, links, (size_t) e->K * sizeof(cfx_movement_flow_link), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemsetAsync(e->move.skip, 0, (size_t) e->K * 3 * sizeof(unsigned long long), e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->move.tick = tick;
    e->tracker[kMoveFlow].baselineDue = false;
    return CFX_OK;
}

int32_t cfx_profile_kernel_count(void) { return kNumProfKernels; }
const char *cfx_profile_kernel_name(int32_t k) { return (k >= 0 && k < kNumProfKernels) ? kProfNames[k] : ""; }

int32_t cfx_profile_enable(cfx_engine *e, int32_t on) {
    if (!e) return CFX_ERR_INVALID;
    (void) hipSetDevice(e->device);
    if (e->profiling && !on) e->profCollect();
    e->profiling = on != 0;
    return CFX_OK;
}

int32_t cfx_profile_read(cfx_engine *e, double *totalMs, int64_t *launches) {
    if (!e) return CFX_ERR_INVALID;
    (void) hipSetDevice(e->device);
    e->profCollect();
    for (int k = 0; k < kNumProfKernels; ++k) {
        if (totalMs) totalMs[k] = e->profMs[k];
        if (launches) launches[k] = e->profLaunches[k];
        e->profMs[k] = 0;
        e->profLaunches[k] = 0;
    }
    return CFX_OK;
}

// The optional entry points are looked up by name, so nothing but these lines holds a definition to the type
// include/cityflow_amd.h declares for its symbol; and the records that cross the ABI whole keep their sizes.
#define CFX_ENTRY_POINT(f) static_assert(std::is_same<decltype(&f), f##_fn>::value, #f)
CFX_ENTRY_POINT(cfx_get_cross_stats);
CFX_ENTRY_POINT(cfx_checkpoint_restore_envs);
CFX_ENTRY_POINT(cfx_checkpoint_create);
CFX_ENTRY_POINT(cfx_checkpoint_save);
CFX_ENTRY_POINT(cfx_checkpoint_restore);
CFX_ENTRY_POINT(cfx_checkpoint_info);
CFX_ENTRY_POINT(cfx_checkpoint_destroy);
CFX_ENTRY_POINT(cfx_stream_handle);
CFX_ENTRY_POINT(cfx_observe_device);
CFX_ENTRY_POINT(cfx_set_tl_phases_device);
CFX_ENTRY_POINT(cfx_device_error);
CFX_ENTRY_POINT(cfx_set_tl_plan_device);
CFX_ENTRY_POINT(cfx_set_tl_plan);
CFX_ENTRY_POINT(cfx_get_tl_phase_durations_device);
CFX_ENTRY_POINT(cfx_get_tl_phase_durations);
CFX_ENTRY_POINT(cfx_restore_tl_plan);
CFX_ENTRY_POINT(cfx_tl_plan_error);
CFX_ENTRY_POINT(cfx_set_lane_speed_limits_device);
CFX_ENTRY_POINT(cfx_set_lane_speed_limits);
CFX_ENTRY_POINT(cfx_get_lane_speed_limits_device);
CFX_ENTRY_POINT(cfx_get_lane_speed_limits);
CFX_ENTRY_POINT(cfx_restore_lane_speed_limits);
CFX_ENTRY_POINT(cfx_observe_lanes_device);
CFX_ENTRY_POINT(cfx_get_lane_features);
CFX_ENTRY_POINT(cfx_observe_lane_obs_device);
CFX_ENTRY_POINT(cfx_get_lane_obs);
CFX_ENTRY_POINT(cfx_observe_vehicles_device);
CFX_ENTRY_POINT(cfx_set_drivable_geometry);
CFX_ENTRY_POINT(cfx_get_waiting_custom_speeds);
CFX_ENTRY_POINT(cfx_set_vehicle_speeds_device);
CFX_ENTRY_POINT(cfx_set_vehicle_speeds);
CFX_ENTRY_POINT(cfx_set_vehicle_routes_device);
CFX_ENTRY_POINT(cfx_set_vehicle_routes);
CFX_ENTRY_POINT(cfx_get_vehicle_routes_device);
CFX_ENTRY_POINT(cfx_get_vehicle_routes);
CFX_ENTRY_POINT(cfx_observe_intersections_device);
CFX_ENTRY_POINT(cfx_get_intersection_features);
CFX_ENTRY_POINT(cfx_lane_flow_enable);
CFX_ENTRY_POINT(cfx_observe_lane_flow_device);
CFX_ENTRY_POINT(cfx_get_lane_flow);
CFX_ENTRY_POINT(cfx_lane_flow_get_state);
CFX_ENTRY_POINT(cfx_lane_flow_set_state);
CFX_ENTRY_POINT(cfx_detectors_define);
CFX_ENTRY_POINT(cfx_detectors_enable);
CFX_ENTRY_POINT(cfx_observe_detectors_device);
CFX_ENTRY_POINT(cfx_get_detectors);
CFX_ENTRY_POINT(cfx_detectors_get_state);
CFX_ENTRY_POINT(cfx_detectors_set_state);
CFX_ENTRY_POINT(cfx_trip_stats_enable);
CFX_ENTRY_POINT(cfx_observe_trip_stats_device);
CFX_ENTRY_POINT(cfx_get_trip_stats);
CFX_ENTRY_POINT(cfx_trip_stats_get_state);
CFX_ENTRY_POINT(cfx_trip_stats_set_state);
CFX_ENTRY_POINT(cfx_trip_log_enable);
CFX_ENTRY_POINT(cfx_observe_trip_log_device);
CFX_ENTRY_POINT(cfx_get_trip_log);
CFX_ENTRY_POINT(cfx_trip_log_set_state);
CFX_ENTRY_POINT(cfx_movement_flow_enable);
CFX_ENTRY_POINT(cfx_observe_movement_flow_device);
CFX_ENTRY_POINT(cfx_get_movement_flow);
CFX_ENTRY_POINT(cfx_movement_flow_get_state);
CFX_ENTRY_POINT(cfx_movement_flow_set_state);
#undef CFX_ENTRY_POINT
static_assert(sizeof(cfx_lane_flow_lane) == 48, "cfx_lane_flow_lane");
static_assert(sizeof(cfx_detector) == 64, "cfx_detector");
static_assert(sizeof(cfx_trip_stats_env) == 56, "cfx_trip_stats_env");
static_assert(sizeof(cfx_movement_flow_link) == 64, "cfx_movement_flow_link");

}  // extern "C"
