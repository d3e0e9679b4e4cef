/*
 * cityflow_amd.h — C ABI of the MI355X-native CityFlow step engine ("cfx").
 *
 * This is the drop-in boundary between the C++ host (JSON loading, flow spawning / RNG, string ids,
 * the pybind11 `cityflow.Engine` class) and the device engine that owns all vehicle state in HBM and
 * advances it with hand-written HIP kernels.  The reference has no internal FFI seam (its only
 * boundary is the pybind11 class, reference src/cityflow.cpp:10-47); the entry points below are what a
 * maintainer of the reference would bind from `CityFlow::Engine` to off-load `Engine::nextStep`
 * (reference src/engine/engine.cpp:566-594) and the RL getters around it (engine.cpp:615-760).
 * INTEGRATION.md shows that binding.
 *
 * Conventions: opaque handle; plain pointers and sizes; caller-allocated outputs; every function
 * returns 0 on success or a negative cfx_status, with a message available from cfx_last_error();
 * no exceptions cross the ABI; one HIP stream per engine; getters are synchronous on return,
 * cfx_step() is asynchronous (ordered on the engine's stream).  Strings never cross this ABI:
 * lanes, laneLinks, intersections, roads, routes, templates and vehicles are dense int32 indices.
 *
 * Index spaces
 *   lane      0..n_lanes-1        reference order RoadNet::getLanes()      (roadnet.cpp:314-318)
 *   laneLink  0..n_lanelinks-1    reference order RoadNet::getLaneLinks()  (roadnet.cpp:319-323)
 *   drivable  lane l -> l ; laneLink k -> n_lanes + k   (== RoadNet::getDrivables())
 *   vid       host-assigned vehicle number, dense, monotone since the last reset
 */
#ifndef CITYFLOW_AMD_H
#define CITYFLOW_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFX_ABI_VERSION 9

typedef enum cfx_status {
    CFX_OK = 0,
    CFX_ERR_INVALID = -1,   /* bad argument / index out of range                    */
    CFX_ERR_DEVICE = -2,    /* HIP runtime failure (no device, launch error, OOM)   */
    CFX_ERR_CAPACITY = -3,  /* an internal fixed-capacity table overflowed          */
    CFX_ERR_STATE = -4      /* call not valid in the current state                  */
} cfx_status;

typedef struct cfx_engine cfx_engine; /* opaque */

/* Flattened, immutable road network (replaces RoadNet / Road / Lane / LaneLink / RoadLink / Cross /
 * Intersection / LightPhase, reference src/roadnet/roadnet.h:64-481, trafficlight.h:15-50).
 * All arrays are copied by cfx_create(); the caller may free them afterwards. */
typedef struct cfx_net {
    int32_t n_roads, n_lanes, n_lanelinks, n_inters;
    int32_t n_xentries;  /* 2 * number of Cross objects: one entry per (laneLink, cross) */
    int32_t n_phases;    /* total LightPhase count over all intersections */
    int32_t n_avail;     /* total size of phase_avail */

    /* per drivable [n_lanes + n_lanelinks] */
    const double *drv_length;    /* Drivable::length (roadnet.cpp:252,502) */
    const double *drv_max_speed; /* lanes: JSON maxSpeed; laneLinks: 10000 (roadnet.h:456) */

    /* per lane [n_lanes] */
    const int32_t *lane_road;     /* owning road */
    const int32_t *lane_index;    /* Lane::laneIndex */
    const int32_t *lane_ll_start; /* [n_lanes+1] CSR offsets into lane_ll */
    const int32_t *lane_ll;       /* [n_lanelinks] laneLink ids in Lane::laneLinks order */

    /* per road [n_roads] : lanes of a road are contiguous */
    const int32_t *road_lane_start; /* [n_roads+1] */

    /* per laneLink [n_lanelinks] */
    const int32_t *ll_start_lane;
    const int32_t *ll_end_lane;
    const int32_t *ll_inter;    /* owning intersection */
    const int32_t *ll_roadlink; /* RoadLink::index inside that intersection (roadnet.h:417) */
    const int32_t *ll_type;     /* RoadLinkType: 1 turn_right, 2 turn_left, 3 go_straight (roadnet.h:401-403) */
    const int32_t *ll_x_start;  /* [n_lanelinks+1] CSR offsets into the x_* arrays */

    /* per cross entry [n_xentries]; a laneLink's entries are sorted ascending by x_dist exactly as
     * Intersection::initCrosses sorts LaneLink::crosses (roadnet.cpp:568-575) */
    const double *x_dist;   /* Cross::distanceOnLane for the owning laneLink */
    const int32_t *x_peer;  /* entry index of the same Cross seen from the other laneLink */
    const int32_t *x_ll;    /* owning laneLink */

    /* per intersection [n_inters] */
    const int32_t *inter_virtual;
    const int32_t *inter_n_roadlinks;
    const int32_t *inter_phase_start; /* [n_inters+1] offsets into phase_time */
    const int32_t *inter_avail_start; /* [n_inters]   offset of this intersection's block in phase_avail */
    const double *phase_time;         /* [n_phases] LightPhase::time */
    const uint8_t *phase_avail;       /* per intersection: n_phases_i x n_roadlinks_i row-major 0/1 */

    /* lane change only (may be NULL when cfx_config::lane_change == 0), per lane [n_lanes] */
    const double *lane_width;         /* Lane::width (roadnet.h:303): lateral offset that completes a change */
    const int32_t *lane_n_segments;   /* Lane::segments.size() (Road::buildSegmentationByInterval roadnet.cpp:687-691) */
} cfx_net;

typedef struct cfx_config {
    double interval;          /* Engine::interval */
    int32_t rl_traffic_light; /* Engine::rlTrafficLight: lights advance only via cfx_set_tl_phase */
    int32_t lane_change;      /* Engine::laneChange (engine.cpp:53): see "Lane change" below */
    int32_t device;           /* HIP device ordinal (ignored by CPU implementations) */
    /* Implementation choices that never change results (all 0 = let the engine decide; CPU implementations ignore them).
     * The host reads them from an optional "cfx" object of the config file, which the reference ignores. */
    int32_t cross_mode;       /* cross walk: CFX_CROSS_AUTO by size, CFX_CROSS_LATENCY (k_cross), CFX_CROSS_THROUGHPUT (k_cross2) */
    int32_t layout;           /* vehicle order in HBM: CFX_LAYOUT_AUTO, CFX_LAYOUT_DENSE (rebuilt every step),
                               * CFX_LAYOUT_RING (per-drivable ring segments, committed in place; not with lane_change) */
    int32_t debug_sync;       /* synchronise after every kernel of a step and name the one that faulted (developer aid) */
    int32_t ring_lanes_per_wave; /* ring layout, developer knob (0 = the engine decides everything): digits v = G + 1000 * (B / 256)
                                  * + 10000 * F.  G: lanes one workgroup of the action kernel owns (0 = adaptive); B: its
                                  * workgroup size (256 / 512); F: form of the step — 0 by size, 2 the action kernel walks the
                                  * lanes (kr_action), 3 one thread per entry of the step's vehicle list (kr_index + kl_action; 6: its tiles handed out by
                                  * ticket, as on networks above 524 k drivables), 4 as 2 with the commit
                                  * as a launch of its own, 7 dense tiles (cfx_halo_config).  Any other F (1, 5, 8, 9) names no
                                  * form: cfx_create fails with CFX_ERR_INVALID.  Results never depend on it (tests/test_parity_pins.py) */
    int32_t ring_capacity_percent; /* ring layout: initial ring capacities as a percentage of the bumper-to-bumper bound
                                    * (0 = 100).  Small values make the growth path run (tests) — of the rings and, below 100,
                                    * of the vehicle tables too (they start at 4 k instead of 4 M vehicle numbers); results
                                    * never depend on it */
    int32_t lane_history;     /* keep Lane::history (roadnet.cpp:900-915; see cfx_get_lane_history), numbers only Archive dumps
                               * show.  Ring layout: the record of a step is taken by spare blocks of the NEXT step's action launch
                               * (or by a launch of its own when cfx_get/set_lane_history, a reset or a load come first).  A tile
                               * (ring layout) takes the step's record behind the step's halo import: the rows of the lanes it
                               * owns are the lanes' history, a ghost lane's rows record its proxy */
    int32_t n_envs;           /* 0 or 1: one simulation.  E > 1: the network is E disjoint copies of one network with their
                               * index spaces concatenated copy by copy (roads, lanes, laneLinks, intersections: n_roads etc. are
                               * multiples of E) — E independent simulations advanced by one engine (batched environments).  Only
                               * lane change needs to know: each environment has its own schedule walk and its own priority
                               * stream (see "Lane change" below) */
    int32_t dense_form;       /* dense layout, developer knob (0 = the engine decides): 256 + a bit mask of how the step's kernels
                               * are organised — 2: the admission kernel over the lanes only (a laneLink's gate record rewritten
                               * only when its intersection's phase has changed, laneLink tails read from the committed
                               * records); 4: up to 1024 (instead of 128) spawn records of a step travel in the admission
                               * kernel's arguments.  256 = both off.  Results never depend on it (tests/test_dense_forms.py) */
} cfx_config;
#define CFX_CROSS_AUTO 0
#define CFX_CROSS_LATENCY 1
#define CFX_CROSS_THROUGHPUT 2
#define CFX_LAYOUT_AUTO 0
#define CFX_LAYOUT_DENSE 1
#define CFX_LAYOUT_RING 2

/* VehicleInfo (reference src/vehicle/vehicle.h:31-45) + the two per-template constants derived from it. */
typedef struct cfx_vehicle_template {
    double len, width, max_pos_acc, max_neg_acc, usual_pos_acc, usual_neg_acc;
    double min_gap, max_speed, headway_time, yield_distance, turn_speed;
    /* maxSpeed^2/usualNegAcc/2 + maxSpeed*interval*2 : ControllerInfo::approachingIntersectionDistance
     * (vehicle.cpp:42-44) and the head-of-lane leader search bound (vehicle.cpp:190-192). */
    double approach_dist;
    double initial_speed; /* VehicleInfo::speed (vehicle.h:32) a vehicle enters its first lane with; only
                           * push_vehicle can set it (engine.cpp:696), flows always create vehicles at rest */
} cfx_vehicle_template;

/* One vehicle entering the simulation this step (Flow::nextStep flow.cpp:6-22 + Engine::planRoute
 * engine.cpp:450-470, both evaluated on the host because they own the mt19937 stream). */
typedef struct cfx_spawn {
    int32_t vid;        /* dense id; must equal the number of vehicles spawned since the last reset */
    int32_t priority;   /* Vehicle::priority (vehicle.cpp:45) */
    int32_t templ;      /* template index */
    int32_t route;      /* route index */
    int32_t lane;       /* first lane (Router::getFirstDrivable router.cpp:23-37) */
    int32_t prev_wait;  /* vid previously pushed on this lane's waitingBuffer since the last reset, or -1 */
    double enter_time;  /* Vehicle::enterTime (vehicle.cpp:46) */
} cfx_spawn;

typedef struct cfx_scalars {
    int64_t step;                  /* Engine::step */
    int64_t active_vehicle_count;  /* Engine::activeVehicleCount (running vehicles) */
    int64_t finished_vehicle_count;/* Engine::finishedVehicleCnt */
    int64_t spawned_vehicle_count; /* vehicles handed to cfx_step since the last reset */
    double cumulative_travel_time; /* Engine::cumulativeTravelTime */
    double live_enter_time_sum;    /* sum of enter_time over spawned-and-not-finished vehicles (0 if not kept) */
    int64_t vehicle_steps;         /* sum over executed steps of the vehicles that took the step (ran phase 4) */
    /* pairs of vehicles that entered the same drivable in one step with EXACTLY equal distances, since the last reset /
     * load.  Engine::updateLocation orders the entrants with an unstable std::sort on distance alone (engine.cpp:480), so
     * the reference's own order of such a pair depends on heap addresses and thread timing; this ABI breaks the tie by
     * vehicle number.  A comparison with the reference is well defined only while this counter stands still. */
    int64_t tie_events;
    /* the drivables (index space above) that received the most recent tie events: event number i (counting from 0 since
     * the last reset / load) is kept at index i % 8; -1 = none yet, or not known (a tiled engine does not report them).
     * A checker uses them to see WHERE two correct engines may differ from then on. */
    int32_t tie_drivables[8];
    /* diagnostic of the last step (0 where an implementation does not count it; never part of a result): vehicles handed to
     * the cross phase */
    int32_t diag_cross_jobs;
    /* cfx_set_vehicle_speed calls for a vehicle number the NEXT cfx_step was expected to create (see there) whose step then did
     * not create it, since the engine was created: such a speed is dropped, and counted here */
    int32_t dropped_future_speeds;
} cfx_scalars;

/* Full per-vehicle state of every running vehicle, caller-allocated SoA (any pointer may be NULL).
 * Order: by drivable (index space above), then front (furthest ahead) to back inside a drivable,
 * i.e. the order of Drivable::vehicles (roadnet.h:245). */
typedef struct cfx_vehicle_view {
    int32_t capacity;       /* in: number of elements each array can hold */
    int32_t count;          /* out: number of running vehicles */
    int32_t *vid;
    int32_t *drivable;
    int32_t *prev_drivable; /* -1 if none */
    int32_t *leader_vid;    /* -1 if none */
    int32_t *blocker_vid;   /* -1 if none */
    int32_t *enter_ll_time; /* INT32_MAX when not on a laneLink */
    int32_t *route_pos;     /* Router::iCurRoad as an index into the route */
    double *dis;
    double *speed;
    double *gap;            /* ControllerInfo::gap: refreshed only where leader_vid >= 0, otherwise the value it last had */
    /* lane change (zero / -1 when it is off) */
    int32_t *lc_partner_vid; /* LaneChangeInfo::partner */
    uint8_t *lc_flags;       /* CFX_LC_* bits */
    double *lc_offset;       /* LaneChangeInfo::offset */
    int32_t *lc_last_dir;    /* LaneChange::lastDir (what the replay log prints, engine.cpp:524) */
    int32_t *lc_target_lane; /* signalSend->target while CFX_LC_CHANGING (the only signal that outlives a step), else -1 */
    int32_t *lc_direction;   /* signalSend->direction, same condition, else 0 */
    double *lc_last_change_time; /* LaneChange::lastChangeTime */
    double *lc_waiting_time;     /* LaneChange::waitingTime */
} cfx_vehicle_view;
#define CFX_LC_SHADOW 1u   /* partnerType == 2: a shadow; its id is "<parent id>_shadow" until the change finishes */
#define CFX_LC_PARENT 2u   /* partnerType == 1: the real vehicle of a changing pair */
#define CFX_LC_CHANGING 4u /* LaneChange::changing */

int32_t cfx_abi_version(void);
int32_t cfx_create(const cfx_net *net, const cfx_config *cfg, cfx_engine **out);
void cfx_destroy(cfx_engine *e);
const char *cfx_last_error(const cfx_engine *e); /* e may be NULL: error of the last failed cfx_create */
const char *cfx_backend_name(void);             /* "hip-gfx950" for the product library */

/* Append vehicle templates / routes (flows at load time; push_vehicle / set_vehicle_route later).
 * A route is its road sequence plus, for every position p and every lane j of road[p], the laneLink
 * Router::getNextDrivable would choose from that lane (router.cpp:49-76,96-129), or -1.
 *   route_start[n_routes+1]           offsets into `roads`
 *   next_start[route_start[n]+1]      offsets into `next_ll`, one block per route position */
int32_t cfx_add_templates(cfx_engine *e, int32_t n, const cfx_vehicle_template *t);
int32_t cfx_add_routes(cfx_engine *e, int32_t n_routes, const int32_t *route_start, const int32_t *roads,
                       const int32_t *next_start, const int32_t *next_ll);

/* One Engine::nextStep (engine.cpp:566-594): enqueue `recs` on their lanes' waiting buffers, admit,
 * notify crosses, get action, update location, commit, leader/gap, traffic lights, step += 1. */
int32_t cfx_step(cfx_engine *e, const cfx_spawn *recs, int32_t n);
int32_t cfx_sync(cfx_engine *e);

/* Engine::reset (engine.cpp:744-760): drop all vehicles and waiting buffers, lights to phase 0, step 0.
 * Templates and routes are kept. */
int32_t cfx_reset(cfx_engine *e);

/* TrafficLight::setPhase (trafficlight.cpp:39-41).  Unlike the reference this is range-checked. */
int32_t cfx_set_tl_phase(cfx_engine *e, int32_t inter, int32_t phase);
/* same for n (intersection, phase) pairs in one call (an RL agent sets every signal each step) */
int32_t cfx_set_tl_phases(cfx_engine *e, int32_t n, const int32_t *inters, const int32_t *phases);
int32_t cfx_get_tl_state(cfx_engine *e, int32_t *cur_phase /*[n_inters]*/, double *remain /*[n_inters]*/);

int32_t cfx_get_scalars(cfx_engine *e, cfx_scalars *out);
/* the vehicle layout this engine runs on: CFX_LAYOUT_DENSE or CFX_LAYOUT_RING (what cfx_config::layout = AUTO resolved to;
 * CPU implementations report CFX_LAYOUT_AUTO) */
int32_t cfx_get_layout(cfx_engine *e);
/* ring layout: total slots of all rings and how often every capacity has been doubled so far (1 = never; 0 slots on other
 * layouts / implementations) */
int32_t cfx_get_ring_info(cfx_engine *e, int64_t *slots, int32_t *capacity_scale);
int32_t cfx_get_lane_counts(cfx_engine *e, int32_t *out /*[n_lanes]*/);         /* getLaneVehicleCount */
int32_t cfx_get_lane_waiting_counts(cfx_engine *e, int32_t *out /*[n_lanes]*/); /* speed < 0.1 (engine.cpp:641) */
int32_t cfx_get_vehicles(cfx_engine *e, cfx_vehicle_view *view);
/* per-vid life-cycle state for vids [first, first+n): 0 waiting, 1 running, 2 finished */
int32_t cfx_get_vehicle_status(cfx_engine *e, int32_t first_vid, int32_t n, uint8_t *out);
/* vids still sitting in lanes' waiting buffers, lane by lane, FIFO order; returns count via *n */
int32_t cfx_get_waiting(cfx_engine *e, int32_t capacity, int32_t *vid, int32_t *lane, int32_t *n);

/* Vehicle::setCustomSpeed (vehicle.h:128-131, used by getCarFollowSpeed vehicle.cpp:214,220-221): overrides
 * the car-following target for the vehicle's next step only (Vehicle::update clears it, vehicle.cpp:120-122).
 * A vid at or beyond the vehicles created so far names a vehicle the NEXT cfx_step's spawn records will create (a vehicle
 * pushed since the last step, which Engine::setVehicleSpeed engine.cpp:827-834 already finds): the speed is kept and is in
 * place before that step's admission; it is dropped if that step does not create the vehicle — counted in
 * cfx_scalars::dropped_future_speeds.  Only the next CFX_FUTURE_SPEED_WINDOW vehicle numbers are accepted that way; anything
 * beyond (or negative) is CFX_ERR_INVALID. */
#define CFX_FUTURE_SPEED_WINDOW 65536
int32_t cfx_set_vehicle_speed(cfx_engine *e, int32_t vid, double speed);
/* Switch a waiting or running vehicle to route `route` (already added with cfx_add_routes) whose first road is the
 * road the vehicle is on; Router::iCurRoad restarts at 0 (Router::setRoute router.cpp:245-264 after its checks,
 * which the host performs). */
int32_t cfx_set_vehicle_route(cfx_engine *e, int32_t vid, int32_t route);
/* state: 0 waiting, 1 running, 2 finished; drivable / route_pos / route are -1 unless running (route: any state) */
int32_t cfx_get_vehicle(cfx_engine *e, int32_t vid, int32_t *state, int32_t *drivable, int32_t *route_pos,
                        int32_t *route);

/* Complete dynamic state, for Archive-style snapshot / restore (reference src/engine/archive.cpp:9-126).
 * Reading it back is done with the getters above; cfx_load_state replaces the engine's whole dynamic state
 * (templates and routes referenced by it must already have been added). */
typedef struct cfx_state {
    int64_t step, finished_vehicle_count, vehicle_steps;
    double cumulative_travel_time;
    /* vehicle table, index = vid */
    int32_t n_vehicles;
    const int32_t *v_priority, *v_templ, *v_route;
    const double *v_enter_time;
    const uint8_t *v_state;          /* 0 waiting, 1 running, 2 finished */
    /* running vehicles in Drivable::vehicles order: by drivable, front to back */
    int32_t n_running;
    const int32_t *r_vid, *r_drivable, *r_prev_drivable, *r_blocker_vid, *r_enter_ll_time, *r_route_pos;
    const double *r_dis, *r_speed;
    const double *r_custom_speed;    /* NaN where no custom speed is pending; may be NULL */
    /* ControllerInfo::gap is STORED state in the reference: Vehicle::getCarFollowSpeed (vehicle.cpp:212-238) reads what
     * updateLeaderAndGap left at the end of the previous step, and Archive::resume restores it with the vehicle.  An engine
     * that derives leader and gap from the order at the start of a step uses r_gap[i] INSTEAD of the derived gap in the first
     * step after the load, for every vehicle that has a leader then (NaN, or r_gap == NULL: the derived one).  The two are the
     * same number unless the archive came through a file whose `dis` / `gap` literals were not read back exactly — the
     * reference's JSON reader is not correctly rounded (csrc/host/json_number.h).  Lane change: makeSignal reads it too. */
    const double *r_gap;
    /* lane change (all may be NULL = no lane-change state): what of LaneChange / LaneChangeInfo outlives a step —
     * signals received, target leader / follower are cleared by every step's clearSignal (engine.cpp:424) */
    const int32_t *r_lc_partner_vid, *r_lc_last_dir, *r_lc_target_lane, *r_lc_direction;
    const uint8_t *r_lc_flags;       /* CFX_LC_* */
    const double *r_lc_offset, *r_lc_last_change_time, *r_lc_waiting_time;
    /* waiting buffers, lane by lane, FIFO order */
    int32_t n_waiting;
    const int32_t *w_vid, *w_lane;
    /* traffic lights [n_inters] */
    const int32_t *tl_phase;
    const double *tl_remain;
} cfx_state;
int32_t cfx_load_state(cfx_engine *e, const cfx_state *s);
/* pending custom speeds of the running vehicles, same order as cfx_get_vehicles (NaN = none) */
int32_t cfx_get_custom_speeds(cfx_engine *e, int32_t capacity, double *out);

/* ---- Lane::history (reference src/roadnet/roadnet.h:305-316, Lane::updateHistory roadnet.cpp:900-915, called for every lane at
 * the end of every step, engine.cpp:429-442): the last steps' {vehicle count, mean speed} per lane — up to
 * CFX_LANE_HISTORY_MAX records, the list is trimmed to 240 BEFORE a step's record is appended — and the two running aggregates
 * historyVehicleNum / historyAverageSpeed, kept up with the reference's own recurrence (the sum of the speeds is taken in the
 * lane's list order; the popped records' share is subtracted from historyVehicleNum * historyAverageSpeed, a product formed anew
 * every step).  It feeds Road::getAverageSpeed / the DURATION router, which nothing in the reference can select (router.h:42);
 * what makes it visible is Archive::dump (archive.cpp:286-294).  Kept only with cfx_config::lane_history; Engine::reset does
 * NOT clear it (Lane::reset roadnet.cpp:832-835), cfx_load_state leaves it alone — Archive::resume's part is cfx_set_lane_history. */
#define CFX_LANE_HISTORY_MAX 241
typedef struct cfx_lane_history {
    int32_t n_lanes;                /* in: must equal the engine's */
    int32_t *len;                   /* [n_lanes] records held */
    int32_t *vehicle_num;           /* [n_lanes * CFX_LANE_HISTORY_MAX] lane-major, oldest record first */
    double *average_speed;          /* [n_lanes * CFX_LANE_HISTORY_MAX] */
    int32_t *history_vehicle_num;   /* [n_lanes] Lane::historyVehicleNum */
    double *history_average_speed;  /* [n_lanes] Lane::historyAverageSpeed */
} cfx_lane_history;
int32_t cfx_get_lane_history(cfx_engine *e, cfx_lane_history *out);       /* CFX_ERR_STATE: the engine does not keep it */
int32_t cfx_set_lane_history(cfx_engine *e, const cfx_lane_history *in);

/* ---- Lane change (cfx_config::lane_change = 1; reference src/vehicle/lanechange.cpp, engine.cpp:374-400,792-820) ----
 * A vehicle that starts to change lane gets a SHADOW in the target lane: a new vehicle (`new Vehicle(*v, id + "_shadow")`,
 * engine.cpp:812-820) that draws its priority from the engine's mt19937 — the stream the host's spawner owns.  So
 *   before cfx_step   cfx_lane_change_supply(e, n, priorities): the next n priorities the generator WOULD hand out
 *                     (already filtered for collisions with live vehicles); the step uses the first k of them, in the
 *                     order the shadows are created;
 *   after cfx_step    cfx_lane_change_poll(e, cap, parent_vid, &k): the vehicles that got a shadow in that step, in
 *                     creation order; shadow i has vid = (vehicles known before the step's spawn records) + (number of
 *                     spawn records) + i.  The host advances its generator past the draws that produced the first k
 *                     priorities and numbers the NEXT step's spawn records after the shadows.
 * cfx_lane_change_poll waits only for the part of the step that creates shadows, not for the whole step.
 * Order: the reference walks the candidates in `std::set<Vehicle*>` (heap address) order, which is not a function of
 * the simulation state, and then sorts them by urgency with std::sort — all urgencies are equal, yet
 * libstdc++'s introsort permutes more than 16 equal elements.  This ABI fixes the walk to: candidates in creation order
 * (ascending vid = the address order of a heap that never reuses memory), put through that very permutation (a closed
 * function of the candidate count; `lcSortedPosition`, csrc/hip/cfx_lc_kernels.h).  Shadows are numbered, and take the
 * supplied priorities, in walk order.  More than n shadows in one step: CFX_ERR_CAPACITY from the poll.
 * Batched environments (cfx_config::n_envs = E > 1): every environment is its own Engine in the reference, so the walk above is
 * taken per environment (its candidates in ascending vid, put through the permutation of ITS candidate count), the
 * environments one after the other; n must be a multiple of E and environment e takes its priorities from
 * priorities[e * n / E ...]; the poll lists the parents environment by environment, shadows are numbered in that order. */
int32_t cfx_lane_change_supply(cfx_engine *e, int32_t n, const int32_t *priorities);
int32_t cfx_lane_change_poll(cfx_engine *e, int32_t capacity, int32_t *parent_vid, int32_t *n);

/* ---- Tiling one road network over several engines / GPUs -----------------------------------
 * An engine may be created on a SUB-network: the intersections one tile owns, their laneLinks, every lane ending
 * in them, plus the "ghost" lanes it feeds that end in a foreign tile.  Vehicles on ghost lanes are frozen proxies
 * of the owner's state.  After every cfx_step the caller performs ONE exchange:
 *   cfx_halo_export(e, send)   fills `send` (host memory, cfx_halo_layout::send_bytes) with
 *                              - for every ghost lane (this tile is upstream): the vehicles that entered it this step
 *                                (migrants), and keeps only the last of them as the lane's proxy;
 *                              - for every import lane (this tile is downstream): the record of the lane's tail;
 *   ... the caller moves each neighbour's slice to that neighbour (RCCL / host copy) ...
 *   cfx_halo_import(e, recv)   appends received migrants to the import lanes and refreshes the proxies of ghost
 *                              lanes that had no entrant of their own this step.
 * Block formats (little endian, offsets are byte offsets into the send / recv buffers):
 *   migrant block (CFX_HALO_MIG_BYTES): int32 count, int32 pad, then CFX_HALO_MAX_MIGRANTS records
 *       {int32 vid, int32 route_pos, int32 prev_lanelink (global id), int32 pad, double dis, double speed}
 *   tail block (CFX_HALO_TAIL_BYTES):   {int32 vid (-1: lane empty), int32 prev_lanelink (global id or -1),
 *                                        double dis, double speed}
 * cfx_load_state on a tile (Archive::resume, archive.cpp:73-126, for one tile of a network-wide archive): the running
 * vehicles of the drivables the tile owns; for every ghost lane at most ONE vehicle, the lane's tail — it becomes the proxy
 * (not counted as running here, never stepped); r_prev_drivable of a vehicle that came from another tile's laneLink as
 * -(global laneLink id + 2), as migrants carry it; waiting buffers of owned AND ghost lanes (a ghost lane mirrors its
 * owner's queue); finished_vehicle_count / cumulative_travel_time / vehicle_steps on one tile of the job only. */
#define CFX_HALO_MAX_MIGRANTS 8
#define CFX_HALO_MIG_BYTES (8 + CFX_HALO_MAX_MIGRANTS * 32)
#define CFX_HALO_TAIL_BYTES 24
typedef struct cfx_halo_layout {
    int32_t n_ghost;                /* ghost lanes (local lane ids), this tile upstream */
    const int32_t *ghost_lane;
    const int32_t *ghost_send_off;  /* migrant block in the send buffer */
    const int32_t *ghost_recv_off;  /* tail block in the recv buffer */
    int32_t n_import;               /* owned lanes fed by a foreign tile */
    const int32_t *import_lane;
    const int32_t *import_recv_off; /* migrant block in the recv buffer */
    const int32_t *import_send_off; /* tail block in the send buffer */
    int32_t send_bytes, recv_bytes;
    int32_t n_global_lanelinks;     /* size of the two maps below */
    const int32_t *lanelink_global; /* [n_lanelinks of this engine] local -> global laneLink id */
    const int32_t *lanelink_local;  /* [n_global_lanelinks] global -> local laneLink id or -1 */
} cfx_halo_layout;
int32_t cfx_halo_config(cfx_engine *e, const cfx_halo_layout *layout);
int32_t cfx_halo_export(cfx_engine *e, void *send_host);      /* NULL: see cfx_halo_device_buffers */
int32_t cfx_halo_import(cfx_engine *e, const void *recv_host);

/* Device-initiated exchange (no host round trip).  Every directed neighbour message gets a MAILBOX in host memory that
 * both engines can reach (the caller maps it into both processes, e.g. POSIX shared memory; the HIP engine registers
 * it with the device): a 128-byte header whose first 8 bytes are the epoch flag, then two message buffers used
 * alternately (a sender is never more than one step ahead of its receiver, because its own next import needs the
 * receiver's next export).  After cfx_halo_attach the per-step exchange is
 *     cfx_halo_post(e)   export straight into the peers' mailboxes, then publish the step's epoch (system-scope release)
 *     cfx_halo_wait(e)   wait until every peer has published this epoch (system-scope acquire), then import
 * both asynchronous on the engine's stream for the HIP engine (the waiting is done by the import kernel, bounded), so a
 * step never synchronises with the host; CPU implementations block in cfx_halo_wait.  Call post on every local engine
 * before wait on any.  Epochs grow monotonically over cfx_reset, so mailboxes are never cleared. */
#define CFX_HALO_MAILBOX_HEADER 128
#define CFX_HALO_MAILBOX_BYTES(message_bytes) (CFX_HALO_MAILBOX_HEADER + 2 * (size_t) (message_bytes))
#define CFX_HALO_MAX_PEERS 16
typedef struct cfx_halo_peer {
    int32_t send_off, send_bytes; /* this peer's slice of the send layout of cfx_halo_config */
    int32_t recv_off, recv_bytes; /* ... and of the recv layout */
    void *send_mailbox;           /* CFX_HALO_MAILBOX_BYTES(send_bytes), written by this engine */
    void *recv_mailbox;           /* CFX_HALO_MAILBOX_BYTES(recv_bytes), written by the peer */
    int32_t device_memory;        /* 0: host memory both processes map (registered with the device by the engine);
                                   * 1: device pointers from cfx_halo_mailbox_alloc / _open — the mailbox lives in the
                                   *    RECEIVER's HBM and the sender's export kernel writes it over xGMI */
    int32_t reserved;
} cfx_halo_peer;

/* Mailboxes in device memory.  The receiver of a message owns its mailbox:
 *   cfx_halo_mailbox_alloc(e, message_bytes, &ptr, handle)  zeroed device memory on e's GPU for one incoming message
 *                              (CFX_HALO_MAILBOX_BYTES(message_bytes)), and a handle another PROCESS can open it with;
 *   cfx_halo_mailbox_open(e, handle, &ptr)                  in the sender's process: the peer's mailbox as a pointer e's GPU
 *                              can write through (hipIpcOpenMemHandle; peer HBM over xGMI between two GPUs of a node).
 * Tiles of ONE process pass `ptr` itself (the engine enables peer access between their GPUs in cfx_halo_attach).
 * CFX_ERR_STATE: this implementation / platform cannot do it — fall back to host-memory mailboxes. */
#define CFX_IPC_HANDLE_BYTES 64
int32_t cfx_halo_mailbox_alloc(cfx_engine *e, int32_t message_bytes, void **device_ptr, uint8_t handle[CFX_IPC_HANDLE_BYTES]);
int32_t cfx_halo_mailbox_open(cfx_engine *e, const uint8_t handle[CFX_IPC_HANDLE_BYTES], void **device_ptr);
/* 1: every mailbox cfx_halo_mailbox_alloc has handed out so far is fine-grained device memory (a kernel on ANOTHER GPU sees
 * the sender's stores while both kernels run); 0: some are plain allocations, because the platform would not export
 * fine-grained memory — good between processes that share one GPU, not guaranteed across two: the caller should then use the
 * host-memory mailboxes unless all tiles sit on one device. */
int32_t cfx_halo_mailbox_fine_grained(cfx_engine *e);
/* The PHYSICAL device the engine runs on, as a NUL-terminated string that is equal for two engines exactly if they share
 * a device whatever each process's visible-device numbering is (HIP: the PCI bus id, e.g. "0000:05:00.0"; a CPU
 * implementation: "cpu").  A caller that is offered plain (coarse-grained) device mailboxes compares it over all ranks. */
int32_t cfx_device_identity(cfx_engine *e, char *buf, int32_t capacity);
/* Free and total memory of that device in bytes (hipMemGetInfo; a CPU implementation: 0, 0) — what a long run is checked
 * against: a step of an ordinary run allocates nothing (tests/test_steady_state.py). */
int32_t cfx_device_memory(cfx_engine *e, int64_t *free_bytes, int64_t *total_bytes);
/* The staged exchange with the messages left in device memory (for a device-to-device transport such as RCCL send / recv
 * on these very buffers): cfx_halo_export(e, NULL) then writes the send buffer only on the device, cfx_halo_import(e, NULL)
 * reads the recv buffer from the device.  Both buffers are fixed for the life of the engine. */
int32_t cfx_halo_device_buffers(cfx_engine *e, void **send_dev, void **recv_dev);
int32_t cfx_halo_attach(cfx_engine *e, int32_t n_peers, const cfx_halo_peer *peers);
int32_t cfx_halo_post(cfx_engine *e);
int32_t cfx_halo_wait(cfx_engine *e);
/* spawn records whose lane is not part of this engine's sub-network carry lane = -1: only the per-vehicle
 * static table is filled (every tile knows every vehicle, so migrants need no static payload). */

/* Optional per-kernel timing with HIP events recorded on the engine's own stream (bench.py roofline).
 * Kernel ids are dense 0..cfx_profile_kernel_count()-1; cfx_profile_read() synchronises, adds the
 * elapsed time of every bracketed launch since the last read into total_ms[] / launches[] and clears. */
int32_t cfx_profile_kernel_count(void);
const char *cfx_profile_kernel_name(int32_t k);
int32_t cfx_profile_enable(cfx_engine *e, int32_t on);
int32_t cfx_profile_read(cfx_engine *e, double *total_ms, int64_t *launches);
/* The symbol of the kernel the engine launched LAST in timing slot k (the slots are roles — "k_action" is the car-following
 * launch whatever its organisation; this names the one that ran: "kr_action<256>", "kl_action", "kd_action", ...).  "" before
 * the first launch in that slot, and from CPU implementations. */
const char *cfx_profile_kernel_symbol(cfx_engine *e, int32_t k);

/* Where the HOST's time inside cfx_step went (never part of a result): every cfx_step call is timed with the host's steady
 * clock; a call that had to wait for the device or allocate says why.  `worst_*` describe the slowest call since the last
 * cfx_get_host_stats(e, out, 1) (reset = 1 clears everything but the *_total counters). */
#define CFX_STALL_TABLES 1       /* new templates / routes were uploaded: the stream was drained first (cfx_add_*) */
#define CFX_STALL_RING_REGROW 2  /* ring layout: the rings were rebuilt with doubled capacities (gather, drain, reallocate) */
#define CFX_STALL_SLOT_GROW 4    /* dense layout: the slot arrays grew (drains) */
#define CFX_STALL_VID_GROW 8     /* the per-vehicle tables grew (allocation only; the copy is ordered on the stream) */
#define CFX_STALL_SCALARS 16     /* the scalars were read back to decide something (overflow report, capacity bound) */
#define CFX_STALL_STAGE_GROW 32  /* the spawn staging buffers grew (drains) */
#define CFX_STALL_LIST_GROW 64   /* the step's vehicle list grew (allocation only) */
typedef struct cfx_host_stats {
    int64_t step_calls;           /* cfx_step calls since the last clearing read */
    double step_call_us_sum;      /* their host time */
    double worst_step_call_us;    /* the slowest of them ... */
    int64_t worst_step_call_at;   /* ... the engine step it submitted ... */
    int32_t worst_step_call_cause;/* ... and the CFX_STALL_* bits raised inside it (0: nothing of the above — the time went into
                                   * the HIP runtime's launch path, e.g. a full queue) */
    int32_t calls_over_1ms;       /* calls that took more than a millisecond */
    int64_t ring_regrows_total;   /* since the engine was created */
    int64_t table_grows_total;    /* vid-table + slot-array + list growths since the engine was created */
    /* the slowest cfx_get_vehicle_status call since the last clearing read (the spawner's priority-collision query: the one
     * call a free-running host makes that waits for the device), split into: launching a pending commit, enqueueing the copy,
     * waiting for the stream */
    double worst_status_query_us, worst_status_query_settle_us, worst_status_query_copy_us, worst_status_query_wait_us;
    int64_t status_queries;
} cfx_host_stats;
int32_t cfx_get_host_stats(cfx_engine *e, cfx_host_stats *out, int32_t reset);
/* Measurement aid: keeps the device busy with plain arithmetic for about `microseconds` on the engine's stream (returns at
 * once; the engine's next kernels queue behind it).  A benchmark calls it right before its warm-up steps so that a short
 * timed region is not measured on clocks that are still ramping up after host-only work.  Touches no engine state. */
int32_t cfx_device_spin(cfx_engine *e, int64_t microseconds);

/* ---- Observations and signals in device memory (an RL policy on the same GPU, e.g. torch tensors).  OPTIONAL entry points:
 * an implementation without device memory (the CPU twin) does not export them, so they are declared as the types of the
 * symbols, and a host resolves them with dlsym without requiring them (a NULL result: fall back to the calls above).
 * Nothing below waits for the device.  Stream order: the caller names ITS stream (a hipStream_t of the engine's HIP runtime;
 * NULL = that runtime's null stream).  The engine's stream waits for everything enqueued on the caller's stream before the
 * call, and the caller's stream waits for the engine's use of the buffer: each an event recorded on one stream and a
 * hipStreamWaitEvent on the other.  A buffer may therefore be freed, reused or overwritten by work enqueued on the caller's
 * stream after the call (a stream-ordered allocator such as torch's needs nothing more).  Every buffer must be device
 * memory of the engine's device (checked with hipPointerGetAttributes: CFX_ERR_INVALID otherwise).
 *   "cfx_stream_handle"         the engine's stream (hipStream_t) and its HIP device ordinal.
 *   "cfx_observe_device"        counts[n_lanes] (as cfx_get_lane_counts) and waiting[n_lanes] (as cfx_get_lane_waiting_counts),
 *                               either may be NULL, written by one kernel on the engine's stream after everything enqueued on
 *                               it (every cfx_step / set call made before); work enqueued on consumer_stream afterwards sees them.
 *                               The same call as "cfx_observe_lanes_device" below with speed_sum and bins NULL.
 *   "cfx_set_tl_phases_device"  phases[n], n == n_inters: cfx_set_tl_phases of every intersection, read after everything
 *                               enqueued on producer_stream before the call.  -1 keeps an intersection's phase, entries of
 *                               virtual intersections are ignored; any other entry outside [0, its phase count) rejects the
 *                               WHOLE call (nothing is applied) and the first such entry is recorded for "cfx_device_error".
 *   "cfx_device_error"          non-blocking read of that record: 1 and *inter / *phase (the record is then cleared), or 0.  It
 *                               shows what the completed kernels recorded: read it after a call that synchronised.
 * Calls that still wait for the device: the first observation on the ring layout (the rings are built) and table growth
 * (templates / routes added since the last step), as for cfx_step. */
typedef int32_t (*cfx_stream_handle_fn)(cfx_engine *e, void **stream, int32_t *device);
typedef int32_t (*cfx_observe_device_fn)(cfx_engine *e, int32_t *counts, int32_t *waiting, void *consumer_stream);
typedef int32_t (*cfx_set_tl_phases_device_fn)(cfx_engine *e, const int32_t *phases, int32_t n, void *producer_stream);
typedef int32_t (*cfx_device_error_fn)(cfx_engine *e, int32_t *inter, int32_t *phase);

/* ---- Per-lane speed and position features (OPTIONAL entry points, as above).  The population of lane l is the vehicles on it,
 * front to back, as cfx_get_lane_counts counts them (lane-change shadows included; vehicles on laneLinks belong to no lane).
 *   speed_sum[l]     double: 0.0 + v0 + v1 + ... summed front to back (Lane::updateHistory's curSpeedSum)
 *   bins[l * n + b]  int32: vehicles with edges[row, b] <= dis < edges[row, b + 1], every bin on its own (an inverted or a NaN
 *                    edge counts nothing); 1 <= n_bins <= 32.  per_lane_edges = 0: edges[n_bins + 1], the same for every lane;
 *                    1: edges[lanes per environment][n_bins + 1], row l % (n_lanes / n_envs) for lane l (cfx_config::n_envs)
 *   "cfx_observe_lanes_device"  counts / waiting (as cfx_observe_device), speed_sum and bins in device memory, any of them NULL
 *                               (at least one given; bins needs edges, in device memory too), written by ONE kernel on the
 *                               engine's stream, ordered against consumer_stream as cfx_observe_device.
 *   "cfx_get_lane_features"     speed_sum and / or bins into host memory, edges read from host memory; synchronous (engine-owned
 *                               device scratch, kept between calls; only [n_lanes] / [n_lanes * n_bins] is copied back). */
typedef int32_t (*cfx_observe_lanes_device_fn)(cfx_engine *e, int32_t *counts, int32_t *waiting, double *speed_sum, int32_t *bins,
                                               const double *edges, int32_t n_bins, int32_t per_lane_edges, void *consumer_stream);
typedef int32_t (*cfx_get_lane_features_fn)(cfx_engine *e, double *speed_sum, int32_t *bins, const double *edges, int32_t n_bins,
                                            int32_t per_lane_edges);
#define CFX_MAX_LANE_BINS 32
#define CFX_MAX_LANE_FRONT 64

/* ---- Every per-lane observation through one descriptor, the first vehicles from the front among them (OPTIONAL entry points,
 * as above).  v(l, k) is lane l's k-th vehicle from the front (the one closest to the lane's end first, the order of
 * cfx_get_vehicles inside a drivable), n(l) = counts[l]; rows of n_front slots, 1 <= n_front <= 64:
 *   front_distance[l * n_front + k]       double: dis of v(l, k), a copy                             padding -1.0
 *   front_speed[...]                      double: speed of v(l, k), a copy                           padding 0.0
 *   front_lane_steps[...]                 int32: s - since(v(l, k)) of the lane-flow tracker below   padding 0
 *   front_waiting_steps[...]              int32: wait(v(l, k)) of the tracker                        padding 0
 * A slot is real exactly if k < n(l); slots k >= n(l) hold the padding (-1.0 is a convenience: counts decides).  Every
 * element of a given output is written.  The two tracker columns need the tracker on ("cfx_lane_flow_enable"; CFX_ERR_STATE otherwise,
 * so never with lane change or on a tile) and show the tracker as of its last tick, s = the step counter then; a
 * vehicle whose record is not {this lane, that tick} reports 0, 0 — what a baseline would give it, so a baseline that is
 * still due (cfx_reset, cfx_load_state) reads as if taken.  Reading changes nothing in the tracker.
 * The descriptor: the caller sets struct_size = sizeof(cfx_lane_obs) and zeroes what it does not use; members behind
 * struct_size read as zero (a library newer than its caller) and a library that knows fewer members than struct_size names
 * rejects the call.  counts / waiting / speed_sum / bins / edges / n_bins / per_lane_edges are cfx_observe_lanes_device's.
 *   "cfx_observe_lane_obs_device"  every pointer device memory (edges too), any output NULL (at least one given), written by
 *                               ONE kernel on the engine's stream, ordered against consumer_stream as cfx_observe_device.  With
 *                               front outputs alone a lane's walk ends behind its first n_front vehicles.
 *   "cfx_get_lane_obs"          the same outputs into host memory, edges read from host memory; synchronous (engine-owned
 *                               device scratch, kept between calls).
 * "cfx_observe_lanes_device", "cfx_observe_device" and "cfx_get_lane_features" are these two calls with the front outputs NULL. */
typedef struct cfx_lane_obs {
    int32_t struct_size;
    int32_t n_bins, per_lane_edges;
    int32_t n_front;             /* slots per lane of the four front outputs (0 allowed when none is given) */
    int32_t *counts, *waiting;
    double *speed_sum;
    int32_t *bins;
    const double *edges;
    double *front_distance, *front_speed;
    int32_t *front_lane_steps, *front_waiting_steps;
} cfx_lane_obs;
typedef int32_t (*cfx_observe_lane_obs_device_fn)(cfx_engine *e, const cfx_lane_obs *obs, void *consumer_stream);
typedef int32_t (*cfx_get_lane_obs_fn)(cfx_engine *e, const cfx_lane_obs *obs);

/* ---- Per-vehicle observations in device memory (an OPTIONAL entry point, as above): every running vehicle, those on laneLinks
 * included, as rows in CSR form.  D = (n_lanes + n_lanelinks) / n_envs drivables per environment, numbered lanes first
 * (0 .. lanes per environment - 1), then laneLinks; the rows are ordered by environment, then by that number, then front to
 * back inside a drivable (one environment: the order of cfx_get_vehicles).
 *   start[r * (D + 1) + d]  int32: the row of the first vehicle of drivable d of environment r; entry D of a row is one past
 *                           the environment's last vehicle (= entry 0 of the next row).  The true offsets whatever n_rows is.
 *   count[0]                int32: the number of running vehicles
 *   row outputs [n_rows]    vehicle  int32: the vehicle number (cfx_spawn::vid)                                  padding -1
 *                           drivable int32: in [0, D), within the environment                                    padding -1
 *                           env      int32                                                                        padding -1
 *                           distance double: dis, a copy                                                          padding -1.0
 *                           speed    double: a copy                                                               padding 0.0
 *                           leader   int32: vehicle number of the leader as cfx_get_vehicles' leader_vid, -1 none padding -1
 *                           gap      double: cfx_get_vehicles' gap where leader >= 0, 0.0 where it is -1           padding 0.0
 * Row i < min(count, n_rows) is vehicle i, rows from count to n_rows hold the padding: every element of a given output is
 * written, nothing beyond n_rows.  Any pointer may be NULL (at least one of start, count or - with n_rows > 0 - a row output
 * given); all device memory.  The descriptor's struct_size as cfx_lane_obs's.  Two kernels on the engine's stream, ordered
 * against consumer_stream as cfx_observe_device; the call never waits for the device (the first call allocates a few KB).
 * CFX_ERR_STATE with lane change (shadows) and on a tile.
 * The POSE row outputs (members behind gap: a caller whose struct_size ends before them gives none), all double [n_rows]:
 *                           x, y          Vehicle::getPoint without its lane-change branch: getPointByDistance over the
 *                                         drivable's polyline at the row's distance (clamped to [0, the polyline's length]) padding NaN
 *                           dir_x, dir_y  Drivable::getDirectionByDistance: the unit vector of the segment the distance
 *                                         falls on (the last one beyond the end)                                    padding 0.0
 *                           length, width the len and width of the vehicle's template                               padding 0.0
 * The values are the reference's doubles to the bit (a last segment of length zero gives a NaN direction at and beyond it).
 * They need the polylines: CFX_ERR_STATE, with a cfx_last_error that says so, when one of the six is given before
 * cfx_set_drivable_geometry was called.  A call that gives none of them launches the kernels it always did. */
typedef struct cfx_vehicle_rows {
    int32_t struct_size;
    int32_t n_rows;              /* elements of every row output, >= 0 */
    int32_t *start, *count;
    int32_t *vehicle, *drivable, *env;
    double *distance, *speed;
    int32_t *leader;
    double *gap;
    double *x, *y, *dir_x, *dir_y, *length, *width;
} cfx_vehicle_rows;
typedef int32_t (*cfx_observe_vehicles_device_fn)(cfx_engine *e, const cfx_vehicle_rows *rows, void *consumer_stream);

/* ---- The polylines of the drivables (an OPTIONAL entry point, as above), which the pose outputs of
 * cfx_observe_vehicles_device walk.  Host arrays for the D drivables of ONE environment, numbered as that call's drivable
 * column (lanes first, then laneLinks): drivable d has the points point_start[d] .. point_start[d + 1] - 1, at least two,
 * point p is (xy[2 * p], xy[2 * p + 1]); point_start[0] == 0, point_start[D] == n_points.  The environments of a batched
 * engine share the one table.  Synchronous; the arrays are not read after the call.  The geometry belongs to the engine as
 * the network does: cfx_reset, cfx_load_state, a checkpoint restore and whatever else moves vehicles leave it alone; a
 * second call replaces it.  The descriptor's struct_size as cfx_lane_obs's.  CFX_ERR_INVALID for arrays that are not such a
 * table, CFX_ERR_STATE on a tile. */
typedef struct cfx_drivable_geometry {
    int32_t struct_size;
    int32_t n_drivables;         /* D = (n_lanes + n_lanelinks) / n_envs */
    int32_t n_points;            /* P */
    const int32_t *point_start;  /* [D + 1] */
    const double *xy;            /* [2 * P] */
} cfx_drivable_geometry;
typedef int32_t (*cfx_set_drivable_geometry_fn)(cfx_engine *e, const cfx_drivable_geometry *geometry);

/* ---- Speed commands for many vehicles at once (OPTIONAL entry points, as above; both or none): Vehicle::setCustomSpeed, as
 * cfx_set_vehicle_speed, for n rows {vehicle[i], speed[i]}, n >= 0.  The vehicle numbers are cfx_observe_vehicles_device's.
 *   vehicle[i] == -1 (that call's padding) or speed[i] NaN      the row is skipped and not counted
 *   vehicle[i] < -1, vehicle[i] >= the numbers issued when the call is made (the vehicles the next cfx_step will create are not
 *   among them: cfx_set_vehicle_speed serves those), or a finished vehicle      the row is skipped and counted in ignored[0]
 *   a waiting or running vehicle      the speed - any other double, untouched - holds for the vehicle's next step
 * A vehicle named by several rows of the second and third kind takes the row with the highest index.  Calls take effect in
 * the order they are made, cfx_set_vehicle_speed among them.  ignored (int32[1]) may be NULL.
 * _device: vehicle, speed and ignored are device memory; two kernels on the engine's stream (three on the dense layout: one
 * pass over the slots for the whole call), ordered against producer_stream as cfx_set_tl_phases_device; the call never waits
 * for the device (it allocates 4 bytes per vehicle number when the numbers have outgrown its scratch).  The host form reads
 * host arrays, runs the same kernels on staging the engine keeps, and waits for the count.
 * CFX_ERR_STATE with lane change (the numbers are cfx_observe_vehicles_device's) and on a tile. */
typedef int32_t (*cfx_set_vehicle_speeds_device_fn)(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n,
                                                    int32_t *ignored, void *producer_stream);
typedef int32_t (*cfx_set_vehicle_speeds_fn)(cfx_engine *e, const int32_t *vehicle, const double *speed, int32_t n, int32_t *ignored);
/* OPTIONAL, beside the two above: the custom speeds that vehicles still WAITING in an entry buffer hold, whichever call set
 * them (cfx_set_vehicle_speed or the two above) - what cfx_get_custom_speeds does not list and cfx_load_state does not take.
 * Writes n[0] pairs {vid[i], speed[i]} in ascending vid; CFX_ERR_CAPACITY when there are more than `capacity`.  Host memory;
 * waits for the device.  A host that renumbers the vehicles (a load of its own state) reads them first and gives them back
 * with cfx_set_vehicle_speed: the device calls never tell it which of their rows named a waiting vehicle. */
typedef int32_t (*cfx_get_waiting_custom_speeds_fn)(cfx_engine *e, int32_t capacity, int32_t *vid, double *speed, int32_t *n);

/* ---- Route changes for many vehicles at once, and the routes the vehicles hold (OPTIONAL entry points, as above; all four or
 * none): Router::setRoute for n rows {vehicle[i], route[i]}, n >= 0.  The vehicle numbers are cfx_observe_vehicles_device's.
 * route[i] is a HANDLE: an index into the route tables of cfx_add_routes as ONE environment has them, [0, routes / n_envs).
 * With cfx_config::n_envs > 1 the vehicle's environment is that of its lane, and the route it gets is environment *
 * (routes / n_envs) + handle: a handle is never read across environments.  status[i] (int32[n], may be NULL) is decided by
 * the first of these that applies:
 *    0   skipped: vehicle[i] == -1 (that call's padding) or route[i] == -1 (leave alone)
 *   -1   no such running vehicle: a number outside [0, issued), a finished vehicle, or one still in its lane's entry buffer
 *   -2   no such handle
 *   -3   superseded: a later row passes the three checks above and names the same vehicle
 *   -4   the vehicle is inside an intersection, on a laneLink (Router::setRoute, router.cpp:246)
 *   -5   the vehicle's road does not occur on the route before the route's last road (a remaining route of one road is
 *        refused, router.cpp:239)
 *   -6   the vehicle's lane has no laneLink towards the route's next road (Router::onValidLane, router.h:66-68) — unless
 *        the vehicle's road is also the route's LAST road (a route that comes back to it): onValidLane holds there, the
 *        row is applied with no next drivable and the vehicle ends its trip on this lane
 *    1   applied: the vehicle holds the route with its cursor on the FIRST position p of its road, its next drivable and its
 *        last-road flag are those of (route, p); cfx_get_vehicle then answers route and route_pos = p
 * Of the rows for one vehicle that pass -1 and -2 only the LAST counts, whatever its verdict: this is not "the last valid
 * row wins" (a vehicle whose last row is refused keeps its old route, its earlier rows read -3).  ignored (int32[1], may be
 * NULL) receives the number of rows with a negative status.  Nothing outside [0, n) of status is written.  Calls take effect
 * in the order they are made, cfx_set_vehicle_route among them.
 * _device: every pointer is device memory; two kernels over the rows on the engine's stream (ring layout), or two over the
 * rows and one pass over the slots (dense layout), ordered against producer_stream as cfx_set_tl_phases_device; the call
 * never waits for the device (it uploads routes added since, and allocates 4 bytes per vehicle number when the numbers have
 * outgrown its scratch).  The host form reads and fills host arrays through the engine's staging and waits.
 * cfx_get_vehicle_routes[_device] writes route_out[i] = the handle vehicle[i] holds (waiting vehicles included), or -1 for
 * vehicle[i] == -1, a number that was not issued and a finished vehicle; one kernel.  The host form takes vehicle == NULL
 * for the numbers 0 .. n-1.
 * CFX_ERR_STATE with lane change (the numbers are cfx_observe_vehicles_device's) and on a tile. */
typedef int32_t (*cfx_set_vehicle_routes_device_fn)(cfx_engine *e, const int32_t *vehicle, const int32_t *route, int32_t n,
                                                    int32_t *status, int32_t *ignored, void *producer_stream);
typedef int32_t (*cfx_set_vehicle_routes_fn)(cfx_engine *e, const int32_t *vehicle, const int32_t *route, int32_t n, int32_t *status,
                                             int32_t *ignored);
typedef int32_t (*cfx_get_vehicle_routes_device_fn)(cfx_engine *e, const int32_t *vehicle, int32_t n, int32_t *route_out,
                                                    void *consumer_stream);
typedef int32_t (*cfx_get_vehicle_routes_fn)(cfx_engine *e, const int32_t *vehicle, int32_t n, int32_t *route_out);

/* ---- Per-intersection movement and phase observations (OPTIONAL entry points, as above).  Intersection i (n_inters of them,
 * virtual ones included) has its roadLinks m < M_i = inter_n_roadlinks[i] ("movements", ll_roadlink) and its phases p < P_i
 * (inter_phase_start; 0 for a virtual intersection).  IN(i, m) / OUT(i, m) are the DISTINCT start / end lanes of the roadLink's
 * laneLinks.  Rows are padded to max_roadlinks = max M_i and max_phases = max P_i over the network; the caller passes both and
 * gets CFX_ERR_INVALID when they are not the network's.
 *   phase[i]                         int32: as cfx_get_tl_state
 *   remain[i]                        double: as cfx_get_tl_state, a copy
 *   in[i * max_roadlinks + m]        int32: sum of cfx_get_lane_counts over IN(i, m)
 *   in_waiting[...]                  int32: sum of cfx_get_lane_waiting_counts over IN(i, m)
 *   out[...]                         int32: sum of cfx_get_lane_counts over OUT(i, m)
 *   inside[...]                      int32: vehicles on the laneLinks of roadLink (i, m)
 *   phase_pressure[i * max_phases + p]  int32: sum of in - out over the roadLinks m with phase_avail[i][p][m]
 * Padding: 0 in the four movement outputs for m >= M_i; INT32_MIN in phase_pressure for p >= P_i (a phase that serves no roadLink
 * has 0).  Every element of a given output is written.
 *   "cfx_observe_intersections_device"  any of the seven NULL (at least one given), all in device memory, written by ONE kernel
 *                               on the engine's stream, ordered against consumer_stream as cfx_observe_device.  The first call
 *                               builds and uploads the roadLink index (it waits for the device once).
 *   "cfx_get_intersection_features"     the same outputs into host memory; synchronous (engine-owned device scratch, kept
 *                               between calls). */
typedef int32_t (*cfx_observe_intersections_device_fn)(cfx_engine *e, int32_t *phase, double *remain, int32_t *in, int32_t *in_waiting,
                                                       int32_t *out, int32_t *inside, int32_t *phase_pressure, int32_t max_roadlinks,
                                                       int32_t max_phases, void *consumer_stream);
typedef int32_t (*cfx_get_intersection_features_fn)(cfx_engine *e, int32_t *phase, double *remain, int32_t *in, int32_t *in_waiting,
                                                    int32_t *out, int32_t *inside, int32_t *phase_pressure, int32_t max_roadlinks,
                                                    int32_t max_phases);

/* ---- Per-lane flow and waiting-time statistics accumulated across steps (OPTIONAL entry points, as above; not with lane
 * change, not on a tile: CFX_ERR_STATE).  Off by default: nothing is allocated or launched.  While it is on, every cfx_step ends
 * with one TICK on the state the step left (s = the step counter after it; P(l) = the vehicles cfx_get_lane_counts counts on
 * lane l, P'(l) = the same at the previous tick or the baseline):
 *   v in P(l) \ P'(l):  entered[l] += 1, since(v) = s, wait(v) = 0
 *   v in P'(l) \ P(l):  left[l] += 1, left_steps[l] += s - since(v), left_waiting_steps[l] += wait(v)
 *   v in P(l) with speed < 0.1 (the criterion of cfx_get_lane_waiting_counts):  wait(v) += 1
 * A BASELINE (enabling, cfx_reset, cfx_load_state) gives every vehicle then on a lane since = s, wait = 0 without counting it as
 * entered, and zeroes the accumulators.  Outputs, [n_lanes] each: entered, left (int32), left_steps, left_waiting_steps (int64):
 * accumulated since the baseline or the last read with reset != 0; waiting_steps (int64) = sum of wait(v) over P(l) and
 * max_waiting_steps (int32) = their maximum (0 on an empty lane), both as of the last tick.
 *   "cfx_lane_flow_enable"         on != 0: allocate (16 bytes per vehicle number the tables hold, 48 per lane) and take a
 *                                  baseline; 0: free.  While it is on the ring layout launches every step's commit with the step.
 *   "cfx_observe_lane_flow_device" any of the six NULL (at least one given unless reset), all in device memory, copied by ONE
 *                                  kernel on the engine's stream, ordered against consumer_stream as cfx_observe_device; reset
 *                                  != 0 zeroes the four accumulators in that launch, after they were read.
 *   "cfx_get_lane_flow"            the same into host memory; synchronous.
 *   "cfx_lane_flow_get_state" / "cfx_lane_flow_set_state"  the tracker as it stands, for a host that renumbers the vehicles through
 *                                  cfx_load_state (which takes a baseline): records[4 v ..] = {lane, tick last seen on it, since,
 *                                  wait} of vehicle number v < n_vehicles (n_vehicles as cfx_load_state last set it plus the
 *                                  vehicles spawned since), lanes[n_lanes], and the tick counter.  set replaces all three and
 *                                  cancels a pending baseline.  Synchronous. */
typedef struct cfx_lane_flow_lane {
    int64_t since_sum;           /* sum of since(v) over the lane's vehicles at the last tick */
    int64_t waiting_steps;       /* sum of wait(v) over them */
    int64_t left_steps, left_waiting_steps;
    int32_t count;               /* vehicles on the lane at the last tick */
    int32_t entered, left;
    int32_t max_waiting_steps;
} cfx_lane_flow_lane;
typedef int32_t (*cfx_lane_flow_enable_fn)(cfx_engine *e, int32_t on);
typedef int32_t (*cfx_observe_lane_flow_device_fn)(cfx_engine *e, int32_t *entered, int32_t *left, int64_t *left_steps,
                                                   int64_t *left_waiting_steps, int64_t *waiting_steps, int32_t *max_waiting_steps,
                                                   int32_t reset, void *consumer_stream);
typedef int32_t (*cfx_get_lane_flow_fn)(cfx_engine *e, int32_t *entered, int32_t *left, int64_t *left_steps,
                                        int64_t *left_waiting_steps, int64_t *waiting_steps, int32_t *max_waiting_steps, int32_t reset);
typedef int32_t (*cfx_lane_flow_get_state_fn)(cfx_engine *e, int32_t *records, int32_t n_vehicles, cfx_lane_flow_lane *lanes,
                                              int32_t *tick);
typedef int32_t (*cfx_lane_flow_set_state_fn)(cfx_engine *e, const int32_t *records, int32_t n_vehicles,
                                              const cfx_lane_flow_lane *lanes, int32_t tick);

/* ---- Per-environment trip statistics and the average travel time accumulated across steps (OPTIONAL entry points, as above;
 * not with lane change, not on a tile: CFX_ERR_STATE).  Off by default: nothing is allocated or launched.  s = the step counter;
 * e(v) = llrint(enter_time(v) / interval) = the step at which vehicle v was created; r(v) = its environment (cfx_config::n_envs:
 * the first road of its route / (n_roads / n_envs); one environment otherwise).  While it is on, every cfx_step ends with one
 * TICK on the state the step left (s counts that step), over the status of every vehicle number (cfx_get_vehicle_status):
 *   v seen for the first time:                             entered[r] += 1
 *   v running now and not at the previous tick:            admitted[r] += 1, admitted_buffer_steps[r] += (s - 1) - e(v)
 *                                                          (the steps it sat in its lane's entry buffer)
 *   v finished now and not at the previous tick:           finished[r] += 1, finished_travel_steps[r] += (s - 1) - e(v)
 *                                                          (what cumulative_travel_time got for it, divided by interval)
 * and as of the last tick  in_system[r] = vehicles created and not finished,  buffered[r] = those of them still waiting,
 * in_system_travel_steps[r] = sum of s - e(v) over them,  average_travel_time[r] = (double) (finished_travel_steps +
 * in_system_travel_steps) * interval / (double) (finished + in_system), 0.0 without vehicles — Engine::getAverageTravelTime
 * per environment, while tracking has been on since cfx_create / cfx_reset.  The accumulators only ever grow: a window is the
 * difference of two reads.  A BASELINE (enabling, cfx_reset, cfx_load_state) zeroes the five accumulators and takes the
 * vehicles alive then into in_system / buffered / in_system_travel_steps with their true e(v), without counting them as
 * entered; they count as admitted or finished when that happens.
 * Outputs, [max(n_envs, 1)] each: counts int32, step sums int64, average_travel_time double.
 *   "cfx_trip_stats_enable"         on != 0: allocate (1 byte per vehicle number the tables hold, 56 per environment) and take a
 *                                   baseline; 0: free.  While it is on the ring layout launches every step's commit with the step.
 *   "cfx_observe_trip_stats_device" any of the nine NULL (at least one given), all in device memory, written by ONE kernel on
 *                                   the engine's stream, ordered against consumer_stream as cfx_observe_device.
 *   "cfx_get_trip_stats"            the same into host memory; synchronous.
 *   "cfx_trip_stats_get_state" / "cfx_trip_stats_set_state"  the per-environment records as they stand, for a host that renumbers
 *                                   the vehicles through cfx_load_state (which takes a baseline) without changing which are alive:
 *                                   set replaces the records after that load; the per-vehicle part is the one the load's
 *                                   baseline built.  Synchronous. */
typedef struct cfx_trip_stats_env {
    int64_t admitted_buffer_steps, finished_travel_steps;
    int64_t enter_sum_created;   /* sum of e(v) over the vehicles alive at the baseline and those seen since */
    int64_t enter_sum_finished;  /* ... over those that finished since the baseline */
    int32_t entered, admitted, finished;
    int32_t base_in_system, base_buffered;  /* alive / waiting at the baseline */
    int32_t reserved;
} cfx_trip_stats_env;
typedef struct cfx_trip_stats_out {
    int32_t *entered, *admitted;
    int64_t *admitted_buffer_steps;
    int32_t *finished;
    int64_t *finished_travel_steps;
    int32_t *in_system, *buffered;
    int64_t *in_system_travel_steps;
    double *average_travel_time;
} cfx_trip_stats_out;
typedef int32_t (*cfx_trip_stats_enable_fn)(cfx_engine *e, int32_t on);
typedef int32_t (*cfx_observe_trip_stats_device_fn)(cfx_engine *e, const cfx_trip_stats_out *out, void *consumer_stream);
typedef int32_t (*cfx_get_trip_stats_fn)(cfx_engine *e, const cfx_trip_stats_out *out);
typedef int32_t (*cfx_trip_stats_get_state_fn)(cfx_engine *e, cfx_trip_stats_env *envs, int32_t n_envs);
typedef int32_t (*cfx_trip_stats_set_state_fn)(cfx_engine *e, const cfx_trip_stats_env *envs, int32_t n_envs);

/* ---- The trip LOG: one row per finished vehicle, kept by the trip tracker (OPTIONAL entry points of their own, as above).  It
 * needs trip tracking on (CFX_ERR_STATE otherwise), so not with lane change and not on a tile; it is off by default and off
 * while only cfx_trip_stats_enable is on; turning trip tracking off frees it.  At the tick that ends step s every vehicle v
 * "finished now and not at the previous tick" (the event that does finished[r] += 1) is appended as one row, seven int32:
 *   env               r(v)
 *   vehicle           the vehicle number v had when it finished (after a host has renumbered the vehicles through
 *                     cfx_load_state + cfx_trip_log_set_state a number may be in use again: rows keep the old one)
 *   origin_road       first road of the route v held when it finished, as an index into ONE environment's roads (road index
 *                     modulo n_roads / n_envs).  cfx_set_vehicle_route replaces the route from the road the vehicle is on: the
 *                     origin of such a vehicle is the first road of the NEW route
 *   destination_road  last road of that route, same indexing
 *   enter_step        e(v)
 *   finish_step       s
 *   travel_steps      (s - 1) - e(v): exactly what finished_travel_steps received for v
 * Rows are in ascending finish_step; the order of the rows of ONE step is unspecified (it differs from run to run on a
 * device).  The capacity is fixed when the log is turned on: a row that does not fit is dropped and counted in `dropped`; the
 * accumulators of the trip statistics do not depend on the log.  A BASELINE (enabling trip tracking, cfx_reset, cfx_load_state)
 * empties the log and zeroes `dropped`; a baseline tick itself logs nothing, so vehicles that had finished before are no rows.
 *   "cfx_trip_log_enable"          capacity > 0: allocate, or replace by, an EMPTY log of that many rows (32 bytes each); 0: free.
 *                                  CFX_ERR_INVALID outside [0, 1 << 26].  The accumulators are not touched.
 *   "cfx_observe_trip_log_device"  any of the nine NULL (at least one given), all in device memory: the columns [capacity] each,
 *                                  count (rows held, at most capacity) and dropped one int32 each.  Rows at and behind count are
 *                                  written as -1: every element given has exactly one writer.  ONE kernel on the engine's stream,
 *                                  ordered against consumer_stream as cfx_observe_device.  reset != 0 empties the log and zeroes
 *                                  dropped behind that kernel, in stream order.  CFX_ERR_STATE while there is no log.
 *   "cfx_get_trip_log"             the same into host memory; synchronous.
 *   "cfx_trip_log_set_state"       replaces the log's content by n rows (the seven columns of `rows` in host memory, [n] each;
 *                                  its count / dropped are not read) and `dropped`, after a renumbering load as
 *                                  cfx_trip_stats_set_state; reading them out before is cfx_get_trip_log with reset = 0.
 *                                  CFX_ERR_INVALID for n beyond the capacity.  Synchronous. */
typedef struct cfx_trip_log_out {
    int32_t *count, *dropped;
    int32_t *env, *vehicle, *origin_road, *destination_road, *enter_step, *finish_step, *travel_steps;
} cfx_trip_log_out;
#define CFX_TRIP_LOG_MAX_CAPACITY (1 << 26)
typedef int32_t (*cfx_trip_log_enable_fn)(cfx_engine *e, int32_t capacity);
typedef int32_t (*cfx_observe_trip_log_device_fn)(cfx_engine *e, const cfx_trip_log_out *out, int32_t reset, void *consumer_stream);
typedef int32_t (*cfx_get_trip_log_fn)(cfx_engine *e, const cfx_trip_log_out *out, int32_t reset);
typedef int32_t (*cfx_trip_log_set_state_fn)(cfx_engine *e, const cfx_trip_log_out *rows, int32_t n, int32_t dropped);

/* ---- Per-movement (roadLink) throughput and delay statistics accumulated across steps (OPTIONAL entry points, as above; not with
 * lane change, not on a tile: CFX_ERR_STATE).  Off by default: nothing is allocated or launched.  Independent of the lane-flow
 * tracker: both on means two ticks and two records per vehicle.  s = the step counter after a step; D(v) = the drivable
 * vehicle v is on then (a lane l < n_lanes or laneLink k as n_lanes + k, the `drivable` column of cfx_get_vehicles; a vehicle
 * in an entry buffer is on nothing), D'(v) = the same at the previous tick or the baseline.  Every vehicle has one record
 * {drivable, tick last seen, since, wait}.  While it is on, every cfx_step ends with one TICK on the state the step left:
 *   1. D(v) = d != D'(v) = p.  Read off the record before it is overwritten with since(v) = s, wait(v) = 0:
 *        d laneLink k, p a lane:      entered[k] += 1, entered_lane_steps[k] += s - since_p(v),
 *                                     entered_lane_waiting_steps[k] += wait_p(v)
 *        d laneLink k, p not a lane:  entered[k] += 1 (p nothing or another laneLink: a lane shorter than one step's travel)
 *        d a lane, p another lane:    the vehicle crossed a whole laneLink inside the step.  k = the first laneLink of p's
 *                                     laneLink list (lane_ll order) whose end lane is d: the three additions of the first case
 *                                     and left[k] += 1 (nothing to left_steps / left_waiting_steps); without such a k, nothing
 *   2. v no longer on laneLink k:     left[k] += 1, left_steps[k] += s - since(v), left_waiting_steps[k] += wait(v)
 *   3. v on any drivable with speed < 0.1 (the criterion of cfx_get_lane_waiting_counts): wait(v) += 1, after rule 1
 * and as of the last tick waiting_steps[k] = sum of wait(v) over the vehicles on laneLink k, max_waiting_steps[k] = their
 * maximum (0 on an empty laneLink).  A BASELINE (enabling, cfx_reset, cfx_load_state) gives every vehicle then on a drivable
 * since = s, wait = 0 without counting it as entered, and zeroes the accumulators.
 * Outputs are per roadLink (i, m), rows of max_roadlinks as in cfx_observe_intersections_device, [n_inters * max_roadlinks]
 * each: the sum (max_waiting_steps: the maximum) over the roadLink's laneLinks; 0 for m >= M_i and in every row of a virtual
 * intersection.  Every element of a given output is written.  The descriptor follows the struct_size rules of cfx_lane_obs.
 *   "cfx_movement_flow_enable"         on != 0: allocate (16 bytes per vehicle number the tables hold, 88 per laneLink) and
 *                                      take a baseline; 0: free.  While it is on the ring layout launches every step's commit
 *                                      with the step.
 *   "cfx_observe_movement_flow_device" any of the eight NULL (at least one given unless reset), all in device memory, written by
 *                                      ONE kernel on the engine's stream, ordered against consumer_stream as
 *                                      cfx_observe_device; reset != 0 zeroes the six accumulators in that launch, after they
 *                                      were read.  The first call builds the roadLink index of cfx_observe_intersections_device.
 *   "cfx_get_movement_flow"            the same into host memory; synchronous.
 *   "cfx_movement_flow_get_state" / "cfx_movement_flow_set_state"  the tracker as it stands, for a host that renumbers the
 *                                      vehicles through cfx_load_state (which takes a baseline): records[4 v ..] of vehicle
 *                                      number v < n_vehicles, links[n_lanelinks] (what crossings of whole laneLinks added
 *                                      folded in), and the tick counter.  set replaces all three and cancels a pending
 *                                      baseline.  Synchronous. */
typedef struct cfx_movement_flow_link {
    int64_t since_sum;           /* sum of since(v) over the laneLink's vehicles at the last tick */
    int64_t waiting_steps;       /* sum of wait(v) over them */
    int64_t left_steps, left_waiting_steps;
    int64_t entered_lane_steps, entered_lane_waiting_steps;
    int32_t count;               /* vehicles on the laneLink at the last tick */
    int32_t entered, left;
    int32_t max_waiting_steps;
} cfx_movement_flow_link;
typedef struct cfx_movement_flow_out {
    int32_t struct_size;
    int32_t max_roadlinks;       /* the network's largest roadLink count (CFX_ERR_INVALID otherwise) */
    int32_t reset;
    int32_t reserved;
    int32_t *entered;
    int64_t *entered_lane_steps, *entered_lane_waiting_steps;
    int32_t *left;
    int64_t *left_steps, *left_waiting_steps;
    int64_t *waiting_steps;
    int32_t *max_waiting_steps;
} cfx_movement_flow_out;
typedef int32_t (*cfx_movement_flow_enable_fn)(cfx_engine *e, int32_t on);
typedef int32_t (*cfx_observe_movement_flow_device_fn)(cfx_engine *e, const cfx_movement_flow_out *out, void *consumer_stream);
typedef int32_t (*cfx_get_movement_flow_fn)(cfx_engine *e, const cfx_movement_flow_out *out);
typedef int32_t (*cfx_movement_flow_get_state_fn)(cfx_engine *e, int32_t *records, int32_t n_vehicles, cfx_movement_flow_link *links,
                                                  int32_t *tick);
typedef int32_t (*cfx_movement_flow_set_state_fn)(cfx_engine *e, const int32_t *records, int32_t n_vehicles,
                                                  const cfx_movement_flow_link *links, int32_t tick);

/* ---- Virtual loop detectors: passage counts, occupancy and speed over zones of lanes, accumulated across steps (OPTIONAL entry
 * points, as above; not with lane change, not on a tile: CFX_ERR_STATE).  Off by default: nothing is allocated or launched.  A
 * detector d = (l, start, end) is a zone of lane l in metres from the lane's start, on the scale of the `dis` column of
 * cfx_get_vehicles; it sees a vehicle's FRONT position only (vehicle length is ignored).  "In the zone": start <= dis(v) < end;
 * end may be +inf or beyond the lane's length (the zone then reaches to the lane's end).  Any number of detectors per lane, and
 * they may overlap; a lane without one costs nothing.  With cfx_config::n_envs > 1 the set is ONE environment's (l < n_lanes /
 * n_envs) and every environment gets it: n_envs * n records and outputs, environment-major.
 * While it is on, every cfx_step ends with one TICK on the state the step left.  on(l) = the vehicles on lane l, front to back
 * (the order of cfx_get_vehicles); dis'(v) = dis(v) at the previous tick if v was on l then.  Per detector:
 *   passed                 int32   += 1 for every v on l with dis(v) >= start that was not on l at the previous tick or had
 *                                  dis'(v) < start; += 1 for every v that was on l with dis'(v) < start and is on l no longer (it
 *                                  went over the rest of the lane in one step).  Kept as a difference: with U = the vehicles on l
 *                                  upstream of start (dis < start), passed += U' - U + entered(l), exact in integers because a
 *                                  vehicle on a lane never moves backwards and a lane is left at its front only
 *   occupied_steps         int32   += 1 if a vehicle is in the zone
 *   vehicle_steps          int64   += the vehicles in the zone
 *   waiting_vehicle_steps  int64   += those of them with speed < 0.1 (the criterion of cfx_get_lane_waiting_counts)
 *   speed_sum              double  acc = acc + t, t = the speeds of the zone's vehicles added front to back in one running
 *                                  double that starts at 0.0 (as the speed_sum of cfx_get_lane_obs adds a lane's)
 *   count                  int32   not accumulated: the vehicles in the zone as of the last tick
 * The first five accumulate since the baseline or the last read with reset != 0.  A BASELINE (enabling, defining again,
 * cfx_reset, cfx_load_state, cfx_checkpoint_restore) counts nothing, zeroes the accumulators and takes count and U as of now:
 * every vehicle then on a lane was "on it at the previous tick" with its current distance.
 *   "cfx_detectors_define"         lane[n], start[n], end[n], n >= 1.  Every entry is checked before anything changes: lane in
 *                                  [0, n_lanes / n_envs), start finite and >= 0, end > start, no NaN — CFX_ERR_INVALID otherwise,
 *                                  with the position in cfx_last_error.  While the tracker is off the set is only kept; while it
 *                                  is on the set replaces the one in force and a baseline is taken.
 *   "cfx_detectors_enable"         on != 0: allocate (16 bytes per vehicle number the tables hold, 64 per detector) and take a
 *                                  baseline (CFX_ERR_STATE before any cfx_detectors_define); 0: free, the set is forgotten.  While
 *                                  it is on the ring layout launches every step's commit with the step.
 *   "cfx_observe_detectors_device" any of the six NULL (at least one given unless reset), all in device memory, copied by ONE
 *                                  kernel on the engine's stream, ordered against consumer_stream as cfx_observe_device; reset
 *                                  != 0 zeroes the five accumulators in that launch, after they were read.
 *   "cfx_get_detectors"            the same into host memory; synchronous.
 *   "cfx_detectors_get_state" / "cfx_detectors_set_state"  the tracker as it stands, for a host that renumbers the vehicles through
 *                                  cfx_load_state (which takes a baseline): records[4 v ..] = {lane, tick last seen on it, 0, 0}
 *                                  of vehicle number v < n_vehicles, detectors[n_detectors] (all environments'), and the tick
 *                                  counter.  set replaces all three and cancels a pending baseline.  Synchronous. */
typedef struct cfx_detector {
    double start, end;           /* the zone */
    double speed_sum;
    int64_t vehicle_steps, waiting_vehicle_steps;
    int32_t lane;                /* of the engine: environment * (n_lanes / n_envs) + l */
    int32_t upstream;            /* U: vehicles on the lane with dis < start at the last tick */
    int32_t passed, occupied_steps;
    int32_t count;               /* vehicles in the zone at the last tick */
    int32_t reserved;
} cfx_detector;
typedef struct cfx_detectors_out {
    int32_t *passed, *occupied_steps;
    int64_t *vehicle_steps, *waiting_vehicle_steps;
    double *speed_sum;
    int32_t *count;
} cfx_detectors_out;
typedef int32_t (*cfx_detectors_define_fn)(cfx_engine *e, const int32_t *lane, const double *start, const double *end, int32_t n);
typedef int32_t (*cfx_detectors_enable_fn)(cfx_engine *e, int32_t on);
typedef int32_t (*cfx_observe_detectors_device_fn)(cfx_engine *e, const cfx_detectors_out *out, int32_t reset, void *consumer_stream);
typedef int32_t (*cfx_get_detectors_fn)(cfx_engine *e, const cfx_detectors_out *out, int32_t reset);
typedef int32_t (*cfx_detectors_get_state_fn)(cfx_engine *e, int32_t *records, int32_t n_vehicles, cfx_detector *detectors,
                                              int32_t n_detectors, int32_t *tick);
typedef int32_t (*cfx_detectors_set_state_fn)(cfx_engine *e, const int32_t *records, int32_t n_vehicles,
                                              const cfx_detector *detectors, int32_t n_detectors, int32_t tick);

/* ---- The fixed-time signal plan as engine state in device memory (OPTIONAL entry points, as above; not on a tile:
 * CFX_ERR_STATE).  The engine keeps two copies of cfx_net::phase_time: the durations IN FORCE, which TrafficLight::passTime of
 * every step and cfx_reset read, and the FILE's, as cfx_create got them.  Rows are padded to max_phases = max P_i as in
 * cfx_observe_intersections_device, and CFX_ERR_INVALID is returned when it is not the network's; n must be n_inters.
 *   durations[i * max_phases + p]  double: seconds of phase p of intersection i; NaN keeps the entry; entries p >= P_i and
 *                                  every row of a virtual intersection are ignored.  A new duration is read the next time the
 *                                  phase is entered (or by cfx_reset); the running phase keeps its remaining time
 *   phase[i]                       int32: -1 keeps, otherwise the current phase (as cfx_set_tl_phases, whatever rl_traffic_light
 *                                  is); the remaining time is not touched
 *   remain[i]                      double: seconds the current phase still has; NaN keeps
 * Any of the three may be NULL (at least one given).  The call is valid if, at every intersection that is not virtual: every
 * given duration is finite and >= 0; the sum over p < P_i of the durations in force AFTER the call is >= cfx_config::interval
 * (what bounds passTime's loop: a cycle of zero length would never leave it); phase is in [-1, P_i); remain is finite and >= 0.
 * One invalid entry rejects the WHOLE call: nothing is applied, and the first offender — lowest intersection; there durations
 * by p, then the sum, then phase, then remain — is recorded for "cfx_tl_plan_error".  cfx_load_state and cfx_reset leave
 * the durations in force alone (cfx_reset's remain is that of phase 0 in force).
 *   "cfx_set_tl_plan_device"             the three in device memory, validated and applied by ONE kernel on the engine's
 *                                        stream, read after everything enqueued on producer_stream (as cfx_set_tl_phases_device)
 *   "cfx_set_tl_plan"                    the same from host memory; synchronous, so cfx_tl_plan_error is current on return
 *   "cfx_get_tl_phase_durations_device"  out[n_inters * max_phases]: the durations in force, 0.0 for p >= P_i and at virtual
 *                                        intersections, every element written, ordered against consumer_stream
 *   "cfx_get_tl_phase_durations"         the same into host memory; synchronous
 *   "cfx_restore_tl_plan"                the file's durations are in force again (a copy on the engine's stream); phases and
 *                                        remaining times stay
 *   "cfx_tl_plan_error"                  non-blocking read of the record, as cfx_device_error: 1 and *what (CFX_TL_PLAN_*),
 *                                        *inter, *phase (the index p for CFX_TL_PLAN_DURATION, else -1) and *value (the offending
 *                                        number; the sum for CFX_TL_PLAN_SUM) — the record is then cleared; 0: no record, and
 *                                        every set call made so far has been validated on the device; 2: no record YET — a set
 *                                        call is still ahead of the device (the caller did not wait for it): ask again later */
#define CFX_TL_PLAN_DURATION 1 /* a duration that is negative or not finite */
#define CFX_TL_PLAN_SUM 2      /* the durations in force after the call would sum to less than the interval */
#define CFX_TL_PLAN_PHASE 3    /* phase outside [-1, P_i) */
#define CFX_TL_PLAN_REMAIN 4   /* a remaining time that is negative or not finite */
typedef int32_t (*cfx_set_tl_plan_device_fn)(cfx_engine *e, const double *durations, const int32_t *phase, const double *remain,
                                             int32_t n, int32_t max_phases, void *producer_stream);
typedef int32_t (*cfx_set_tl_plan_fn)(cfx_engine *e, const double *durations, const int32_t *phase, const double *remain, int32_t n,
                                      int32_t max_phases);
typedef int32_t (*cfx_get_tl_phase_durations_device_fn)(cfx_engine *e, double *out, int32_t max_phases, void *consumer_stream);
typedef int32_t (*cfx_get_tl_phase_durations_fn)(cfx_engine *e, double *out, int32_t max_phases);
typedef int32_t (*cfx_restore_tl_plan_fn)(cfx_engine *e);
typedef int32_t (*cfx_tl_plan_error_fn)(cfx_engine *e, int32_t *what, int32_t *inter, int32_t *phase, double *value);

/* ---- The lanes' speed limits as engine state in device memory (OPTIONAL entry points, as above; all five or none; not on a
 * tile: CFX_ERR_STATE).  The engine keeps two copies of the lanes' part of cfx_net::drv_max_speed (Lane::maxSpeed): the limits
 * IN FORCE, which the car-following of every step reads once per vehicle (min2double(v, drivable->getMaxSpeed()),
 * vehicle.cpp:314), and the FILE's, as cfx_create got them.  LaneLinks are not covered: they keep the reference's 10000.
 * n must be n_lanes, else CFX_ERR_INVALID; with n_envs > 1 the array is environment-major, as the lanes are.
 *   limits[l]  double: NaN keeps lane l's limit; a finite value >= 0 is in force, bit for bit, from the next cfx_step on for
 *              every vehicle then on the lane (0.0 closes the lane; above 30 is allowed — the reference only warns); a negative
 *              or infinite value is not applied and counted.  A limit caps the speed a step computes; it is no deceleration.
 * Entries are judged one by one: a rejected entry leaves the others of the call applied.  cfx_reset, cfx_load_state and
 * cfx_checkpoint_restore leave the limits in force alone.
 *   "cfx_set_lane_speed_limits_device"  limits in device memory, applied by ONE kernel on the engine's stream, read after
 *                                       everything enqueued on producer_stream (as cfx_set_tl_phases_device); rejected: NULL, or
 *                                       one int32 in device memory that is set to this call's number of rejected entries (cleared
 *                                       by a 4-byte fill ahead of the kernel) and is valid on producer_stream on return
 *   "cfx_set_lane_speed_limits"         the same from host memory (rejected: NULL or one int32 in host memory); synchronous
 *   "cfx_get_lane_speed_limits_device"  out[n_lanes]: the limits in force, every element written, ordered against
 *                                       consumer_stream (as cfx_observe_device)
 *   "cfx_get_lane_speed_limits"         the same into host memory; synchronous
 *   "cfx_restore_lane_speed_limits"     the file's limits are in force again, in every environment (one kernel on the engine's
 *                                       stream) */
typedef int32_t (*cfx_set_lane_speed_limits_device_fn)(cfx_engine *e, const double *limits, int32_t n, int32_t *rejected,
                                                       void *producer_stream);
typedef int32_t (*cfx_set_lane_speed_limits_fn)(cfx_engine *e, const double *limits, int32_t n, int32_t *rejected);
typedef int32_t (*cfx_get_lane_speed_limits_device_fn)(cfx_engine *e, double *out, int32_t n, void *consumer_stream);
typedef int32_t (*cfx_get_lane_speed_limits_fn)(cfx_engine *e, double *out, int32_t n);
typedef int32_t (*cfx_restore_lane_speed_limits_fn)(cfx_engine *e);

/* ---- What the grids of the ring layout's latency cross kernel (kr_cross) did (OPTIONAL entry point, as above; a diagnostic:
 * results never depend on a grid).  A launch gives every queued vehicle a 16-lane group; the host sizes it from job counts the
 * device reported some steps ago, and a group of a grid that is too small takes a second vehicle when the first is through.
 *   "cfx_get_cross_stats"  waits for the stream (a deferred commit is launched first) and fills *out; reset != 0 then clears
 *                          the device counters.  cfx_reset and cfx_load_state clear them too.
 * cfx_config::ring_lanes_per_wave / 100000 (the digits above the form digit), where > 0, is the number of blocks every such
 * launch gets instead (at least 16, one per shard of the queue; developer knob for the tests). */
typedef struct cfx_cross_stats {
    int64_t multi_pass_launches; /* launches in which some group took more than one job */
    int32_t max_passes;          /* the most jobs one group took in a launch (0: no launch) */
    int32_t last_jobs;           /* jobs of the last launch */
    int32_t last_grid_blocks;    /* blocks of the last launch (256 threads, 16 groups each) */
    int32_t held_jobs;           /* the job count the next grid would be sized from (the decayed peak of the reports) */
    int32_t action_multi_pass_blocks; /* blocks of the lane-walking action kernel (kr_action) that held more vehicles than one
                                       * pass of theirs takes, over all launches (cleared with the two counters above) */
    int32_t action_lanes_per_block;   /* lanes the host currently gives a block of that kernel (it follows the fullest block) */
} cfx_cross_stats;
typedef int32_t (*cfx_get_cross_stats_fn)(cfx_engine *e, cfx_cross_stats *out, int32_t reset);

/* ---- Checkpoints in device memory (OPTIONAL entry points, as above; all five or none).  A checkpoint holds what cfx_load_state
 * replaces — the running vehicles in cfx_state's order with leader and gap, the vehicle table up to the numbers handed out, the
 * waiting queues, the lights' phases and remaining times, the scalars, Lane::history where the engine keeps it — in memory of
 * the engine's device; nothing per vehicle crosses the link in either direction.  The ring layout only (engines without
 * lane_change and tiles, not created with CFX_LAYOUT_DENSE): otherwise cfx_checkpoint_create returns CFX_ERR_STATE and
 * cfx_last_error says why.  A checkpoint belongs to the engine that created it and is independent of the rings' and the vehicle
 * table's capacities, so it stays valid across their growth, cfx_load_state and cfx_reset.  The durations set by
 * cfx_set_tl_plan are not part of it (as for cfx_load_state).
 *   "cfx_checkpoint_create"   a new, empty checkpoint of e in *out
 *   "cfx_checkpoint_save"     overwrite ck with the state as of now (a deferred commit and Lane::history record are launched first);
 *                             waits for the device once, for the number of running vehicles, which sizes ck's memory
 *   "cfx_checkpoint_restore"  cfx_load_state from ck: the same reset, capacity checks, ring growth and rebuild, with device-to-device
 *                             sources; every running vehicle keeps its route position (cfx_state::r_route_pos as cfx_get_vehicles
 *                             reports it).  ck is not consumed.  Statistics kept by the backend take a new baseline, as after a load.
 *                             CFX_ERR_INVALID for a checkpoint of another engine or one never saved
 *   "cfx_checkpoint_info"     what ck holds
 *   "cfx_checkpoint_destroy"  frees ck; checkpoints still alive at cfx_destroy lose their device memory there and can only be destroyed */
typedef struct cfx_checkpoint cfx_checkpoint;
typedef struct cfx_checkpoint_desc {
    int64_t step;         /* cfx_state::step of the saved state (-1: never saved) */
    int64_t device_bytes; /* device memory held (0 after cfx_destroy of the engine) */
    int32_t n_running;    /* running vehicles */
    int32_t n_vehicles;   /* vehicle numbers handed out (rows of the vehicle table) */
} cfx_checkpoint_desc;
typedef int32_t (*cfx_checkpoint_create_fn)(cfx_engine *e, cfx_checkpoint **out);
typedef int32_t (*cfx_checkpoint_save_fn)(cfx_engine *e, cfx_checkpoint *ck);
typedef int32_t (*cfx_checkpoint_restore_fn)(cfx_engine *e, cfx_checkpoint *ck);
typedef int32_t (*cfx_checkpoint_info_fn)(const cfx_checkpoint *ck, cfx_checkpoint_desc *out);
typedef void (*cfx_checkpoint_destroy_fn)(cfx_checkpoint *ck);

/* ---- "cfx_checkpoint_restore_envs" (OPTIONAL, and only beside the five above): cfx_checkpoint_restore on an engine of
 * cfx_config::n_envs environments, with environment r taking the state that environment src_env[r] has in ck.  Repeats are
 * allowed; an environment named nowhere is dropped.  Everything an environment owns moves with it: its running vehicles, entry
 * buffers, lights (phase and remaining time) and Lane::history; lane, laneLink, intersection and route indices are shifted by
 * (r - src_env[r]) times the per-environment counts.  Vehicle numbers are the caller's to hand out, because a state taken twice
 * needs two sets of them: after the call environment r owns the numbers env_first[r] .. env_first[r + 1] - 1, and number
 * env_first[r] + k is the vehicle that ck knows as the k-th of environment src_env[r]:
 *   old_env[o], old_local[o]   for every vehicle number o of ck: its environment, and its rank k among that environment's numbers
 *   new_src[v]                 for every number v after the call: the number of ck that it copies
 * The tables are checked against each other (CFX_ERR_INVALID; nothing has happened then).  The engine-wide counts of running and
 * finished vehicles, the per-drivable counts the rings are fitted to and the lanes that may admit are those of the environments
 * taken; cfx_scalars::cumulative_travel_time and ::vehicle_steps, which no record splits by environment, stay the totals of ck.
 * Speeds set for vehicles that do not exist yet (cfx_set_vehicle_speed) are dropped.  ck is not consumed and not modified.
 * Returns CFX_ERR_STATE / CFX_ERR_INVALID where cfx_checkpoint_restore does, CFX_ERR_STATE also for a ck that counts finished
 * vehicles outside its vehicle table (a state that came from cfx_load_state with such a count). */
typedef struct cfx_env_gather {
    int32_t n_envs;           /* cfx_config::n_envs of the engine */
    const int32_t *src_env;   /* [n_envs] */
    const int32_t *env_first; /* [n_envs + 1], env_first[0] = 0, env_first[n_envs] = n_new */
    int32_t n_old;            /* cfx_checkpoint_desc::n_vehicles of ck */
    const int32_t *old_env;   /* [n_old] */
    const int32_t *old_local; /* [n_old] */
    int32_t n_new;
    const int32_t *new_src;   /* [n_new] */
} cfx_env_gather;
typedef int32_t (*cfx_checkpoint_restore_envs_fn)(cfx_engine *e, cfx_checkpoint *ck, const cfx_env_gather *g);

#ifdef __cplusplus
}
#endif
#endif /* CITYFLOW_AMD_H */
