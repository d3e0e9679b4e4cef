"""Lane and intersection observations and signal control as torch tensors (Engine and VectorEngine).

    eng.get_lane_vehicle_count_tensor(out=None)          int32 [L]   (VectorEngine: [R, L])
    eng.get_lane_waiting_vehicle_count_tensor(out=None)  int32 [L]   (VectorEngine: [R, L])
    eng.set_tl_phases_tensor(phases)                     integer [I] (VectorEngine: [R, I])
    eng.get_lane_speed_sum_tensor(out=None)              float64 [L] (VectorEngine: [R, L])
    eng.get_lane_vehicle_bins_tensor(edges, out=None)    int32 [L, B] (VectorEngine: [R, L, B])
    eng.observe_lanes_tensor(counts=None, waiting=None, speed_sum=None, bins=None, edges=None, front_distance=None,
                             front_speed=None, front_lane_steps=None, front_waiting_steps=None)
                                                         fills every given tensor with one kernel launch
    eng.get_lane_front_vehicles_tensor(k, distance=None, speed=None)
                                                         float64 [L, k] each: the k vehicles nearest every lane's end
    eng.get_lane_front_vehicles_array(k)                 the front outputs as numpy arrays (waits for the device)
    eng.observe_vehicles_tensor(start=None, count=None, vehicle=None, drivable=None, env=None, distance=None, speed=None,
                                leader=None, gap=None, x=None, y=None, dir_x=None, dir_y=None, length=None, width=None)
                                                         every running vehicle as a row, grouped by drivable (CSR): int32
                                                         start [D+1] ([R, D+1]) and count (0-dim), and rows [N] of the caller's N,
                                                         its pose in the plane among them; two kernel launches, no host wait
                                                         (see its docstring)
    eng.observe_vehicles_array(poses=False)              the same outputs as numpy arrays, exactly `count` rows (waits for the device)
    eng.drivable_geometry()                              {"point_start": int32 [D+1], "points": float64 [P, 2]}: the drivables' polylines
    eng.set_vehicle_speeds_tensor(vehicle, speed, ignored=None)
                                                         set_vehicle_speed() for the rows of int32 [N] vehicle numbers (those of
                                                         observe_vehicles_tensor) and float64 [N] speeds, NaN = leave alone;
                                                         two or three kernel launches, no host wait (see its docstring)
    eng.set_vehicle_speeds(vehicle, speed) -> int        the same from numpy arrays; returns the rows ignored (waits for the device)
    eng.set_vehicle_routes_tensor(vehicle, route, status=None, ignored=None)
                                                         set_vehicle_route() for the rows of int32 [N] vehicle numbers and int32
                                                         [N] handles of registered routes (Engine.add_routes, VectorEngine(routes=)),
                                                         -1 = leave alone; a verdict per row in `status`; no host wait
    eng.set_vehicle_routes(vehicle, route) -> (status, ignored)
                                                         the same from numpy arrays (waits for the device)
    eng.get_vehicle_routes_tensor(vehicle, out=None)     the handle each of those vehicles holds, -1 where there is none
    eng.get_vehicle_routes(vehicle) -> ndarray           the same from a numpy array (waits for the device)
    eng.observe_intersections_tensor(phase=None, phase_remain=None, movement_in=None, movement_in_waiting=None,
                                     movement_out=None, movement_inside=None, phase_pressure=None)
                                                         per-intersection observations, one kernel launch (see its docstring)
    eng.get_tl_phases_tensor(out=None)                   int32 [I]   (VectorEngine: [R, I]): the reading side of set_tl_phases_tensor
    eng.observe_intersections_array()                    the same seven outputs as numpy arrays (waits for the device)
    eng.intersection_layout()                            the static signal plan and movement tables (host only, numpy)
    eng.track_lane_flow(on=True) / eng.lane_flow_tracking()
                                                         per-lane flow and waiting-time statistics ACROSS steps (off by default)
    eng.observe_lane_flow_tensor(entered=None, left=None, left_steps=None, left_waiting_steps=None, waiting_steps=None,
                                 max_waiting_steps=None, reset=False)
                                                         drains them into the given tensors, one kernel launch (see its docstring)
    eng.observe_lane_flow_array(reset=False)             the same six outputs as numpy arrays (waits for the device)
    eng.track_movement_flow(on=True) / eng.movement_flow_tracking()
                                                         per-movement throughput and delay statistics ACROSS steps (off by default)
    eng.observe_movement_flow_tensor(entered=None, entered_lane_steps=None, entered_lane_waiting_steps=None, left=None,
                                     left_steps=None, left_waiting_steps=None, waiting_steps=None, max_waiting_steps=None,
                                     reset=False)        drains them into the given [I, M] tensors, one kernel launch
    eng.observe_movement_flow_array(reset=False)         the same eight outputs as numpy arrays (waits for the device)
    eng.track_trips(on=True) / eng.trip_tracking()       trip statistics per environment ACROSS steps (off by default)
    eng.observe_trips_tensor(entered=None, admitted=None, admitted_buffer_steps=None, finished=None,
                             finished_travel_steps=None, in_system=None, buffered=None, in_system_travel_steps=None,
                             average_travel_time=None)   0-dim (VectorEngine: [R]) each, one kernel launch (see its docstring)
    eng.observe_trips_array()                            the same nine outputs as numpy arrays (waits for the device)
    eng.get_average_travel_time_tensor(out=None)         float64 0-dim (VectorEngine: [R]): get_average_travel_time() on the device
    eng.track_trips(on=True, log=N) / eng.trip_log_capacity()
                                                         the trip LOG: one row per finished vehicle, N rows of room (off by default)
    eng.observe_trip_log_tensor(count=None, dropped=None, env=None, vehicle=None, origin_road=None, destination_road=None,
                                enter_step=None, finish_step=None, travel_steps=None, reset=False)
                                                         drains it into int32 tensors, [N] per column, one kernel launch
    eng.observe_trip_log_array(reset=False)              the same as numpy columns trimmed to count, in a canonical order
    eng.track_detectors(lane=None, start=None, end=None, on=True) / eng.detector_tracking() / eng.detector_layout()
                                                         N virtual loop detectors, zones [start, end) of lanes: what passed them,
                                                         how long they were occupied and how fast the traffic over them was,
                                                         ACROSS steps (off by default)
    eng.observe_detectors_tensor(passed=None, occupied_steps=None, vehicle_steps=None, waiting_vehicle_steps=None,
                                 speed_sum=None, count=None, reset=False)
                                                         drains them into the given [N] tensors, one kernel launch (see its docstring)
    eng.observe_detectors_array(reset=False)             the same six outputs as numpy arrays (waits for the device)
    eng.set_tl_plan_tensor(durations=None, phase=None, phase_remain=None)
                                                         the fixed-time signal plan as engine state: float64 [I, P] phase durations,
                                                         integer [I] current phase, float64 [I] its remaining time (VectorEngine:
                                                         [R, ...], one plan per environment); validated on the device, whole call or
                                                         nothing, one kernel launch (see its docstring)
    eng.get_tl_phase_durations_tensor(out=None)          float64 [I, P]: the durations in force
    eng.set_tl_plan(...) / eng.get_tl_phase_durations_array()
                                                         the same over numpy arrays (wait for the device)
    eng.restore_tl_plan()                                the roadnet file's durations are in force again
    eng.set_lane_speed_limits_tensor(limits, rejected=None)
                                                         the lanes' speed limits as engine state: float64 [L] (VectorEngine: [R, L],
                                                         one scheme per environment), NaN = keep; negative or infinite entries are
                                                         left out and counted in int32 [1] `rejected`; one kernel launch, no host wait
    eng.get_lane_speed_limits_tensor(out=None)           float64 [L]: the limits in force
    eng.set_lane_speed_limits(limits) -> int / eng.get_lane_speed_limits_array()
                                                         the same over numpy arrays (wait for the device)
    eng.restore_lane_speed_limits()                      the roadnet file's limits are in force again

On the HIP engine the tensors live on the engine's GPU and nothing here waits for the device:
  * a getter's kernel writes the caller's tensor on the engine's stream after everything already enqueued there and on the
    caller's current torch stream; work enqueued on the current stream afterwards sees the result;
  * set_tl_phases_tensor reads `phases` on the engine's stream after everything already enqueued on the current stream, so a
    policy's output can be passed in directly.  -1 keeps a signal's phase; entries of virtual intersections are ignored; any
    other entry outside [0, phase count) rejects the whole call, and the next call that waits for the device (sync(), a
    getter that reads to the host, snapshot, reset) raises IndexError naming the intersection (and env);
  * lifetimes follow torch's own stream order: the current stream waits for the engine's use of a tensor (an event the
    engine records after its kernel), so the caching allocator may hand the memory out again, and the caller may overwrite
    it, with work enqueued there afterwards.  (record_stream on an ExternalStream over the engine's stream would make the
    allocator record an event on that stream when the tensor is freed — after the engine, and its stream, may be gone.)
The exceptions to "no host wait" are the engine's own: table or ring growth and a spawner priority collision (these drain),
laneChange (every step polls the device), an open replay log (every step is read back).

A backend without device buffers (the CPU twin) takes and returns CPU tensors, over the array calls, with the same
semantics; an invalid entry raises at once there.  The HIP engine never falls back: a CPU tensor is a TypeError.

torch is imported by the first call, never by `import cityflow_amd`.
"""


def _torch():
    import torch
    return torch


def _check_phases(torch, phases, shape, device):
    if not isinstance(phases, torch.Tensor):
        raise TypeError("phases must be a torch.Tensor, not %s" % type(phases).__name__)
    if phases.device != device:
        raise TypeError("phases is on %s; this engine's tensors live on %s" % (phases.device, device))
    if phases.dtype == torch.bool or phases.is_floating_point() or phases.is_complex():
        raise TypeError("phases must be an integer tensor, not %s" % phases.dtype)
    if tuple(phases.shape) != shape:
        raise ValueError("phases must have shape %s, not %s" % (shape, tuple(phases.shape)))


def _set_phases_host(eng, torch, phases, shape):
    import numpy as np

    if not eng._rl_traffic_light():
        eng.set_tl_phases(np.zeros(shape, dtype=np.int32))  # (prints the reference's message, changes nothing)
        return
    want = phases.detach().numpy().astype(np.int64).reshape(-1, shape[-1])
    counts = eng._phase_counts()
    bad = (counts >= 0) & ((want < -1) | (want >= counts))
    if bad.any():
        env, inter = [int(x[0]) for x in np.nonzero(bad)]
        where = "intersection '%s'" % eng.intersection_ids()[inter]
        if len(shape) == 2:
            where += " of env %d" % env
        raise IndexError("set_tl_phases_tensor: phase %d out of range for %s (the call was not applied)"
                         % (want[env, inter], where))
    current = np.asarray(eng._tl_state()[0]).reshape(want.shape)
    eng.set_tl_phases(np.where(want == -1, current, want).astype(np.int32).reshape(shape))


def set_tl_phases_tensor(self, phases):
    """Set every signal from an integer tensor of shape [I] ([R, I] for VectorEngine) on the engine's device, read after
    everything enqueued on the current torch stream.  -1 keeps the phase, entries of virtual intersections are ignored; an
    entry outside [-1, phase count) rejects the whole call, and the next call that waits for the device raises IndexError."""
    torch = _torch()
    shape = tuple(self._tensor_shapes()[1])
    if not self._device_buffers():
        _check_phases(torch, phases, shape, torch.device("cpu"))
        return _set_phases_host(self, torch, phases, shape)
    device = torch.device("cuda", self._stream_handle()[1])
    _check_phases(torch, phases, shape, device)
    p = phases
    if p.dtype != torch.int32:  # (values beyond int32 stay invalid instead of wrapping into range)
        p = p.to(torch.int64).clamp(-2, 2 ** 31 - 1).to(torch.int32)
    p = p.contiguous()
    self._set_tl_phases_device(p.data_ptr(), p.numel(), torch.cuda.current_stream(device).cuda_stream)


MAX_BINS = 32  # CFX_MAX_LANE_BINS


def _engine_device(torch, eng):
    return torch.device("cuda", eng._stream_handle()[1]) if eng._device_buffers() else torch.device("cpu")


def _check_buf(torch, t, name, shape, dtype, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor, not %s" % (name, type(t).__name__))
    if t.device != device:
        raise TypeError("%s is on %s; this engine's tensors live on %s" % (name, t.device, device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, not %s" % (name, dtype, t.dtype))
    if tuple(t.shape) != shape:
        raise ValueError("%s must have shape %s, not %s" % (name, shape, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)


def _check_edges(torch, edges, n_lanes, device):
    """-> (float64 contiguous edges, B, per_lane).  edges: [L, B+1] (a row per lane) or [B+1] (shared), 1 <= B <= 32."""
    if not isinstance(edges, torch.Tensor):
        raise TypeError("edges must be a torch.Tensor, not %s" % type(edges).__name__)
    if edges.device != device:
        raise TypeError("edges is on %s; this engine's tensors live on %s" % (edges.device, device))
    if not edges.is_floating_point():
        raise TypeError("edges must be a floating tensor, not %s" % edges.dtype)
    if edges.dim() == 1:
        per_lane = False
    elif edges.dim() == 2 and edges.shape[0] == n_lanes:
        per_lane = True
    else:
        raise ValueError("edges must have shape [B+1] or [%d, B+1], not %s" % (n_lanes, tuple(edges.shape)))
    n_bins = edges.shape[-1] - 1
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("edges must give 1 to %d bins (B+1 edges), not %d" % (MAX_BINS, n_bins))
    return edges.to(torch.float64).contiguous(), n_bins, per_lane


MAX_FRONT = 64  # CFX_MAX_LANE_FRONT
LANE_FRONT_OUTPUTS = ("front_distance", "front_speed", "front_lane_steps", "front_waiting_steps")


def observe_lanes_tensor(self, counts=None, waiting=None, speed_sum=None, bins=None, edges=None, front_distance=None,
                         front_speed=None, front_lane_steps=None, front_waiting_steps=None):
    """Fill every given tensor with one kernel launch on the engine's stream, ordered against the current torch stream:
    counts / waiting (int32 [L], as get_lane_vehicle_count_tensor / get_lane_waiting_vehicle_count_tensor), speed_sum
    (float64 [L], as get_lane_speed_sum_tensor) and bins (int32 [L, B], as get_lane_vehicle_bins_tensor, with `edges`).

    The front outputs hold, per lane, its first K vehicles from the front (nearest the lane's end first, the order of
    get_lane_vehicles()); K, 1 to 64, is their last dimension and the same for all of them:

        front_distance       float64 [L, K]  distance from the lane's start, as get_vehicle_distance()   padding -1.0
        front_speed          float64 [L, K]  as get_vehicle_speed()                                       padding 0.0
        front_lane_steps     int32 [L, K]    steps the vehicle has been on the lane (s - since)           padding 0
        front_waiting_steps  int32 [L, K]    steps it has waited there (wait)                             padding 0

    Slot k of lane l is a vehicle exactly if k < counts[l] (lane-change shadows count, as in counts); the slots behind hold the
    padding, -1.0 being a convenience, not the rule.  Every element is written.  The last two read the track_lane_flow tracker
    (observe_lane_flow_tensor has its rules) as of the last step, changing nothing in it: RuntimeError while tracking is off, so
    never with laneChange.  With front outputs alone a lane is read only as far as its K-th vehicle.
    VectorEngine: a leading [R] on every output.  At least one output; every argument is checked before anything is enqueued."""
    torch = _torch()
    shape = tuple(self._tensor_shapes()[0])
    fronts = dict(zip(LANE_FRONT_OUTPUTS, (front_distance, front_speed, front_lane_steps, front_waiting_steps)))
    if counts is None and waiting is None and speed_sum is None and bins is None and all(t is None for t in fronts.values()):
        raise ValueError("observe_lanes_tensor: give at least one of counts, waiting, speed_sum, bins, " + ", ".join(LANE_FRONT_OUTPUTS))
    if bins is not None and edges is None:
        raise ValueError("observe_lanes_tensor: bins requires edges")
    device = _engine_device(torch, self)
    n_bins, per_lane = 0, False
    if edges is not None:
        edges, n_bins, per_lane = _check_edges(torch, edges, shape[-1], device)
    if counts is not None:
        _check_buf(torch, counts, "counts", shape, torch.int32, device)
    if waiting is not None:
        _check_buf(torch, waiting, "waiting", shape, torch.int32, device)
    if speed_sum is not None:
        _check_buf(torch, speed_sum, "speed_sum", shape, torch.float64, device)
    if bins is not None:
        _check_buf(torch, bins, "bins", shape + (n_bins,), torch.int32, device)
    n_front = 0
    for name, t in fronts.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, not %s" % (name, type(t).__name__))
        if not n_front:
            n_front = _check_front_k(t.shape[-1] if t.dim() else 0)
        _check_buf(torch, t, name, shape + (n_front,), torch.float64 if name in LANE_FRONT_OUTPUTS[:2] else torch.int32, device)
    tracker = front_lane_steps is not None or front_waiting_steps is not None
    if tracker and not self._lane_flow_tracking():
        raise RuntimeError("observe_lanes_tensor: front_lane_steps / front_waiting_steps need lane-flow tracking "
                           "(track_lane_flow(True) turns it on)")
    if not self._device_buffers():  # (the twin: over the array calls)
        if counts is not None:
            counts.copy_(torch.from_numpy(self.get_lane_vehicle_count_array().reshape(shape)))
        if waiting is not None:
            waiting.copy_(torch.from_numpy(self.get_lane_waiting_vehicle_count_array().reshape(shape)))
        if speed_sum is not None:
            speed_sum.copy_(torch.from_numpy(self.get_lane_speed_sum_array()))
        if bins is not None:
            bins.copy_(torch.from_numpy(self.get_lane_vehicle_bins_array(edges.detach().numpy())))
        if n_front:
            arrays = _lane_fronts(self, n_front, tracker)
            for name, t in fronts.items():
                if t is not None:
                    t.copy_(torch.from_numpy(arrays[name]))
        return
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    self._observe_lanes_device(ptr(counts), ptr(waiting), ptr(speed_sum), ptr(bins), ptr(edges) if bins is not None else 0,
                               n_bins, per_lane, ptr(front_distance), ptr(front_speed), ptr(front_lane_steps),
                               ptr(front_waiting_steps), n_front, torch.cuda.current_stream(device).cuda_stream)


def _check_front_k(k):
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError("k must be an int, not %s" % type(k).__name__)
    if not 1 <= k <= MAX_FRONT:
        raise ValueError("the front outputs hold 1 to %d vehicles per lane (their last dimension), not %d" % (MAX_FRONT, k))
    return k


def _lane_fronts(eng, k, tracker):
    """{front output: numpy array [L, k]} over the array call; the tracker columns only with `tracker`."""
    shape = tuple(eng._tensor_shapes()[0]) + (k,)
    names = LANE_FRONT_OUTPUTS if tracker else LANE_FRONT_OUTPUTS[:2]
    return {name: a.reshape(shape) for name, a in zip(names, eng._lane_fronts(k, tracker))}


def get_lane_front_vehicles_tensor(self, k, distance=None, speed=None):
    """(distance, speed) of the first k vehicles of every lane from the front, float64 [L, k] each on the engine's device, valid
    on the current torch stream: the front_distance and front_speed outputs of observe_lanes_tensor (its docstring has the
    order and the padding), 1 <= k <= 64.  `distance` / `speed`: contiguous tensors of that shape, filled in place; what is not
    given is allocated."""
    torch = _torch()
    shape = tuple(self._tensor_shapes()[0]) + (_check_front_k(k),)
    device = _engine_device(torch, self)
    if distance is None:
        distance = torch.empty(shape, dtype=torch.float64, device=device)
    elif isinstance(distance, torch.Tensor) and tuple(distance.shape) != shape:
        raise ValueError("distance must have shape %s, not %s" % (shape, tuple(distance.shape)))
    if speed is None:
        speed = torch.empty(shape, dtype=torch.float64, device=device)
    observe_lanes_tensor(self, front_distance=distance, front_speed=speed)
    return distance, speed


def get_lane_front_vehicles_array(self, k):
    """The front outputs of observe_lanes_tensor as a dict of numpy arrays [L, k] (same names, dtypes and padding):
    front_distance and front_speed, and front_lane_steps and front_waiting_steps exactly when track_lane_flow is on.  Waits for
    the device."""
    return _lane_fronts(self, _check_front_k(k), self._lane_flow_tracking())


def _lane_out(eng, dtype_name):
    torch = _torch()
    return torch.empty(tuple(eng._tensor_shapes()[0]), dtype=getattr(torch, dtype_name), device=_engine_device(torch, eng))


def get_lane_vehicle_count_tensor(self, out=None):
    """Vehicles on every lane (get_lane_vehicle_count_array's order) as an int32 tensor on the engine's device, valid on the
    current torch stream; `out`: a contiguous int32 tensor of that shape on that device, filled in place."""
    if out is None:
        out = _lane_out(self, "int32")
    observe_lanes_tensor(self, counts=out)
    return out


def get_lane_waiting_vehicle_count_tensor(self, out=None):
    """Vehicles with speed < 0.1 on every lane, as get_lane_vehicle_count_tensor."""
    if out is None:
        out = _lane_out(self, "int32")
    observe_lanes_tensor(self, waiting=out)
    return out


def get_lane_speed_sum_tensor(self, out=None):
    """Sum of the speeds of every lane's vehicles, front to back (mean speed = sum / count), as a float64 tensor on the
    engine's device, valid on the current torch stream; `out`: a contiguous float64 tensor of that shape, filled in place."""
    if out is None:
        out = _lane_out(self, "float64")
    observe_lanes_tensor(self, speed_sum=out)
    return out


def get_lane_vehicle_bins_tensor(self, edges, out=None):
    """Vehicles of every lane with edges[l, b] <= distance < edges[l, b+1] (distance from the lane's start, as
    get_vehicle_distance), as an int32 tensor [L, B] on the engine's device; `edges`: a floating tensor [L, B+1] or [B+1] on
    that device, 1 <= B <= 32 (VectorEngine: the same edges for every environment)."""
    torch = _torch()
    if out is None:
        shape = tuple(self._tensor_shapes()[0])
        device = _engine_device(torch, self)
        _, n_bins, _ = _check_edges(torch, edges, shape[-1], device)
        out = torch.empty(shape + (n_bins,), dtype=torch.int32, device=device)
    observe_lanes_tensor(self, bins=out, edges=edges)
    return out


INTERSECTION_OUTPUTS = ("phase", "phase_remain", "movement_in", "movement_in_waiting", "movement_out", "movement_inside",
                        "phase_pressure")


def _intersection_shapes(eng):
    """{output: shape} of the seven intersection outputs ([R] in front on a VectorEngine)."""
    lead = tuple(eng._tensor_shapes()[1])
    n_roadlinks, n_phases = eng._intersection_dims()
    shapes = {name: lead + (n_roadlinks,) for name in INTERSECTION_OUTPUTS[2:6]}
    shapes["phase"] = shapes["phase_remain"] = lead
    shapes["phase_pressure"] = lead + (n_phases,)
    return shapes


def observe_intersections_tensor(self, phase=None, phase_remain=None, movement_in=None, movement_in_waiting=None,
                                 movement_out=None, movement_inside=None, phase_pressure=None):
    """Fill every given tensor with one kernel launch on the engine's stream, ordered against the current torch stream as
    observe_lanes_tensor.  Intersections in intersection_ids() order (I, virtual ones included); the roadLinks ("movements")
    of intersection i in the roadnet file's order, m < M_i; its phases p < P_i; M = max M_i, P = max P_i (intersection_layout()).
    IN(i, m) / OUT(i, m): the distinct start / end lanes of the roadLink's laneLinks (a lane counts once).

        phase                int32 [I]      the current phase (0 at a virtual intersection)
        phase_remain         float64 [I]    seconds the phase still has (TrafficLight::remainDuration)
        movement_in          int32 [I, M]   vehicles on the lanes of IN(i, m), as get_lane_vehicle_count_array counts them
        movement_in_waiting  int32 [I, M]   ... of them the waiting ones (speed < 0.1), as get_lane_waiting_vehicle_count_array
        movement_out         int32 [I, M]   vehicles on the lanes of OUT(i, m)
        movement_inside      int32 [I, M]   vehicles inside the intersection, on a laneLink of roadLink (i, m)
        phase_pressure       int32 [I, P]   sum of movement_in - movement_out over the roadLinks phase p serves

    Lane-change shadows count like vehicles, as in the count getters.  Padding: movement_*[i, m] = 0 for m >= M_i (a virtual
    intersection has no roadLinks); phase_pressure[i, p] = INT32_MIN for p >= P_i and for every p of a virtual intersection, so
    phase_pressure.argmax(-1) is a valid phase wherever one exists and can be handed to set_tl_phases_tensor as it is (entries
    of virtual intersections are ignored there).  A phase that serves no roadLink has pressure 0, not the padding value.  Every
    element is written, so the tensors need no zeroing.  VectorEngine: a leading [R] on every output.  At least one output;
    every argument is checked before anything is enqueued."""
    torch = _torch()
    given = dict(zip(INTERSECTION_OUTPUTS, (phase, phase_remain, movement_in, movement_in_waiting, movement_out,
                                            movement_inside, phase_pressure)))
    if all(t is None for t in given.values()):
        raise ValueError("observe_intersections_tensor: give at least one of " + ", ".join(INTERSECTION_OUTPUTS))
    shapes = _intersection_shapes(self)
    device = _engine_device(torch, self)
    for name, t in given.items():
        if t is not None:
            _check_buf(torch, t, name, shapes[name], torch.float64 if name == "phase_remain" else torch.int32, device)
    if not self._device_buffers():  # (the twin: over the array call)
        arrays = self.observe_intersections_array()
        for name, t in given.items():
            if t is not None:
                t.copy_(torch.from_numpy(arrays[name]))
        return
    n_roadlinks, n_phases = self._intersection_dims()
    self._observe_intersections_device(*[0 if given[name] is None else given[name].data_ptr() for name in INTERSECTION_OUTPUTS],
                                       n_roadlinks, n_phases, torch.cuda.current_stream(device).cuda_stream)


def get_tl_phases_tensor(self, out=None):
    """The current phase of every intersection (0 at virtual ones) as an int32 tensor [I] ([R, I] for VectorEngine) on the
    engine's device, valid on the current torch stream: the `phase` output of observe_intersections_tensor alone, the reading
    side of set_tl_phases_tensor.  `out`: a contiguous int32 tensor of that shape on that device, filled in place."""
    torch = _torch()
    if out is None:
        out = torch.empty(tuple(self._tensor_shapes()[1]), dtype=torch.int32, device=_engine_device(torch, self))
    observe_intersections_tensor(self, phase=out)
    return out


def observe_intersections_array(self):
    """The seven outputs of observe_intersections_tensor as a dict of numpy arrays (same names, dtypes, shapes and padding);
    waits for the device."""
    shapes = _intersection_shapes(self)
    return {name: a.reshape(shapes[name]) for name, a in zip(INTERSECTION_OUTPUTS, self._intersection_features())}


def intersection_layout(self):
    """The static tables behind observe_intersections_tensor, of ONE environment, as numpy arrays (host only):
        n_roadlinks    int32 [I]          M_i (0 at a virtual intersection)
        n_phases       int32 [I]          P_i, -1 = virtual
        phase_avail    bool [I, P, M]     phase p of intersection i serves roadLink m (False in the padding)
        roadlink_type  int32 [I, M]       1 turn right, 2 turn left, 3 go straight, 0 = padding
        in_lanes       int32 [I, M, Kin]  IN(i, m) as indices into lane_ids(), ascending, -1 = padding
        out_lanes      int32 [I, M, Kout] OUT(i, m) likewise"""
    import numpy as np

    d = dict(self._intersection_layout())
    d["phase_avail"] = d["phase_avail"].astype(np.bool_)
    return d


def _observe_tracker_tensor(eng, what, names, tensors, dtype_of, shape, tracking, off, arrays, device_call, extra=()):
    """What observe_lane_flow_tensor, observe_movement_flow_tensor and observe_trips_tensor do.  `tensors`: the outputs in the
    order of `names` (None: not asked for), each of `shape()` and `dtype_of(torch, name)`; `tracking()`, and the message `off`
    while it is not on; `arrays()`: the array call, for an engine without device buffers (the twin); `device_call(*pointers,
    *extra, stream)`, 0 for an output not asked for.  In this order: at least one output, every buffer, tracking on — and
    nothing is enqueued before all of that."""
    torch = _torch()
    given = dict(zip(names, tensors))
    if all(t is None for t in given.values()):
        raise ValueError(what + ": give at least one of " + ", ".join(names))
    shape = shape()
    device = _engine_device(torch, eng)
    for name, t in given.items():
        if t is not None:
            _check_buf(torch, t, name, shape, dtype_of(torch, name), device)
    if not tracking():
        raise RuntimeError(what + ": " + off)
    if not eng._device_buffers():  # (the twin: over the array call)
        for name, a in arrays().items():
            if given[name] is not None:
                given[name].copy_(torch.from_numpy(a))
        return
    device_call(*[0 if given[name] is None else given[name].data_ptr() for name in names], *extra,
                torch.cuda.current_stream(device).cuda_stream)


LANE_FLOW_OUTPUTS = ("entered", "left", "left_steps", "left_waiting_steps", "waiting_steps", "max_waiting_steps")
_LANE_FLOW_INT64 = ("left_steps", "left_waiting_steps", "waiting_steps")


def track_lane_flow(self, on=True):
    """Turn the per-lane flow tracker on or off (off by default: nothing is allocated or launched, and it frees its memory when
    turned off).  While it is on, every next_step() ends with one tracker update (one extra kernel launch on the HIP engine).
    Turning it on takes a baseline: the vehicles then on a lane start with no waiting time and are not counted as entered, all
    accumulators are zero; reset(), load() and load_from_file() take a new baseline and keep it on.  Not with laneChange
    (NotImplementedError)."""
    self._track_lane_flow(bool(on))


def lane_flow_tracking(self):
    """Whether track_lane_flow is on."""
    return self._lane_flow_tracking()


def observe_lane_flow_tensor(self, entered=None, left=None, left_steps=None, left_waiting_steps=None, waiting_steps=None,
                             max_waiting_steps=None, reset=False):
    """Fill every given tensor with one kernel launch on the engine's stream, ordered against the current torch stream as
    observe_lanes_tensor (no host wait).  Lanes in lane_ids() order; s = steps taken, P(l) = the vehicles get_lane_vehicles()
    lists on lane l (vehicles inside an intersection are on no lane).  After every step, per lane: a vehicle new on the lane
    counts as entered and starts with since = s, wait = 0; a vehicle no longer on it (gone into the intersection, or finished)
    counts as left, with the steps it spent there and the steps it spent waiting there; every vehicle on it with speed < 0.1 (the
    criterion of get_lane_waiting_vehicle_count) waits one step more.

        entered             int32 [L]  vehicles that entered      \
        left                int32 [L]  vehicles that left          | accumulated since the last call with reset=True,
        left_steps          int64 [L]  sum of their s - since      | or since the baseline (track_lane_flow)
        left_waiting_steps  int64 [L]  sum of their wait          /
        waiting_steps       int64 [L]  now: sum of wait over the vehicles on the lane
        max_waiting_steps   int32 [L]  now: the largest wait on the lane (0 on an empty lane)

    Seconds = steps * interval.  reset=True zeroes the four accumulators in the same launch, after they were read — all four,
    whether or not they were asked for.  Every element is written.  VectorEngine: a leading [R] on every output.  At least one
    output; every argument is checked before anything is enqueued; RuntimeError while tracking is off."""
    _observe_tracker_tensor(
        self, "observe_lane_flow_tensor", LANE_FLOW_OUTPUTS,
        (entered, left, left_steps, left_waiting_steps, waiting_steps, max_waiting_steps),
        lambda torch, name: torch.int64 if name in _LANE_FLOW_INT64 else torch.int32, lambda: tuple(self._tensor_shapes()[0]),
        self._lane_flow_tracking, "lane-flow tracking is off (track_lane_flow(True) turns it on)",
        lambda: observe_lane_flow_array(self, reset=reset), self._observe_lane_flow_device, (bool(reset),))


def observe_lane_flow_array(self, reset=False):
    """The six outputs of observe_lane_flow_tensor as a dict of numpy arrays (same names, dtypes and shapes); waits for the
    device.  RuntimeError while tracking is off."""
    if not self._lane_flow_tracking():
        raise RuntimeError("observe_lane_flow_array: lane-flow tracking is off (track_lane_flow(True) turns it on)")
    shape = tuple(self._tensor_shapes()[0])
    return {name: a.reshape(shape) for name, a in zip(LANE_FLOW_OUTPUTS, self._lane_flow_features(bool(reset)))}


MOVEMENT_FLOW_OUTPUTS = ("entered", "entered_lane_steps", "entered_lane_waiting_steps", "left", "left_steps", "left_waiting_steps",
                         "waiting_steps", "max_waiting_steps")
_MOVEMENT_FLOW_INT32 = ("entered", "left", "max_waiting_steps")


def track_movement_flow(self, on=True):
    """Turn the per-movement flow tracker on or off (off by default: nothing is allocated or launched, and it frees its memory
    when turned off).  While it is on, every next_step() ends with one tracker update (one extra kernel launch on the HIP
    engine; independent of track_lane_flow: both on means two updates).  Turning it on takes a baseline: every vehicle then on
    a lane or inside an intersection starts with no waiting time and is not counted as entered, all accumulators are zero;
    reset(), load() and load_from_file() take a new baseline and keep it on.  Not with laneChange (NotImplementedError)."""
    self._track_movement_flow(bool(on))


def movement_flow_tracking(self):
    """Whether track_movement_flow is on."""
    return self._movement_flow_tracking()


def _movement_flow_shape(eng):
    return tuple(eng._tensor_shapes()[1]) + (eng._intersection_dims()[0],)


def observe_movement_flow_tensor(self, entered=None, entered_lane_steps=None, entered_lane_waiting_steps=None, left=None,
                                 left_steps=None, left_waiting_steps=None, waiting_steps=None, max_waiting_steps=None, reset=False):
    """Fill every given tensor with one kernel launch on the engine's stream, ordered against the current torch stream as
    observe_lane_flow_tensor (no host wait).  Per roadLink ("movement") (i, m), in the indexing of observe_intersections_tensor:
    the sum (max_waiting_steps: the maximum) over the roadLink's laneLinks.  s = steps taken; a vehicle is on a lane or on a
    laneLink (inside the intersection), the `drivable` of get_vehicle_info; it keeps since (the step it came onto its drivable)
    and wait (the steps it has stood there with speed < 0.1, the criterion of get_lane_waiting_vehicle_count).  After every step:
    a vehicle new on a laneLink counts as entered, with — if it came off a lane — the steps it spent on that lane and the
    steps it waited there; a vehicle no longer on a laneLink counts as left, with the steps it spent and waited inside.  A
    vehicle that went from a lane to the next lane in one step counts as entered and left on the first laneLink joining the two
    (in the lane's laneLink order), with its lane steps and nothing inside.

        entered                     int32 [I, M]  vehicles that crossed the stop line             \\
        entered_lane_steps          int64 [I, M]  sum of the steps they spent on the approach lane  | accumulated since the
        entered_lane_waiting_steps  int64 [I, M]  sum of the steps they waited there                | last call with
        left                        int32 [I, M]  vehicles that left the intersection               | reset=True, or since
        left_steps                  int64 [I, M]  sum of the steps they spent inside                | the baseline
        left_waiting_steps          int64 [I, M]  sum of the steps they waited inside              /
        waiting_steps               int64 [I, M]  now: sum of wait over the vehicles inside
        max_waiting_steps           int32 [I, M]  now: the largest wait inside (0 if there is none)

    Seconds = steps * interval.  Rows m >= M_i and every row of a virtual intersection are 0; every element is written.
    reset=True zeroes the six accumulators in the same launch, after they were read — all six, whether or not they were asked
    for.  VectorEngine: a leading [R] on every output.  At least one output; every argument is checked before anything is
    enqueued; RuntimeError while tracking is off."""
    _observe_tracker_tensor(
        self, "observe_movement_flow_tensor", MOVEMENT_FLOW_OUTPUTS,
        (entered, entered_lane_steps, entered_lane_waiting_steps, left, left_steps, left_waiting_steps, waiting_steps, max_waiting_steps),
        lambda torch, name: torch.int32 if name in _MOVEMENT_FLOW_INT32 else torch.int64, lambda: _movement_flow_shape(self),
        self._movement_flow_tracking, "movement-flow tracking is off (track_movement_flow(True) turns it on)",
        lambda: observe_movement_flow_array(self, reset=reset), self._observe_movement_flow_device, (bool(reset),))


def observe_movement_flow_array(self, reset=False):
    """The eight outputs of observe_movement_flow_tensor as a dict of numpy arrays (same names, dtypes and shapes); waits for
    the device.  RuntimeError while tracking is off."""
    if not self._movement_flow_tracking():
        raise RuntimeError("observe_movement_flow_array: movement-flow tracking is off (track_movement_flow(True) turns it on)")
    shape = _movement_flow_shape(self)
    return {name: a.reshape(shape) for name, a in zip(MOVEMENT_FLOW_OUTPUTS, self._movement_flow_features(bool(reset)))}


TRIP_OUTPUTS = ("entered", "admitted", "admitted_buffer_steps", "finished", "finished_travel_steps", "in_system", "buffered",
                "in_system_travel_steps", "average_travel_time")
_TRIP_INT64 = ("admitted_buffer_steps", "finished_travel_steps", "in_system_travel_steps")


def _trip_dtype(torch, name):
    return torch.float64 if name == "average_travel_time" else torch.int64 if name in _TRIP_INT64 else torch.int32


TRIP_LOG_MAX_CAPACITY = 1 << 26


def track_trips(self, on=True, log=None):
    """Turn the trip tracker on or off (off by default: nothing is allocated or launched, and it frees its memory when turned
    off).  While it is on, every next_step() ends with one tracker update (one extra kernel launch on the HIP engine).
    Turning it on takes a baseline: the five accumulators are zero, and the vehicles alive then are in in_system / buffered /
    in_system_travel_steps with their true enter times without being counted as entered (they count as admitted or finished
    when that happens); reset(), load() and load_from_file() take a new baseline and keep it on.  Not with laneChange
    (NotImplementedError).

    log: the trip LOG, one row per finished vehicle (observe_trip_log_tensor), off by default and off while only the statistics
    are on.  log=N (1 <= N <= 2**26, 32 bytes of device memory per row) turns it on with room for N rows, or replaces the log
    there by an empty one; log=0 drops it; None leaves it as it is.  Changing `log` while tracking is on does not touch the
    accumulators.  Turning tracking off drops the log; with on=False only None or 0 make sense.  ValueError for a capacity that
    is no integer in [0, 2**26], before anything is changed."""
    import numbers

    if log is not None:
        if isinstance(log, bool) or not isinstance(log, numbers.Integral) or not 0 <= int(log) <= TRIP_LOG_MAX_CAPACITY:
            raise ValueError("track_trips: log must be an integer in [0, %d] or None, not %r" % (TRIP_LOG_MAX_CAPACITY, log))
        if not on and int(log) > 0:
            raise ValueError("track_trips: a log needs trip tracking on")
    self._track_trips(bool(on))
    if on and log is not None:
        self._track_trip_log(int(log))


def trip_tracking(self):
    """Whether track_trips is on."""
    return self._trip_tracking()


def observe_trips_tensor(self, entered=None, admitted=None, admitted_buffer_steps=None, finished=None, finished_travel_steps=None,
                         in_system=None, buffered=None, in_system_travel_steps=None, average_travel_time=None):
    """Fill every given tensor with one kernel launch on the engine's stream, ordered against the current torch stream as
    observe_lanes_tensor (no host wait).  Every output is 0-dim on an Engine and [R], one element per environment, on a
    VectorEngine.  s = steps taken, e(v) = the step at which vehicle v was created (enter time / interval).  After every step:

        entered                 int32  vehicles seen for the first time (created, whether or not a lane has admitted them)
        admitted                int32  vehicles that left their first lane's entry buffer and started to run
        admitted_buffer_steps   int64  sum over those of the steps they sat in the buffer, (s - 1) - e(v)
        finished                int32  vehicles that reached the end of their route
        finished_travel_steps   int64  sum over those of (s - 1) - e(v): cumulative travel time / interval
      all five accumulated since the baseline (track_trips; reset(), load(), load_from_file()) and never reset in between — a
      window is the difference of two reads — and, as of the last step,
        in_system               int32  vehicles created and not finished (in an entry buffer or running)
        buffered                int32  those of them still in an entry buffer: on no lane, invisible to the lane observations
        in_system_travel_steps  int64  sum over the vehicles in the system of s - e(v)
        average_travel_time     float64  (finished_travel_steps + in_system_travel_steps) * interval / (finished + in_system),
                                         0.0 without vehicles

    average_travel_time equals get_average_travel_time() (per environment) only while tracking has been on since the engine
    was created or last reset(), and only while no push_vehicle() has happened since the last step: the reference counts a
    pushed vehicle at once, the tracker sees it with the next step.  Seconds = steps * interval.  Every element is written.
    At least one output; every argument is checked before anything is enqueued; RuntimeError while tracking is off."""
    _observe_tracker_tensor(
        self, "observe_trips_tensor", TRIP_OUTPUTS,
        (entered, admitted, admitted_buffer_steps, finished, finished_travel_steps, in_system, buffered, in_system_travel_steps,
         average_travel_time),
        _trip_dtype, lambda: tuple(self._tensor_shapes()[0])[:-1], self._trip_tracking,
        "trip tracking is off (track_trips(True) turns it on)", lambda: observe_trips_array(self), self._observe_trips_device)


def observe_trips_array(self):
    """The nine outputs of observe_trips_tensor as a dict of numpy arrays (same names, dtypes and shapes); waits for the
    device.  RuntimeError while tracking is off."""
    if not self._trip_tracking():
        raise RuntimeError("observe_trips_array: trip tracking is off (track_trips(True) turns it on)")
    shape = tuple(self._tensor_shapes()[0])[:-1]
    return {name: a.reshape(shape) for name, a in zip(TRIP_OUTPUTS, self._trip_features())}


TRIP_LOG_OUTPUTS = ("count", "dropped", "env", "vehicle", "origin_road", "destination_road", "enter_step", "finish_step", "travel_steps")
TRIP_LOG_COLUMNS = TRIP_LOG_OUTPUTS[2:]


def trip_log_capacity(self):
    """The rows the trip log has room for (track_trips(log=N)); 0 while there is no log."""
    return self._trip_log_capacity()


def _require_trip_log(eng, what):
    if not eng._trip_tracking():
        raise RuntimeError(what + ": trip tracking is off (track_trips(True, log=N) turns it and the log on)")
    if eng._trip_log_capacity() <= 0:
        raise RuntimeError(what + ": there is no trip log (track_trips(True, log=N) turns it on)")


def observe_trip_log_tensor(self, count=None, dropped=None, env=None, vehicle=None, origin_road=None, destination_road=None,
                            enter_step=None, finish_step=None, travel_steps=None, reset=False):
    """Drain the trip log into the given tensors with one kernel launch on the engine's stream, ordered against the current
    torch stream as observe_lanes_tensor (no host wait).  The log holds one row per vehicle that finished since the last
    baseline (track_trips; reset(), load(), load_from_file(), rollback()) or the last call with reset=True: the event that adds
    1 to `finished` of observe_trips_tensor.  All int32 on the engine's device; N = trip_log_capacity():

        count             0-dim  rows held, at most N
        dropped           0-dim  rows that found the log full and were dropped (the trip statistics still counted them)
        env               [N]    the vehicle's environment (0 on an Engine; ONE log serves all environments of a VectorEngine)
        vehicle           [N]    its vehicle number when it finished, as observe_vehicles_tensor showed it.  After a vehicle
                                 compaction a number may be in use again; rows keep the number they were logged with
        origin_road       [N]    first road of the route it held when it finished, an index into road_ids()
        destination_road  [N]    last road of that route.  set_vehicle_route() replaces a vehicle's route from the road it is
                                 on: such a vehicle's origin_road is the first road of the NEW route
        enter_step        [N]    e(v), the step at which it was created (enter time / interval)
        finish_step       [N]    s, the steps taken when it was found finished
        travel_steps      [N]    (s - 1) - e(v): what finished_travel_steps got for it; seconds = steps * interval

    Rows are in ascending finish_step; the order of the rows of one step is unspecified and differs from run to run on the
    device (observe_trip_log_array sorts).  Rows at and behind `count` are -1 in every column: every element is written.
    reset=True empties the log and zeroes `dropped` after the copy, in stream order.  At least one output; every argument is
    checked before anything is enqueued; RuntimeError while tracking is off or there is no log.  Returns a dict of the tensors
    that were given."""
    torch = _torch()
    given = dict(zip(TRIP_LOG_OUTPUTS, (count, dropped, env, vehicle, origin_road, destination_road, enter_step, finish_step, travel_steps)))
    if all(t is None for t in given.values()):
        raise ValueError("observe_trip_log_tensor: give at least one of " + ", ".join(TRIP_LOG_OUTPUTS))
    _require_trip_log(self, "observe_trip_log_tensor")
    device = _engine_device(torch, self)
    cap = self._trip_log_capacity()
    for name, t in given.items():
        if t is not None:
            _check_buf(torch, t, name, () if name in ("count", "dropped") else (cap,), torch.int32, device)
    if not self._device_buffers():  # (the twin: over the array call's raw columns)
        for name, a in zip(TRIP_LOG_OUTPUTS, self._trip_log_features(bool(reset))):
            if given[name] is not None:
                given[name].copy_(torch.from_numpy(a).reshape(given[name].shape))
    else:
        self._observe_trip_log_device(*[0 if given[name] is None else given[name].data_ptr() for name in TRIP_LOG_OUTPUTS],
                                      bool(reset), torch.cuda.current_stream(device).cuda_stream)
    return {name: t for name, t in given.items() if t is not None}


def observe_trip_log_array(self, reset=False):
    """The trip log as a dict of numpy int32 columns (the seven columns of observe_trip_log_tensor, trimmed to the rows held)
    plus "dropped" as an int; waits for the device.  The rows are sorted by (finish_step, env, vehicle), so two runs give equal
    arrays.  reset=True empties the log.  RuntimeError while tracking is off or there is no log."""
    import numpy as np

    _require_trip_log(self, "observe_trip_log_array")
    raw = dict(zip(TRIP_LOG_OUTPUTS, self._trip_log_features(bool(reset))))
    n = int(raw["count"][0])
    cols = {name: raw[name][:n] for name in TRIP_LOG_COLUMNS}
    order = np.lexsort((cols["vehicle"], cols["env"], cols["finish_step"]))
    out = {name: np.ascontiguousarray(a[order]) for name, a in cols.items()}
    out["dropped"] = int(raw["dropped"][0])
    return out


def get_average_travel_time_tensor(self, out=None):
    """The average_travel_time output of observe_trips_tensor alone: float64, 0-dim ([R] on a VectorEngine), into `out` or a
    new tensor; no host wait on the HIP engine.  It equals get_average_travel_time() only while tracking has been on since the
    engine's creation or last reset() and no push_vehicle() has happened since the last step (observe_trips_tensor)."""
    torch = _torch()
    if out is None:
        out = torch.empty(tuple(self._tensor_shapes()[0])[:-1], dtype=torch.float64, device=_engine_device(torch, self))
    observe_trips_tensor(self, average_travel_time=out)
    return out


DETECTOR_OUTPUTS = ("passed", "occupied_steps", "vehicle_steps", "waiting_vehicle_steps", "speed_sum", "count")
_DETECTOR_INT64 = ("vehicle_steps", "waiting_vehicle_steps")


def _detector_dtype(torch, name):
    return torch.float64 if name == "speed_sum" else torch.int64 if name in _DETECTOR_INT64 else torch.int32


def _detector_lanes(lane):
    """`lane` of track_detectors as a list of ints: TypeError for anything that is not a sequence or array of integers (a bool
    and a float are not)."""
    import numbers

    dtype = getattr(lane, "dtype", None)
    if dtype is not None:  # (numpy array, CPU tensor: judged by its dtype, an empty one too)
        kind = getattr(dtype, "kind", None)
        if kind is None:  # a torch dtype
            if dtype.is_floating_point or dtype.is_complex or str(dtype) == "torch.bool":
                raise TypeError("track_detectors: lane must hold integers, not %s" % (dtype,))
        elif kind not in "iu":
            raise TypeError("track_detectors: lane must hold integers, not %s" % (dtype,))
    if hasattr(lane, "tolist"):
        lane = lane.tolist()
    if isinstance(lane, (str, bytes)) or not hasattr(lane, "__len__") or not hasattr(lane, "__iter__"):
        raise TypeError("track_detectors: lane must be a sequence of integers, not %s" % type(lane).__name__)
    lane = list(lane)
    for i, l in enumerate(lane):
        if isinstance(l, bool) or type(l).__name__ == "bool_" or not isinstance(l, numbers.Integral):
            raise TypeError("track_detectors: lane[%d] = %r is not an integer" % (i, l))
    return [int(l) for l in lane]


def _detector_edges(a, name):
    """`start` / `end` of track_detectors as a list of floats: TypeError for anything that is not a sequence or array of real
    numbers."""
    import numbers

    if hasattr(a, "tolist"):
        a = a.tolist()
    if isinstance(a, (str, bytes)) or not hasattr(a, "__len__") or not hasattr(a, "__iter__"):
        raise TypeError("track_detectors: %s must be a sequence of floats, not %s" % (name, type(a).__name__))
    a = list(a)
    for i, x in enumerate(a):
        if isinstance(x, bool) or type(x).__name__ == "bool_" or not isinstance(x, numbers.Real):
            raise TypeError("track_detectors: %s[%d] = %r is not a number" % (name, i, x))
    return [float(x) for x in a]


def track_detectors(self, lane=None, start=None, end=None, on=True):
    """Define N virtual loop detectors and turn the detector tracker on (off by default: nothing is allocated or launched), or,
    with on=False, turn it off and free everything.  Detector d is the zone start[d] <= distance < end[d] of lane lane[d]:

        lane   integer sequence or array [N]  indices into lane_ids()
        start  floating [N]                   metres from the lane's start, on the scale of get_vehicle_distance()
        end    floating [N]                   likewise; +inf, or anything beyond the lane's length: the zone reaches to the lane's end

    A detector sees a vehicle's FRONT position only — the project's `distance`; vehicle length is ignored.  Any number of
    detectors per lane, and they may overlap; lanes without one cost nothing.  VectorEngine: the set is one environment's (lane <
    L) and every environment gets it.  While the tracker is on, every next_step() ends with one tracker update (one extra
    kernel launch on the HIP engine, over the lanes that have a detector).  Defining takes a baseline — nothing is counted,
    the accumulators are zero, `count` is as of now, and every vehicle then on a lane counts as having been there, at its
    current distance, at the previous update; so do reset(), load(), load_from_file() and rollback(), which keep the tracker
    on.  Calling it again while it is on replaces the set and takes a new baseline.  Vehicle compaction does not show.

    Every argument is checked before anything changes, in this order: a bool or a float in `lane` (TypeError); unequal lengths
    or N = 0 (ValueError); then lane in [0, L), start finite and >= 0, end > start, no NaN (ValueError naming the position).
    Not with laneChange (NotImplementedError)."""
    if not on:
        self._drop_detectors()
        return
    if lane is None and start is None and end is None:
        if self._detector_tracking():
            return
        raise ValueError("track_detectors: give lane, start and end (the tracker is off and has no detectors)")
    if lane is None or start is None or end is None:
        raise ValueError("track_detectors: lane, start and end come together")
    import math

    import numpy as np

    lane = _detector_lanes(lane)
    start = _detector_edges(start, "start")
    end = _detector_edges(end, "end")
    if not len(lane) == len(start) == len(end):
        raise ValueError("track_detectors: lane, start and end must have one length, not %d, %d and %d" % (len(lane), len(start), len(end)))
    if not lane:
        raise ValueError("track_detectors: at least one detector")
    n_lanes = tuple(self._tensor_shapes()[0])[-1]
    for i, (l, a, b) in enumerate(zip(lane, start, end)):
        if not 0 <= l < n_lanes:
            raise ValueError("track_detectors: lane[%d] = %d is not an index into lane_ids() (position %d; valid: 0 .. %d)" % (i, l, i, n_lanes - 1))
        if not (math.isfinite(a) and a >= 0.0):
            raise ValueError("track_detectors: start[%d] = %r is not finite and >= 0 (position %d)" % (i, a, i))
        if not b > a:
            raise ValueError("track_detectors: end[%d] = %r is not beyond start[%d] = %r (position %d)" % (i, b, i, a, i))
    self._define_detectors(np.asarray(lane, dtype=np.int32), np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64))


def detector_tracking(self):
    """Whether track_detectors is on."""
    return self._detector_tracking()


def detector_layout(self):
    """The detectors in force as they were defined, of ONE environment, as numpy arrays (host only): {"lane": int32 [N],
    "start": float64 [N], "end": float64 [N]}.  RuntimeError while tracking is off."""
    if not self._detector_tracking():
        raise RuntimeError("detector_layout: detector tracking is off (track_detectors(lane, start, end) turns it on)")
    return dict(zip(("lane", "start", "end"), self._detector_layout()))


def _detector_shape(eng, what):
    """[N] ([R, N] on a VectorEngine).  (While tracking is off there is no N to check a buffer against: RuntimeError here.)"""
    if not eng._detector_tracking():
        raise RuntimeError(what + ": detector tracking is off (track_detectors(lane, start, end) turns it on)")
    return tuple(eng._tensor_shapes()[0])[:-1] + (eng._detector_count(),)


def observe_detectors_tensor(self, passed=None, occupied_steps=None, vehicle_steps=None, waiting_vehicle_steps=None, speed_sum=None,
                             count=None, reset=False):
    """Fill every given tensor with one kernel launch on the engine's stream, ordered against the current torch stream as
    observe_lanes_tensor (no host wait).  Detectors in the order of track_detectors (detector_layout()); a detector sees a
    vehicle's front position only (vehicle length is ignored).  For detector d = (l, start, end): on(l) = the vehicles
    get_lane_vehicles() lists on lane l, front to back; dis(v), speed(v) as get_vehicle_distance() / get_vehicle_speed();
    dis'(v) = dis(v) after the previous step if v was on l then; "in the zone" = start <= dis(v) < end.  After every step:

        passed                 int32 [N]    +1 for every v on l with dis(v) >= start that was not on l before or had       \\
                                            dis'(v) < start; +1 for every v that was on l with dis'(v) < start and has left   |
                                            l (it went over the rest of the lane in one step)                                 | accumulated
        occupied_steps         int32 [N]    +1 if at least one vehicle is in the zone                                       | since the last
        vehicle_steps          int64 [N]    + the vehicles in the zone                                                      | call with
        waiting_vehicle_steps  int64 [N]    + those of them with speed < 0.1 (as get_lane_waiting_vehicle_count)            | reset=True, or
        speed_sum              float64 [N]  + t, the zone's speeds added front to back in one running float64 — as            | the baseline
                                            get_lane_speed_sum_tensor sums a lane; the order is part of the definition      /
        count                  int32 [N]    now: the vehicles in the zone

    Derived: occupancy = occupied_steps / steps since the reset; space-mean speed = speed_sum / vehicle_steps; a detector
    (l, 0, inf) gives passed = `entered` of track_lane_flow and count = the lane's vehicle count.  reset=True zeroes the five
    accumulators in the same launch, after they were read — all five, whether or not they were asked for.  Every element is
    written.  VectorEngine: a leading [R] on every output.  At least one output; every argument is checked before anything is
    enqueued; RuntimeError while tracking is off."""
    _observe_tracker_tensor(
        self, "observe_detectors_tensor", DETECTOR_OUTPUTS,
        (passed, occupied_steps, vehicle_steps, waiting_vehicle_steps, speed_sum, count), _detector_dtype,
        lambda: _detector_shape(self, "observe_detectors_tensor"), self._detector_tracking,
        "detector tracking is off (track_detectors(lane, start, end) turns it on)",
        lambda: observe_detectors_array(self, reset=reset), self._observe_detectors_device, (bool(reset),))


def observe_detectors_array(self, reset=False):
    """The six outputs of observe_detectors_tensor as a dict of numpy arrays (same names, dtypes and shapes); waits for the
    device.  RuntimeError while tracking is off."""
    shape = _detector_shape(self, "observe_detectors_array")
    return {name: a.reshape(shape) for name, a in zip(DETECTOR_OUTPUTS, self._detector_features(bool(reset)))}


def _plan_shapes(eng):
    """(shape of durations [.., I, P], shape of phase / phase_remain [.., I])."""
    lead = tuple(eng._tensor_shapes()[1])
    return lead + (eng._intersection_dims()[1],), lead


def _need_plan_calls(eng, what):
    if not eng._tl_plan_calls():
        raise NotImplementedError("%s: the backend %r does not keep the signal plan as engine state" % (what, eng.backend_name()))


def set_tl_plan_tensor(self, durations=None, phase=None, phase_remain=None):
    """Set the fixed-time signal plan — each phase's green time, and where every intersection stands in its cycle — from tensors
    on the engine's device, with one kernel launch on the engine's stream, read after everything enqueued on the current torch
    stream (no host wait).  I, P and P_i as in observe_intersections_tensor / intersection_layout().  At least one of:

        durations     float64 [I, P]  seconds of phase p of intersection i; NaN keeps the entry.  Entries p >= P_i and every row
                                      of a virtual intersection are ignored.  A new duration takes effect the next time the phase
                                      is entered: the running phase keeps its remaining time unless phase_remain says otherwise
                                      — what the reference would do if LightPhase::time were changed between two steps
        phase         integer [I]     the current phase; -1 keeps it.  Allowed whatever rlTrafficLight is; the remaining time is
                                      not touched
        phase_remain  float64 [I]     seconds the current phase still has; NaN keeps the value

    The whole call is validated on the device before anything is applied.  At every intersection that is not virtual: every
    given duration is finite and >= 0; the durations that would be in force after the call sum to at least the step interval
    over p < P_i (a cycle of no length would never let the lights' advance end); phase is in [-1, P_i); phase_remain is finite
    and >= 0.  One invalid entry rejects the WHOLE call — nothing is applied, valid rows and the other arguments included — and
    the next call that waits for the device (sync(), a getter that reads to the host, snapshot, reset) raises ValueError naming
    the argument, the intersection (the phase index, the env) and saying that the call was not applied.

    The durations in force belong to the engine, like the roadnet: reset() keeps them (its lights go to phase 0 with the
    remaining time durations[i, 0] in force), snapshot / load / load_from_file and vehicle compaction neither save nor change
    them (an Archive carries the phase and the remaining time only); restore_tl_plan() brings the roadnet file's back.  With
    rlTrafficLight the lights do not advance, so durations matter to reset() alone.  VectorEngine: a leading [R] on every
    argument — one plan per environment.  Every argument is checked before anything is enqueued; NotImplementedError on a
    backend without the call (the CPU twin)."""
    torch = _torch()
    if durations is None and phase is None and phase_remain is None:
        raise ValueError("set_tl_plan_tensor: give at least one of durations, phase, phase_remain")
    d_shape, i_shape = _plan_shapes(self)
    device = _engine_device(torch, self)
    if durations is not None:
        _check_buf(torch, durations, "durations", d_shape, torch.float64, device)
    if phase is not None:
        _check_phases(torch, phase, i_shape, device)
        if not phase.is_contiguous():
            raise ValueError("phase must be contiguous")
    if phase_remain is not None:
        _check_buf(torch, phase_remain, "phase_remain", i_shape, torch.float64, device)
    _need_plan_calls(self, "set_tl_plan_tensor")
    p = phase
    if p is not None and p.dtype != torch.int32:  # (values beyond int32 stay invalid instead of wrapping into range)
        p = p.to(torch.int64).clamp(-2, 2 ** 31 - 1).to(torch.int32)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    self._set_tl_plan_device(ptr(durations), ptr(p), ptr(phase_remain), torch.cuda.current_stream(device).cuda_stream)


def get_tl_phase_durations_tensor(self, out=None):
    """The phase durations in force as a float64 tensor [I, P] ([R, I, P] on a VectorEngine) on the engine's device, valid on the
    current torch stream (no host wait): the reading side of set_tl_plan_tensor's `durations`.  0.0 for p >= P_i and in every row
    of a virtual intersection; every element is written.  `out`: a contiguous float64 tensor of that shape, filled in place.
    (The current phase and its remaining time are observe_intersections_tensor's phase / phase_remain.)"""
    torch = _torch()
    shape = _plan_shapes(self)[0]
    device = _engine_device(torch, self)
    if out is not None:
        _check_buf(torch, out, "out", shape, torch.float64, device)
    _need_plan_calls(self, "get_tl_phase_durations_tensor")
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=device)
    self._tl_phase_durations_device(out.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    return out


def _plan_array(a, name, shape, dtype):
    import numpy as np

    if a is None:
        return None
    a = np.asarray(a)
    if dtype == np.int32:
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise TypeError("%s must be an integer array, not %s" % (name, a.dtype))
        a = np.clip(a.astype(np.int64), -2, 2 ** 31 - 1)
    elif not np.issubdtype(a.dtype, np.floating):
        raise TypeError("%s must be a floating array, not %s" % (name, a.dtype))
    if tuple(a.shape) != shape:
        raise ValueError("%s must have shape %s, not %s" % (name, shape, tuple(a.shape)))
    return np.ascontiguousarray(a, dtype=dtype)


def set_tl_plan(self, durations=None, phase=None, phase_remain=None):
    """set_tl_plan_tensor from numpy arrays (same shapes, rules and validation).  Waits for the device: an invalid entry raises
    ValueError at once, and nothing was applied."""
    import numpy as np

    if durations is None and phase is None and phase_remain is None:
        raise ValueError("set_tl_plan: give at least one of durations, phase, phase_remain")
    d_shape, i_shape = _plan_shapes(self)
    durations = _plan_array(durations, "durations", d_shape, np.float64)
    phase = _plan_array(phase, "phase", i_shape, np.int32)
    phase_remain = _plan_array(phase_remain, "phase_remain", i_shape, np.float64)
    _need_plan_calls(self, "set_tl_plan")
    self._set_tl_plan(durations, phase, phase_remain)


def get_tl_phase_durations_array(self):
    """get_tl_phase_durations_tensor as a numpy array; waits for the device."""
    _need_plan_calls(self, "get_tl_phase_durations_array")
    return self._tl_phase_durations().reshape(_plan_shapes(self)[0])


def restore_tl_plan(self):
    """Put the roadnet file's phase durations back in force, for every environment; the current phases and remaining times
    stay as they are.  Ordered on the engine's stream, no host wait."""
    _need_plan_calls(self, "restore_tl_plan")
    self._restore_tl_plan()


def _lane_limit_shape(eng):
    return tuple(eng._tensor_shapes()[0])


def _need_lane_limit_calls(eng, what):
    if not eng._lane_limit_calls():
        raise NotImplementedError("%s: the backend %r does not keep the lanes' speed limits as engine state"
                                  % (what, eng.backend_name()))


def set_lane_speed_limits_tensor(self, limits, rejected=None):
    """Set the lanes' speed limits (Lane::maxSpeed) from a float64 tensor [L] ([R, L] on a VectorEngine: one scheme per
    environment) in lane_ids() order on the engine's device, read after everything enqueued on the current torch stream.  One
    kernel launch on the engine's stream (and a 4-byte fill ahead of it where `rejected` is given); the call never waits for the
    host and allocates nothing.  Entry by entry:

        NaN                    keeps the lane's limit
        finite and >= 0        applied bit for bit; 0.0 closes the lane; values above 30 are allowed (the reference only warns)
        negative or infinite   not applied, counted in `rejected`; the other entries of the call are applied

    `rejected`: an optional int32 [1] tensor on the engine's device, set to this call's count and valid on the current torch
    stream.  A new limit takes effect in the next next_step() for every vehicle then on the lane — what the reference would do
    if Lane::maxSpeed were changed between two steps.  It caps the speed the step computes and is no deceleration: a vehicle
    that moves onto a slower lane during a step can hold a higher speed for that one step.  LaneLinks keep the reference's 10000.

    The limits belong to the engine, like the roadnet: reset() keeps them; snapshot / load / load_from_file, vehicle compaction,
    checkpoint() / rollback() (with envs too: every slot keeps its own) neither save nor change them — read them with
    get_lane_speed_limits_tensor() and set them again to carry them over; restore_lane_speed_limits() brings the roadnet
    file's back.  Every argument is checked before anything is enqueued; NotImplementedError on a backend without the call
    (the CPU twin)."""
    torch = _torch()
    shape = _lane_limit_shape(self)
    device = _engine_device(torch, self)
    _check_buf(torch, limits, "limits", shape, torch.float64, device)
    if rejected is not None:
        _check_buf(torch, rejected, "rejected", (1,), torch.int32, device)
    _need_lane_limit_calls(self, "set_lane_speed_limits_tensor")
    self._set_lane_speed_limits_device(limits.data_ptr(), 0 if rejected is None else rejected.data_ptr(),
                                       torch.cuda.current_stream(device).cuda_stream)


def get_lane_speed_limits_tensor(self, out=None):
    """The lanes' speed limits in force as a float64 tensor [L] ([R, L] on a VectorEngine) on the engine's device, valid on the
    current torch stream (no host wait): the reading side of set_lane_speed_limits_tensor.  Every element is written.  `out`: a
    contiguous float64 tensor of that shape, filled in place."""
    torch = _torch()
    shape = _lane_limit_shape(self)
    device = _engine_device(torch, self)
    if out is not None:
        _check_buf(torch, out, "out", shape, torch.float64, device)
    _need_lane_limit_calls(self, "get_lane_speed_limits_tensor")
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=device)
    self._lane_speed_limits_device(out.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    return out


def set_lane_speed_limits(self, limits):
    """set_lane_speed_limits_tensor from a numpy array (same shape and rules), through the engine's staging arena.  Waits for
    the device and returns the number of rejected entries."""
    import numpy as np

    limits = _plan_array(limits, "limits", _lane_limit_shape(self), np.float64)
    if limits is None:
        raise TypeError("limits must be a floating array, not None")
    _need_lane_limit_calls(self, "set_lane_speed_limits")
    return int(self._set_lane_speed_limits(limits))


def get_lane_speed_limits_array(self):
    """get_lane_speed_limits_tensor as a numpy array; waits for the device."""
    _need_lane_limit_calls(self, "get_lane_speed_limits_array")
    return self._lane_speed_limits().reshape(_lane_limit_shape(self))


def restore_lane_speed_limits(self):
    """Put the roadnet file's speed limits back in force, for every environment.  Ordered on the engine's stream, no host
    wait."""
    _need_lane_limit_calls(self, "restore_lane_speed_limits")
    self._restore_lane_speed_limits()


def _need_checkpoint_calls(eng, what):
    why = eng._checkpoint_unsupported()
    if why:
        raise NotImplementedError("%s: %s" % (what, why))


def checkpoint(self, into=None):
    """The whole simulation state as a DeviceCheckpoint held in device memory: every running and waiting vehicle, the lights'
    phases and remaining times, the counters, Lane::history where it is kept, and the spawners' state on the host — what
    `snapshot()` puts into an Archive, without any of it crossing the link.  `into`: a checkpoint of this engine that has not
    been released, overwritten in place (its memory is reused while it is large enough).  Ordered on the engine's stream; waits
    for the device once.  Needs neither torch nor numpy.  The durations set by set_tl_plan_tensor are the engine's, not the
    checkpoint's.  The ring layout only — NotImplementedError with laneChange, on the dense layout and on a backend without
    the call (the CPU twin); ValueError for a checkpoint of another engine or a released one."""
    _need_checkpoint_calls(self, "checkpoint")
    return self._checkpoint(into)


def rollback(self, checkpoint):
    """Return to the state `checkpoint` holds, as `load(snapshot())` would — except that the vehicles keep their place in their
    routes (get_vehicle_info's route), so the run continues bit for bit as if it had never left that state.  The checkpoint is
    not consumed: roll back to it as often as needed ("roll back, try the next plan").  It stays valid across ring and table
    growth, vehicle compaction and reset().  Trackers (track_lane_flow, track_movement_flow, track_trips) take a new baseline
    and stay on, as after load().  ValueError for a checkpoint of another engine or a released one."""
    _need_checkpoint_calls(self, "rollback")
    self._rollback(checkpoint)


def _env_map(envs, num_envs):
    """`envs` of VectorEngine.rollback as a list of ints: the type of every entry first, then the length, then the range."""
    import numbers

    device = getattr(envs, "device", None)
    if device is not None and getattr(device, "type", "cpu") != "cpu":
        raise TypeError("rollback: envs is a host argument (the spawners' states are copied by it) and a tensor on %s would be "
                        "read with a silent wait for the device: pass envs.tolist()" % (device,))
    if hasattr(envs, "tolist"):  # (numpy array, CPU tensor: Python scalars from here on)
        envs = envs.tolist()
    if isinstance(envs, (str, bytes)) or not hasattr(envs, "__len__") or not hasattr(envs, "__iter__"):
        raise TypeError("rollback: envs must be a sequence of num_envs ints, not %s" % type(envs).__name__)
    envs = list(envs)
    for r, s in enumerate(envs):
        if isinstance(s, bool) or type(s).__name__ == "bool_" or not isinstance(s, numbers.Integral):
            raise TypeError("rollback: envs[%d] = %r is not an integer" % (r, s))
    if len(envs) != num_envs:
        raise ValueError("rollback: envs must hold num_envs = %d entries, not %d" % (num_envs, len(envs)))
    for r, s in enumerate(envs):
        if not 0 <= s < num_envs:
            raise ValueError("rollback: envs[%d] = %d is not an environment (position %d; valid: 0 .. %d)" % (r, s, r, num_envs - 1))
    return [int(s) for s in envs]


def rollback_envs(self, checkpoint, envs=None):
    """rollback(checkpoint) of a VectorEngine, with `envs` a gathered one: afterwards environment r is in the state that
    environment envs[r] had when `checkpoint` was saved.  `envs`: a sequence or integer numpy array (or CPU tensor) of num_envs
    values in [0, num_envs); repeats are allowed, an environment named nowhere is dropped — "keep the best k, continue all R from
    them".  envs=None is the plain rollback, on its own code path.

    Environment r takes from envs[r]: its running vehicles (position, speed, place in the route, the leader and gap of the first
    step, a custom speed and its pending flag), its entry buffers in queue order, every intersection's phase and remaining time,
    Lane::history where the engine keeps it, and its spawner's state with the mt19937 — so r continues bit for bit as envs[r]
    would have, with per-environment seeds as with equal ones.  The durations set by set_tl_plan_tensor stay slot r's own, as in
    a plain rollback: replicate the survivors' states, then give every slot its next candidate plan.  As in a plain rollback the
    trackers take a new baseline and stay on, pending set_tl_phases calls are dropped and the step becomes the checkpoint's.  The
    engine-wide counts of running and finished vehicles are those of the environments taken; _scalars()'s cumulative_travel_time
    and vehicle_steps, which nothing splits by environment, stay the checkpoint's totals (per-environment travel times are
    track_trips').  Vehicle ids stay the source's (two slots that took one state hold vehicles of the same ids).

    The checkpoint is neither consumed nor modified: any number of maps, and envs=None afterwards.  `envs` is a host argument
    (the spawners' states are copied on the host): a tensor on a device is a TypeError that says to pass .tolist(); nothing here
    waits for the device unseen.  Checked first, in this order: an entry that is not an integer (bools included) TypeError, a
    wrong length ValueError, an entry out of range ValueError naming the position; then rollback's own checks."""
    if envs is None:
        return rollback(self, checkpoint)
    envs = _env_map(envs, self.num_envs)
    _need_checkpoint_calls(self, "rollback")
    self._rollback_envs(checkpoint, envs)


rollback_envs.__name__ = rollback_envs.__qualname__ = "rollback"  # (VectorEngine.rollback)


VEHICLE_ROW_TILE = 256  # kRowTile: drivables per scan tile of the vehicle-row kernels
VEHICLE_ROW_OUTPUTS = ("vehicle", "drivable", "env", "distance", "speed", "leader", "gap")
VEHICLE_ROW_PADDING = {"vehicle": -1, "drivable": -1, "env": -1, "distance": -1.0, "speed": 0.0, "leader": -1, "gap": 0.0}
VEHICLE_POSE_OUTPUTS = ("x", "y", "dir_x", "dir_y", "length", "width")  # all float64
VEHICLE_POSE_PADDING = {"x": float("nan"), "y": float("nan"), "dir_x": 0.0, "dir_y": 0.0, "length": 0.0, "width": 0.0}
VEHICLE_ROW_PADDING.update(VEHICLE_POSE_PADDING)
_VEHICLE_ROW_FLOATS = ("distance", "speed", "gap") + VEHICLE_POSE_OUTPUTS


def _vehicle_rows(eng, poses=False):
    """The array form: {name: numpy array} of `start`, `count` and the seven row outputs (with `poses`: and the six pose
    outputs) with exactly `count` rows."""
    import numpy as np

    if eng._lane_change():
        raise RuntimeError("observe_vehicles: not with laneChange (a shadow is a second row of its vehicle)")
    lanes, links = eng._drivable_counts()
    lead = tuple(eng._tensor_shapes()[0])[:-1]
    got = eng._vehicle_rows(True) if poses else eng._vehicle_rows()
    out = {"start": got[0].reshape(lead + (lanes + links + 1,)), "count": np.array(got[1], dtype=np.int32)}
    out.update(zip(VEHICLE_ROW_OUTPUTS + (VEHICLE_POSE_OUTPUTS if poses else ()), got[2:]))
    return out


def observe_vehicles_array(self, poses=False):
    """The outputs of observe_vehicles_tensor as a dict of numpy arrays (same names and dtypes): `start`, `count` (0-dim) and
    the seven row outputs with exactly `count` rows, so no padding; with poses=True also `x`, `y`, `dir_x`, `dir_y`, `length`
    and `width`, computed on the host.  Waits for the device.  RuntimeError with laneChange."""
    return _vehicle_rows(self, poses)


def drivable_geometry(self):
    """The polylines the pose outputs of observe_vehicles_tensor walk: {"point_start": int32 [D+1], "points": float64 [P, 2]}.
    Drivable d — the `drivable` column's numbering: lane_ids() first, then the laneLinks — has the points
    points[point_start[d]:point_start[d+1]], at least two, exactly the doubles the loader computed (a lane: the road's points
    moved sideways; a laneLink: the roadnet file's points or the generated curve).  A VectorEngine returns one copy: its
    environments share the roadnet."""
    start, xy = self._drivable_geometry()
    return {"point_start": start, "points": xy.reshape(-1, 2)}


def observe_vehicles_tensor(self, start=None, count=None, vehicle=None, drivable=None, env=None, distance=None, speed=None,
                            leader=None, gap=None, x=None, y=None, dir_x=None, dir_y=None, length=None, width=None):
    """Every running vehicle — on a lane or on a laneLink inside an intersection — as one row of the given tensors, in CSR
    form, filled by two kernel launches on the engine's stream, ordered against the current torch stream as
    observe_lanes_tensor.  D = L + K drivables per environment: 0 .. L-1 are lane_ids(), L .. L+K-1 the laneLinks.

    Row order: by drivable, front to back inside one (nearest the drivable's end first, the order of get_lane_vehicles()).
    VectorEngine: environment-major — environment 0's lanes, then its laneLinks, then environment 1's — so an environment's
    vehicles are one contiguous run of rows.

        start     int32 [D+1] ([R, D+1])  start[d]: row of the first vehicle of drivable d; start[D]: one past the last
                                          (start[r, D] == start[r+1, 0]).  The true offsets even when the rows are too short.
        count     int32 0-dim             the true number of running vehicles

    and the row outputs, all [N] with ONE N >= 0 of the caller's choosing:

        vehicle   int32    the engine's vehicle number (Engine._vehicle_id(n) names it; unique across the environments of a
                           VectorEngine).  It stays the vehicle's while it lives and the numbers are not assigned anew
                           (reset, load, rollback, a vehicle compaction)                                      padding -1
        drivable  int32    index in [0, D) within its environment                                             padding -1
        env       int32    environment (0 on an Engine)                                                       padding -1
        distance  float64  as get_vehicle_distance()                                                          padding -1.0
        speed     float64  as get_vehicle_speed()                                                             padding 0.0
        leader    int32    vehicle number of the leader (get_leader()), -1 if none                            padding -1
        gap       float64  the gap to the leader, 0.0 where leader is -1; a vehicle not stepped since a load
                           reports the loaded state's gap                                                     padding 0.0

    and the POSE outputs, float64 [N] with the same N, where the vehicle is in the plane:

        x, y          float64  the point at `distance` along the drivable's polyline (drivable_geometry()): what the replay
                               file writes for the vehicle, to the bit                                        padding NaN
        dir_x, dir_y  float64  the unit vector of the polyline's segment there (the last one beyond the end)  padding 0.0
        length, width float64  of the vehicle (its flow's or push_vehicle's "length" and "width")             padding 0.0

    No heading angle is produced: a device atan2 is not the host libm's, so it could not equal the replay file's angle to the
    bit; torch.atan2(dir_y, dir_x) is the caller's to make.  A polyline whose last segment has length zero gives NaN in
    dir_x and dir_y of a vehicle at its end, as on the host.  The first call that asks for a pose output uploads the polylines, once
    per engine (that call waits for the copy); a call without them launches exactly what it did before they existed.

    Row i < min(count, N) is vehicle i; rows from count to N hold the padding; every element of every given tensor is
    written.  If count > N the rows beyond N are dropped and nothing is written outside a tensor.  The call never waits for
    the device, which is why N is the caller's and count stays on the device: size N once, e.g. from get_vehicle_count() with
    head room.  The leader is looked for only if leader or gap is given.

    At least one output (start and / or count alone are allowed); every argument is checked before anything is enqueued.  A
    backend without device buffers takes CPU tensors and fills them from observe_vehicles_array().  RuntimeError with
    laneChange: true (a shadow would be a second row of its vehicle)."""
    torch = _torch()
    rows = dict(zip(VEHICLE_ROW_OUTPUTS + VEHICLE_POSE_OUTPUTS,
                    (vehicle, drivable, env, distance, speed, leader, gap, x, y, dir_x, dir_y, length, width)))
    poses = any(rows[name] is not None for name in VEHICLE_POSE_OUTPUTS)
    if start is None and count is None and all(t is None for t in rows.values()):
        raise ValueError("observe_vehicles_tensor: give at least one of start, count, " +
                         ", ".join(VEHICLE_ROW_OUTPUTS + VEHICLE_POSE_OUTPUTS))
    lanes, links = self._drivable_counts()
    lead = tuple(self._tensor_shapes()[0])[:-1]
    device = _engine_device(torch, self)
    if start is not None:
        _check_buf(torch, start, "start", lead + (lanes + links + 1,), torch.int32, device)
    if count is not None:
        _check_buf(torch, count, "count", (), torch.int32, device)
    n_rows = None
    for name, t in rows.items():
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor, not %s" % (name, type(t).__name__))
        if n_rows is None:
            if t.dim() != 1:
                raise ValueError("%s must have shape [N], not %s" % (name, tuple(t.shape)))
            n_rows = int(t.shape[0])
        _check_buf(torch, t, name, (n_rows,), torch.float64 if name in _VEHICLE_ROW_FLOATS else torch.int32, device)
    if n_rows is not None and n_rows >= 2 ** 31:
        raise ValueError("the row outputs hold fewer than 2**31 rows, not %d" % n_rows)
    if self._lane_change():
        raise RuntimeError("observe_vehicles_tensor: not with laneChange (a shadow is a second row of its vehicle)")
    if not self._device_buffers() or not (self._vehicle_poses_device() if poses else self._vehicle_rows_device()):
        arrays = _vehicle_rows(self, poses)  # (the twin, an older library: over the array call)
        n = int(arrays["count"])
        if start is not None:
            start.copy_(torch.from_numpy(arrays["start"]))
        if count is not None:
            count.copy_(torch.from_numpy(arrays["count"]))
        for name, t in rows.items():
            if t is None:
                continue
            keep = min(n, n_rows)
            t[:keep].copy_(torch.from_numpy(arrays[name][:keep]))
            t[keep:].fill_(VEHICLE_ROW_PADDING[name])
        return
    if not n_rows and start is None and count is None:
        return  # (tensors without an element: nothing to write)
    ptr = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    self._observe_vehicles_device(ptr(start), ptr(count), *[ptr(rows[name]) for name in VEHICLE_ROW_OUTPUTS], n_rows or 0,
                                  torch.cuda.current_stream(device).cuda_stream, *[ptr(rows[name]) for name in VEHICLE_POSE_OUTPUTS])


def set_vehicle_speeds(self, vehicle, speed):
    """The numpy form of set_vehicle_speeds_tensor: `vehicle` int32 [N] vehicle numbers (observe_vehicles_array()'s),
    `speed` float64 [N]; returns the number of rows ignored.  Needs no torch; waits for the device.  On a backend without
    device buffers the host commands the vehicles row by row.  RuntimeError with laneChange."""
    import numpy as np

    for name, a, dtype in (("vehicle", vehicle, np.int32), ("speed", speed, np.float64)):
        if not isinstance(a, np.ndarray):
            raise TypeError("%s must be a numpy array, not %s" % (name, type(a).__name__))
        if a.dtype != dtype:
            raise TypeError("%s must be %s, not %s" % (name, np.dtype(dtype).name, a.dtype))
        if a.ndim != 1:
            raise ValueError("%s must have shape [N], not %s" % (name, a.shape))
        if not a.flags.c_contiguous:
            raise ValueError("%s must be contiguous" % name)
    if vehicle.shape != speed.shape:
        raise ValueError("speed must have shape %s as vehicle, not %s" % (vehicle.shape, speed.shape))
    if vehicle.shape[0] >= 2 ** 31:
        raise ValueError("a call holds fewer than 2**31 rows, not %d" % vehicle.shape[0])
    if self._lane_change():
        raise RuntimeError("set_vehicle_speeds: not with laneChange (the vehicle numbers are observe_vehicles')")
    return int(self._set_vehicle_speeds(vehicle, speed))


def set_vehicle_speeds_tensor(self, vehicle, speed, ignored=None):
    """set_vehicle_speed() for many vehicles at once, from tensors: row i commands the vehicle with the engine's number
    vehicle[i] — the numbers observe_vehicles_tensor() writes — to drive at speed[i] in its next step, and only in that one
    (Vehicle::setCustomSpeed: the speed is taken as it is, negative and infinite values included, and car following may still
    slow the vehicle down further).  A vehicle still in its lane's entry buffer keeps the speed for its first step.

        vehicle   int32   [N]    N >= 0
        speed     float64 [N]    NaN: leave this vehicle alone
        ignored   int32   0-dim  optional output: the rows that named no vehicle to command

        vehicle[i] == -1 (observe_vehicles_tensor's padding) or speed[i] NaN      skipped, not counted
        vehicle[i] < -1, a number not issued yet, a vehicle that has finished      skipped, counted in `ignored`
        a running or waiting vehicle                                               commanded

    A vehicle named by several commanding rows takes the one with the HIGHEST row index (rows with NaN do not compete), so
    the result never depends on the device's scheduling.  Calls take effect in the order they are made, set_vehicle_speed()
    among them: the later call wins.  "Issued" are the numbers as of the last step; a vehicle pushed since has none yet
    (set_vehicle_speed(id, ...) serves it).  On a VectorEngine the numbers are unique across the environments, and one call
    commands vehicles of any of them.  Numbers go stale where observe_vehicles_tensor says they do (reset, load, rollback, a
    vehicle compaction); a compaction also drops a command that a vehicle in an entry buffer has not used yet.

    Two kernel launches on the engine's stream (three on the dense layout), ordered after the current torch stream; the torch
    stream is ordered after them, so `ignored` can be read there and the inputs reused.  The call never waits for the device.
    Every argument is checked before anything is enqueued.  A backend without device buffers takes CPU tensors and goes
    through set_vehicle_speeds().  RuntimeError with laneChange: true."""
    torch = _torch()
    device = _engine_device(torch, self)
    if not isinstance(vehicle, torch.Tensor):
        raise TypeError("vehicle must be a torch.Tensor, not %s" % type(vehicle).__name__)
    if vehicle.dim() != 1:
        raise ValueError("vehicle must have shape [N], not %s" % (tuple(vehicle.shape),))
    n_rows = int(vehicle.shape[0])
    _check_buf(torch, vehicle, "vehicle", (n_rows,), torch.int32, device)
    _check_buf(torch, speed, "speed", (n_rows,), torch.float64, device)
    if ignored is not None:
        _check_buf(torch, ignored, "ignored", (), torch.int32, device)
    if n_rows >= 2 ** 31:
        raise ValueError("a call holds fewer than 2**31 rows, not %d" % n_rows)
    if self._lane_change():
        raise RuntimeError("set_vehicle_speeds_tensor: not with laneChange (the vehicle numbers are observe_vehicles')")
    if not self._device_buffers() or not self._vehicle_speeds_device():  # (the twin, an older library: over the array call)
        count = set_vehicle_speeds(self, vehicle.detach().numpy(), speed.detach().numpy())
        if ignored is not None:
            ignored.fill_(count)
        return
    if n_rows == 0 and ignored is None:
        return
    ptr = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    self._set_vehicle_speeds_device(ptr(vehicle), ptr(speed), n_rows, ptr(ignored), torch.cuda.current_stream(device).cuda_stream)


def _check_rows_array(np, a, name):
    if not isinstance(a, np.ndarray):
        raise TypeError("%s must be a numpy array, not %s" % (name, type(a).__name__))
    if a.dtype != np.int32:
        raise TypeError("%s must be int32, not %s" % (name, a.dtype))
    if a.ndim != 1:
        raise ValueError("%s must have shape [N], not %s" % (name, a.shape))
    if not a.flags.c_contiguous:
        raise ValueError("%s must be contiguous" % name)
    if a.shape[0] >= 2 ** 31:
        raise ValueError("a call holds fewer than 2**31 rows, not %d" % a.shape[0])


def set_vehicle_routes(self, vehicle, route):
    """The numpy form of set_vehicle_routes_tensor: `vehicle` int32 [N] vehicle numbers (observe_vehicles_array()'s), `route`
    int32 [N] route handles; returns (status int32 [N], the number of rows with a negative status).  Needs no torch; waits for
    the device.  RuntimeError with laneChange, and on a backend without the device call."""
    import numpy as np

    _check_rows_array(np, vehicle, "vehicle")
    _check_rows_array(np, route, "route")
    if vehicle.shape != route.shape:
        raise ValueError("route must have shape %s as vehicle, not %s" % (vehicle.shape, route.shape))
    if self._lane_change():
        raise RuntimeError("set_vehicle_routes: not with laneChange (the vehicle numbers are observe_vehicles')")
    status, ignored = self._set_vehicle_routes(vehicle, route)
    return status, int(ignored)


def set_vehicle_routes_tensor(self, vehicle, route, status=None, ignored=None):
    """set_vehicle_route() for many vehicles at once, from tensors: row i gives the vehicle with the engine's number vehicle[i]
    — the numbers observe_vehicles_tensor() writes — the registered route with the handle route[i]: Engine.add_routes() /
    VectorEngine(routes=...) and added_routes(), or any index below route_count().  The vehicle keeps driving where it is;
    its route's cursor stands on the first occurrence of its road in the new route, so get_vehicle_info(...)["route"] lists
    the remaining roads, as after the reference's setRoute.

        vehicle   int32 [N]   N >= 0
        route     int32 [N]   -1: leave this vehicle alone
        status    int32 [N]   optional output, one verdict per row
        ignored   int32 [1]   optional output (0-dim is taken too): the rows with a negative status

    status[i] is decided by the first of these that applies:

         0   skipped: vehicle[i] == -1 (observe_vehicles_tensor's padding) or route[i] == -1
        -1   no such running vehicle: a number not issued, a finished vehicle, or one still in its lane's entry buffer
        -2   no such route handle
        -3   superseded: a later row that passes the checks above names the same vehicle
        -4   the vehicle is inside an intersection (on a laneLink)
        -5   the vehicle's road does not occur on the route before the route's last road
        -6   the vehicle's lane has no laneLink towards the route's next road: it is in the wrong turning lane (where the
             route also ENDS on the vehicle's road the reference accepts that: applied, and the trip ends on this lane)
         1   applied

    Of several rows for one vehicle only the LAST one that passes -1 and -2 counts, whatever its verdict — this is not "the
    last valid row wins": if that row is refused the vehicle keeps its old route.  The result never depends on the device's
    scheduling.  On a VectorEngine a handle is one environment's own index; the vehicle's environment decides which copy of
    the route it gets, and one call commands vehicles of any environment.  The trip log names a re-routed vehicle's
    destination by the new route's last road and its origin by the new route's FIRST road.

    Two kernel launches on the engine's stream (three on the dense layout), ordered after the current torch stream; the torch
    stream is ordered after them, so `status` and `ignored` can be read there and the inputs reused.  The call never waits for
    the device.  Every argument is checked before anything is enqueued.  RuntimeError with laneChange: true, and on a backend
    without the device call (the CPU twin): set_vehicle_route(), which restarts a route at its first road, cannot stand in."""
    torch = _torch()
    device = _engine_device(torch, self)
    if not isinstance(vehicle, torch.Tensor):
        raise TypeError("vehicle must be a torch.Tensor, not %s" % type(vehicle).__name__)
    if vehicle.dim() != 1:
        raise ValueError("vehicle must have shape [N], not %s" % (tuple(vehicle.shape),))
    n_rows = int(vehicle.shape[0])
    _check_buf(torch, vehicle, "vehicle", (n_rows,), torch.int32, device)
    _check_buf(torch, route, "route", (n_rows,), torch.int32, device)
    if status is not None:
        _check_buf(torch, status, "status", (n_rows,), torch.int32, device)
    if ignored is not None:
        _check_buf(torch, ignored, "ignored", () if isinstance(ignored, torch.Tensor) and ignored.dim() == 0 else (1,), torch.int32, device)
    if n_rows >= 2 ** 31:
        raise ValueError("a call holds fewer than 2**31 rows, not %d" % n_rows)
    if self._lane_change():
        raise RuntimeError("set_vehicle_routes_tensor: not with laneChange (the vehicle numbers are observe_vehicles')")
    ptr = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()  # noqa: E731
    stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    self._set_vehicle_routes_device(ptr(vehicle), ptr(route), n_rows, ptr(status), ptr(ignored), stream)


def get_vehicle_routes(self, vehicle):
    """The numpy form of get_vehicle_routes_tensor: `vehicle` int32 [N]; returns int32 [N].  Waits for the device."""
    import numpy as np

    _check_rows_array(np, vehicle, "vehicle")
    if self._lane_change():
        raise RuntimeError("get_vehicle_routes: not with laneChange (the vehicle numbers are observe_vehicles')")
    return self._vehicle_routes(vehicle)


def get_vehicle_routes_tensor(self, vehicle, out=None):
    """The route handle each vehicle holds: out[i] is the handle of the vehicle with the number vehicle[i] (waiting vehicles
    included; on a VectorEngine the index within its environment), or -1 where vehicle[i] is -1, not a number issued, or a
    finished vehicle.  `vehicle` int32 [N], `out` int32 [N] (allocated when None); returns `out`.  One kernel launch in the
    current torch stream's order, no host wait.  RuntimeError as set_vehicle_routes_tensor."""
    torch = _torch()
    device = _engine_device(torch, self)
    if not isinstance(vehicle, torch.Tensor):
        raise TypeError("vehicle must be a torch.Tensor, not %s" % type(vehicle).__name__)
    if vehicle.dim() != 1:
        raise ValueError("vehicle must have shape [N], not %s" % (tuple(vehicle.shape),))
    n_rows = int(vehicle.shape[0])
    _check_buf(torch, vehicle, "vehicle", (n_rows,), torch.int32, device)
    if out is not None:
        _check_buf(torch, out, "out", (n_rows,), torch.int32, device)
    if n_rows >= 2 ** 31:
        raise ValueError("a call holds fewer than 2**31 rows, not %d" % n_rows)
    if self._lane_change():
        raise RuntimeError("get_vehicle_routes_tensor: not with laneChange (the vehicle numbers are observe_vehicles')")
    if out is None:
        out = torch.empty((n_rows,), dtype=torch.int32, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0
    self._vehicle_routes_device(vehicle.data_ptr() if n_rows else 0, n_rows, out.data_ptr() if n_rows else 0, stream)
    return out


def install(*classes):
    for cls in classes:
        cls.set_vehicle_routes_tensor = set_vehicle_routes_tensor
        cls.set_vehicle_routes = set_vehicle_routes
        cls.get_vehicle_routes_tensor = get_vehicle_routes_tensor
        cls.get_vehicle_routes = get_vehicle_routes
        cls.set_vehicle_speeds_tensor = set_vehicle_speeds_tensor
        cls.set_vehicle_speeds = set_vehicle_speeds
        cls.observe_vehicles_tensor = observe_vehicles_tensor
        cls.observe_vehicles_array = observe_vehicles_array
        cls.drivable_geometry = drivable_geometry
        cls.checkpoint = checkpoint
        cls.rollback = rollback_envs if hasattr(cls, "_rollback_envs") else rollback
        cls.set_tl_plan_tensor = set_tl_plan_tensor
        cls.get_tl_phase_durations_tensor = get_tl_phase_durations_tensor
        cls.set_tl_plan = set_tl_plan
        cls.get_tl_phase_durations_array = get_tl_phase_durations_array
        cls.restore_tl_plan = restore_tl_plan
        cls.set_lane_speed_limits_tensor = set_lane_speed_limits_tensor
        cls.get_lane_speed_limits_tensor = get_lane_speed_limits_tensor
        cls.set_lane_speed_limits = set_lane_speed_limits
        cls.get_lane_speed_limits_array = get_lane_speed_limits_array
        cls.restore_lane_speed_limits = restore_lane_speed_limits
        cls.get_lane_vehicle_count_tensor = get_lane_vehicle_count_tensor
        cls.get_lane_waiting_vehicle_count_tensor = get_lane_waiting_vehicle_count_tensor
        cls.set_tl_phases_tensor = set_tl_phases_tensor
        cls.get_lane_speed_sum_tensor = get_lane_speed_sum_tensor
        cls.get_lane_vehicle_bins_tensor = get_lane_vehicle_bins_tensor
        cls.observe_lanes_tensor = observe_lanes_tensor
        cls.get_lane_front_vehicles_tensor = get_lane_front_vehicles_tensor
        cls.get_lane_front_vehicles_array = get_lane_front_vehicles_array
        cls.observe_intersections_tensor = observe_intersections_tensor
        cls.get_tl_phases_tensor = get_tl_phases_tensor
        cls.observe_intersections_array = observe_intersections_array
        cls.intersection_layout = intersection_layout
        cls.track_lane_flow = track_lane_flow
        cls.lane_flow_tracking = lane_flow_tracking
        cls.observe_lane_flow_tensor = observe_lane_flow_tensor
        cls.observe_lane_flow_array = observe_lane_flow_array
        cls.track_movement_flow = track_movement_flow
        cls.movement_flow_tracking = movement_flow_tracking
        cls.observe_movement_flow_tensor = observe_movement_flow_tensor
        cls.observe_movement_flow_array = observe_movement_flow_array
        cls.track_trips = track_trips
        cls.trip_tracking = trip_tracking
        cls.observe_trips_tensor = observe_trips_tensor
        cls.observe_trips_array = observe_trips_array
        cls.trip_log_capacity = trip_log_capacity
        cls.observe_trip_log_tensor = observe_trip_log_tensor
        cls.observe_trip_log_array = observe_trip_log_array
        cls.get_average_travel_time_tensor = get_average_travel_time_tensor
        cls.track_detectors = track_detectors
        cls.detector_tracking = detector_tracking
        cls.detector_layout = detector_layout
        cls.observe_detectors_tensor = observe_detectors_tensor
        cls.observe_detectors_array = observe_detectors_array
