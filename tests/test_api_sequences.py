"""CPU: random sequences of `cityflow.Engine` calls applied to the unmodified reference (oracle/_ref) and to this host on the
CPU twin alike — steps in runs of varying length, the dict getters, signal phases, custom speeds, snapshot / load, reset —
whatever either returns must be equal, and so must the state at the end of every round.  (The same kind of sequence pins the
HIP engine against the twin: tests/test_deferred_commit.py.)  Reference semantics: /root/reference/src/engine/engine.cpp
:566-594 (nextStep), 615-691 (getters), 719-725 (setTrafficLightPhase), 827-834 (setVehicleSpeed), 744-760 (reset),
src/engine/archive.cpp:9-126 (snapshot / load)."""
import json
import os
import time

import numpy as np
import pytest

from conftest import TWIN_LIB, checkpoint_record


def _config(scen, workdir, rl):
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_seq.json"), 180, seed=29, interval=4.0,
                            base_flow=os.path.join(d, "flow.json"))
    return scen.materialize("grid_6x6", workdir, flow_file=flow, rlTrafficLight=rl)


def _compacting(cfg, every):
    """The same config with `"cfx": {"compactVehicles": every}` (ignored by the reference): this engine forgets its finished
    vehicles and renumbers the others every time that many have been created (EngineHost::compactVehicles) — which nothing a
    caller can see may show."""
    if not every:
        return cfg
    with open(cfg) as f:
        c = json.load(f)
    c["cfx"] = dict(c.get("cfx", {}), compactVehicles=every)
    path = cfg.replace(".json", "_compact%d.json" % every)
    with open(path, "w") as f:
        json.dump(c, f)
    return path


@pytest.mark.parametrize("rl,seed,compact", [(True, 5, 0), (True, 6, 0), (False, 7, 0), (True, 5, 60), (False, 7, 25)])
def test_random_call_sequences_equal_reference(mod, ref_module, scen, workdir, rl, seed, compact):
    cfg = _compacting(_config(scen, workdir, rl), compact)
    ref, tw = ref_module.Engine(cfg, 1), mod.Engine._with_backend(cfg, 1, TWIN_LIB)
    rng = np.random.default_rng(seed)
    with open(os.path.join(os.path.dirname(cfg), "roadnet.json")) as f:
        inters = [i["id"] for i in json.load(f)["intersections"] if not i["virtual"]]
    archives = None
    for round_ in range(30):
        for _ in range(int(rng.integers(1, 7))):
            op = int(rng.integers(0, 9))
            if op <= 3:
                for _ in range(int(rng.integers(1, 15))):
                    ref.next_step()
                    tw.next_step()
            elif op == 4:
                assert ref.get_lane_vehicle_count() == tw.get_lane_vehicle_count()
                assert ref.get_lane_waiting_vehicle_count() == tw.get_lane_waiting_vehicle_count()
            elif op == 5 and rl:
                for i in rng.choice(len(inters), size=5, replace=False):
                    ph = int(rng.integers(0, 8))
                    ref.set_tl_phase(inters[int(i)], ph)
                    tw.set_tl_phase(inters[int(i)], ph)
            elif op == 6:
                speeds = tw.get_vehicle_speed()
                assert speeds == ref.get_vehicle_speed()
                if speeds:
                    vid = sorted(speeds)[int(rng.integers(0, len(speeds)))]
                    v = float(rng.uniform(0.0, 12.0))
                    ref.set_vehicle_speed(vid, v)
                    tw.set_vehicle_speed(vid, v)
                    assert ref.get_vehicle_info(vid) == tw.get_vehicle_info(vid)
            elif op == 7:
                assert ref.get_vehicle_count() == tw.get_vehicle_count()
                assert ref.get_vehicles(True) == tw.get_vehicles(True)
                assert ref.get_lane_vehicles() == tw.get_lane_vehicles()
            elif op == 8:
                if archives is None or rng.random() < 0.5:
                    archives = (ref.snapshot(), tw.snapshot())
                else:
                    ref.load(archives[0])
                    tw.load(archives[1])
        if round_ == 19:
            ref.reset(False)
            tw.reset(False)
            archives = None
        assert checkpoint_record(tw) == checkpoint_record(ref), "rl %s seed %d round %d" % (rl, seed, round_)
        assert ref.get_current_time() == tw.get_current_time()
    assert (tw._vehicle_table()[1] > 3) == bool(compact), tw._vehicle_table()
    time.sleep(0.2)  # reference destructor race
    del ref


@pytest.mark.parametrize("seed,compact", [(11, 0), (12, 0), (13, 0), (14, 0), (12, 30), (14, 80)])
def test_random_control_and_query_calls_equal_reference(mod, ref_module, scen, workdir, seed, compact):
    """... with the per-vehicle calls: get_vehicle_info (every field), get_leader, get_vehicle_distance, set_vehicle_route with
    random anchors (the return value and everything that follows), push_vehicle, set_random_seed + reset(True)."""
    cfg = _compacting(_config(scen, workdir, False), compact)
    ref, tw = ref_module.Engine(cfg, 1), mod.Engine._with_backend(cfg, 1, TWIN_LIB)
    rng = np.random.default_rng(seed)
    with open(os.path.join(os.path.dirname(cfg), "roadnet.json")) as f:
        roads = [r["id"] for r in json.load(f)["roads"]]
    for round_ in range(24):
        for _ in range(int(rng.integers(1, 7))):
            op = int(rng.integers(0, 9))
            if op <= 2:
                for _ in range(int(rng.integers(1, 20))):
                    ref.next_step()
                    tw.next_step()
            elif op in (3, 4, 5):
                ids = ref.get_vehicles(True)
                assert ids == tw.get_vehicles(True)
                if ids:
                    vid = sorted(ids)[int(rng.integers(0, len(ids)))]
                    if op == 3:
                        assert ref.get_vehicle_info(vid) == tw.get_vehicle_info(vid), (round_, vid)
                        assert ref.get_leader(vid) == tw.get_leader(vid), (round_, vid)
                    elif vid.startswith("manually_pushed") and ref.get_vehicle_info(vid)["running"] == "0":
                        pass  # (pushed since the last step: it has no drivable yet, Router::setRoute would dereference null)
                    elif op == 4:
                        anchors = [roads[int(i)] for i in rng.integers(0, len(roads), size=int(rng.integers(1, 3)))]
                        a, b = ref.set_vehicle_route(vid, anchors), tw.set_vehicle_route(vid, anchors)
                        assert a == b, (round_, vid, anchors, a, b)
                        assert ref.get_vehicle_info(vid) == tw.get_vehicle_info(vid), (round_, vid, anchors)
                    else:
                        info = ref.get_vehicle_info(vid)
                        if info.get("road"):  # towards a road next to the one it is on: usually a valid reroute
                            x, y, dirn = (int(t) for t in info["road"].split("_")[1:])
                            nx, ny = x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn]
                            anchors = ["road_%d_%d_%d" % (nx, ny, int(rng.integers(0, 4)))]
                            if anchors[0] in roads:
                                a, b = ref.set_vehicle_route(vid, anchors), tw.set_vehicle_route(vid, anchors)
                                assert a == b, (round_, vid, anchors, a, b)
                                assert ref.get_vehicle_info(vid) == tw.get_vehicle_info(vid), (round_, vid, anchors)
            elif op == 6:
                assert ref.get_vehicle_distance() == tw.get_vehicle_distance()
                assert ref.get_vehicle_speed() == tw.get_vehicle_speed()
            elif op == 7:
                info = {"length": float(rng.uniform(3.0, 8.0)), "maxSpeed": float(rng.uniform(8.0, 16.0)), "minGap": 2.5}
                start = roads[int(rng.integers(0, len(roads)))]
                x, y, dirn = (int(t) for t in start.split("_")[1:])
                nxt = "road_%d_%d_%d" % (x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn], dirn)
                route = [start, nxt] if nxt in roads else [start]
                ref.push_vehicle(info, route)
                tw.push_vehicle(info, route)
            elif op == 8 and round_ in (9, 17):
                # (one step first: the reference's reset frees the vehicles but leaves those pushed since the last step in
                # their road's planRouteBuffer — the next step would walk freed memory)
                ref.next_step()
                tw.next_step()
                ref.set_random_seed(int(seed) + round_)
                tw.set_random_seed(int(seed) + round_)
                ref.reset(True)
                tw.reset(True)
        assert checkpoint_record(tw) == checkpoint_record(ref), "seed %d round %d" % (seed, round_)
    time.sleep(0.2)  # reference destructor race
    del ref


@pytest.mark.parametrize("interval,seed,compact", [(0.5, 21, 0), (0.5, 22, 0), (1.0, 23, 0), (0.5, 22, 8), (1.0, 23, 40)])
def test_waiting_finished_and_reseeded_vehicles_equal_reference(mod, ref_module, scen, workdir, interval, seed, compact):
    """... with a step length other than 1 s, and the calls whose subject is NOT a running vehicle: a custom speed for a vehicle
    that still waits in its lane's buffer (it takes effect in its first step), queries about a vehicle that has left the
    network (both raise), a new random seed without a reset, `reset(False)` in the middle."""
    # (0.5 s: the 1x1 example; 1 s: the congested 6x6 grid, whose entry lanes have vehicles waiting)
    base = (scen.materialize("example_1x1", workdir, interval=interval, rlTrafficLight=True, seed=int(seed)) if interval != 1.0
            else _config(scen, workdir, True))
    base = _compacting(base, compact)
    ref, tw = ref_module.Engine(base, 1), mod.Engine._with_backend(base, 1, TWIN_LIB)
    rng = np.random.default_rng(seed)
    seen = set()
    exercised = {"waiting": 0, "gone": 0}
    for round_ in range(40):
        for _ in range(int(rng.integers(1, 6))):
            op = int(rng.integers(0, 8))
            if op <= 2:
                for _ in range(int(rng.integers(1, 25))):
                    ref.next_step()
                    tw.next_step()
            elif op == 3:  # a vehicle that waits in a lane's buffer
                everybody, running = tw.get_vehicles(True), set(tw.get_vehicles())
                assert everybody == ref.get_vehicles(True) and running == set(ref.get_vehicles())
                waiting = [v for v in everybody if v not in running]
                if waiting:
                    vid = waiting[int(rng.integers(0, len(waiting)))]
                    v = float(rng.uniform(0.0, 9.0))
                    ref.set_vehicle_speed(vid, v)
                    tw.set_vehicle_speed(vid, v)
                    assert ref.get_vehicle_info(vid) == tw.get_vehicle_info(vid) == {"running": "0"}
                    assert ref.get_leader(vid) == tw.get_leader(vid) == ""
                    exercised["waiting"] += 1
            elif op == 4:  # a vehicle that has left the network
                now = set(tw.get_vehicles(True))
                gone = sorted(seen - now)
                seen |= now
                if gone:
                    vid = gone[int(rng.integers(0, len(gone)))]
                    for e in (ref, tw):
                        for call in (lambda: e.get_vehicle_info(vid), lambda: e.get_leader(vid), lambda: e.set_vehicle_speed(vid, 1.0)):
                            with pytest.raises(RuntimeError, match="not found"):
                                call()
                        assert e.set_vehicle_route(vid, ["road_1_0_1"]) is False
                    exercised["gone"] += 1
            elif op == 5:
                ref.set_random_seed(int(seed) * 100 + round_)
                tw.set_random_seed(int(seed) * 100 + round_)
            elif op == 6:
                ph = int(rng.integers(0, 8))
                ref.set_tl_phase("intersection_1_1", ph)
                tw.set_tl_phase("intersection_1_1", ph)
            elif op == 7 and round_ == 25:
                ref.reset(False)
                tw.reset(False)
                seen.clear()
        assert checkpoint_record(tw) == checkpoint_record(ref), "interval %s seed %d round %d" % (interval, seed, round_)
        assert ref.get_current_time() == tw.get_current_time()
        assert ref.get_lane_waiting_vehicle_count() == tw.get_lane_waiting_vehicle_count()
    assert exercised["gone"] > 0 and (interval != 1.0 or exercised["waiting"] > 0), exercised
    time.sleep(0.2)  # reference destructor race
    del ref


@pytest.mark.parametrize("seed", [1, 2, 27])
def test_tiled_random_calls_equal_single_engine(mod, scen, workdir, seed):
    """The same kind of sequence on `TiledEngine` (2x2, 2x3, 3x2 or 1x3 tiles of the 6x6 grid, all on the CPU twin) and on a
    single engine: every getter's return value, `set_vehicle_route`'s verdicts, vehicles pushed and listed before their first
    step, snapshot / load and reset in the middle — equal call by call (seed 27: a reroute right after a load)."""
    rl = seed % 2 == 0
    cfg = _config(scen, workdir, rl)
    rows, cols = ((2, 2), (2, 3), (3, 2), (1, 3))[seed % 4]
    one, til = mod.Engine._with_backend(cfg, 1, TWIN_LIB), mod.TiledEngine(cfg, rows, cols, [], TWIN_LIB)
    rng = np.random.default_rng(seed)
    with open(os.path.join(os.path.dirname(cfg), "roadnet.json")) as f:
        net = json.load(f)
    roads = [r["id"] for r in net["roads"]]
    inters = [i["id"] for i in net["intersections"] if not i["virtual"]]
    archives = None

    def both(name, *a):
        x, y = getattr(one, name)(*a), getattr(til, name)(*a)
        assert x == y, (name, a, str(x)[:200], str(y)[:200])
        return x

    for round_ in range(20):
        for _ in range(int(rng.integers(1, 7))):
            op = int(rng.integers(0, 12))
            if op <= 2:
                for _ in range(int(rng.integers(1, 15))):
                    one.next_step()
                    til.next_step()
            elif op == 3:
                both("get_lane_vehicle_count")
                both("get_lane_waiting_vehicle_count")
                both("get_vehicle_count")
            elif op == 4 and rl:
                for i in rng.choice(len(inters), size=5, replace=False):
                    ph = int(rng.integers(0, 8))
                    one.set_tl_phase(inters[int(i)], ph)
                    til.set_tl_phase(inters[int(i)], ph)
            elif op == 5:
                sp = both("get_vehicle_speed")
                both("get_vehicle_distance")
                if sp:
                    vid = sorted(sp)[int(rng.integers(0, len(sp)))]
                    v = float(rng.uniform(0, 12))
                    one.set_vehicle_speed(vid, v)
                    til.set_vehicle_speed(vid, v)
                    both("get_vehicle_info", vid)
                    both("get_leader", vid)
            elif op == 6:
                both("get_vehicles", True)
                both("get_vehicles", False)
                both("get_lane_vehicles")
            elif op == 7:
                ids = both("get_vehicles", True)
                if ids:
                    vid = sorted(ids)[int(rng.integers(0, len(ids)))]
                    info = both("get_vehicle_info", vid)
                    if info.get("road"):
                        x, y, dirn = (int(q) for q in info["road"].split("_")[1:])
                        a = "road_%d_%d_%d" % (x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn], int(rng.integers(0, 4)))
                        if a in roads:
                            both("set_vehicle_route", vid, [a])
                            both("get_vehicle_info", vid)
            elif op == 8:
                info = {"length": float(rng.uniform(3, 8)), "maxSpeed": float(rng.uniform(8, 16)), "minGap": 2.5}
                start = roads[int(rng.integers(0, len(roads)))]
                x, y, dirn = (int(q) for q in start.split("_")[1:])
                nxt = "road_%d_%d_%d" % (x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn], dirn)
                route = [start, nxt] if nxt in roads else [start]
                one.push_vehicle(info, route)
                til.push_vehicle(info, route)
                both("get_vehicles", True)
                both("get_average_travel_time")
            elif op == 9:
                if archives is None or rng.random() < 0.5:
                    archives = (one.snapshot(), til.snapshot())
                else:
                    one.load(archives[0])
                    til.load(archives[1])
            elif op == 10 and round_ == 12:
                one.reset(False)
                til.reset(False)
                archives = None
            elif op == 11:
                both("get_average_travel_time")
                both("get_current_time")
        assert checkpoint_record(one) == checkpoint_record(til), (seed, round_)


def _comparable_dump(path, written_by_reference, keep_history=False):
    """An Archive file without the two things that cannot be equal: Lane::history (it feeds only the unused DURATION router
    and is not kept by this engine) and ControllerInfo::gap of a vehicle without a leader (uninitialised memory in the
    reference's dump)."""
    from cityflow_amd import _cityflow
    # The numbers each writer MEANT.  The reference's writer (rapidjson's Writer: near-shortest digits) guarantees them to a
    # correctly rounding reader; this engine's writer guarantees them to the reference's own reader (rapidjson's default number
    # reader, csrc/host/json_number.h), for which no such literal exists for about one double in a thousand.
    with open(path) as f:
        d = json.load(f) if written_by_reference else json.load(f, parse_float=lambda lit: _cityflow._parse_json_number(lit)[0])
    for dv in d["drivables"].values():
        for k in ("history", "historyVehicleNum", "historyAverageSpeed"):
            if not keep_history:
                dv.pop(k, None)
    for v in d["vehicles"]:
        if not v.get("leader"):
            v.pop("gap", None)
    return d


@pytest.mark.parametrize("seed,history,compact", [pytest.param(3, False, 0, id="3-False"), pytest.param(4, False, 0, id="4-False"),
                                                  pytest.param(5, True, 0, id="5-True"), pytest.param(6, True, 0, id="6-True"),
                                                  (3, False, 25), (6, True, 40)])
def test_archive_files_cross_loaded_in_the_middle_of_sequences(mod, ref_module, scen, workdir, tmp_path, seed, history, compact):
    """`snapshot().dump()` of the reference and of this engine at random moments of a sequence with custom speeds, pushed
    vehicles and full waiting buffers: the files are equal (see _comparable_dump), both engines load one of the two files
    and go on identically — again and again in one run (archive.cpp:153-550).  With `compact`, this engine forgets its finished
    vehicles in between: a file it loads names vehicles the last compaction renumbered (csrc/host/archive.cpp readArchiveFile)."""
    rl = seed % 2 == 0
    cfg = _config(scen, workdir, rl)
    if history:  # Lane::history kept ("cfx": {"laneHistory": true}) and compared too: it travels with the files (archive.cpp:286-294)
        c = json.load(open(cfg))
        c["cfx"] = {"laneHistory": True}
        cfg = cfg.replace(".json", "_history.json")
        with open(cfg, "w") as f:
            json.dump(c, f)
    cfg = _compacting(cfg, compact)
    ref, tw = ref_module.Engine(cfg, 1), mod.Engine._with_backend(cfg, 1, TWIN_LIB)
    rng = np.random.default_rng(seed)
    exchanged = 0
    for round_ in range(14):
        for _ in range(int(rng.integers(1, 5))):
            op = int(rng.integers(0, 7))
            if op <= 2:
                for _ in range(int(rng.integers(1, 25))):
                    ref.next_step()
                    tw.next_step()
            elif op == 3:
                sp = tw.get_vehicle_speed()
                assert sp == ref.get_vehicle_speed()
                if sp:
                    vid = sorted(sp)[int(rng.integers(0, len(sp)))]
                    v = float(rng.uniform(0, 12))
                    ref.set_vehicle_speed(vid, v)
                    tw.set_vehicle_speed(vid, v)
            elif op == 4:
                exchanged += 1
                p_ref, p_tw = str(tmp_path / ("ref%d.json" % exchanged)), str(tmp_path / ("tw%d.json" % exchanged))
                ref.snapshot().dump(p_ref)
                tw.snapshot().dump(p_tw)
                assert _comparable_dump(p_ref, True, history) == _comparable_dump(p_tw, False, history), (seed, round_)
                # Both load the SAME file, the reference's or this engine's.  The reference's reader (rapidjson's default
                # number reader, restated in csrc/host/json_number.h) is not correctly rounded: a file the reference wrote
                # (near-shortest digits) can come back an ulp off — in both engines alike, `dis`, `speed` and the stored `gap`
                # each on its own; this engine's file (literals chosen to survive that reader) comes back as it was saved.
                which = p_ref if rng.random() < 0.5 else p_tw
                tw.load_from_file(which)
                ref.load_from_file(which)
            elif op == 5:
                assert ref.get_lane_vehicle_count() == tw.get_lane_vehicle_count()
            elif op == 6:
                info = {"length": float(rng.uniform(3, 8)), "maxSpeed": float(rng.uniform(8, 16)), "minGap": 2.5}
                ref.push_vehicle(info, ["road_1_1_0", "road_2_1_0"])
                tw.push_vehicle(info, ["road_1_1_0", "road_2_1_0"])
                ref.next_step()
                tw.next_step()
        assert checkpoint_record(tw) == checkpoint_record(ref), (seed, round_)
    assert exchanged >= 2
    assert (tw._vehicle_table()[1] > 3) == bool(compact), tw._vehicle_table()
    time.sleep(0.2)  # reference destructor race
    del ref
