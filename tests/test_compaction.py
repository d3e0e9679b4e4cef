"""Bounded memory: the engine forgets its finished vehicles.  The reference frees a vehicle when it finishes
(src/engine/engine.cpp:296-310); here host and device keep a table row per vehicle NUMBER, and `EngineHost::compactVehicles`
(csrc/host/archive.cpp) — automatic once enough numbers have been handed out, `"cfx": {"compactVehicles": N}` — renumbers the
vehicles that are still waiting or running, in their old order, through the path a load takes.  Nothing a caller can see may
change: the random call sequences of tests/test_api_sequences.py run against the unmodified reference with a compaction every
few vehicles; here: the tables stay bounded, a compacting engine equals one that never compacts, on the twin (CPU) and on the
GPU."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import REF_DIR, TWIN_LIB, assert_hip_backend, checkpoint_record


def compacting(cfg, every, **more):
    with open(cfg) as f:
        c = json.load(f)
    c["cfx"] = dict(c.get("cfx", {}), compactVehicles=every, **more)
    path = cfg.replace(".json", "_compact%d.json" % every)
    with open(path, "w") as f:
        json.dump(c, f)
    return path


def unsaturated_grid(scen, workdir):
    cfg = scen.generate_grid(6, 6, workdir, flow_interval=12.0)
    with open(cfg) as f:
        c = json.load(f)
    c["rlTrafficLight"] = True
    path = cfg.replace(".json", "_rl.json")
    with open(path, "w") as f:
        json.dump(c, f)
    return path


def visible(e):
    return {"lanes": e.get_lane_vehicle_count(), "waiting": e.get_lane_waiting_vehicle_count(), "speed": e.get_vehicle_speed(),
            "distance": e.get_vehicle_distance(), "lane_vehicles": e.get_lane_vehicles(), "vehicles": e.get_vehicles(True),
            "count": e.get_vehicle_count(), "time": e.get_current_time(), "travel": e.get_average_travel_time()}


def run_pair(a, b, steps, check_every, rl=True):
    """`a` compacts, `b` never does; both take the same calls."""
    n_inter = len(a.intersection_ids())
    rng = np.random.default_rng(3)
    for s in range(steps):
        if rl and s % 5 == 0:
            ph = rng.integers(0, 4, n_inter).astype(np.int32)
            a.set_tl_phases(ph)
            b.set_tl_phases(ph)
        a.next_step()
        b.next_step()
        if s % 7 == 0:
            assert np.array_equal(a.get_lane_vehicle_count_array(), b.get_lane_vehicle_count_array()), s
        if s % check_every == check_every - 1:
            va, vb = visible(a), visible(b)
            for k in va:
                assert va[k] == vb[k], (s, k)
            some = va["vehicles"][:: max(1, len(va["vehicles"]) // 12)]
            for v in some:
                assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (s, v)
                assert a.get_leader(v) == b.get_leader(v), (s, v)
            ha, hb = a._lane_history(), b._lane_history()
            for k in ha:
                assert np.array_equal(ha[k], hb[k]), (s, "lane history", k)


def test_compaction_bounds_the_tables_and_changes_nothing_twin(mod, scen, workdir):
    # (a grid whose demand the network carries: on the stock 6x6 flows most vehicles WAIT in their lanes' buffers for ever — the
    # reference keeps those too — and there is little to forget)
    base = unsaturated_grid(scen, workdir)
    a = mod.Engine._with_backend(compacting(base, 300), 1, TWIN_LIB)
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    peak = 0
    for chunk in range(6):
        run_pair(a, b, 250, 125)
        peak = max(peak, a._vehicle_table()[0])
    held, compactions = a._vehicle_table()
    created = b._vehicle_table()[0]
    assert b._vehicle_table()[1] == 0 and created > 2500
    assert compactions >= 6 and peak <= 300 + len(a.get_vehicles(True)) + 400, (held, compactions, peak)
    # a vehicle that has left is gone on both, whatever its number was
    gone = sorted(set("flow_%d_0" % f for f in range(5)) - set(a.get_vehicles(True)))
    for v in gone:
        for e in (a, b):
            with pytest.raises(RuntimeError, match="not found"):
                e.get_vehicle_info(v)
    # archives of the two still travel in both directions (the numbering is nobody's business)
    arch_a, arch_b = a.snapshot(), b.snapshot()
    run_pair(a, b, 40, 20)
    a.load(arch_b)
    b.load(arch_a)
    run_pair(a, b, 120, 40)
    a._compact_vehicles()  # on request, too
    run_pair(a, b, 60, 30)


def test_compaction_with_lane_change_and_off_by_zero(mod, scen, workdir):
    """Lane change: an id travels along a chain of copies (vehicle, shadow, the shadow's shadow ...): the chains of the vehicles
    alive stay whole, as rows of finished vehicles, and every id still finds who carries it (reference goldens with lane
    change while compacting: tests/test_lane_change.py)."""
    base = scen.materialize("example_1x1", workdir, laneChange=True)
    a = mod.Engine._with_backend(compacting(base, 9), 1, TWIN_LIB)
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    shadows = 0
    for s in range(400):
        a.next_step()
        b.next_step()
        if s % 20 == 19:
            va, vb = visible(a), visible(b)
            for k in va:
                assert va[k] == vb[k], (s, k)
            shadows += sum(v.endswith("_shadow") for vs in va["lane_vehicles"].values() for v in vs)
            for v in va["vehicles"]:
                assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (s, v)
    assert shadows > 0 and a._vehicle_table()[1] > 20 and a._vehicle_table()[0] < b._vehicle_table()[0] // 3
    off = mod.Engine._with_backend(compacting(scen.materialize("example_1x1", workdir), 0), 1, TWIN_LIB)
    for _ in range(400):
        off.next_step()
    assert off._vehicle_table()[1] == 0


@pytest.mark.gpu
def test_compaction_hip_equals_a_twin_that_never_compacts(mod, scen, workdir):
    base = unsaturated_grid(scen, workdir)
    a = mod.Engine(compacting(base, 200), 1)
    assert_hip_backend(a)
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    run_pair(a, b, 1200, 150)
    assert a._vehicle_table()[1] >= 6 and a._vehicle_table()[0] <= len(a.get_vehicles(True)) + 200 < b._vehicle_table()[0], (a._vehicle_table(), b._vehicle_table())
    free0 = a._device_memory()[0]
    run_pair(a, b, 600, 200)
    assert abs(free0 - a._device_memory()[0]) < (4 << 20)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_compaction_on_the_bench_workload(mod, workdir, layout):
    """30x30 with ~97 k vehicles: an engine that compacts on request in the middle of the run against one that does not —
    every visible number equal afterwards, ties included (the renumbering keeps creation order)."""
    import bench
    cfg = bench.build_workload(workdir, 0, scenario="grid_30x30")
    a = mod.Engine(compacting(cfg, 0, layout=layout), 1)
    b = mod.Engine(compacting(cfg, 0, layout=layout), 1)
    assert_hip_backend(a)
    for s in range(bench.BUILD_UP_STEPS):
        a.next_step()
        b.next_step()
    before = a._vehicle_table()[0]
    a._compact_vehicles()
    assert a._vehicle_table()[0] < before and a._vehicle_table()[0] == len(a.get_vehicles(True))
    for s in range(60):
        a.next_step()
        b.next_step()
        if s == 30:
            a._compact_vehicles()
    assert a.get_lane_vehicle_count() == b.get_lane_vehicle_count()
    assert a.get_vehicle_speed() == b.get_vehicle_speed() and a.get_vehicle_distance() == b.get_vehicle_distance()
    assert a.get_average_travel_time() == b.get_average_travel_time() and a.get_vehicles(True) == b.get_vehicles(True)
    sa, sb = a._scalars(), b._scalars()
    for k in ("active_vehicle_count", "finished_vehicle_count", "vehicle_steps", "cumulative_travel_time", "step"):
        assert sa[k] == sb[k], k


@pytest.mark.gpu
def test_compaction_with_lane_change_hip_equals_a_twin_that_never_compacts(mod, scen, workdir):
    base = scen.materialize("example_1x1", workdir, laneChange=True)
    a = mod.Engine(compacting(base, 11), 1)
    assert_hip_backend(a)
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    shadows = 0
    for s in range(500):
        a.next_step()
        b.next_step()
        if s % 25 == 24:
            va, vb = visible(a), visible(b)
            for k in va:
                assert va[k] == vb[k], (s, k)
            shadows += sum(v.endswith("_shadow") for vs in va["lane_vehicles"].values() for v in vs)
    assert shadows > 0 and a._vehicle_table()[1] > 20


# ---- load_from_file after a compaction (csrc/host/archive.cpp readArchiveFile): the file names its vehicles by id, the loader
#      fills the number -> vid tables by absolute vehicle number, so whatever bases a compaction had moved up before must not
#      survive the load — a stale base resolves every id to another vehicle (or to none) and makes the next spawn index below
#      its table (Spawner::step refuses that)
def with_lane_history(cfg, keep):
    with open(cfg) as f:
        c = json.load(f)
    c["cfx"] = dict(c.get("cfx", {}), laneHistory=keep)
    path = cfg.replace(".json", "_history%d.json" % keep)
    with open(path, "w") as f:
        json.dump(c, f)
    return path


def signals_and_roads(cfg):
    with open(cfg) as f:
        c = json.load(f)
    with open(c["dir"] + c["roadnetFile"]) as f:
        net = json.load(f)
    return [i["id"] for i in net["intersections"] if not i["virtual"]], set(r["id"] for r in net["roads"])


def push_some(engines, k):
    """The same pushed vehicle on every engine, then one step (the reference's manual counter never goes back: every engine
    compared after a load has taken the same pushes before it)."""
    info = {"length": 4.0 + k % 3, "maxSpeed": 10.0 + k % 4, "minGap": 2.5}
    for e in engines:
        e.push_vehicle(info, ["road_1_1_0", "road_2_1_0"])
    for e in engines:
        e.next_step()


def same_per_vehicle_answers(engines, roads, gone, where):
    """Every id the engines list answers alike on all of them (get_vehicle_info, get_leader, its distance); ids that are not in
    the network any more are unknown to all of them; set_vehicle_route / set_vehicle_speed give the same verdicts."""
    ids = engines[0].get_vehicles(True)
    for e in engines[1:]:
        assert e.get_vehicles(True) == ids, where
    dist = engines[0].get_vehicle_distance()
    for e in engines[1:]:
        assert e.get_vehicle_distance() == dist, where
    for v in ids:
        info = engines[0].get_vehicle_info(v)
        leader = engines[0].get_leader(v)
        for e in engines[1:]:
            assert e.get_vehicle_info(v) == info, (where, v)
            assert e.get_leader(v) == leader, (where, v)
    absent = sorted(gone - set(ids))
    for v in absent[:: max(1, len(absent) // 20)]:
        for e in engines:
            with pytest.raises(RuntimeError, match="not found"):
                e.get_vehicle_info(v)
    running = engines[0].get_vehicles(False)
    for v in running[:: max(1, len(running) // 6)]:
        road = engines[0].get_vehicle_info(v).get("road")
        if not road:  # (on a lane link)
            continue
        x, y, dirn = (int(q) for q in road.split("_")[1:])
        anchor = "road_%d_%d_%d" % (x + (1, 0, -1, 0)[dirn], y + (0, 1, 0, -1)[dirn], dirn)
        if anchor not in roads:
            continue
        verdicts = [e.set_vehicle_route(v, [anchor]) for e in engines]
        assert len(set(verdicts)) == 1, (where, v, anchor, verdicts)
        for e in engines:
            e.set_vehicle_speed(v, 4.5)
        info = engines[0].get_vehicle_info(v)
        for e in engines[1:]:
            assert e.get_vehicle_info(v) == info, (where, "after set_vehicle_route / set_vehicle_speed", v)
    return len(ids)


def load_file_after_compaction(mod, scen, workdir, tmp_path, make_a, ref_module, history):
    """`a` compacts every 40 vehicle numbers, `b` (twin) never does, `r` is the unmodified reference (None: not compared); all
    take the same calls.  Four files — (a) dumped by `a` before its first compaction, (b) by `a` between two compactions, (c)
    by `b`, (d) by `r` — each loaded by all of them once `a` has compacted at least 5 times since the file was written, then
    300 steps on from there through compactions, automatic and on request."""
    base = with_lane_history(unsaturated_grid(scen, workdir), history)
    a = make_a(base)
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    r = ref_module.Engine(base, 1) if ref_module is not None else None
    engines = [e for e in (a, b, r) if e is not None]
    signals, roads = signals_and_roads(base)
    rng = np.random.default_rng(17)
    seen = set()

    def steps(n, check_every=50):
        for s in range(n):
            if s % 5 == 0:
                for i in rng.choice(len(signals), size=6, replace=False):
                    ph = int(rng.integers(0, 4))
                    for e in engines:
                        e.set_tl_phase(signals[int(i)], ph)
            for e in engines:
                e.next_step()
            if s % check_every == check_every - 1:
                rec = checkpoint_record(a)
                for e in engines[1:]:
                    assert checkpoint_record(e) == rec, s
                va, vb = visible(a), visible(b)
                for k in va:
                    assert va[k] == vb[k], (s, k)
                assert a._vehicle_table()[0] <= 40 + len(a.get_vehicles(True)) + 400, a._vehicle_table()
                seen.update(va["vehicles"])

    files, written_at = {}, {}

    def dump(name, e):
        files[name] = str(tmp_path / ("%s.json" % name))
        e.snapshot().dump(files[name])
        written_at[name] = a._vehicle_table()[1]

    steps(3, 1)
    push_some(engines, 0)
    steps(6, 3)
    assert a._vehicle_table()[1] == 0 and a.get_vehicle_count() > 0
    dump("a_before_compacting", a)
    steps(60)
    assert a._vehicle_table()[1] >= 1
    push_some(engines, 1)
    dump("a_between_compactions", a)
    steps(40)
    dump("b_never_compacting", b)
    steps(30)
    if r is not None:
        dump("reference", r)
    for name in files:
        steps(250)
        assert a._vehicle_table()[1] - written_at[name] >= 5, (name, a._vehicle_table(), written_at[name])
        seen.update(a.get_vehicles(True))
        for e in engines:
            e.load_from_file(files[name])
        n = same_per_vehicle_answers(engines, roads, seen, name)
        assert n > 0, name
        push_some(engines, 2)
        compactions = a._vehicle_table()[1]
        steps(150)
        a._compact_vehicles()
        assert a._vehicle_table()[0] == len(a.get_vehicles(True)), name
        push_some(engines, 3)
        steps(150)
        assert a._vehicle_table()[1] - compactions >= 4, (name, a._vehicle_table(), compactions)  # 3 automatic + 1 on request
        same_per_vehicle_answers(engines, roads, seen, name + " +300")
        assert a._keeps_lane_history() == b._keeps_lane_history() == history
        if history:
            ha, hb = a._lane_history(), b._lane_history()
            for k in ha:
                assert np.array_equal(ha[k], hb[k]), (name, "lane history", k)
    assert len(files) == (4 if r is not None else 3)
    return a


@pytest.mark.parametrize("history", [False, True])
def test_load_from_file_after_compaction_twin(mod, ref_module, scen, workdir, tmp_path, history):
    load_file_after_compaction(mod, scen, workdir, tmp_path, lambda c: mod.Engine._with_backend(compacting(c, 40), 1, TWIN_LIB),
                               ref_module, history)


def test_load_from_file_after_compaction_with_lane_change_twin(mod, scen, workdir, tmp_path):
    """Lane change: a dump holding shadows, taken before the compactions that forget rows of their id chains, loaded after many
    of them — every id (a shadow's too) finds who carries it, and the engines go on equal."""
    base = scen.materialize("example_1x1", workdir, laneChange=True)
    a = mod.Engine._with_backend(compacting(base, 9), 1, TWIN_LIB)
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    path, written_at = str(tmp_path / "lc.json"), None
    for s in range(600):
        a.next_step()
        b.next_step()
        if written_at is None and any(v.endswith("_shadow") for vs in a.get_lane_vehicles().values() for v in vs):
            a.snapshot().dump(path)
            written_at = a._vehicle_table()[1]
        if written_at is not None and a._vehicle_table()[1] - written_at >= 5 and s >= 150:
            break
    assert written_at is not None and a._vehicle_table()[1] - written_at >= 5, (written_at, a._vehicle_table())
    with open(path) as f:
        assert any(v["id"].endswith("_shadow") for v in json.load(f)["vehicles"])
    gone = set(b.get_vehicles(True))
    a.load_from_file(path)
    b.load_from_file(path)
    compactions = a._vehicle_table()[1]
    shadows = 0
    for s in range(300):
        if s % 20 == 0:
            va, vb = visible(a), visible(b)
            for k in va:
                assert va[k] == vb[k], (s, k)
            shadows += sum(v.endswith("_shadow") for vs in va["lane_vehicles"].values() for v in vs)
            for v in va["vehicles"]:
                assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (s, v)
                assert a.get_leader(v) == b.get_leader(v), (s, v)
            for v in sorted(gone - set(va["vehicles"]))[:10]:
                for e in (a, b):
                    with pytest.raises(RuntimeError, match="not found"):
                        e.get_vehicle_info(v)
        a.next_step()
        b.next_step()
    assert shadows > 0 and a._vehicle_table()[1] - compactions >= 5, (shadows, a._vehicle_table())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_load_from_file_after_compaction_hip(mod, scen, workdir, tmp_path, layout):
    """The HIP engine in the scenario above against the twin that never compacts, and — where oracle/_ref holds it — the
    unmodified reference at the same checkpoints (the CPU test pins the same scenario to the reference unconditionally)."""
    if REF_DIR not in sys.path:
        sys.path.insert(0, REF_DIR)
    try:
        import cityflow_ref as ref
    except ImportError:  # (not built or not shipped: the twin that never compacts still holds the HIP engine to the result)
        ref = None

    def make(c):
        e = mod.Engine(compacting(c, 40, layout=layout), 1)
        assert_hip_backend(e)
        return e
    load_file_after_compaction(mod, scen, workdir, tmp_path, make, ref, True)


# ---- tiles (TiledEngineHost::compactFromParts, csrc/host/tile_engine.cpp): every tile's part of the state, the vehicles alive
#      renumbered, every tile loading its part of the whole — automatic with every tile in one process, a collective over ranks
#      (cityflow_amd/tiled.py: DistributedEngine.compact_vehicles; tests/test_tiling.py::test_two_ranks_compaction_gloo)
def run_tiled_pair(a, b, steps, check_every):
    """`a`: tiles, compacting; `b`: one engine that never compacts; both take the same calls."""
    n_inter = len(b.intersection_ids())
    rng = np.random.default_rng(5)
    for s in range(steps):
        if s % 5 == 0:
            ph = rng.integers(0, 4, n_inter).astype(np.int32)
            a.set_tl_phases(ph)
            b.set_tl_phases(ph)
        a.next_step()
        b.next_step()
        if s % 7 == 0:
            assert np.array_equal(a.get_lane_vehicle_count_array(), b.get_lane_vehicle_count_array()), s
        if s % check_every == check_every - 1:
            va, vb = visible(a), visible(b)
            for k in va:
                assert va[k] == vb[k], (s, k)
            some = va["vehicles"][:: max(1, len(va["vehicles"]) // 12)]
            for v in some:
                assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (s, v)
                assert a.get_leader(v) == b.get_leader(v), (s, v)


def _tiled_compaction(mod, scen, workdir, make_tiled, steps):
    base = unsaturated_grid(scen, workdir)
    a = make_tiled(compacting(base, 250))
    b = mod.Engine._with_backend(compacting(base, 0), 1, TWIN_LIB)
    peak = 0
    files = {}
    for chunk in range(steps // 250):
        run_tiled_pair(a, b, 250, 125)
        peak = max(peak, a._vehicle_table()[0])
        if chunk == 0:  # files for the load_from_file leg below: the tiles' between two compactions, the single engine's
            assert a._vehicle_table()[1] >= 1, a._vehicle_table()
            for name, e in (("tiles", a), ("one", b)):
                files[name] = os.path.join(workdir, "tiled_compaction_%s_%d.json" % (name, os.getpid()))
                e.snapshot().dump(files[name])
            written_at = a._vehicle_table()[1]
        if chunk == 1:  # a custom speed for a vehicle still in its lane's waiting buffer rides through the next compaction
            waiting = [v for v in b.get_vehicles(True) if v not in set(b.get_vehicles(False))]
            for v in waiting[:3]:
                a.set_vehicle_speed(v, 3.25)
                b.set_vehicle_speed(v, 3.25)
    held, compactions = a._vehicle_table()
    assert b._vehicle_table()[1] == 0 and b._vehicle_table()[0] > peak and held < b._vehicle_table()[0]
    assert compactions >= steps // 250 - 1 and peak <= 250 + len(a.get_vehicles(True)) + 400, (held, compactions, peak)
    # archives still travel both ways between tiles that compact and an engine that does not
    arch_a, arch_b = a.snapshot(), b.snapshot()
    run_tiled_pair(a, b, 40, 20)
    a.load(arch_b)
    b.load(arch_a)
    run_tiled_pair(a, b, 100, 50)
    a._compact_vehicles()  # on request, too
    run_tiled_pair(a, b, 60, 30)
    # the files written after the first compaction, loaded after the later ones: every id resolves to its vehicle, and the
    # first compaction after the load starts from the tables the file gave
    assert a._vehicle_table()[1] - written_at >= 3, (a._vehicle_table(), written_at)
    for name, path in files.items():
        a.load_from_file(path)
        b.load_from_file(path)
        ids = b.get_vehicles(True)
        assert a.get_vehicles(True) == ids and len(ids) > 0, name
        for v in ids:
            assert a.get_vehicle_info(v) == b.get_vehicle_info(v), (name, v)
            assert a.get_leader(v) == b.get_leader(v), (name, v)
        compactions = a._vehicle_table()[1]
        run_tiled_pair(a, b, 300, 100)
        assert a._vehicle_table()[1] > compactions and a._vehicle_table()[0] <= 250 + len(a.get_vehicles(True)) + 400, (
            name, a._vehicle_table(), compactions)
    a.reset()
    b.reset()
    run_tiled_pair(a, b, 60, 30)


def test_tiled_compaction_bounds_the_tables_and_changes_nothing_twin(mod, scen, workdir):
    _tiled_compaction(mod, scen, workdir, lambda c: mod.TiledEngine(c, 2, 3, [], TWIN_LIB), 1250)


@pytest.mark.gpu
def test_tiled_compaction_hip_equals_a_twin_engine_that_never_compacts(mod, scen, workdir):
    def make(c):
        t = mod.TiledEngine(c, 2, 2)
        t.enable_mailboxes("compact_%d" % __import__("os").getpid())
        return t
    _tiled_compaction(mod, scen, workdir, make, 1000)
