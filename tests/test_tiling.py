"""One network tiled over several engines: partition and halo layout, and the property that matters —
the tiled network evolves bit-identically to the same network on one engine (every per-vehicle field, lane counts,
scalars), with all tiles in one process and with one tile per process over torch.distributed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, TWIN_LIB, free_port

KEYS = ["vid", "drivable", "prev_drivable", "leader", "blocker", "enter_ll_time", "route_pos", "dis", "speed", "gap"]


def dense_cfg(scen, workdir, name, n_extra, seed, interval, **config):
    base = scen.materialize(name, workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_tiled_%d_%d.json" % (n_extra, seed)), n_extra,
                            seed=seed, interval=interval, base_flow=os.path.join(d, "flow.json"))
    return scen.materialize(name, workdir, flow_file=flow, **config)


def same_state(va, vb, where):
    for k in KEYS:
        if k == "gap":  # only defined where a leader exists (the reference leaves it stale otherwise, vehicle.cpp:157-196)
            has = va["leader"] >= 0
            assert np.array_equal(va[k][has], vb[k][has]), "%s field gap" % where
        else:
            assert np.array_equal(va[k], vb[k]), "%s field %s" % (where, k)


def run_pair(mod, cfg, rows, cols, steps, lib, phases_rng=None, check_every=1, mailboxes=False):
    ref = mod.Engine._with_backend(cfg, 1, lib)
    til = mod.TiledEngine(cfg, rows, cols, [], lib)
    if mailboxes == "device":
        assert til.enable_device_mailboxes("testd_%d_%d%d" % (os.getpid(), rows, cols))
        assert til.halo_transport() == "device mailboxes"
    elif mailboxes:
        til.enable_mailboxes("test_%d_%d%d" % (os.getpid(), rows, cols))
    assert til.num_tiles == rows * cols and til.num_local == rows * cols
    n_inter = len(ref.intersection_ids())
    moved = False
    for s in range(steps):
        if phases_rng is not None and s % 10 == 0:
            ph = phases_rng.integers(0, 8, size=n_inter).astype(np.int32)
            ref.set_tl_phases(ph)
            til.set_tl_phases(ph)
        ref.next_step()
        til.next_step()
        if s % check_every:
            continue
        assert np.array_equal(ref.get_lane_vehicle_count_array(), til.get_lane_vehicle_count_array()), "step %d" % s
        va, vb = ref._vehicle_state(), til._vehicle_state()
        same_state(va, vb, "step %d" % s)
        sa, sb = ref._scalars(), til._scalars()
        for k in ("active_vehicle_count", "finished_vehicle_count", "cumulative_travel_time", "vehicle_steps",
                  "spawned_vehicle_count", "step"):
            assert sa[k] == sb[k], (s, k, sa[k], sb[k])
        moved = moved or sa["finished_vehicle_count"] > 0
    assert np.array_equal(ref.get_lane_waiting_vehicle_count_array(), til.get_lane_waiting_vehicle_count_array())
    assert ref.get_lane_vehicle_count() == til.get_lane_vehicle_count()
    return ref, til, moved


def test_partition_and_halo_layout(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    til = mod.TiledEngine(cfg, 2, 3, [], TWIN_LIB)
    owner = np.array(til.owner())
    assert set(owner.tolist()) == set(range(6))
    # message a -> b and b's expectation of it have the same size, for every pair of neighbours
    peers = {til.local_rank(i): til.peers(i) for i in range(til.num_local)}
    for a, plist in peers.items():
        for (b, so, sb, ro, rb) in plist:
            back = [p for p in peers[b] if p[0] == a]
            assert len(back) == 1 and back[0][2] == rb and back[0][4] == sb
        assert sum(p[2] for p in plist) == til.send_buffer(a).shape[0]
        assert sum(p[4] for p in plist) == til.recv_buffer(a).shape[0]
    # a tile never talks to itself, and 2x3 blocks have 2..3 neighbours each (no diagonal roads in a grid)
    assert all(a not in [p[0] for p in pl] and 2 <= len(pl) <= 3 for a, pl in peers.items())


@pytest.mark.parametrize("rows,cols", [(1, 2), (2, 2), (3, 3)])
def test_tiled_equals_single_twin(mod, scen, workdir, rows, cols):
    cfg = scen.materialize("grid_6x6", workdir)
    _, _, moved = run_pair(mod, cfg, rows, cols, 700, TWIN_LIB)
    assert moved  # vehicles crossed the whole grid, i.e. several tile borders


def test_tiled_mailboxes_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    run_pair(mod, cfg, 2, 3, 400, TWIN_LIB, mailboxes=True)


def test_tiled_rl_lights_and_reset_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    ref, til, _ = run_pair(mod, cfg, 2, 2, 300, TWIN_LIB, phases_rng=np.random.default_rng(5), mailboxes=True)
    ref.reset(True)
    til.reset(True)
    for _ in range(50):
        ref.next_step()
        til.next_step()
    assert np.array_equal(ref.get_lane_vehicle_count_array(), til.get_lane_vehicle_count_array())
    assert ref._scalars()["active_vehicle_count"] == til._scalars()["active_vehicle_count"] > 0


def test_tiled_dense_30x30_twin(mod, scen, workdir):
    cfg = dense_cfg(scen, workdir, "grid_30x30", 300, 3, 4.0)
    run_pair(mod, cfg, 2, 4, 160, TWIN_LIB, check_every=8)


def test_short_cut_lanes_are_rejected(mod, scen, workdir):
    # the 1x1 example has 300 m roads but no second real intersection: no valid 1x2 partition
    cfg = scen.materialize("example_1x1", workdir)
    with pytest.raises(RuntimeError):
        mod.TiledEngine(cfg, 1, 2, [], TWIN_LIB)


def _torchrun(tmp_path, cfg, lib, rows, cols, steps, nproc, port, extra_env=None):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", TMPDIR=str(tmp_path))
    env.update(extra_env or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % nproc, "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "tiled_worker.py"), cfg, lib, str(rows),
           str(cols), str(steps)]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)


@pytest.mark.parametrize("mailboxes", ["0", "1"])
def test_two_ranks_gloo(scen, workdir, tmp_path, mailboxes):
    """One tile per process; halo staged over gloo ("0") or through shared-memory mailboxes ("1")."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 1, 2, 200, 2, free_port(), {"CFX_TEST_MAILBOXES": mailboxes})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 200" in out.stdout


@pytest.mark.parametrize("mailboxes", ["0", "1"])
def test_two_ranks_archive_and_routes_gloo(scen, workdir, tmp_path, mailboxes):
    """snapshot (one part per rank) / load (no communication) / setRoute (position merged over ranks) with one tile per
    process: tests/tiled_worker.py, CFX_TEST_ARCHIVE."""
    cfg = dense_cfg(scen, workdir, "grid_6x6", 60, 5, 1.0)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 2, 1, 120, 2, free_port(), {"CFX_TEST_MAILBOXES": mailboxes, "CFX_TEST_ARCHIVE": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 120" in out.stdout and "ARCHIVE_OK" in out.stdout


@pytest.mark.parametrize("mailboxes", ["0", "1"])
def test_two_ranks_compaction_gloo(scen, workdir, tmp_path, mailboxes):
    """Bounded memory over ranks: the tiles forget their finished vehicles every 300 vehicle numbers — every rank's part of the
    state gathered on every rank, the vehicles alive renumbered, every rank keeping its tile's part (DistributedEngine.
    compact_vehicles, TiledEngineHost::compactFromParts; the reference frees a vehicle when it finishes, engine.cpp:296-310) —
    and stay equal, id by id, to one engine that never forgets."""
    cfg = scen.generate_grid(6, 6, workdir, flow_interval=12.0)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 1, 2, 700, 2, free_port(), {"CFX_TEST_MAILBOXES": mailboxes, "CFX_TEST_COMPACT": "300"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 700" in out.stdout and "COMPACT_OK" in out.stdout


def test_two_ranks_compaction_then_load_from_file_gloo(scen, workdir, tmp_path):
    """... and an Archive file the single engine wrote before the compactions, loaded afterwards by every rank's tiles
    (DistributedEngine.load_from_file: every rank reads the same file and keeps its tile's part) and by the single engine: every
    id resolves to its vehicle and both go on equal through the next compaction (tests/tiled_worker.py: CFX_TEST_LOAD_FILE)."""
    cfg = scen.generate_grid(6, 6, workdir, flow_interval=12.0)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 1, 2, 700, 2, free_port(),
                    {"CFX_TEST_MAILBOXES": "1", "CFX_TEST_COMPACT": "300", "CFX_TEST_LOAD_FILE": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 700" in out.stdout and "COMPACT_OK" in out.stdout and "LOAD_FILE_OK" in out.stdout


def test_two_ranks_replay_gloo(scen, workdir, tmp_path):
    """saveReplay with one tile per process: the replay file rank 0 writes equals the single engine's (tests/tiled_worker.py)."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 1, 2, 30, 2, free_port(), {"CFX_TEST_MAILBOXES": "1", "CFX_TEST_REPLAY": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "REPLAY_OK" in out.stdout


def test_two_ranks_device_resident_messages_gloo(scen, workdir, tmp_path):
    """The "rccl" transport's code path (messages stay in the engine's buffers, one P2P batch on the default group) with
    the CPU twin, whose device buffers are host memory, over gloo."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 1, 2, 200, 2, free_port(), {"CFX_TEST_TRANSPORT": "rccl"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 200" in out.stdout and "transport rccl" in out.stdout


def test_transport_fallback_order_gloo(scen, workdir, tmp_path):
    """transport=None: a CPU engine cannot share heap mailboxes between processes, so "device" is skipped by every rank
    together and the host-memory mailboxes are taken."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 1, 2, 60, 2, free_port(), {"CFX_TEST_TRANSPORT": "", "CFX_TEST_MAILBOXES": "auto"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "transport host" in out.stdout


def test_tiled_device_mailboxes_in_process_twin(mod, scen, workdir):
    """All tiles in one process with the mailboxes allocated through cfx_halo_mailbox_alloc (heap memory for the CPU
    engine, HBM for the HIP engine)."""
    cfg = scen.materialize("grid_6x6", workdir)
    run_pair(mod, cfg, 2, 2, 300, TWIN_LIB, mailboxes="device")


def test_four_ranks_separate_halo_group(scen, workdir, tmp_path):
    """2x2 tiles over four processes, the halo on its own gloo group (as under an RCCL default group), staged transport."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, TWIN_LIB, 2, 2, 120, 4, free_port(), {"CFX_TEST_MAILBOXES": "0", "CFX_TEST_SUBGROUP": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 120" in out.stdout


# ------------------------------------------------------------------------------------------------ MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("name,rows,cols,steps", [("grid_6x6", 2, 2, 700), ("grid_6x6", 3, 3, 400)])
def test_tiled_equals_single_hip(mod, scen, workdir, name, rows, cols, steps):
    cfg = scen.materialize(name, workdir)
    _, _, moved = run_pair(mod, cfg, rows, cols, steps, mod._default_backend_path())
    assert moved or steps < 500


@pytest.mark.gpu
def test_tiled_dense_30x30_hip_vs_twin(mod, scen, workdir):
    """2x4 tiles of the dense 30x30 workload on the GPU against the single-engine CPU twin."""
    cfg = dense_cfg(scen, workdir, "grid_30x30", 600, 3, 4.0)
    ref = mod.Engine._with_backend(cfg, 1, TWIN_LIB)
    til = mod.TiledEngine(cfg, 2, 4)
    for s in range(240):
        ref.next_step()
        til.next_step()
        if s % 20 == 19:
            assert np.array_equal(ref.get_lane_vehicle_count_array(), til.get_lane_vehicle_count_array()), "step %d" % s
    va, vb = ref._vehicle_state(), til._vehicle_state()
    same_state(va, vb, "final")
    assert va["vid"].shape[0] > 20000


@pytest.mark.gpu
def test_tiled_rl_lights_hip(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    run_pair(mod, cfg, 2, 3, 300, mod._default_backend_path(), phases_rng=np.random.default_rng(11))


@pytest.mark.gpu
def test_tiled_mailboxes_hip(mod, scen, workdir):
    """All tiles in one process, halo device to device through the mailboxes (import kernels wait on epochs)."""
    cfg = scen.materialize("grid_6x6", workdir)
    run_pair(mod, cfg, 2, 3, 500, mod._default_backend_path(), mailboxes=True)


@pytest.mark.gpu
def test_tiled_device_mailboxes_hip(mod, scen, workdir):
    """All tiles in one process, mailboxes in device memory (cfx_halo_mailbox_alloc), export kernels write them directly."""
    cfg = scen.materialize("grid_6x6", workdir)
    run_pair(mod, cfg, 2, 3, 500, mod._default_backend_path(), mailboxes="device")


@pytest.mark.gpu
def test_two_ranks_one_gpu_peer_memory(scen, workdir, tmp_path):
    """Two processes, one tile each, the halo through mailboxes in the RECEIVER's HBM opened with hipIpc (here both on
    this box's one GPU; on a node the same handles are peer memory over xGMI)."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, "", 1, 2, 150, 2, free_port(), {"CITYFLOW_AMD_DEVICE": "0", "CFX_TEST_TRANSPORT": "device"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 150" in out.stdout and "transport device" in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("transport", ["device", "rccl"])
def test_one_tile_per_physical_gpu(scen, workdir, tmp_path, transport):
    """One tile per PHYSICAL GPU (needs >= 2): peer-HBM mailboxes over xGMI, and RCCL send / recv of the messages."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs on this box")
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, "", 1, 2, 150, 2, free_port(), {"CFX_TEST_TRANSPORT": transport, "CFX_TEST_DIST_BACKEND": "nccl"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 150" in out.stdout and ("transport " + transport) in out.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("mailboxes", ["0", "1"])
def test_two_ranks_one_gpu(scen, workdir, tmp_path, mailboxes):
    """Two processes (sharing this box's one GPU), one tile each; halo over gloo ("0") or GPU-written mailboxes ("1")."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, "", 1, 2, 150, 2, free_port(),
                    {"CITYFLOW_AMD_DEVICE": "0", "CFX_TEST_MAILBOXES": mailboxes})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 150" in out.stdout


@pytest.mark.gpu
def test_two_ranks_one_gpu_compaction_and_archive(scen, workdir, tmp_path):
    """Two processes sharing this box's GPU, HIP tiles, GPU-written mailboxes: the tiles forget their finished vehicles every 300
    vehicle numbers (a collective: every rank's part of the state on every rank, `Lane::history` in the parts) and stay equal,
    id by id, to one engine that never forgets, also after both load a file the single engine wrote before the compactions; then snapshot / dump (the single engine's file, history included) / load /
    setRoute over the ranks (tests/tiled_worker.py: CFX_TEST_COMPACT, CFX_TEST_ARCHIVE)."""
    cfg = scen.generate_grid(6, 6, workdir, flow_interval=12.0)
    out = _torchrun(tmp_path, cfg, "", 1, 2, 700, 2, free_port(), {"CITYFLOW_AMD_DEVICE": "0", "CFX_TEST_MAILBOXES": "1", "CFX_TEST_COMPACT": "300",
                                                                   "CFX_TEST_LOAD_FILE": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 700" in out.stdout and "COMPACT_OK" in out.stdout and "LOAD_FILE_OK" in out.stdout
    cfg = dense_cfg(scen, workdir, "grid_6x6", 60, 5, 1.0)
    out = _torchrun(tmp_path, cfg, "", 2, 1, 120, 2, free_port(), {"CITYFLOW_AMD_DEVICE": "0", "CFX_TEST_MAILBOXES": "1", "CFX_TEST_ARCHIVE": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 120" in out.stdout and "ARCHIVE_OK" in out.stdout


@pytest.mark.gpu
def test_four_ranks_one_gpu_mailboxes(scen, workdir, tmp_path):
    """2x2 tiles, four processes on this box's GPU: every tile has two neighbours, mailboxes in both directions."""
    cfg = scen.materialize("grid_6x6", workdir)
    out = _torchrun(tmp_path, cfg, "", 2, 2, 150, 4, free_port(), {"CITYFLOW_AMD_DEVICE": "0", "CFX_TEST_MAILBOXES": "1"})
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "TILED_OK 150" in out.stdout


def _api_compare(mod, cfg, lib, rows, cols):
    """Every query / control call of the reference API on the tiled engine vs the single engine."""
    ref = mod.Engine._with_backend(cfg, 1, lib)
    til = mod.TiledEngine(cfg, rows, cols, [], lib)
    info = {"length": 4.0, "maxSpeed": 12.0, "minGap": 2.0}
    route = ["road_0_1_0", "road_1_1_0", "road_2_1_0", "road_3_1_0"]  # crosses the vertical cut of a 2x2 tiling of 6x6
    slowed = None
    for s in range(260):
        if s in (5, 40):
            ref.push_vehicle(info, route)
            til.push_vehicle(info, route)
        if s == 120:  # slow one running vehicle down on both
            slowed = sorted(ref.get_vehicle_speed())[7]
            ref.set_vehicle_speed(slowed, 1.5)
            til.set_vehicle_speed(slowed, 1.5)
        ref.next_step()
        til.next_step()
        if s % 20 == 19 or s in (120, 121):
            assert ref.get_vehicle_speed() == til.get_vehicle_speed(), "step %d" % s
            assert ref.get_vehicle_distance() == til.get_vehicle_distance(), "step %d" % s
            assert ref.get_lane_vehicles() == til.get_lane_vehicles(), "step %d" % s
            assert ref.get_vehicles(True) == til.get_vehicles(True), "step %d" % s
            assert ref.get_vehicles() == til.get_vehicles()
            assert ref.get_average_travel_time() == til.get_average_travel_time()
            assert ref.get_vehicle_count() == til.get_vehicle_count()
    running = ref.get_vehicles()
    assert "manually_pushed_0" in ref.get_vehicles(True) or ref.get_vehicle_info("manually_pushed_0")["running"] == "0"
    for vid in running[:40] + ["manually_pushed_1"]:
        assert ref.get_vehicle_info(vid) == til.get_vehicle_info(vid), vid
        assert ref.get_leader(vid) == til.get_leader(vid), vid
    with pytest.raises(RuntimeError):
        til.get_leader("flow_999_0")
    assert slowed is not None


def test_tiled_full_api_twin(mod, scen, workdir):
    _api_compare(mod, scen.materialize("grid_6x6", workdir), TWIN_LIB, 2, 2)


@pytest.mark.gpu
def test_tiled_full_api_hip(mod, scen, workdir):
    _api_compare(mod, scen.materialize("grid_6x6", workdir), mod._default_backend_path(), 2, 2)


# ---- archive, routes, replay on the tiled engine (reference src/engine/archive.cpp, engine.cpp:852-866, 518-554) ----------
def _same_now(ref, til, where):
    assert np.array_equal(ref.get_lane_vehicle_count_array(), til.get_lane_vehicle_count_array()), where
    assert np.array_equal(ref.get_lane_waiting_vehicle_count_array(), til.get_lane_waiting_vehicle_count_array()), where
    same_state(ref._vehicle_state(), til._vehicle_state(), where)
    sa, sb = ref._scalars(), til._scalars()
    for k in ("active_vehicle_count", "finished_vehicle_count", "cumulative_travel_time", "step"):
        assert sa[k] == sb[k], (where, k, sa[k], sb[k])


def without_lane_history(dump, tiles_keep_it=True):
    """Tiles keep Lane::history where one engine does by default (ring tiles, networks up to 20 k lanes; the step's record is
    taken behind the step's halo import): the dumps are compared whole.  Where they do not (dense tiles), the single engine's
    is blanked the way a dump of such tiles has it."""
    if tiles_keep_it:
        return dump
    for dv in dump["drivables"].values():
        if "history" in dv:
            dv.update(history=[], historyVehicleNum=0, historyAverageSpeed=0.0)
    return dump


def _archive_compare(mod, cfg, lib, rows, cols, tmp_path, mailboxes=False):
    """snapshot / load / dump / load_from_file on tiles: archives travel in both directions between one engine and the tiles,
    in memory and through the reference's JSON format, and the run that follows a load is the run that followed the snapshot"""
    ref = mod.Engine._with_backend(cfg, 1, lib)
    til = mod.TiledEngine(cfg, rows, cols, [], lib)
    if mailboxes:
        til.enable_mailboxes("testa_%d_%d%d" % (os.getpid(), rows, cols))
    for s in range(140):
        if s == 100:
            v = sorted(ref.get_vehicle_speed())[3]
            ref.set_vehicle_speed(v, 2.5)  # a custom speed pending in the archive
            til.set_vehicle_speed(v, 2.5)
        ref.next_step()
        til.next_step()
    ref.set_vehicle_speed(sorted(ref.get_vehicle_speed())[5], 1.0)
    til.set_vehicle_speed(sorted(til.get_vehicle_speed())[5], 1.0)
    a_ref, a_til = ref.snapshot(), til.snapshot()
    p_ref, p_til = str(tmp_path / "ref.json"), str(tmp_path / "til.json")
    a_ref.dump(p_ref)
    a_til.dump(p_til)
    import json
    assert til._keeps_lane_history()
    assert without_lane_history(json.load(open(p_ref)), til._keeps_lane_history()) == json.load(open(p_til))  # the tiles' archive IS the single engine's
    after = []
    for s in range(60):
        ref.next_step()
        til.next_step()
        after.append((ref.get_lane_vehicle_count_array().copy(), ref._scalars()["cumulative_travel_time"]))
    _same_now(ref, til, "after the snapshot")
    # tiles <- their own archive; tiles <- the single engine's archive; single engine <- the tiles' archive
    for name, load in (("tiles <- tiles", lambda: til.load(a_til)), ("tiles <- engine", lambda: til.load(a_ref)),
                       ("tiles <- file", lambda: til.load_from_file(p_ref))):
        load()
        if name == "tiles <- file":
            ref.load_from_file(p_ref)  # (a file load numbers the vehicles anew)
        else:
            ref.load(a_til)
        _same_now(ref, til, name + ": right after the load")
        for s in range(60):
            ref.next_step()
            til.next_step()
            if name != "tiles <- file":  # (the JSON format does not carry pending custom speeds: reference archive.cpp)
                assert np.array_equal(til.get_lane_vehicle_count_array(), after[s][0]), (name, s)
        if name == "tiles <- file":
            ref.load_from_file(p_til)
            til.load_from_file(p_til)
            for s in range(60):
                ref.next_step()
                til.next_step()
        _same_now(ref, til, name + ": 60 steps later")
    # an older archive after a newer state, and a reset in between
    til.reset()
    ref.reset()
    til.load(a_ref)
    ref.load(a_ref)
    for s in range(30):
        ref.next_step()
        til.next_step()
    _same_now(ref, til, "load after reset")


def test_tiled_archive_twin(mod, scen, workdir, tmp_path):
    _archive_compare(mod, dense_cfg(scen, workdir, "grid_6x6", 80, 3, 1.0), TWIN_LIB, 2, 2, tmp_path)


def test_tiled_archive_mailboxes_twin(mod, scen, workdir, tmp_path):
    _archive_compare(mod, dense_cfg(scen, workdir, "grid_6x6", 80, 3, 1.0), TWIN_LIB, 2, 3, tmp_path, mailboxes=True)


@pytest.mark.gpu
def test_tiled_archive_hip(mod, scen, workdir, tmp_path):
    _archive_compare(mod, dense_cfg(scen, workdir, "grid_6x6", 80, 3, 1.0), mod._default_backend_path(), 2, 2, tmp_path)


def _route_compare(mod, cfg, lib, rows, cols):
    """Engine::setRoute on tiles: same verdicts, same traffic afterwards (the vehicle takes its new route across the cut)"""
    ref = mod.Engine._with_backend(cfg, 1, lib)
    til = mod.TiledEngine(cfg, rows, cols, [], lib)
    info = {"length": 4.0, "maxSpeed": 12.0, "minGap": 2.0}
    ref.push_vehicle(info, ["road_0_1_0", "road_1_1_0"])
    til.push_vehicle(info, ["road_0_1_0", "road_1_1_0"])
    verdicts = []
    for s in range(200):
        if s in (3, 30, 31, 60):
            # waiting or running on its first roads: send it across the vertical cut; once with a road that does not exist;
            # once with a road that cannot follow
            for anchors in (["road_2_1_0", "road_3_1_0", "road_4_1_0"], ["no_such_road"], ["road_0_1_0"]):
                a = ref.set_vehicle_route("manually_pushed_0", anchors)
                b = til.set_vehicle_route("manually_pushed_0", anchors)
                assert a == b, (s, anchors, a, b)
                verdicts.append(a)
        if s == 100:  # some flow vehicles as well, whatever state they are in
            for v in sorted(ref.get_vehicles(True))[:12]:
                assert ref.set_vehicle_route(v, ["road_3_2_1"]) == til.set_vehicle_route(v, ["road_3_2_1"]), v
        ref.next_step()
        til.next_step()
        if s % 10 == 9:
            _same_now(ref, til, "step %d" % s)
    assert any(verdicts) and not all(verdicts)
    assert ref.set_vehicle_route("flow_999_0", ["road_1_1_0"]) is False and til.set_vehicle_route("flow_999_0", ["road_1_1_0"]) is False
    assert ref.get_vehicle_info("manually_pushed_0") == til.get_vehicle_info("manually_pushed_0")


def test_tiled_set_route_twin(mod, scen, workdir):
    _route_compare(mod, scen.materialize("grid_6x6", workdir), TWIN_LIB, 2, 2)


@pytest.mark.gpu
def test_tiled_set_route_hip(mod, scen, workdir):
    _route_compare(mod, scen.materialize("grid_6x6", workdir), mod._default_backend_path(), 2, 2)


def test_tiled_replay_twin(mod, scen, workdir, tmp_path):
    """saveReplay on tiles: the same roadnet log and the same replay lines as one engine (engine.cpp:518-554)"""
    outs = []
    for kind in ("single", "tiled"):
        cfg = scen.materialize("grid_6x6", workdir, saveReplay=True, roadnetLogFile="rn_%s.json" % kind, replayLogFile="rp_%s.txt" % kind)
        eng = mod.Engine._with_backend(cfg, 1, TWIN_LIB) if kind == "single" else mod.TiledEngine(cfg, 2, 2, [], TWIN_LIB)
        for s in range(120):
            if s == 60:
                eng.set_save_replay(False)
            if s == 80:
                eng.set_save_replay(True)
            eng.next_step()
        d = os.path.dirname(cfg)
        del eng
        outs.append((open(os.path.join(d, "rn_%s.json" % kind)).read(), open(os.path.join(d, "rp_%s.txt" % kind)).read()))
    assert outs[0][0] == outs[1][0]
    assert outs[0][1] == outs[1][1] and outs[0][1].count("\n") == 100
