"""GPU (-m gpu): the size of kr_cross's grid never changes a result.

The host sizes the launch from job counts the device reported some steps ago (csrc/hip/cfx_launch_policy.h); a grid that is too
small makes its groups take several vehicles one after the other, one that is too large is mostly blocks that find no job
— the lights, advanced by the LAST blocks of the grid, and block 0's bookkeeping must not depend on either.  The digits of `ringLanesPerWave` above the form digit force the number of blocks:

  16    one block per shard of the queue: every group loops over many vehicles
  0     the policy's own choice (at these sizes the floor of 64 blocks)
  4096  nearly every block finds no job

on the stock 6x6 grid, the 1x1 example and the seven-arm star (42 roadLinks at one junction: more crosses per laneLink than a
four-arm grid has), ring layout with the latency form of the cross phase, 150 steps of the fixed-time plan.  After every 10
steps everything conftest.assert_same_state compares — the vehicles, the lane counts, the scalars, the signals' phases and
remaining times — and `tie_events` equal the CPU twin's, which runs once per network.  The device's own count of launches with a
second pass (Engine._host_stats) must be above zero under 16 blocks and zero under 4096."""
import json

import numpy as np
import pytest

from conftest import SHADOW_GPU, TWIN_LIB, assert_hip_backend, full_state

import star_networks

pytestmark = pytest.mark.gpu

NETWORKS = ("grid_6x6", "example_1x1", "star7")
FORCED = (16, 0, 4096)
STEPS, EVERY = 150, 10
VEHICLE_KEYS = ("vid", "drivable", "prev_drivable", "dis", "speed", "leader", "blocker", "enter_ll_time", "route_pos")
SCALAR_KEYS = ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time", "tie_events")


def _config(scen, workdir, name, blocks):
    base = star_networks.make(workdir, name) if name.startswith("star") else scen.materialize(name, workdir)
    with open(base) as f:
        c = json.load(f)
    # (form digit 2: the action kernel walks the lanes, as on the bench workload; the blocks of kr_cross above it)
    c["cfx"] = {"layout": "ring", "crossMode": "latency", "ringLanesPerWave": 20000 + 100000 * blocks}
    out = base.replace(".json", "_crossgrid%d.json" % blocks)
    with open(out, "w") as f:
        json.dump(c, f)
    return out


def _record(eng):
    """What conftest.assert_same_state compares between two engines, and tie_events, of one engine."""
    s = full_state(eng)
    has = s["leader"] >= 0
    sc = eng._scalars()
    phase, remain = eng._tl_state()[:2]
    rec = {k: s[k].copy() for k in VEHICLE_KEYS}
    rec["gap of followers"] = s["gap"][has].copy()
    rec["lane counts"] = np.array(eng.get_lane_vehicle_count_array())
    rec["signal phase"], rec["signal remaining time"] = np.array(phase), np.array(remain)
    for k in SCALAR_KEYS:
        rec[k] = np.array(sc[k])
    return rec


_twin_records = {}


def _twin(mod, scen, workdir, name):
    if name not in _twin_records:
        eng = mod.Engine._with_backend(_config(scen, workdir, name, 0), 1, TWIN_LIB)
        recs, switches, last = [], 0, None
        for s in range(STEPS):
            eng.next_step()
            phase = eng._tl_state()[0].tolist()
            switches += int(last is not None and phase != last)
            last = phase
            if s % EVERY == EVERY - 1:
                recs.append(_record(eng))
        assert switches >= 3, "%s: the fixed plan switched %d times in %d steps" % (name, switches, STEPS)
        assert recs[-1]["active_vehicle_count"] > 0
        _twin_records[name] = recs
    return _twin_records[name]


@pytest.mark.parametrize("blocks", FORCED)
@pytest.mark.parametrize("name", NETWORKS)
def test_grid_size_never_changes_a_result(mod, scen, workdir, name, blocks):
    want = _twin(mod, scen, workdir, name)
    eng = mod.Engine(_config(scen, workdir, name, blocks), 1)
    assert_hip_backend(eng)
    assert eng._layout() == "ring"
    for s in range(STEPS):
        eng.next_step()
        if s % EVERY != EVERY - 1:
            continue
        got, ref = _record(eng), want[s // EVERY]
        for k in ref:
            assert got[k].shape == ref[k].shape, "%s, %d blocks, step %d: %s has shape %s, the twin's %s" % (
                name, blocks, s + 1, k, got[k].shape, ref[k].shape)
            assert np.array_equal(got[k], ref[k]), "%s, %d blocks, step %d: %s differs from the twin's" % (name, blocks, s + 1, k)
    if SHADOW_GPU:
        return  # (the twin launches nothing)
    hs = eng._host_stats(False)
    print("%s, %d blocks forced: %d launches with a second pass, at most %d passes, last grid %d blocks, %d jobs in the last step" % (
        name, blocks, hs["cross_multi_pass_launches"], hs["cross_max_passes"], hs["cross_last_grid_blocks"], hs["cross_last_jobs"]))
    if blocks:
        assert hs["cross_last_grid_blocks"] == blocks
    else:
        assert hs["cross_last_grid_blocks"] >= 64
    if blocks == 16:
        assert hs["cross_multi_pass_launches"] > 0 and hs["cross_max_passes"] > 1, hs
    if blocks == 4096:
        assert hs["cross_multi_pass_launches"] == 0 and hs["cross_max_passes"] == 1, hs
