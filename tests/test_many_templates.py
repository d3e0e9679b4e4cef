"""More vehicle templates than the step kernels stage in LDS.

Up to kLdsTempl = 32 templates (csrc/hip/cfx_kernels.h) a step kernel reads the template table from its block's LDS copy;
beyond that the host launches the instantiation that reads it from global memory (`templatesOf`, `Impl::manyTempl`).  The
stock scenarios have one template, so nothing else reaches the second set of kernels: here grid_6x6 carries flows with 32
(the last count that is staged), 33 (the first that is not) and 40 distinct templates.

GPU (-m gpu): every organisation of the step — ring layout lane-walking, the forced list form with both cross kernels, the dense
layout with both cross kernels, lane change — against the CPU twin on every field, 120 steps.
CPU: the flows do produce that many templates after the loader's deduplication, and the twin equals the unmodified
reference on them (the oracle is pinned there too; without lane change, whose reference run needs a process of its own)."""
import json
import os

import numpy as np
import pytest

from conftest import TWIN_LIB, assert_hip_backend, assert_same_state, checkpoint_record, full_state

COUNTS = (32, 33, 40)
STEPS = 120
N_FLOWS = 48  # (the grid's own 24 straight flows + 24 seeded random walks: every template is on the road from step 0)

FORMS = {
    "ring": {},
    "ring-list-throughput": {"layout": "ring", "ringLanesPerWave": 30000, "crossMode": "throughput"},
    "ring-list-latency": {"layout": "ring", "ringLanesPerWave": 30000, "crossMode": "latency"},
    "dense-latency": {"layout": "dense", "denseForm": 256 + 2, "crossMode": "latency"},
    "dense-throughput": {"layout": "dense", "denseForm": 256 + 2 + 4, "crossMode": "throughput"},
}


def _template(scen, i):
    """Template `i`: the generator's, with every field the kernels read from the table moved by a binary fraction (a literal
    both JSON readers turn into the same double).  Two templates never agree in all fields."""
    v = dict(scen.GRID_VEHICLE)
    v["length"] = 4.0 + 0.25 * (i % 8)
    v["minGap"] = 2.0 + 0.125 * (i % 5)
    v["maxSpeed"] = 12.0 + 0.5 * (i % 11)
    v["maxPosAcc"] = 1.5 + 0.125 * (i % 7)
    v["usualPosAcc"] = 1.5 + 0.125 * (i % 7)
    v["maxNegAcc"] = 4.0 + 0.25 * (i % 4)
    v["usualNegAcc"] = 3.5 + 0.25 * (i % 4)
    v["headwayTime"] = 1.25 + 0.0625 * i
    return v


def _flows(scen, workdir, n):
    """grid_6x6 with N_FLOWS flows that carry `n` distinct templates; returns (flow file, roadnet file)."""
    d = os.path.dirname(scen.materialize("grid_6x6", workdir))
    roadnet = os.path.join(d, "roadnet.json")
    base = os.path.join(d, "flow_templ_base.json")
    scen.dense_flows(roadnet, base, N_FLOWS - 24, seed=4242, interval=3.0, base_flow=os.path.join(d, "flow.json"))
    with open(base) as f:
        flows = json.load(f)
    assert len(flows) == N_FLOWS
    for i, fl in enumerate(flows):
        fl["vehicle"] = _template(scen, i % n)
        fl["interval"] = 2.0 + (i % 3)
    out = os.path.join(d, "flow_templ%d.json" % n)
    with open(out, "w") as f:
        json.dump(flows, f)
    return out, roadnet


def _cfg(scen, workdir, n, **config):
    flow, _ = _flows(scen, workdir, n)
    return scen.materialize("grid_6x6", workdir, flow_file=flow, **config)


@pytest.mark.parametrize("n", COUNTS)
def test_flows_carry_that_many_templates(mod, scen, workdir, n):
    flow, roadnet = _flows(scen, workdir, n)
    sched = mod._spawn_schedule(roadnet, flow, 1.0, 0, 1, 8, 0)
    templates = {rec[4] for step in sched for rec in step}
    assert templates == set(range(n)), "the loader's table has %d templates in use, %d wanted" % (len(templates), n)
    assert len(sched[0]) == N_FLOWS  # (all of them on their way in the very first step)


@pytest.mark.parametrize("n", COUNTS)
def test_twin_equals_reference_with_many_templates(mod, ref_module, scen, workdir, n):
    cfg = _cfg(scen, workdir, n)
    twin, ref = mod.Engine._with_backend(cfg, 1, TWIN_LIB), ref_module.Engine(cfg, 1)
    for s in range(STEPS):
        twin.next_step()
        ref.next_step()
        if s % 10 == 9:
            assert checkpoint_record(twin) == checkpoint_record(ref), "%d templates, step %d" % (n, s + 1)
    assert twin.get_vehicle_count() > 500  # (the comparison is about traffic, not an empty grid)


@pytest.mark.gpu
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("n", COUNTS)
def test_hip_equals_twin_with_many_templates(mod, scen, workdir, n, form):
    cfg = _cfg(scen, workdir, n, **({"cfx": FORMS[form]} if FORMS[form] else {}))
    hip, twin = mod.Engine(cfg, 1), mod.Engine._with_backend(cfg, 1, TWIN_LIB)
    assert_hip_backend(hip)
    for s in range(STEPS):
        hip.next_step()
        twin.next_step()
        if s % 20 == 19:
            assert_same_state(hip, twin, "%s, %d templates, step %d" % (form, n, s + 1))
    assert hip.get_vehicle_count() > 500


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
def test_hip_lane_change_equals_twin_with_many_templates(mod, scen, workdir, n):
    """laneChange runs the dense layout's k_action / k_cross<true> (or k_cross2<true>): the third set of instantiations"""
    for cross in ("latency", "throughput"):
        cfg = _cfg(scen, workdir, n, laneChange=True, cfx={"crossMode": cross})
        hip, twin = mod.Engine(cfg, 1), mod.Engine._with_backend(cfg, 1, TWIN_LIB)
        assert_hip_backend(hip)
        for s in range(STEPS):
            hip.next_step()
            twin.next_step()
            if s % 20 == 19:  # (every column of the state, the lane-change ones included: tests/test_lane_change.py)
                a, b = full_state(hip), full_state(twin)
                assert a.keys() == b.keys() and "lc_flags" in a
                for k in a:
                    assert np.array_equal(a[k], b[k]), "lane change, %s cross, %d templates, step %d: %s" % (cross, n, s + 1, k)
                assert np.array_equal(hip.get_lane_vehicle_count_array(), twin.get_lane_vehicle_count_array())
