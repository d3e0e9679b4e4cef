"""The lane-flow, movement-flow and trip trackers on at once (cityflow_amd/torch_io.py; one scaffold in csrc/hip/cfx_hip.hip and
csrc/host/trackers.h): through growth of the vehicle tables and of the rings, across a snapshot / load and a reset.  Every
tracker has its own suite (test_lane_flow.py, test_movement_flow.py, test_trip_stats.py); what they share — when a baseline is
due, which shadow grows with the vehicle tables, who ticks in which order — is only exercised together here.

One body, run twice.  On the device an engine that starts with small rings and vehicle tables runs against one that starts
large: all 6 + 8 + 9 outputs and the tracker columns of the front vehicles must be equal.  On the twin, where the host trackers
run and the capacity knob is inert, the peer is the three suites' Python models fed from the pre-existing getters.  Everything
is an integer or a copy: every comparison is array_equal."""
import copy
import os

import numpy as np
import pytest

from conftest import SHADOW_GPU, assert_hip_backend

torch = pytest.importorskip("torch")

import test_lane_flow as lane  # noqa: E402
import test_movement_flow as movement  # noqa: E402
import test_trip_stats as trips  # noqa: E402
from test_lane_features import twin  # noqa: E402
from test_lane_fronts import TRACKER, dict_lanes, filled, want_fronts  # noqa: E402

STEPS, SNAPSHOT_AT, LOAD_AT, RESET_AT, K = 300, 120, 140, 220, 4


def engine_outputs(eng, reset):
    return {"lane": eng.observe_lane_flow_array(reset=reset), "movement": eng.observe_movement_flow_array(reset=reset),
            "trips": eng.observe_trips_array()}


def engine_fronts(eng):
    t = filled(eng, TRACKER, K)
    eng.observe_lanes_tensor(**t)
    return {name: t[name].cpu().numpy() for name in TRACKER}


class SecondEngine:
    """The peer on the device: another engine taken through the same calls."""

    def __init__(self, eng):
        self.eng = eng

    def step(self):
        self.eng.next_step()

    def snapshot(self):
        self.archive = self.eng.snapshot()

    def load(self):
        self.eng.load(self.archive)

    def reset(self):
        self.eng.reset()

    def outputs(self, reset):
        return engine_outputs(self.eng, reset)

    def fronts(self):
        return engine_fronts(self.eng)


class ThreeModels:
    """The peer on the twin: the models of the three suites, fed by `eng`'s own pre-existing getters after each of its steps.
    `s` is the engine's step counter: a load puts it back, a reset zeroes it."""

    def __init__(self, eng):
        self.eng, self.s = eng, 0
        self.feed = movement.own_feed(eng)
        self.lane = lane.Model(eng.lane_ids())
        self.lane.baseline(eng.get_lane_vehicles(), 0)
        self.movement = movement.Model(eng._flat_net(), len(eng.intersection_ids()))
        self.movement.baseline(self.feed()[0], 0)
        self.trips = trips.Model()

    def step(self):
        self.s += 1
        self.lane.tick(self.eng.get_lane_vehicles(), self.eng.get_vehicle_speed(), self.s)
        self.movement.tick(*self.feed(), self.s)
        self.trips.tick(self.eng, self.s)

    def snapshot(self):
        self.kept = (self.s, copy.deepcopy(self.trips))

    def _baseline(self, s, trip_model):
        self.s, self.trips = s, trip_model
        self.lane.baseline(self.eng.get_lane_vehicles(), s)
        self.movement.baseline(self.feed()[0], s)
        self.trips.baseline()

    def load(self):  # (the engine has loaded: its getters show the archive's state)
        self._baseline(self.kept[0], copy.deepcopy(self.kept[1]))

    def reset(self):
        self._baseline(0, trips.Model())

    def outputs(self, reset):
        return {"lane": self.lane.drain(reset), "movement": self.movement.drain(reset),
                "trips": {k: np.asarray(v, dtype=trips.DTYPES[k]) for k, v in self.trips.outputs().items()}}

    def fronts(self):
        want = want_fronts(dict_lanes(self.eng, self.lane, self.s), K)
        return {name: want[name] for name in TRACKER}


def dense_config(scen, workdir, **cfx):
    base = scen.materialize("grid_6x6", workdir)
    d = os.path.dirname(base)
    flow = scen.dense_flows(os.path.join(d, "roadnet.json"), os.path.join(d, "flow_dense.json"), 400, seed=7, interval=2.0,
                            base_flow=os.path.join(d, "flow.json"))
    return scen.materialize("grid_6x6", workdir, flow_file=flow, cfx=dict(layout="ring", **cfx))


def track_all(eng):
    eng.track_lane_flow(True)
    eng.track_movement_flow(True)
    eng.track_trips(True)
    return eng


def all_trackers_body(eng, peer):
    names = {"lane": lane.NAMES, "movement": movement.NAMES, "trips": trips.NAMES}
    plan = lane.drain_plan(STEPS)
    seen = dict.fromkeys((("lane", "left"), ("lane", "waiting_steps"), ("movement", "left"), ("movement", "waiting_steps"),
                          ("trips", "finished")), 0)
    for i in range(STEPS):
        if i == SNAPSHOT_AT:
            archive = eng.snapshot()
            peer.snapshot()
        if i == LOAD_AT:
            eng.load(archive)
            peer.load()
        if i == RESET_AT:
            eng.reset()
            peer.reset()
        eng.next_step()
        peer.step()
        if i not in plan:
            continue
        got, want = engine_outputs(eng, plan[i]), peer.outputs(plan[i])
        for tracker, keys in names.items():
            assert sorted(got[tracker]) == sorted(keys)
            for k in keys:
                assert np.array_equal(got[tracker][k], want[tracker][k]), "call %d: %s %s differs (reset=%s)" % (i, tracker, k, plan[i])
        fronts, want_f = engine_fronts(eng), peer.fronts()
        for k in TRACKER:
            assert np.array_equal(fronts[k], want_f[k]), "call %d: %s differs at k = %d" % (i, k, K)
        for tracker, k in seen:
            seen[tracker, k] += int(got[tracker][k].sum())
    for (tracker, k), v in seen.items():  # (not a comparison of zeros)
        assert v > 0, "%s %s was zero at every drain" % (tracker, k)


def test_all_trackers_through_growth_reset_and_load_twin(mod, scen, workdir):
    eng = track_all(twin(mod, dense_config(scen, workdir)))
    all_trackers_body(eng, ThreeModels(eng))


@pytest.mark.gpu
def test_all_trackers_through_growth_reset_and_load(mod, scen, workdir):
    small = track_all(mod.Engine(dense_config(scen, workdir, ringCapacityPercent=30), 1))
    large = track_all(mod.Engine(dense_config(scen, workdir), 1))
    assert_hip_backend(small)
    all_trackers_body(small, SecondEngine(large))
    if not SHADOW_GPU:  # (on the twin the capacity knob is inert)
        assert small._host_stats(False)["table_grows_total"] > large._host_stats(False)["table_grows_total"]
