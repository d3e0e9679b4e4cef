"""Star junctions: one signalised intersection `C` whose arms differ in lane count and length — networks the grid generator cannot
make.  A plain helper module (not collected by pytest, no fixtures); tests/test_star_networks.py says which kernel branch each
of the three star* networks below exists for, tests/test_lane_change_paths.py does so for the lane-change runs.

star(): arm i lies at angle 2 pi i / arms.  Road in_i runs from the arm's outer node to C and out_i back, both with lanes[i]
lanes of lengths[i] metres.  C has one roadLink per ordered pair of arms (index = the pair's position in `pairs(arms)`), a
laneLink from every start lane to every end lane, no laneLink points (the engine generates the curves), one 15 s phase per arm
and five more phases: all right turns / exactly the roadLinks >= 32 / the roadLinks < 32 with index % 3 == 0 / none / the last.
With mid=True arm 0's outer node is a second, two-roadLink signal S (straight through both ways, 2 phases, one of them
serving only one roadLink) with 200 m roads far_in / far_out behind it: the network's rows become ragged."""
import json
import math
import os

from cityflow_amd import scenarios

LANE_WIDTH = 4.0
MAX_SPEED = 16.67
S_WIDTH = 10.0
FAR_LENGTH = 200.0
INTERVALS = (3.0, 4.0, 6.0)
ARM_PHASE_TIME = 15
EXTRA_PHASE_TIME = 5

# name -> star()'s arguments (tests/test_star_networks.py asserts what each is for from the JSON it produced)
NETWORKS = {
    "star7": dict(arms=7, lanes=[1] * 7, lengths=[300, 150, 60, 800, 300, 25, 300], width=20, mid=True),
    "star5": dict(arms=5, lanes=[1, 2, 3, 5, 2], lengths=[300, 300, 700, 300, 120], width=40, mid=True),
    "star3": dict(arms=3, lanes=[18, 1, 2], lengths=[200, 300, 300], width=80, mid=False),
    # with lane_change=True (tests/test_lane_change_paths.py): a 9-lane road whose many candidates share few target lanes ...
    "wide3": dict(arms=3, lanes=[9, 4, 3], lengths=[500, 700, 2000], width=60, mid=False),
    # ... and 5-lane roads of 1950 m (28 segments) and 940 m that come to hold more than 400 vehicles
    "long5": dict(arms=5, lanes=[5, 2, 3, 5, 2], lengths=[1900, 300, 700, 900, 120], width=40, mid=True),
}


def pairs(arms):
    """The ordered pairs (i, j) in C's roadLink order."""
    return [(i, j) for i in range(arms) for j in range(arms) if i != j]


def turn_type(i, j, arms):
    if j == (i + 1) % arms:
        return "turn_right"
    if j == (i - 1) % arms:
        return "turn_left"
    return "go_straight"


def phase_lists(arms):
    """availableRoadLinks of C's phases: one per arm, then the five described in the module docstring."""
    pr = pairs(arms)
    M = len(pr)
    phases = [[m for m, (i, _) in enumerate(pr) if i == a] for a in range(arms)]
    phases.append([m for m, (i, j) in enumerate(pr) if turn_type(i, j, arms) == "turn_right"])
    phases.append([m for m in range(M) if m >= 32])
    phases.append([m for m in range(M) if m < 32 and m % 3 == 0])
    phases.append([])
    phases.append([M - 1])
    return phases


def _road(rid, a, b, pa, pb, n_lanes):
    return {"id": rid, "startIntersection": a, "endIntersection": b, "points": [dict(pa), dict(pb)],
            "lanes": [{"width": LANE_WIDTH, "maxSpeed": MAX_SPEED} for _ in range(n_lanes)]}


def _road_link(kind, start, end, n_start, n_end):
    return {"type": kind, "startRoad": start, "endRoad": end, "direction": 0,
            "laneLinks": [{"startLaneIndex": a, "endLaneIndex": b} for a in range(n_start) for b in range(n_end)]}


def _virtual(iid, point, roads):
    return {"id": iid, "point": dict(point), "width": 0, "roads": roads, "roadLinks": [],
            "trafficLight": {"roadLinkIndices": [], "lightphases": [{"time": 30, "availableRoadLinks": []}]}, "virtual": True}


def star_roadnet(arms, lanes, lengths, width, mid):
    origin = {"x": 0.0, "y": 0.0}
    roads, inters = [], []
    for i in range(arms):
        ang = 2.0 * math.pi * i / arms
        has_s = mid and i == 0
        # (a lane is its road less the widths of the road's two intersections: the outer node lies that much further out)
        r = lengths[i] + width + (S_WIDTH if has_s else 0.0)
        p = {"x": r * math.cos(ang), "y": r * math.sin(ang)}
        outer = "S" if has_s else "V%d" % i
        roads.append(_road("in_%d" % i, outer, "C", p, origin, lanes[i]))
        roads.append(_road("out_%d" % i, "C", outer, origin, p, lanes[i]))
        if not has_s:
            inters.append(_virtual(outer, p, ["in_%d" % i, "out_%d" % i]))
            continue
        q = {"x": r + FAR_LENGTH + S_WIDTH, "y": 0.0}
        roads.append(_road("far_in", "V0", "S", q, p, lanes[0]))
        roads.append(_road("far_out", "S", "V0", p, q, lanes[0]))
        inters.append(_virtual("V0", q, ["far_in", "far_out"]))
        inters.append({"id": "S", "point": p, "width": S_WIDTH, "roads": ["far_in", "in_0", "out_0", "far_out"],
                       "roadLinks": [_road_link("go_straight", "far_in", "in_0", lanes[0], lanes[0]),
                                     _road_link("go_straight", "out_0", "far_out", lanes[0], lanes[0])],
                       "trafficLight": {"roadLinkIndices": [0, 1],
                                        "lightphases": [{"time": 20, "availableRoadLinks": [0, 1]},
                                                        {"time": 10, "availableRoadLinks": [1]}]},
                       "virtual": False})
    links = [_road_link(turn_type(i, j, arms), "in_%d" % i, "out_%d" % j, lanes[i], lanes[j]) for i, j in pairs(arms)]
    phases = [{"time": ARM_PHASE_TIME if p < arms else EXTRA_PHASE_TIME, "availableRoadLinks": served}
              for p, served in enumerate(phase_lists(arms))]
    inters.append({"id": "C", "point": origin, "width": width,
                   "roads": [rid % i for i in range(arms) for rid in ("in_%d", "out_%d")], "roadLinks": links,
                   "trafficLight": {"roadLinkIndices": list(range(len(links))), "lightphases": phases}, "virtual": False})
    return {"intersections": inters, "roads": roads}


def star_flows(arms, mid):
    flows = []
    for n, (i, j) in enumerate(pairs(arms)):
        route = (["far_in"] if mid and i == 0 else []) + ["in_%d" % i, "out_%d" % j] + (["far_out"] if mid and j == 0 else [])
        flows.append({"vehicle": dict(scenarios.GRID_VEHICLE), "route": route, "interval": INTERVALS[n % len(INTERVALS)],
                      "startTime": 0, "endTime": -1})
    return flows


def star(workdir, name, arms, lanes, lengths, width=30, mid=True, seed=0, layout="auto", lane_change=False):
    """Write roadnet.json, flow.json and a config into workdir/<name>/; returns the config path.  layout="dense" asks for the
    dense layout (cfx: {"layout": "dense"}), lane_change for "laneChange": true; every (seed, layout, lane_change) has a
    config file of its own beside the one network."""
    assert len(lanes) == len(lengths) == arms and layout in ("auto", "dense")
    d = os.path.join(workdir, name)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "roadnet.json"), "w") as f:
        json.dump(star_roadnet(arms, lanes, lengths, width, mid), f)
    with open(os.path.join(d, "flow.json"), "w") as f:
        json.dump(star_flows(arms, mid), f)
    cfg = {"interval": 1.0, "seed": seed, "dir": d + "/", "roadnetFile": "roadnet.json", "flowFile": "flow.json",
           "rlTrafficLight": False, "laneChange": bool(lane_change), "saveReplay": False}
    if layout == "dense":
        cfg["cfx"] = {"layout": "dense"}
    path = os.path.join(d, "config_seed%d_%s%s.json" % (seed, layout, "_lanechange" if lane_change else ""))
    with open(path, "w") as f:
        json.dump(cfg, f)
    return path


def make(workdir, name, seed=0, layout="auto", lane_change=False):
    """One of NETWORKS by name."""
    return star(workdir, name, seed=seed, layout=layout, lane_change=lane_change, **NETWORKS[name])
