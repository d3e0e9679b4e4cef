"""set_vehicle_speeds_tensor inside random call sequences: every settle survives the transitions.

A short driver of this file's own, in the manner of tests/test_vehicle_rows_sequences.py.  One stream of random operations — runs
of steps (long enough for a step to defer its commit), pushed vehicles, route changes, per-vehicle speed calls, snapshot / load,
checkpoint / rollback, reset, the lane-flow tracker on and off — drives two engines.  A batched speed call is one more operation
of the stream: the first engine takes set_vehicle_speeds_tensor, the second set_vehicle_speed() for the rows in force, in row
order — of a vehicle named twice the higher row, so the duplicates of a call are in the stream too, beside padding, masked rows
and numbers that name no vehicle.  A per-vehicle call may follow or precede a batched one before the same step: the later call
wins on both.  After every round conftest.assert_same_state holds between the two."""
import numpy as np
import pytest

from conftest import assert_same_state

torch = pytest.importorskip("torch")

from test_device_sequences import neighbour, pushed_route  # noqa: E402
from test_device_tensors import tensor_device, twin  # noqa: E402
from test_lane_flow import hip_engine  # noqa: E402
from test_vehicle_speeds import NAN, dev, issued, live_numbers  # noqa: E402

OPS = (("steps", 8.0), ("batched", 5.0), ("speed", 2.0), ("push", 1.5), ("reroute", 1.5), ("reset", 0.4), ("snapshot", 1.0),
       ("load", 1.0), ("checkpoint", 1.0), ("rollback", 1.0), ("track", 1.0))
ROUNDS = 40
SEED = 93


def batched(a, b, rng, where):
    """-> (rows in force, rows ignored, vehicles named twice)"""
    live = live_numbers(b)
    n = int(rng.choice([0, 1, 64, 65, len(live) + 9]))
    vehicle = np.full(n, -1, dtype=np.int32)
    speed = rng.uniform(0.0, 12.0, n)
    kind = rng.random(n)
    named = kind < 0.7 if len(live) else np.zeros(n, dtype=bool)
    vehicle[named] = rng.choice(live, int(named.sum())) if len(live) else -1  # (with replacement: duplicates)
    speed[(kind >= 0.6) & (kind < 0.8)] = NAN  # (masked rows, some of them with a live number)
    stray = kind >= 0.95
    vehicle[stray] = rng.choice(np.array([-5, issued(b) + 2, 2 ** 31 - 1], dtype=np.int64), int(stray.sum())).astype(np.int32)
    want_ignored = int((stray & ~np.isnan(speed)).sum())
    ignored = torch.full((), -7, dtype=torch.int32, device=tensor_device(a))
    a.set_vehicle_speeds_tensor(dev(a, vehicle), dev(a, speed), ignored)
    assert int(ignored.item()) == want_ignored, where
    in_force = {}
    for i in np.flatnonzero(named & ~np.isnan(speed) & ~stray).tolist():  # (row order: the higher row replaces the lower)
        in_force.pop(int(vehicle[i]), None)
        in_force[int(vehicle[i])] = float(speed[i])
    rows = int((named & ~np.isnan(speed) & ~stray).sum())
    for v, s in in_force.items():
        b.set_vehicle_speed(b._vehicle_id(v), s)
    return len(in_force), want_ignored, rows - len(in_force)


def run_sequence(a, b, seed, rounds, where):
    rng = np.random.default_rng(seed)
    kinds, weights = [k for k, _ in OPS], np.array([w for _, w in OPS])
    roads = sorted({lane.rsplit("_", 1)[0] for lane in b.lane_ids()})
    checkpoints = a._checkpoint_calls() and not a._checkpoint_unsupported()
    archives = cks = None
    tracking = False
    done = dict.fromkeys(kinds + ["commanded", "ignored", "twice", "long runs", "batched then stepped"], 0)
    steps, fresh_call = 0, False
    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 7))):
            op = kinds[int(rng.choice(len(kinds), p=weights / weights.sum()))]
            at = "%s seed %d, round %d, step %d" % (where, seed, round_, steps)
            if op == "steps":
                n = int(rng.integers(1, 15))
                for _ in range(n):
                    a.next_step()
                    b.next_step()
                steps += n
                done["long runs"] += n >= 10
                done["batched then stepped"] += fresh_call
                fresh_call = False
            elif op == "batched":
                c, i, t = batched(a, b, rng, at)
                done["commanded"], done["ignored"], done["twice"] = done["commanded"] + c, done["ignored"] + i, done["twice"] + t
                fresh_call = fresh_call or c > 0
            elif op == "speed":
                speeds = b.get_vehicle_speed()
                if not speeds:
                    continue
                vid = sorted(speeds)[int(rng.integers(0, len(speeds)))]
                v = float(rng.uniform(0.0, 12.0))
                a.set_vehicle_speed(vid, v)
                b.set_vehicle_speed(vid, v)
            elif op == "push":
                info = {"length": float(rng.uniform(3.0, 8.0)), "maxSpeed": float(rng.uniform(8.0, 16.0)), "minGap": 2.5}
                route = pushed_route(roads, 0, rng)
                a.push_vehicle(info, route)
                b.push_vehicle(info, route)
            elif op == "reroute":
                ids = sorted(b.get_vehicles())
                if not ids:
                    continue
                vid = ids[int(rng.integers(0, len(ids)))]
                info = b.get_vehicle_info(vid)
                anchor = neighbour(info["road"], 0, rng) if info.get("road") else None
                if anchor not in roads:
                    continue
                assert a.set_vehicle_route(vid, [anchor]) == b.set_vehicle_route(vid, [anchor]), at
            elif op == "reset":
                a.next_step()  # (one step first: the reference's reset leaves the vehicles pushed since the last step behind)
                b.next_step()
                a.reset()
                b.reset()
                archives = cks = None
                steps, fresh_call = 0, False
            elif op == "snapshot":
                archives = (a.snapshot(), b.snapshot(), steps)
            elif op == "load":
                if archives is None:
                    continue
                a.load(archives[0])
                b.load(archives[1])
                steps, fresh_call = archives[2], False
            elif op == "checkpoint":
                cks = (a.checkpoint() if checkpoints else a.snapshot(), b.snapshot(), steps)
            elif op == "rollback":
                if cks is None:
                    continue
                if checkpoints:
                    a.rollback(cks[0])
                else:
                    a.load(cks[0])
                b.load(cks[1])
                steps, fresh_call = cks[2], False
            elif op == "track":
                tracking = not tracking
                a.track_lane_flow(tracking)
                b.track_lane_flow(tracking)
            done[op] += 1
        assert_same_state(a, b, "%s seed %d, round %d" % (where, seed, round_))
    assert a.get_vehicle_speed() == b.get_vehicle_speed() and a.get_vehicle_distance() == b.get_vehicle_distance(), where
    for op in kinds:
        assert done[op] > 0, "%s never ran: %s" % (op, done)
    assert done["commanded"] > 100 and done["ignored"] > 0 and done["twice"] > 0 and done["long runs"] > 0 and \
        done["batched then stepped"] > 3, done
    return done


def test_sequence_twin_against_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir)
    run_sequence(twin(mod, cfg), twin(mod, cfg), SEED, ROUNDS, "grid_6x6 twin")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_sequence_equals_the_twin(mod, scen, workdir, layout):
    cfg = scen.materialize("grid_6x6", workdir, **({"cfx": {"layout": "dense"}} if layout == "dense" else {}))
    run_sequence(hip_engine(mod, cfg, layout), twin(mod, cfg), SEED, ROUNDS, "grid_6x6 " + layout)
