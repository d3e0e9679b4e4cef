"""set_vehicle_routes_tensor / set_vehicle_routes inside random call sequences, beside the speed commands, the trip log, archives,
checkpoints and rollbacks; and pointed tests for what such a sequence only reaches by chance.

The driver (`run_sequence`) is built like tests/test_vehicle_speeds_sequences.py: one seeded stream of operations drives the
engine under test `a` and the CPU twin `tw`.  A batched route call is judged row by row by test_vehicle_routes.model_status and
mirrored on the twin by command_twin (the per-vehicle set_vehicle_route with the roads of the route behind the vehicle's);
after every round the vehicle states, lane counts, scalars and lights of the two are compared with array_equal / ==.

Two properties of the yardstick, and how the driver handles them:

* Rollback.  The twin has no checkpoint in device memory, and load(snapshot()) on it restarts every cursor.  A rollback on `a` is
  therefore followed by a FRESH twin replayed from step 0: every state-changing call on the twin goes through `Recorded`,
  which appends (step, call, args); `replay` gives the record to a new twin (milliseconds on a 6x6 grid).  Nothing cuts the
  record: a reset() is an entry of it like a step, because reset() keeps the random generator's state and the count of pushed
  vehicles, so a reset twin is not a fresh one.  snapshot / load stay load on both engines, but the twin never loads another
  twin's Archive (an Archive names routes and templates by their index in its engine's tables, and every per-vehicle call
  interns a route): a snapshot saves the record, and a load is a new twin replayed to there that then loads its OWN snapshot —
  the entry ("load") of the record from then on.  On a HIP engine without checkpoints in device memory (the dense layout)
  checkpoint / rollback fall back to snapshot / load in this sense on both; where `a` is itself a twin (the model test) `a`
  is replayed too, so the replay is proven without a GPU.
* After a load.  Between a load() and a vehicle's next lane the twin's cursor names its route's first road and a command is planned
  from there, while `a` lists the registered route from its start ("One visible difference").  Until a vehicle's route
  string on the twin begins with the road it is on, the driver gives it no row with a valid handle, no per-vehicle reroute and no
  get_vehicle_info comparison; rows with bad handles or padding may still name it.  A vehicle that a batched call commanded
  BEFORE the load shows the same difference until it is on another lane than the load found it on (the twin's string begins
  with the road of the command, which is the vehicle's): it is left out of reroute and the get_vehicle_info comparison until
  then, and still named in rows with valid handles (both plan from the lane's road).  Nothing else is narrowed.

`route_pos` is compared for the vehicles that no call has commanded since they were created (tests/test_vehicle_routes.py's
docstring says why a commanded vehicle's cursor differs); of the commanded ones three per round are compared by
get_vehicle_info.  Between a batched route call and the next step `leader` and `gap` are left out (test_vehicle_routes.lockstep).
The driver's own records are keyed by vehicle id, not number: a vehicle compaction gives the running vehicles new numbers."""
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_device_sequences import neighbour, pushed_route  # noqa: E402
from test_device_tensors import twin  # noqa: E402
from test_lane_flow import hip_engine, layout_config  # noqa: E402
from test_vehicle_routes import (AFTER, call, check_call, command_twin, grid_routes, has_next, lane_links_of, lockstep,  # noqa: E402
                                 midroute_rows, model_status, not_on_the_twin, started)
from test_vehicle_speeds import command, issued, same_state  # noqa: E402
from test_vehicle_speeds_sequences import batched as speed_rows  # noqa: E402

OPS = (("steps", 8.0), ("routes", 5.0), ("speeds", 2.0), ("routes+speeds", 2.5), ("reroute", 2.5), ("speed", 1.0), ("push", 1.0),
       ("reset", 0.4), ("snapshot", 1.0), ("load", 0.8), ("checkpoint", 1.2), ("rollback", 1.2), ("info", 1.5), ("track", 0.7),
       ("trips", 1.0), ("drain", 1.5), ("readback", 1.5))
ROUNDS = 40
SEED = {"auto": 25, "dense": 25}  # (chosen on the twins so that the coverage conditions hold: test_sequence_model_on_twins)
COMPACT = {"compactVehicles": 150}
TRIP_COLUMNS = ("env", "vehicle", "origin_road", "destination_road", "enter_step", "finish_step", "travel_steps")


# ----------------------------------------------------------------------------------------------------------------- helpers
class Recorded:
    """A twin whose state-changing calls are appended to `record` as (next_step calls so far, call, args), for `replay`."""
    CALLS = ("next_step", "set_vehicle_route", "set_vehicle_speed", "push_vehicle", "reset")

    def __init__(self, eng, record=()):
        self.eng, self.record = eng, list(record)
        self.step = sum(1 for _, name, _ in self.record if name == "next_step")

    def __getattr__(self, name):
        f = getattr(self.eng, name)
        if name not in self.CALLS:
            return f

        def recorded(*args):
            self.record.append((self.step, name, args))
            self.step += name == "next_step"
            return f(*args)
        return recorded


def replay(fresh, record, load=False):
    """A new twin that was given `record` from step 0 (load: and then loaded what it held, as the entry "load" of a record
    does: an Archive names routes and templates by their index in ITS engine's tables, so it is not given to another engine).
    -> Recorded"""
    eng = fresh()
    record = list(record) + ([(0, "load", ())] if load else [])
    for _, name, args in record:
        if name == "load":
            eng.load(eng.snapshot())
        else:
            getattr(eng, name)(*args)
    return Recorded(eng, record)


def right_turn_loops(eng, links, count=4):
    """[g[0], g[1], three roads around a block to the right of g[1], g[1] again, g[2]] for flow routes g.  -> road lists"""
    out_of = {}
    for (road, _), ends in links.items():
        out_of.setdefault(road, set()).update(e for e, _ in ends)

    def right(road):
        x, y, d = (int(t) for t in road.split("_")[1:])
        nx, ny = x + (1, 0, -1, 0)[d], y + (0, 1, 0, -1)[d]
        r = "road_%d_%d_%d" % (nx, ny, (d + 3) % 4)
        return r if r in out_of.get(road, ()) else None

    lists = []
    for h in range(eng.route_count()):
        g = eng.route_roads(h)
        if len(g) < 3:
            continue
        t1 = right(g[1])
        t2 = right(t1) if t1 else None
        t3 = right(t2) if t2 else None
        if t3 and right(t3) == g[1]:
            lists.append([g[0], g[1], t1, t2, t3, g[1], g[2]])
    return lists[:: max(1, len(lists) // count)][:count]


def register(a, tw, links):
    """grid_routes and the loop routes on both engines.  -> (the added road lists by handle order, loop handles)"""
    n0 = a.route_count()
    assert grid_routes(a, links) == grid_routes(tw, links)
    loops = []
    for g in right_turn_loops(a, links):
        try:
            h = a.add_routes([g])
        except ValueError:
            continue  # (a candidate the reference's rules refuse)
        assert tw.add_routes([g]) == h
        if a.route_roads(h[0]) == g:
            loops.append(h[0])
    assert len(loops) >= 2, "fewer than two loop routes were registered: %s" % loops
    assert a.route_count() == tw.route_count()
    return [a.route_roads(h) for h in range(n0, a.route_count())], loops


def numbers_to_ids(tw):
    return {int(v): tw._vehicle_id(int(v)) for v in tw._vehicle_state()["vid"].tolist()}


def unsettled_ids(tw, ids):
    """The vehicles whose route string on the twin does not begin with the road they are on (module docstring, after a load)."""
    out = set()
    for vid in ids:
        info = tw.get_vehicle_info(vid)
        if "road" in info and info["route"].split()[0] != info["road"]:
            out.add(vid)
    return out


def draw_rows(a, tw, rng, n, loops, unsettled, id_of, registered):
    """`n` rows in the manner of midroute_rows, with padding, duplicates, a bad handle and numbers that name no vehicle.  The
    handles are drawn from the `registered` first routes: a per-vehicle call interns one more, on the twin for every command."""
    routes = [a.route_roads(h) for h in range(registered)]
    live = tw._vehicle_state()["vid"].astype(np.int32)
    vehicle, route = np.full(n, -1, dtype=np.int32), np.full(n, -1, dtype=np.int32)
    if n == 0 or len(live) == 0:
        return vehicle, route
    k = min(n, len(live))
    chosen = live if n >= len(live) else rng.choice(live, k, replace=False)
    vehicle[:k] = chosen
    route[:k] = rng.integers(0, len(routes), k)
    for i, v in enumerate(chosen.tolist()):
        road = tw.get_vehicle_info(id_of[v]).get("road")
        fits = [h for h, g in enumerate(routes) if road in g[:-1]]
        on_loop = [h for h in loops if road in routes[h][:2]]
        if on_loop and rng.random() < 0.6:
            route[i] = on_loop[int(rng.integers(0, len(on_loop)))]
        elif fits and rng.random() < 0.5:
            route[i] = fits[int(rng.integers(0, len(fits)))]
    extra = n - k
    if extra >= 1:  # the tail: a duplicate, a bad handle, two numbers that name no vehicle, padding
        tail = [(int(chosen[0]), int(rng.integers(0, len(routes)))), (int(chosen[-1]), a.route_count()), (-5, 0), (issued(tw) + 2, 0),
                (int(chosen[k // 2]), -1), (int(chosen[k // 2]), int(route[k // 2]))]
        for j, (v, h) in enumerate(tail[:extra]):
            vehicle[k + j], route[k + j] = v, h
    elif n >= 64:  # (no room behind the vehicles: the same rows over the first ones)
        vehicle[1], route[2], vehicle[3], vehicle[4] = vehicle[0], a.route_count(), -5, issued(tw) + 2
    for i, v in enumerate(vehicle.tolist()):  # (module docstring: after a load)
        if v in id_of and id_of[v] in unsettled and 0 <= route[i] < len(routes):
            route[i] = -1 if i % 2 else a.route_count()
    return vehicle, route


def route_call(a, tw, links, vehicle, route, form, where, batched_form):
    """One batched route call on `a` and its mirror on the twin.  -> (status, rows, ids applied)"""
    want, rows = model_status(a, tw, links, vehicle, route)
    if batched_form:
        got, ignored = call(a, vehicle, route, form)
        assert np.array_equal(got, want), "%s: status\n got  %s\n want %s" % (where, got.tolist(), want.tolist())
        assert ignored == int((want < 0).sum()), "%s: ignored %d, negative rows %d" % (where, ignored, int((want < 0).sum()))
    else:
        command_twin(a, want, rows)
    return want, rows, command_twin(tw, want, rows)


def compare(a, tw, where, commanded, dirty):
    skip = ("route_pos",) + (("leader", "gap") if dirty else ())
    same_state(a, tw, where, skip)
    sa, sb = a._vehicle_state(), tw._vehicle_state()
    keep = np.array([tw._vehicle_id(int(v)) not in commanded for v in sb["vid"].tolist()], dtype=bool)
    assert np.array_equal(sa["route_pos"][keep], sb["route_pos"][keep]), where + ": route_pos of the vehicles never commanded"
    assert np.array_equal(a.get_lane_vehicle_count_array(), tw.get_lane_vehicle_count_array()), where + ": lane counts"
    ca, cb = a._scalars(), tw._scalars()
    for k in ("active_vehicle_count", "finished_vehicle_count", "spawned_vehicle_count", "cumulative_travel_time"):
        assert ca[k] == cb[k], "%s: scalar %s differs (%r vs %r)" % (where, k, ca[k], cb[k])
    pa, pb = a._tl_state(), tw._tl_state()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), where + ": traffic-light state differs"


# ------------------------------------------------------------------------------------------------------------------ the driver
def run_sequence(a, tw, seed, rounds, where, batched, cfg=None, fresh=None, loads=False):
    """a: the engine under test (batched: it takes the batched route calls; otherwise a second twin that is commanded with
    command_twin; loads: that twin's rollback is a load, as on a HIP engine without checkpoints in device memory).  tw: a
    twin.  cfg: their config file.  fresh(): another twin of it, nothing registered.  -> the counters"""
    rng = np.random.default_rng(seed)
    kinds, weights = [k for k, _ in OPS], np.array([w for _, w in OPS])
    links = lane_links_of(cfg)
    lists, loops = register(a, tw, links)
    registered = a.route_count()
    roads = sorted({lane.rsplit("_", 1)[0] for lane in tw.lane_ids()})
    road_ids = tw.road_ids()

    def fresh_registered():
        t = fresh()
        n0 = t.route_count()
        assert t.add_routes(lists) == list(range(n0, n0 + len(lists)))
        return t

    tw = Recorded(tw)
    model = not batched  # (`a` is a second twin: it is replayed wherever the twin is)
    checkpoints = bool(a._checkpoint_calls() and not a._checkpoint_unsupported())
    by_load = loads if model else not checkpoints  # a rollback that is snapshot / load on both engines
    archives = cks = None
    held, commanded, by_batch = {}, set(), set()       # {vehicle id: handle}; ids commanded by any call; by a batched call
    loaded_on = {}                                      # {vehicle id: the drivable a load() found it on}: its cursor is restarted
    exempt = set()                                      # vehicle numbers whose origin_road in the trip log is not compared
    tracking = trips = False
    since_ck = set()
    done = dict.fromkeys(kinds + ["applied", "applied at p > 0", "applied on a loop", "routes first", "speeds first",
                                  "reroutes after a batch", "rollback after reset or info", "compactions", "trip rows"], 0)
    statuses, counts, forms, reroutes = set(), 0, 0, 0
    steps, dirty = 0, False
    recent = []
    compactions = tw._vehicle_table()[1]

    def saved():
        return dict(held), set(commanded), set(by_batch), dict(loaded_on)

    def loaded():
        """A load() restarted every cursor; a vehicle's catches up when it enters its next lane.  Of the vehicles a batched call
        has commanded the two engines list other routes meanwhile (module docstring)."""
        loaded_on.clear()
        loaded_on.update({vid: tw.get_vehicle_info(vid)["drivable"] for vid in tw.get_vehicles(False) if vid in by_batch})

    def restarted(vid):
        if vid in loaded_on:
            info = tw.get_vehicle_info(vid)
            if "road" not in info or info["drivable"] == loaded_on[vid]:
                return True
            del loaded_on[vid]  # (on another lane: the cursor has caught up)
        return False

    def note_applied(want, rows, vehicle, route):
        for i in rows:
            if want[i] == 1:
                vid, road, g, p = rows[i]
                held[vid] = int(route[i])
                commanded.add(vid)
                by_batch.add(vid)
                exempt.add(int(vehicle[i]))
                done["applied"] += 1
                done["applied at p > 0"] += p > 0
                done["applied on a loop"] += int(route[i]) in loops and g[1] == road and p == 1
        statuses.update(want.tolist())

    def settled_commanded(pool):
        ids = sorted(set(pool) & set(tw.get_vehicles(False)))
        return [v for v in ids if v not in unsettled_ids(tw, [v]) and not restarted(v)]

    def trackers(engines):
        for e in engines:
            e.track_lane_flow(tracking)
            if trips:
                e.track_trips(True, log=4096)

    def of_a(vid):
        """`a`'s id of the twin's vehicle `vid`: a replayed twin counts its pushed vehicles anew, `a` never counts back."""
        return a._vehicle_id(number_of(vid))

    def number_of(vid):
        return next(v for v, i in numbers_to_ids(tw).items() if i == vid)

    def baseline():
        exempt.clear()
        exempt.update(v for v, vid in numbers_to_ids(tw).items() if vid in commanded)

    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 7))):
            op = kinds[int(rng.choice(len(kinds), p=weights / weights.sum()))]
            recent.append(op)
            at = "%s seed %d, round %d, step %d (after %s)" % (where, seed, round_, steps, ", ".join(recent[-8:]))
            if op == "steps":
                n = int(rng.integers(1, 15))
                for _ in range(n):
                    a.next_step()
                    tw.next_step()
                steps += n
                dirty = False
                now = tw._vehicle_table()[1]
                if now != compactions:  # (new numbers: the old ones stay exempt, rows of the log keep them)
                    done["compactions"] += now - compactions
                    compactions = now
                    exempt.update(v for v, vid in numbers_to_ids(tw).items() if vid in commanded)
                compare(a, tw, at, commanded, dirty)
            elif op == "routes":
                id_of = numbers_to_ids(tw)
                n = (0, 1, 64, 65, len(id_of) + 9)[counts % 5]
                counts += 1
                vehicle, route = draw_rows(a, tw, rng, n, loops, unsettled_ids(tw, id_of.values()), id_of, registered)
                forms += 1
                want, rows, _ = route_call(a, tw, links, vehicle, route, ("tensor", "array")[forms % 2], at, batched)
                note_applied(want, rows, vehicle, route)
                dirty = dirty or bool((want == 1).any())
            elif op == "speeds":
                speed_rows(a, tw, rng, at)
            elif op == "routes+speeds":
                id_of = numbers_to_ids(tw)
                if len(id_of) < 16:
                    continue
                n = max(257, len(id_of) + 9)
                vehicle, route = draw_rows(a, tw, rng, n, loops, unsettled_ids(tw, id_of.values()), id_of, registered)
                few = vehicle[len(id_of) - 8:len(id_of)].copy()  # (named in the HIGH rows of the first call, in rows 0..7 of the second)
                routes_first = (done["routes first"] + done["speeds first"]) % 2 == 0
                if routes_first:
                    want, rows, _ = route_call(a, tw, links, vehicle, route, "tensor", at + " first", batched)
                    note_applied(want, rows, vehicle, route)
                    speed = rng.uniform(0.0, 6.0, len(few))
                    command(a, tw, few, speed, list(zip(few.tolist(), speed.tolist())), 0, "tensor", at + " second")
                    done["routes first"] += 1
                else:
                    speed = rng.uniform(0.0, 12.0, n)
                    waiting = tw._waiting()[0].astype(np.int32)  # (vehicles in entry buffers take a speed too: over the padding)
                    free = np.flatnonzero(vehicle == -1)[:len(waiting)]
                    vehicle[free] = waiting[:len(free)]
                    in_force = {}
                    for v, s in zip(vehicle.tolist(), speed.tolist()):  # (row order: the higher row replaces the lower)
                        if v in id_of or v in waiting:
                            in_force.pop(v, None)
                            in_force[v] = s
                    ignored = int(sum(1 for v in vehicle.tolist() if v != -1 and v not in id_of and v not in waiting))
                    command(a, tw, vehicle, speed, list(in_force.items()), ignored, "tensor", at + " first")
                    small = np.array([route[np.flatnonzero(vehicle == v)[0]] for v in few.tolist()], dtype=np.int32)
                    want, rows, _ = route_call(a, tw, links, few, small, "array", at + " second", batched)
                    note_applied(want, rows, few, small)
                    done["speeds first"] += 1
                dirty = True
            elif op == "reroute":
                reroutes += 1
                pool = [v for v in settled_commanded(by_batch) if "road" in tw.get_vehicle_info(v)] if reroutes % 2 else []
                ids = pool or sorted(tw.get_vehicles(False))
                if not ids:
                    continue
                vid = ids[int(rng.integers(0, len(ids)))]
                info = tw.get_vehicle_info(vid)
                anchor = None
                for _ in range(4 if info.get("road") else 0):  # (a road beyond the border of the grid is drawn again)
                    anchor = neighbour(info["road"], 0, rng)
                    if anchor in roads:
                        break
                if anchor not in roads or vid in unsettled_ids(tw, [vid]) or restarted(vid):
                    continue
                ok = tw.set_vehicle_route(vid, [anchor])
                assert a.set_vehicle_route(of_a(vid), [anchor]) == ok, at
                if ok:
                    dirty = True
                    done["reroutes after a batch"] += vid in by_batch
                    held.pop(vid, None)
                    commanded.add(vid)
                    by_batch.discard(vid)
                    exempt.add(number_of(vid))
                    assert a.get_vehicle_info(of_a(vid)) == tw.get_vehicle_info(vid), at
            elif op == "speed":
                speeds = tw.get_vehicle_speed()
                if not speeds:
                    continue
                vid = sorted(speeds)[int(rng.integers(0, len(speeds)))]
                v = float(rng.uniform(0.0, 12.0))
                a.set_vehicle_speed(of_a(vid), v)
                tw.set_vehicle_speed(vid, v)
            elif op == "push":
                info = {"length": float(rng.uniform(3.0, 8.0)), "maxSpeed": float(rng.uniform(8.0, 16.0)), "minGap": 2.5}
                route = pushed_route(roads, 0, rng)
                a.push_vehicle(info, route)
                tw.push_vehicle(info, route)
            elif op == "reset":
                a.next_step()  # (one step first: the reference's reset leaves the vehicles pushed since the last step behind)
                tw.next_step()
                a.reset()
                tw.reset()
                held, commanded, by_batch = {}, set(), set()
                loaded_on.clear()
                steps, dirty = 0, False
                compactions = tw._vehicle_table()[1]
                baseline()
            elif op == "snapshot":
                archives = (None if model else a.snapshot(), list(tw.record), steps, saved(), dirty)
            elif op == "load":
                if archives is None:
                    continue
                tw = replay(fresh_registered, archives[1], load=True)
                if model:
                    a = replay(fresh_registered, archives[1], load=True).eng
                else:
                    a.load(archives[0])
                trackers((a, tw) if model else (tw,))
                steps, dirty = archives[2], archives[4]  # (a state saved between a route call and a step is such a state again)
                held, commanded, by_batch, _ = (x.copy() for x in archives[3])
                loaded()
                compactions = tw._vehicle_table()[1]
                baseline()
            elif op == "checkpoint":
                if checkpoints:
                    into = cks[0] if cks is not None and done["checkpoint"] % 2 else None
                    ck = a.checkpoint(into=into) if into is not None else a.checkpoint()
                    cks = (ck, list(tw.record), steps, saved(), dirty)
                else:
                    cks = (None if model else a.snapshot(), list(tw.record), steps, saved(), dirty)
                since_ck = set()
            elif op == "rollback":
                if cks is None:
                    continue
                tw = replay(fresh_registered, cks[1], load=by_load)
                if model:
                    a = replay(fresh_registered, cks[1], load=by_load).eng
                elif checkpoints:
                    a.rollback(cks[0])
                else:
                    a.load(cks[0])
                trackers((a, tw) if model else (tw,))
                steps, dirty = cks[2], cks[4]
                held, commanded, by_batch, before = (x.copy() for x in cks[3])
                if not by_load:
                    loaded_on.clear()
                    loaded_on.update(before)
                else:
                    loaded()
                compactions = tw._vehicle_table()[1]
                baseline()
                done["rollback after reset or info"] += bool(since_ck & {"reset", "info"})
            elif op == "info":
                pool = settled_commanded(commanded)
                if not pool:
                    continue
                vid = pool[int(rng.integers(0, len(pool)))]
                assert a.get_vehicle_info(of_a(vid)) == tw.get_vehicle_info(vid), "%s: %s" % (at, vid)
            elif op == "track":
                tracking = not tracking
                a.track_lane_flow(tracking)
                tw.track_lane_flow(tracking)
            elif op == "trips":
                trips = not trips
                for e in (a, tw):
                    if trips:
                        e.track_trips(True, log=4096)
                    else:
                        e.track_trips(False)
                baseline()
            elif op == "drain":
                if not trips:
                    continue
                got, want = a.observe_trip_log_array(reset=True), tw.observe_trip_log_array(reset=True)
                assert got["dropped"] == want["dropped"] == 0, at
                free = ~np.isin(want["vehicle"], np.fromiter(exempt, dtype=np.int64, count=len(exempt)))
                for k in TRIP_COLUMNS:
                    x, y = (got[k], want[k]) if k != "origin_road" else (got[k][free], want[k][free])
                    assert np.array_equal(x, y), "%s: column %s of the trip log" % (at, k)
                done["trip rows"] += len(want["vehicle"])
                baseline()
            elif op == "readback":
                id_of = numbers_to_ids(tw)
                known = [(v, held[vid]) for v, vid in sorted(id_of.items()) if vid in held]
                if batched and known:
                    numbers = np.array([v for v, _ in known] + [-1, issued(tw) + 2], dtype=np.int32)
                    got = a.get_vehicle_routes(numbers)
                    assert got.tolist() == [h for _, h in known] + [-1, -1], at
                    every = a.get_vehicle_routes(np.array(sorted(id_of), dtype=np.int32))
                    assert (every >= 0).all() and (every < a.route_count()).all(), at
            done[op] += 1
            since_ck.add(op)
        at = "%s seed %d, round %d (after %s)" % (where, seed, round_, ", ".join(recent[-8:]))
        compare(a, tw, at, commanded, dirty)
        pool = settled_commanded(commanded)
        for vid in [pool[int(i)] for i in rng.choice(len(pool), min(3, len(pool)), replace=False)] if pool else ():
            assert a.get_vehicle_info(of_a(vid))["route"] == tw.get_vehicle_info(vid)["route"], "%s: the route of %s" % (at, vid)
    for getter in ("get_vehicle_speed", "get_vehicle_distance"):  # (by number: see of_a)
        got, want = ({e._vehicle_id(int(v)): int(v) for v in e._vehicle_state()["vid"]} for e in (a, tw))
        x, y = getattr(a, getter)(), getattr(tw, getter)()
        assert {got[k]: v for k, v in x.items() if k in got} == {want[k]: v for k, v in y.items() if k in want}, "%s: %s" % (where, getter)
    for op in kinds:
        assert done[op] > 0, "%s never ran: %s" % (op, done)
    assert statuses >= set(range(-6, 2)), "statuses that never occurred: %s" % sorted(set(range(-6, 2)) - statuses)
    assert done["applied"] >= 100 and done["applied at p > 0"] >= 10 and done["applied on a loop"] >= 1, done
    assert done["routes first"] >= 3 and done["speeds first"] >= 3 and done["reroutes after a batch"] >= 3, done
    assert done["rollback after reset or info"] >= 1 and done["compactions"] >= 1 and done["trip rows"] >= 1, done
    return done


def sequence_config(scen, workdir, layout):
    return layout_config(scen, workdir, "grid_6x6", layout, **COMPACT)


@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_sequence_model_on_twins(mod, scen, workdir, layout):
    """The driver itself, the replay, model_status's verdicts and every coverage condition, with a second twin as `a`: the
    stream of operations of test_sequence_equals_the_twin[layout] (on the dense layout a rollback is a load, and the vehicles
    left out after a load make it another stream from there on)."""
    cfg = sequence_config(scen, workdir, "auto")
    done = run_sequence(twin(mod, cfg), twin(mod, cfg), SEED[layout], ROUNDS, "grid_6x6 twins", False, cfg=cfg, fresh=lambda: twin(mod, cfg),
                        loads=layout == "dense")
    print("route sequence on twins, as %s: %s" % (layout, json.dumps({k: int(v) for k, v in done.items()})))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_sequence_equals_the_twin(mod, scen, workdir, layout):
    not_on_the_twin()
    cfg = sequence_config(scen, workdir, layout)
    done = run_sequence(hip_engine(mod, cfg, layout), twin(mod, cfg), SEED[layout], ROUNDS, "grid_6x6 " + layout, True, cfg=cfg,
                        fresh=lambda: twin(mod, cfg))
    print("route sequence %s: %s" % (layout, json.dumps({k: int(v) for k, v in done.items()})))


# ------------------------------------------------------------------------------------------------------------ pointed tests
def grid_started(mod, scen, workdir, layout, steps=90, **cfx):
    """-> cfg, links, the HIP engine and the twin with grid_routes registered, after `steps` steps"""
    cfg = layout_config(scen, workdir, "grid_6x6", layout, **cfx)
    links = lane_links_of(cfg)
    a, tw, _ = started(mod, lambda c: hip_engine(mod, c, layout), cfg, steps, register=lambda e: grid_routes(e, links))
    return cfg, links, a, tw


def padded(vehicle, route, n=257):
    k = max(0, n - len(vehicle))
    return np.concatenate([vehicle, np.full(k, -1, dtype=np.int32)]), np.concatenate([route, np.full(k, -1, dtype=np.int32)])


def refusing_rows(a, tw, links):
    """Every running vehicle with a handle that is refused for it: -4 on a laneLink, -6 where a route holds its road but its lane
    does not lead on, -5 otherwise."""
    routes = [a.route_roads(h) for h in range(a.route_count())]
    vehicle = tw._vehicle_state()["vid"].astype(np.int32)
    route = np.zeros(len(vehicle), dtype=np.int32)
    for i, v in enumerate(vehicle.tolist()):
        info = tw.get_vehicle_info(tw._vehicle_id(v))
        road = info.get("road")
        if road is None:
            continue
        index = int(info["drivable"].rsplit("_", 1)[1])
        wrong_lane = [h for h, g in enumerate(routes) if road in g[:-1] and road != g[-1] and not has_next(links, road, index, g, g.index(road))]
        route[i] = wrong_lane[0] if wrong_lane else next(h for h, g in enumerate(routes) if road not in g[:-1])
    return vehicle, route


def applied_rows(a, tw, links, rng, count):
    """`count` running vehicles from the END of _vehicle_state()'s order, each with a handle the model applies."""
    vehicle, route = midroute_rows(a, tw, rng)
    want, _ = model_status(a, tw, links, vehicle, route)
    at = np.flatnonzero(want == 1)[-count:]
    assert len(at) == count and at[0] > len(vehicle) // 2, "too few rows that apply in the upper half: %s" % at
    return vehicle[at], route[at]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
@pytest.mark.parametrize("first", ["routes", "speeds", "refused routes"])
def test_stamp_is_idle_between_calls(mod, scen, workdir, layout, first):
    """A large call, then a small one for vehicles the large one named in HIGH rows, before one step: a stamp the first call
    left standing (its row index) would beat the second call's rows 0..4 without a sign."""
    cfg, links, a, tw = grid_started(mod, scen, workdir, layout)
    rng = np.random.default_rng(21)
    where = "%s first, %s" % (first, layout)
    ids = []
    if first == "speeds":
        vehicle = tw._vehicle_state()["vid"].astype(np.int32)
        assert len(vehicle) >= 257
        speed = rng.uniform(6.0, 12.0, len(vehicle))
        command(a, tw, vehicle, speed, list(zip(vehicle.tolist(), speed.tolist())), 0, "tensor", where)
        few, handles = applied_rows(a, tw, links, rng, 5)
        want, _, ids = check_call(a, tw, links, few, handles, where)
        assert want.tolist() == [1] * 5
    else:
        if first == "routes":
            vehicle, route = padded(*midroute_rows(a, tw, rng))
            _, _, ids = check_call(a, tw, links, vehicle, route, where, need=(1, -4, -5, -6))
        else:
            vehicle, route = refusing_rows(a, tw, links)
            assert len(vehicle) >= 257
            want, _, _ = check_call(a, tw, links, vehicle, route, where, need=(-4, -5, -6))
            assert set(want.tolist()) <= {-4, -5, -6}
            few, handles = applied_rows(a, tw, links, rng, 5)  # (a refused winner's stamp is cleared too: these rows apply)
            want, _, ids = check_call(a, tw, links, few, handles, where + ", the route rows behind the refused ones")
            assert want.tolist() == [1] * 5
        live = tw._vehicle_state()
        fast = [int(v) for v, s in zip(live["vid"].tolist(), live["speed"].tolist()) if s > 9.0][-5:]
        before = dict(zip(live["vid"].tolist(), live["speed"].tolist()))
        assert len(fast) == 5 and min(np.flatnonzero(np.isin(vehicle, fast))) > 128
        command(a, tw, fast, [3.0] * 5, [(v, 3.0) for v in fast], 0, "tensor", where)
    a.next_step()
    tw.next_step()
    same_state(a, tw, where + " after one step", AFTER)
    if first != "speeds":  # (a command below the speed is followed as fast as the vehicle brakes: every one of the five is slower)
        speeds = a.get_vehicle_speed()
        assert all(speeds[tw._vehicle_id(v)] < before[v] - 1.0 for v in fast), [(before[v], speeds[tw._vehicle_id(v)]) for v in fast]
    lockstep(a, tw, 10, where, ids)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_second_command_and_per_vehicle_call_after_one(mod, scen, workdir, layout):
    """Vehicles commanded at p > 0 hold a cursor into a registered route; some then enter their next lane, some do not.  A second
    batched call for some of them and the per-vehicle set_vehicle_route for others (the host's record of their route is stale
    until refreshRoutes) must both plan from the road the vehicle is on."""
    cfg, links, a, tw = grid_started(mod, scen, workdir, layout)
    rng = np.random.default_rng(22)
    vehicle, route = midroute_rows(a, tw, rng)
    want, rows, ids = check_call(a, tw, links, vehicle, route, "first command", need=(1,))
    first = {rows[i][0]: (int(vehicle[i]), rows[i][1]) for i in rows if want[i] == 1 and rows[i][3] > 0}  # id: (number, road then)
    assert len(first) >= 8
    for s in range(40):
        a.next_step()
        tw.next_step()
        alive = set(tw.get_vehicles(False))
        entered = sorted(v for v in first if v in alive and tw.get_vehicle_info(v).get("road", first[v][1]) != first[v][1])
        stayed = sorted(v for v in first if v in alive and tw.get_vehicle_info(v).get("road") == first[v][1])
        if len(entered) >= 4 and len(stayed) >= 4:
            break
    assert len(entered) >= 4 and len(stayed) >= 4, (len(entered), len(stayed))
    same_state(a, tw, "before the second command", AFTER)
    # (a) a second batched call: another handle that holds the vehicle's road
    routes = [a.route_roads(h) for h in range(a.route_count())]
    again = entered[::2] + stayed[::2]
    numbers = np.array([first[v][0] for v in again], dtype=np.int32)
    held = a.get_vehicle_routes(numbers)
    handles = held.copy()
    for i, v in enumerate(again):
        road = tw.get_vehicle_info(v).get("road")
        fits = [h for h, g in enumerate(routes) if road in g[:-1] and h != held[i]]
        if fits:
            handles[i] = fits[int(rng.integers(0, len(fits)))]
    want2, rows2, ids2 = check_call(a, tw, links, numbers, handles, "second command", need=(1,))
    for group in (entered[::2], stayed[::2]):
        assert any(want2[i] == 1 and handles[i] != held[i] for i, v in enumerate(again) if v in group), "no second command applied"
    assert np.array_equal(a.get_vehicle_routes(numbers), np.where(want2 == 1, handles, held))
    # (b) the per-vehicle call, in lockstep with the twin
    taken = {True: 0, False: 0}
    for v in entered[1::2] + stayed[1::2]:
        info = tw.get_vehicle_info(v)
        if "road" not in info:
            continue
        index = int(info["drivable"].rsplit("_", 1)[1])
        ends = sorted({end for end, _ in links.get((info["road"], index), [])})
        anchor = ends[int(rng.integers(0, len(ends)))] if ends and rng.random() < 0.8 else neighbour(info["road"], 0, rng)
        ok = tw.set_vehicle_route(v, [anchor])
        assert a.set_vehicle_route(v, [anchor]) == ok, "%s towards %s" % (v, anchor)
        assert a.get_vehicle_info(v) == tw.get_vehicle_info(v), v
        taken[ok] += 1
    assert taken[True] >= 2, taken
    lockstep(a, tw, 30, "after the second commands", sorted(first))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["info", "reset", "into", "refreshed before"])
def test_stale_flag_through_checkpoints(mod, scen, workdir, order):
    """routesStale_ is stored by checkpoint() without a read-back, restored by rollback(), overwritten by checkpoint(into=).  A
    wrong host record shows at the next snapshot(): every order ends with load(snapshot()) and 20 steps against the twin, which
    stays where the checkpoint was taken and is never loaded."""
    cfg, links, a, tw = grid_started(mod, scen, workdir, "auto")
    rng = np.random.default_rng(23)
    ck = a.checkpoint() if order == "into" else None
    held = {}

    def commanded(where):
        vehicle, route = midroute_rows(a, tw, rng)
        want, rows, ids = check_call(a, tw, links, vehicle, route, where, need=(1,))
        held.update({int(vehicle[i]): int(route[i]) for i in rows if want[i] == 1})
        return ids

    ids = commanded(order)
    if order == "refreshed before":  # the checkpoint stores a clean flag and a fresh record; the command after it is rolled back
        a.get_vehicle_info(ids[0])
    ck = a.checkpoint(into=ck) if order == "into" else a.checkpoint()
    if order == "refreshed before":
        vehicle, route = midroute_rows(a, tw, rng)
        status, _ = call(a, vehicle, route)
        assert (status == 1).sum() > 0
    else:
        for vid in ids[:3]:
            a.get_vehicle_info(vid)  # (refreshRoutes: the flag is clean now, the checkpoint holds it raised)
    for _ in range(3):
        a.next_step()
    if order == "reset":
        a.reset()
    a.rollback(ck)
    numbers = np.array(sorted(held), dtype=np.int32)
    assert a.get_vehicle_routes(numbers).tolist() == [held[int(v)] for v in numbers], order
    a.load(a.snapshot())
    assert a.get_vehicle_routes(numbers).tolist() == [held[int(v)] for v in numbers], order + ", after the load"
    lockstep(a, tw, 20, order)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_archive_file_after_a_command(mod, scen, workdir, layout, tmp_path):
    """Archive.dump writes a commanded vehicle's REGISTERED route from its start, the twin the roads from the call on; everything
    else in the two files is equal, and both engines go on from the HIP engine's file alike."""
    cfg, links, a, tw = grid_started(mod, scen, workdir, layout)
    vehicle, route = midroute_rows(a, tw, np.random.default_rng(24))
    want, rows, ids = check_call(a, tw, links, vehicle, route, "archive", need=(1,))
    lists = {rows[i][0]: (rows[i][2], rows[i][3]) for i in rows if want[i] == 1}
    for _ in range(3):
        a.next_step()
        tw.next_step()
    ours, theirs = str(tmp_path / "hip.json"), str(tmp_path / "twin.json")
    a.snapshot().dump(ours)
    tw.snapshot().dump(theirs)
    with open(ours) as f, open(theirs) as g:
        fa, ft = json.load(f), json.load(g)
    assert sorted(fa) == sorted(ft)
    for k in fa:
        assert k == "vehicles" or fa[k] == ft[k], "%s differs between the files" % k
    assert len(fa["vehicles"]) == len(ft["vehicles"])
    seen = {"commanded at p > 0": 0, "commanded at 0": 0, "never commanded": 0}
    for va, vt in zip(fa["vehicles"], ft["vehicles"]):
        assert {k: v for k, v in va.items() if k != "route"} == {k: v for k, v in vt.items() if k != "route"}, va["id"]
        if va["id"] in lists:
            g, p = lists[va["id"]]
            assert va["route"] == g, "%s: not the registered route from its start" % va["id"]
            assert vt["route"] == g[p:] and va["route"][va["route"].index(vt["route"][0]):] == vt["route"], va["id"]
            seen["commanded at p > 0" if p > 0 else "commanded at 0"] += 1
        else:
            assert va["route"] == vt["route"], va["id"]
            seen["never commanded"] += 1
    assert seen["commanded at p > 0"] >= 4 and seen["never commanded"] > 0, seen
    a2, tw2 = hip_engine(mod, cfg, layout), twin(mod, cfg)
    a2.load_from_file(ours)
    tw2.load_from_file(ours)
    for s in range(30):
        same_state(a2, tw2, "from the HIP engine's file, step +%d" % s, AFTER)
        a2.next_step()
        tw2.next_step()
    same_state(a2, tw2, "from the HIP engine's file", AFTER)
    assert a2.get_vehicle_speed() == tw2.get_vehicle_speed() and a2.get_vehicle_distance() == tw2.get_vehicle_distance()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_trip_log_after_a_mid_route_command(mod, scen, workdir, layout):
    """At p > 0 the registered route's first road is not the vehicle's: the device log names the route's first road as the
    origin, the twin's host log the road of the call.  Every other column, and every other vehicle's origin, is equal."""
    cfg, links, a, tw = grid_started(mod, scen, workdir, layout)
    a.track_trips(True, log=4096)
    tw.track_trips(True, log=4096)
    vehicle, route = midroute_rows(a, tw, np.random.default_rng(25))
    want, rows, ids = check_call(a, tw, links, vehicle, route, "trip log", need=(1,))
    deep = {int(vehicle[i]): rows[i] for i in rows if want[i] == 1 and rows[i][3] > 0}  # (the route's first road is not the vehicle's)
    moved = {v: row for v, row in deep.items() if len(row[2]) == 3}  # (with two roads to go: they finish soon)
    assert len(moved) >= 4, "fewer than four vehicles commanded at p > 0"
    waiting_for = {vid for vid, _, _, _ in moved.values()}
    for s in range(400):
        a.next_step()
        tw.next_step()
        if s % 10 == 9 and not waiting_for & set(tw.get_vehicles(True)):
            break
    assert not waiting_for & set(tw.get_vehicles(True)), "commanded vehicles are still on their way after 400 steps"
    same_state(a, tw, "trip log", AFTER)
    log, theirs = a.observe_trip_log_array(), tw.observe_trip_log_array()
    assert log["dropped"] == theirs["dropped"] == 0
    others = ~np.isin(theirs["vehicle"], np.array(sorted(deep), dtype=np.int32))
    for k in TRIP_COLUMNS:
        x, y = (log[k], theirs[k]) if k != "origin_road" else (log[k][others], theirs[k][others])
        assert np.array_equal(x, y), "%s differs from the twin's host log" % k
    roads = a.road_ids()
    row_of = {v: i for i, v in enumerate(log["vehicle"].tolist())}
    assert set(moved) <= set(row_of)
    for v, (vid, road, g, p) in deep.items():
        if v not in row_of:
            continue
        i = row_of[v]
        assert roads[log["origin_road"][i]] == g[0] and roads[theirs["origin_road"][i]] == road == g[p], vid
        assert roads[log["destination_road"][i]] == g[-1], vid


def ending_on_its_road(a, tw, links, where, batched_form):
    """Routes that come back to their second road and END there, for vehicles on that road in a lane without a laneLink towards
    the route's third road: Router::onValidLane holds (the road is route.back()), the trip ends on this lane."""
    lists = [g[:-1] for g in right_turn_loops(a, links, count=8)]
    handles = a.add_routes(lists)
    assert tw.add_routes(lists) == handles and all(a.route_roads(h) == g for h, g in zip(handles, lists))
    for _ in range(90):
        if a is not tw:
            a.next_step()
        tw.next_step()
    vehicle, route, special = [], [], []
    for v in tw._vehicle_state()["vid"].tolist():
        info = tw.get_vehicle_info(tw._vehicle_id(v))
        for h, g in zip(handles, lists):
            if info.get("road") == g[1]:
                vehicle.append(v)
                route.append(h)
                if not has_next(links, g[1], int(info["drivable"].rsplit("_", 1)[1]), g, 1):
                    special.append(len(vehicle) - 1)
    vehicle, route = np.array(vehicle, dtype=np.int32), np.array(route, dtype=np.int32)
    want, rows, ids = route_call(a, tw, links, vehicle, route, "tensor", where, batched_form)
    assert len(special) >= 4 and (want[special] == 1).all(), (special, want.tolist())
    return [rows[i][0] for i in special]


def test_set_vehicle_route_accepts_a_route_that_ends_on_the_vehicles_road(mod, scen, workdir):
    """The verdict is EngineHost::setRoute's on the twin (`lastRoad = seq.back() == laneRoad`), the project's restatement of
    Router::setRoute, whose onValidLane (router.h:66-68) is "a next drivable, or onLastRoad()" with isLastRoad comparing against
    route.back(); model_status and the device's routeVerdict must agree with it, and the vehicles end their trips on that lane."""
    cfg = scen.materialize("grid_6x6", workdir)
    tw = twin(mod, cfg)
    ids = ending_on_its_road(tw, tw, lane_links_of(cfg), "twin", False)
    before = tw._scalars()["finished_vehicle_count"]
    for _ in range(60):
        tw.next_step()
    assert not set(ids) & set(tw.get_vehicles(True)) and tw._scalars()["finished_vehicle_count"] >= before + len(ids)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_route_that_ends_on_the_vehicles_road(mod, scen, workdir, layout):
    not_on_the_twin()
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    a, tw = hip_engine(mod, cfg, layout), twin(mod, cfg)
    ids = ending_on_its_road(a, tw, lane_links_of(cfg), layout, True)
    lockstep(a, tw, 60, "a route that ends on the vehicle's road, " + layout, ids)
    assert not set(ids) & set(tw.get_vehicles(True)), "the vehicles have not ended their trips"


# ----------------------------------------------------------------------------------- VectorEngine: a gathered rollback
def slot_rows(vec, r, e):
    """Environment r's rows of observe_vehicles_array and its twin's: row j of the one is row j of the other.
    -> the batched engine's numbers, the twin's numbers"""
    got, D = vec.observe_vehicles_array(), sum(vec._drivable_counts())
    lo, hi = int(got["start"][r, 0]), int(got["start"][r, D])
    rows = e.observe_vehicles_array()
    assert hi - lo == int(rows["count"]), r
    return got["vehicle"][lo:hi].astype(np.int32), rows["vehicle"].astype(np.int32)


def command_slots(vec, twins, links, rng, where):
    """One batched call that commands every slot's running vehicles (midroute_rows on the slot's twin), the rows of the slots
    shuffled together.  -> per slot {the twin's number: handle applied}, per slot the rows applied at p > 0"""
    numbers, handles, want, slot = [], [], [], []
    applied, deep = [], []
    for r, e in enumerate(twins):
        ours, theirs = slot_rows(vec, r, e)
        number_of = dict(zip(theirs.tolist(), ours.tolist()))
        lv, lh = midroute_rows(vec, e, rng)  # (the handles are the batched engine's: the twin interns a route per command)
        s, rows = model_status(vec, e, links, lv, lh)
        command_twin(e, s, rows)
        numbers.append(np.array([number_of[v] for v in lv.tolist()], dtype=np.int32))
        handles.append(lh)
        want.append(s)
        slot.append(np.full(len(lv), r))
        applied.append({int(lv[i]): int(lh[i]) for i in rows if s[i] == 1})
        deep.append(sum(1 for i in rows if s[i] == 1 and rows[i][3] > 0))
    order = rng.permutation(sum(len(x) for x in numbers))
    numbers, handles, want = (np.concatenate(x).astype(np.int32)[order] for x in (numbers, handles, want))
    status, ignored = call(vec, numbers, handles)
    assert np.array_equal(status, want), "%s: status" % where
    assert ignored == int((want < 0).sum()), where
    assert np.array_equal(vec.get_vehicle_routes(numbers)[want == 1], handles[want == 1]), where
    return applied, deep


def assert_slots(vec, twins, where):
    got, D = vec.observe_vehicles_array(), sum(vec._drivable_counts())
    lanes = vec.get_lane_vehicle_count_array().reshape(len(twins), -1)
    for r, e in enumerate(twins):
        assert vec.get_vehicle_speed(r) == e.get_vehicle_speed(), "%s: slot %d get_vehicle_speed" % (where, r)
        lo, hi = int(got["start"][r, 0]), int(got["start"][r, D])
        rows = e.observe_vehicles_array()
        for k in ("distance", "speed"):
            assert np.array_equal(got[k][lo:hi], rows[k]), "%s: slot %d %s" % (where, r, k)
        assert np.array_equal(np.diff(got["start"][r]), np.diff(rows["start"].reshape(-1))), "%s: slot %d rows per drivable" % (where, r)
        assert np.array_equal(lanes[r], e.get_lane_vehicle_count_array()), "%s: slot %d lane counts" % (where, r)


@pytest.mark.gpu
def test_gathered_rollback_with_commanded_routes(mod, scen, workdir):
    """k_env_gather_table shifts vt.route by delta * routesPerEnv, k_env_gather_running copies routePos: after the gather a slot
    holds registered handles with cursors p > 0 that another environment was given.  The yardstick is standalone twins that
    never load (tests/test_rollback_envs.py): the twin of slot r is seeded as envs[r] and given that environment's commands."""
    not_on_the_twin()
    R, envs = 3, [2, 0, 0]
    cfg = layout_config(scen, workdir, "grid_6x6", "auto")
    links = lane_links_of(cfg)
    probe = twin(mod, cfg)
    n0 = probe.route_count()
    grid_routes(probe, links)
    lists = [probe.route_roads(h) for h in range(n0, probe.route_count())]
    vec = mod.VectorEngine(cfg, R, 1, routes=lists)
    assert vec.backend_name() == "hip-gfx950" and vec._checkpoint_calls()
    handles = vec.added_routes()

    def fresh(seed):
        e = twin(mod, scen.materialize("grid_6x6", workdir, seed=seed))
        assert e.add_routes(lists) == handles
        return e

    def steps(n, twins, where, every=1):
        for s in range(1, n + 1):
            vec.next_step()
            for e in twins:
                e.next_step()
            if s % every == 0:
                assert_slots(vec, twins, "%s, step +%d" % (where, s))

    rng = np.random.default_rng(26)
    singles = [Recorded(fresh(r)) for r in range(R)]
    steps(90, singles, "before any command", every=30)
    applied, deep = command_slots(vec, singles, links, rng, "the first command")
    assert min(deep) >= 1, "an environment without a row applied at p > 0: %s" % deep
    assert any(sum(h in set(x.values()) for x in applied) >= 2 for h in handles), "no handle applied in two environments"
    steps(5, singles, "after the first command")
    held = []
    for r, e in enumerate(singles):
        ours, _ = slot_rows(vec, r, e)
        held.append(vec.get_vehicle_routes(ours))
    ck = vec.checkpoint()
    records = [list(e.record) for e in singles]
    for _ in range(3):
        vec.next_step()
    vec.rollback(ck, envs=envs)
    twins = [singles[2], singles[0], replay(lambda: fresh(0), records[0])]  # (the twins stayed where the checkpoint was taken)
    assert_slots(vec, twins, "right after the rollback")
    for r, e in enumerate(twins):
        ours, _ = slot_rows(vec, r, e)  # (the new numbers)
        assert np.array_equal(vec.get_vehicle_routes(ours), held[envs[r]]), "slot %d does not hold environment %d's routes" % (r, envs[r])
    steps(30, twins, "after the rollback")
    # slots 1 and 2 hold one state: a second command gives them different handles
    applied, deep = command_slots(vec, twins, links, rng, "the second command")
    assert applied[1] != applied[2] and min(deep) >= 1, deep
    steps(20, twins, "after the second command")
    lanes = vec.get_lane_vehicle_count_array().reshape(R, -1)
    assert not np.array_equal(lanes[1], lanes[2]), "slots 1 and 2 never diverged under their own routes"


def test_load_refuses_an_archive_that_names_routes_the_engine_does_not_hold(mod, scen, workdir):
    """An Archive names routes by their index in its engine's tables: one taken after a set_vehicle_route interned a route is
    refused by another engine (it used to read beyond the tables), and still loads where it was taken."""
    cfg = scen.materialize("grid_6x6", workdir)
    a, b = twin(mod, cfg), twin(mod, cfg)
    for _ in range(30):
        a.next_step()
    plain = a.snapshot()
    rng = np.random.default_rng(27)
    roads = sorted({lane.rsplit("_", 1)[0] for lane in a.lane_ids()})
    n0 = a.route_count()
    for vid in sorted(a.get_vehicles(False)):
        anchor = neighbour(a.get_vehicle_info(vid)["road"], 0, rng)
        if anchor in roads and a.set_vehicle_route(vid, [anchor]) and a.route_count() > n0:
            break
    assert a.route_count() > n0 == b.route_count()
    b.load(plain)  # (flow routes only: the indices are the same on every engine of the config)
    before = b.get_vehicle_distance()
    a.next_step()
    with pytest.raises(RuntimeError, match="load_from_file"):
        b.load(a.snapshot())
    assert b.get_vehicle_distance() == before and b._scalars()["step"] == 30  # (nothing was changed)
    a.load(a.snapshot())
    a.next_step()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_a_waiting_vehicle_keeps_its_batched_speed_through_a_compaction(mod, scen, workdir, layout):
    """A batched speed command for vehicles still in an entry buffer, then a vehicle compaction before their first step: the
    host never learnt which rows were waiting, so the compaction reads the commands back from the device and hands them over
    (cfx_get_waiting_custom_speeds).  The twin takes the per-vehicle calls, whose commands the host notes itself."""
    not_on_the_twin()
    cfg = layout_config(scen, workdir, "grid_6x6", layout)
    a, tw = hip_engine(mod, cfg, layout), twin(mod, cfg)
    for _ in range(400):
        a.next_step()
        tw.next_step()
        waiting = tw._waiting()[0].astype(np.int32)
        if len(waiting) >= 3:
            break
    assert len(waiting) >= 3, "no vehicles in entry buffers within 400 steps"
    speed = np.linspace(0.5, 2.5, len(waiting))
    ids = [tw._vehicle_id(int(v)) for v in waiting]
    command(a, tw, waiting, speed, list(zip(waiting.tolist(), speed.tolist())), 0, "tensor", "waiting vehicles")
    compactions = a._vehicle_table()[1]
    a._compact_vehicles()
    tw._compact_vehicles()
    assert a._vehicle_table()[1] == compactions + 1
    admitted = set()
    for s in range(1, 41):
        a.next_step()
        tw.next_step()
        same_state(a, tw, "step +%d after the compaction" % s)
        admitted |= set(ids) & set(tw.get_vehicles(False))
    assert admitted, "none of the commanded vehicles left its entry buffer"
    assert a.get_vehicle_speed() == tw.get_vehicle_speed() and a.get_vehicle_distance() == tw.get_vehicle_distance()
