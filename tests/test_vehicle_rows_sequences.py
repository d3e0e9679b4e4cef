"""observe_vehicles_tensor inside random call sequences: the call changes no result.

tests/test_device_sequences.py's driver draws from a fixed table of operations and counts the launches of a step against what it
drew, so a call of another kind cannot be added from outside; this is a short driver of this file's own, in its manner.  One
stream of random operations — runs of steps (long enough for a step to defer its commit), signal phases, reset, snapshot / load,
checkpoint / rollback — drives two engines; only the first also makes observe_vehicles_tensor calls, at random points between the
operations and with random subsets of the outputs, each compared with the _vehicle_state() oracle of tests/test_vehicle_rows.py.
After every round assert_same_state holds against the engine that never made the call."""
import numpy as np
import pytest

from conftest import assert_same_state

torch = pytest.importorskip("torch")

from test_device_tensors import twin  # noqa: E402
from test_lane_flow import hip_engine  # noqa: E402
from test_vehicle_rows import ROWS, at_length, same, state_rows, tensors  # noqa: E402

OPS = (("steps", 8.0), ("phases", 2.0), ("reset", 0.5), ("snapshot", 1.0), ("load", 1.2), ("checkpoint", 1.0), ("rollback", 1.2))
ROUNDS = 40
SEED = 77


def observe(eng, rng, where):
    want = state_rows(eng)
    count = int(want["count"])
    n_rows = int(rng.choice([0, max(count - 1, 0), count, count + 7]))
    names = tuple(k for k in ROWS + ("start", "count") if rng.random() < 0.6) or ("count",)
    t = tensors(eng, n_rows, names)
    eng.observe_vehicles_tensor(**t)
    rows = dict(at_length(want, n_rows), start=want["start"], count=want["count"])
    for k in names:
        same(t[k], rows[k], "%s: %s of %s, N = %d" % (where, k, names, n_rows))
    return count


def run_sequence(observed, plain, seed, rounds, where):
    rng = np.random.default_rng(seed)
    obs_rng = np.random.default_rng(seed + 1)  # (the operations do not depend on how often the rows were read)
    phase_counts = plain._phase_counts()
    kinds, weights = [k for k, _ in OPS], np.array([w for _, w in OPS])
    checkpoints = observed._checkpoint_calls() and not observed._checkpoint_unsupported() and \
        plain._checkpoint_calls() and not plain._checkpoint_unsupported()
    archives = cks = None
    done = dict.fromkeys(kinds + ["observe", "observed vehicles", "long runs"], 0)
    steps = 0
    for round_ in range(rounds):
        for _ in range(int(rng.integers(1, 7))):
            op = kinds[int(rng.choice(len(kinds), p=weights / weights.sum()))]
            at = "%s seed %d, round %d, step %d" % (where, seed, round_, steps)
            if op == "steps":
                n = int(rng.integers(1, 15))
                for i in range(n):
                    observed.next_step()
                    plain.next_step()
                    steps += 1
                    if obs_rng.random() < 0.15:  # (inside a run too: a step behind it may have deferred its commit)
                        done["observed vehicles"] += observe(observed, obs_rng, at + " inside a run")
                        done["observe"] += 1
                done["long runs"] += n >= 10
            elif op == "phases":
                ph = np.array([int(rng.integers(0, c)) if c > 0 else 0 for c in phase_counts], dtype=np.int32)
                observed.set_tl_phases(ph)
                plain.set_tl_phases(ph)
            elif op == "reset":
                observed.reset()
                plain.reset()
                steps = 0
            elif op == "snapshot":
                archives = (observed.snapshot(), plain.snapshot(), steps)
            elif op == "load":
                if archives is None:
                    continue
                observed.load(archives[0])
                plain.load(archives[1])
                steps = archives[2]
            elif op == "checkpoint":
                if not checkpoints:
                    continue
                cks = (observed.checkpoint(), plain.checkpoint(), steps)
            elif op == "rollback":
                if cks is None:
                    continue
                observed.rollback(cks[0])
                plain.rollback(cks[1])
                steps = cks[2]
            done[op] += 1
            if obs_rng.random() < 0.7:
                done["observed vehicles"] += observe(observed, obs_rng, at + " after " + op)
                done["observe"] += 1
        assert_same_state(observed, plain, "%s seed %d, round %d" % (where, seed, round_))
    assert done["observe"] >= rounds and done["observed vehicles"] > 0 and done["long runs"] > 0, done
    for op in kinds:
        assert done[op] > 0 or (op in ("checkpoint", "rollback") and not checkpoints), "%s never ran: %s" % (op, done)
    return done


def test_sequence_twin_against_twin(mod, scen, workdir):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True)
    run_sequence(twin(mod, cfg), twin(mod, cfg), SEED, ROUNDS, "grid_6x6 twin")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["auto", "dense"])
def test_sequence_with_observations_equals_the_twin_without(mod, scen, workdir, layout):
    cfg = scen.materialize("grid_6x6", workdir, rlTrafficLight=True, **({"cfx": {"layout": "dense"}} if layout == "dense" else {}))
    run_sequence(hip_engine(mod, cfg, layout), twin(mod, cfg), SEED, ROUNDS, "grid_6x6 " + layout)
