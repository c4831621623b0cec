"""The lane-per-problem kernel (csrc/qp_lane.hip) against the CPU oracle and against the 8-lanes-per-problem kernel it relieves.

It serves cold starts of one-pattern batches of at most 8 x 2 (bench.py's headline workload), with or without the state written back; by default
only for more than 16 384 members -- RSQP_LANE=1 (read per batch) sends every eligible batch to it. Bar as everywhere: working sets,
statuses and iteration counts exact, x / y / objective within 1e-9 relative. The launch, the comparisons and the generators are
tests/lane_cases.py's."""
import numpy as np
import pytest

from conftest import oracle_cold
from lane_cases import (assert_eight_lane_agreement, assert_oracle_answer, assert_same_solution, continue_hot, hs071_path_batch, lane_cold,
                        one_pattern_batch, oracle_handles, own_pattern_batch)
from restartsqp_amd import problems

pytestmark = pytest.mark.gpu


def cold_closed(capi, monkeypatch, probs, lane):
    """lane_cold without kept state -> (results, test_optimality()), the batch closed"""
    b, res = lane_cold(capi, monkeypatch, probs, lane=lane)
    ok, kkt = b.test_optimality()
    b.close()
    return res, ok, kkt


def test_hs071_batch_on_the_lane_kernel(capi, oracle, monkeypatch):
    probs = problems.hs071_scale_batch(1000)
    res, ok, kkt = cold_closed(capi, monkeypatch, probs, "1")
    for q, r, o in zip(probs, res, ok):
        qp, rc, n = oracle_cold(oracle, q)
        assert_oracle_answer(qp, r, n)
        assert rc == 0 and o == 1 and r["nWSR"] == 2


@pytest.mark.parametrize("shape", [(8, 2), (8, 1), (8, 0), (5, 2), (3, 1), (1, 2), (2, 0)])
@pytest.mark.parametrize("free", [False, True])
def test_one_pattern_batches_match_the_oracle_and_the_eight_lane_kernel(capi, oracle, monkeypatch, shape, free):
    nV, nC = shape
    rng = np.random.default_rng(1000 + 10 * nV + nC + (100 if free else 0))
    probs = one_pattern_batch(rng, nV, nC, 200, free=free and nV >= 2)
    lane, ok, kkt = cold_closed(capi, monkeypatch, probs, "1")
    tiny, _, _ = cold_closed(capi, monkeypatch, probs, "0")
    for q, r, t, o, k in zip(probs, lane, tiny, ok, kkt):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
        assert_eight_lane_agreement(r, t)
        if rc == 0:
            assert o == 1 and k < 1e-9
            assert_oracle_answer(qp, r, n)


def test_infeasible_unbounded_and_inconsistent_members(capi, oracle, monkeypatch):
    """Members of one pattern that end differently: solved, infeasible constraints, inconsistent bounds (lb > ub), a ragged tail
    (the batch size is no multiple of 64)."""
    rng = np.random.default_rng(4242)
    probs = one_pattern_batch(rng, 6, 2, 131)
    for k in range(0, 131, 7):
        probs[k].lbA = probs[k].ubA + 50.0; probs[k].ubA = probs[k].lbA + 1.0          # far from the box: infeasible
    for k in range(3, 131, 11):
        probs[k].lb[2] = probs[k].ub[2] + 1.0                                            # inconsistent bounds
    lane, _, _ = cold_closed(capi, monkeypatch, probs, "1")
    tiny, _, _ = cold_closed(capi, monkeypatch, probs, "0")
    seen = set()
    for q, r, t in zip(probs, lane, tiny):
        qp, rc, n = oracle_cold(oracle, q)
        seen.add(r["status"])
        assert r["status"] == qp.exitflag() == t["status"]
        if rc == 0:
            assert_same_solution(qp, r, n)
    assert len(seen) >= 2


def test_default_threshold_and_the_calls_the_lane_kernel_does_not_take(capi, oracle, monkeypatch):
    """Default: batches of at most 16 384 members stay on the 8-lane kernel; a hot start that follows a cold start which kept nothing
    runs cold, as the handle promises; a warm re-initialisation from (x0, y0) goes to the 8-lane kernel."""
    rng = np.random.default_rng(9)
    probs = one_pattern_batch(rng, 8, 2, 70)
    b, _ = lane_cold(capi, monkeypatch, probs)
    p2 = [problems.perturb(rng, q, 0.05) for q in probs]
    b.set_vectors_from(p2)
    b.solve(capi.MODE_HOT_VECTORS, 1000)              # no state was kept: a cold start on the new vectors
    assert b.last_kernel() == 2
    for q, r in zip(p2, b.results()):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
    b.close()
    monkeypatch.delenv("RSQP_LANE")
    b = capi.Batch(probs)
    b.set_keep_state(False)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 1                       # 70 members: below the default threshold
    b.close()


@pytest.mark.parametrize("shape", [(8, 2), (6, 1), (4, 2), (8, 0)])
def test_hot_starts_continue_from_the_state_the_lane_kernel_wrote(capi, oracle, monkeypatch, shape):
    """A batch that keeps its state: the cold start runs on the lane kernel, which writes every member's state block in the layout of
    the 8-lane kernel; the hot starts that follow (new vectors, new matrices, new vectors) run on the 8-lane kernel FROM that state.
    Every member against the oracle's init / hotstart / hotstart(H, g, A, ...) sequence: working sets, statuses and nWSR exact --
    a hot start from a wrong tableau or slot state would take another path."""
    nV, nC = shape
    rng = np.random.default_rng(300 + 10 * nV + nC)
    probs = one_pattern_batch(rng, nV, nC, 150, free=(nV == 6))
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), rng, ("vectors", "matrices", "vectors"))
    b.close()


def test_a_sequence_of_calls_gives_the_same_answers_with_and_without_the_lane_kernel(capi, oracle, monkeypatch):
    """cold start (state kept), hot start on new vectors, hot start with new matrices: the same answers, state-dependent results
    included (nWSR of every hot start), whether the cold start ran on the lane kernel or on the 8-lane kernel."""
    rng = np.random.default_rng(77)
    probs = one_pattern_batch(rng, 8, 2, 90)
    p2 = [problems.perturb(rng, q, 0.3) for q in probs]
    p3 = [problems.perturb(rng, q, 0.3) for q in p2]
    out = {}
    for lane in ("0", "1"):
        b, first = lane_cold(capi, monkeypatch, probs, keep=True, lane=lane)
        seq = [first]
        b.set_vectors_from(p2); b.solve(capi.MODE_HOT_VECTORS, 1000); seq.append(b.results())
        b.set_vectors_from(p3); b.solve(capi.MODE_HOT_MATRICES, 1000); seq.append(b.results())
        assert b.last_kernel() == 1
        out[lane] = seq
        b.close()
    for ra, rb in zip(out["0"], out["1"]):
        for a, c in zip(ra, rb):
            assert_eight_lane_agreement(c, a)


@pytest.mark.parametrize("shape", [(8, 2), (5, 1), (7, 0)])
def test_one_shape_with_patterns_of_their_own(capi, oracle, monkeypatch, shape):
    """Members of one SHAPE whose sparsity patterns differ (three base problems of different density, interleaved member by member;
    entry counts differ as well): the vectors still travel through the wave's block, every lane walks the CSC arrays of its own
    problem. Cold start with the state kept, then a hot start on new vectors (8-lane kernel, from that state): the oracle's sequence."""
    nV, nC = shape
    rng = np.random.default_rng(900 + 10 * nV + nC)
    probs = own_pattern_batch(rng, nV, nC, 201)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), rng)
    b.close()


def test_members_that_take_different_paths(capi, oracle, monkeypatch):
    """The QPs of the hs071 SQP trajectory that share one sparsity pattern (tests/golden/sqp_traces.json: 5 of its 6 iterates), each
    with seeded perturbations, interleaved: neighbouring lanes of a wave take different paths of 5 changes each (entering and leaving
    bounds and constraints, exchanges) -- the wave executes their union, every lane must still end where the oracle does."""
    probs = hs071_path_batch(640)
    res, ok, kkt = cold_closed(capi, monkeypatch, probs, "1")
    paths = set()
    for q, r, o in zip(probs, res, ok):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
        assert rc == 0 and o == 1
        paths.add((r["nWSR"], tuple(r["ws_b"]), tuple(r["ws_c"])))
    assert len(paths) >= 2


@pytest.mark.parametrize("limit", [0, 1, 2])
def test_iteration_limit(capi, oracle, monkeypatch, limit):
    """nWSR limits below / at what the members need (the hs071 QP takes 2 changes): status, return code and the iterate where the
    homotopy was stopped as the oracle has them; the 8-lane kernel agrees."""
    probs = problems.hs071_scale_batch(100)
    out = {}
    for lane in ("1", "0"):
        monkeypatch.setenv("RSQP_LANE", lane)
        b = capi.Batch(probs)
        b.set_keep_state(False)
        b.solve(capi.MODE_COLD, limit)
        assert b.last_kernel() == (2 if lane == "1" else 1)
        out[lane] = b.results()
        b.close()
    for q, r, t in zip(probs, out["1"], out["0"]):
        qp, rc, n = oracle_cold(oracle, q, nWSR=limit)
        assert r["status"] == qp.exitflag() == t["status"] and r["nWSR"] == n == t["nWSR"]
        assert (r["status"] == 20) == (limit >= 2)
        assert np.array_equal(qp.ws_bounds, r["ws_b"]) and np.array_equal(qp.ws_constraints, r["ws_c"])
        assert np.abs(qp.x - r["x"]).max() <= 1e-9 * max(1.0, np.abs(qp.x).max())
