"""The lane-per-problem kernel's pivots (csrc/qp_lane.hip: pivot1, pivot2, the copy of pivot1 in the set-up): the headline build
walks the tableau's stored triangle in chunks -- a chunk's LDS reads together, then its FMAs, then its stores -- where the builds
that keep the state or hold H in full go pair by pair. Only the order between independent entries differs, so every result
bit must be the same whichever build answers, and the oracle's.

One shape (8 x 2), one pattern, H in its leading 4 x 4 block (so the batch takes `HB = 4`); the members differ in every vector and
in the matrix values, and neighbouring lanes of a wave pivot on different rows at once. Variable 0 has no bounds (variable 2 of
every other member neither): they enter by pivots during the set-up; the variables 4 .. 7 have no curvature, so a bound of theirs
that leaves with no free curvature around flips to its other side. The oracle's own paths (the working set after each change)
say which changes ran: a test without a GPU counts them per batch, and checks that the answers are unambiguous (strict
complementarity, no tie in a ratio test: test_gpu_lane_io.py's margin check). Batches of 65 and 129: full waves and a ragged
wave of one, whose member also sits in a full wave."""
from collections import Counter

import numpy as np
import pytest

from conftest import oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc
from test_gpu_lane_io import FIELDS, _path
from test_gpu_parity import assert_same_solution

SEED, DISTINCT = 9100, 128
# batch size -> the distinct member that its ragged wave holds: 22 sits in the first wave of both batches as well, 100 in the second
# wave of the larger one (both take an exchange; 100 the only one with a constraint as partner)
RAGGED = {65: 100, 129: 22}
CHANGES = ("set-up pivot", "bound leaves", "constraint enters", "variable fixed", "constraint leaves", "exchange, constraint as partner",
           "exchange, bound as partner", "flip")
_cache = {}


def distinct_members():
    if "members" not in _cache:
        rng = np.random.default_rng(SEED)
        M = rng.normal(size=(4, 4))
        H0 = np.zeros((8, 8)); H0[:4, :4] = M @ M.T / 4 + np.eye(4)
        A0 = rng.normal(size=(2, 8))
        out = []
        for k in range(DISTINCT):
            H = H0.copy(); H[:4, :4] *= 1.0 + 0.05 * np.abs(rng.normal())
            A = A0 * (1.0 + 0.05 * rng.normal(size=A0.shape))
            g = 3.0 * rng.normal(size=8)
            xh = rng.normal(size=8)
            lb = xh - np.abs(rng.normal(size=8)); ub = xh + np.abs(rng.normal(size=8))
            lb[0] = -np.inf; ub[0] = np.inf
            if k % 2: lb[2] = -np.inf; ub[2] = np.inf
            if k % 3 == 0: lb[1] = -np.inf
            w = 0.3 if k % 4 == 0 else 1.0
            lbA = A @ xh - w * np.abs(rng.normal(size=2)); ubA = A @ xh + w * np.abs(rng.normal(size=2))
            out.append(QPData(8, 2, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, lbA, ubA, name="m%d" % k))
        _cache["members"] = out
    return _cache["members"]


def batch(size):
    """(the members, the index among the distinct ones of each): full waves of distinct members, then the ragged wave's one"""
    idx = list(range(size - 1)) + [RAGGED[size]]
    D = distinct_members()
    return [D[i] for i in idx], idx


def oracle_of(oracle, k):
    """the oracle's cold start of distinct member k, computed once, left as it is"""
    if ("oracle", k) not in _cache:
        _cache[("oracle", k)] = oracle_cold(oracle, distinct_members()[k])
    return _cache[("oracle", k)]


def changes_of(oracle, k):
    """what the oracle did on distinct member k: a Counter over CHANGES, from the working set after each of its changes"""
    if ("changes", k) not in _cache:
        qp, rc, n = oracle_of(oracle, k)
        ws = [np.array(b + c) for _, b, c in _path(oracle, distinct_members()[k], n)]
        ev = Counter({"set-up pivot": int(np.sum(ws[0][:8] == 0))})
        for a, b in zip(ws[:-1], ws[1:]):
            moved = np.nonzero(a != b)[0]
            left = [i for i in moved if a[i] != 0 and b[i] == 0]
            came = [i for i in moved if a[i] == 0 and b[i] != 0]
            if len(moved) == 1 and a[moved[0]] == -b[moved[0]]:
                ev["flip"] += 1
            elif len(moved) == 1 and left:
                ev["constraint leaves" if left[0] >= 8 else "bound leaves"] += 1
            elif len(moved) == 1 and came:
                ev["constraint enters" if came[0] >= 8 else "variable fixed"] += 1
            else:
                assert len(moved) == 2 and len(left) == 1 and len(came) == 1, (k, a, b)
                ev["exchange, constraint as partner" if left[0] >= 8 else "exchange, bound as partner"] += 1
        assert ev["flip"] == qp.nflips(), (k, ev, qp.nflips())
        _cache[("changes", k)] = ev
    return _cache[("changes", k)]


def test_the_members_share_one_pattern_with_H_in_its_leading_block():
    D = distinct_members()
    key = lambda q: (tuple(q.A_jc), tuple(q.A_ir), tuple(q.H_jc), tuple(q.H_ir))
    assert len({key(q) for q in D}) == 1
    assert int(D[0].A_jc[8]) == 16 and int(D[0].H_jc[8]) == 16 and D[0].H_ir.max() < 4 and int(D[0].H_jc[4]) == 16
    assert any(not np.array_equal(q.A_val, D[0].A_val) for q in D[1:]) and any(not np.array_equal(q.H_val, D[0].H_val) for q in D[1:])


@pytest.mark.parametrize("size", sorted(RAGGED))
def test_the_oracle_runs_every_kind_of_change(oracle, size):
    """(no GPU) per batch: each kind of change at least once among its members -- and in the member of the ragged wave an exchange --,
    and in every full wave lanes that differ in what they do at a given change (the kinds are mixed inside the waves)"""
    probs, idx = batch(size)
    total = Counter()
    for k in idx:
        total.update(changes_of(oracle, k))
    print(size, dict(total))
    for c in CHANGES:
        assert total[c] >= 1, (size, c, dict(total))
    rag = changes_of(oracle, RAGGED[size])
    assert rag["exchange, constraint as partner"] + rag["exchange, bound as partner"] >= 1, dict(rag)
    for w0 in range(0, size - 1, 64):
        assert len({tuple(sorted(changes_of(oracle, k).items())) for k in idx[w0:w0 + 64]}) >= 16


def test_the_oracle_answers_are_unambiguous(oracle):
    """(no GPU) test_gpu_lane_io.py's margins on every distinct member: solved; the multiplier of every active bound / constraint
    away from zero and every inactive one away from its limits; no ratio test ties -- the path does not move with the vectors"""
    rng = np.random.default_rng(1)
    for k, q in enumerate(distinct_members()):
        qp, rc, n = oracle_of(oracle, k)
        assert rc == 0 and qp.exitflag() == 20, (k, rc)
        x, y = qp.x, qp.y
        val = np.concatenate([x, q.dense_A() @ x]); lo = np.concatenate([q.lb, q.lbA]); hi = np.concatenate([q.ub, q.ubA])
        ws = np.concatenate([qp.ws_bounds, qp.ws_constraints])
        assert np.all(np.abs(y[ws != 0]) > 1e-6), k
        assert np.all((val - lo)[ws == 0] > 1e-6) and np.all((hi - val)[ws == 0] > 1e-6), k
        d = [1e-10 * rng.normal(size=v.shape) for v in (q.g, q.lb, q.ub, q.lbA, q.ubA)]
        ref = _path(oracle, q, n)
        assert ref[-1][0] == n
        assert _path(oracle, q, n, d, 1.0) == ref and _path(oracle, q, n, d, -1.0) == ref, k


def lane_cold(capi, monkeypatch, probs, full_H=False, keep=False):
    monkeypatch.setenv("RSQP_LANE", "1")
    if full_H:
        monkeypatch.setenv("RSQP_LANE_HBLOCK", "0")
    else:
        monkeypatch.delenv("RSQP_LANE_HBLOCK", raising=False)
    b = capi.Batch(probs)
    b.set_keep_state(keep)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 2
    assert b.lane_hblock() == (8 if full_H else 4)
    return b, b.results()


def block_results(capi, monkeypatch, size):
    """the batch's cold start on the HB = 4 build, solved once"""
    if ("results", size) not in _cache:
        b, res = lane_cold(capi, monkeypatch, batch(size)[0])
        b.close()
        _cache[("results", size)] = res
    return _cache[("results", size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(RAGGED))
def test_chunked_pivots_give_the_oracles_answers_and_the_full_builds_bits(capi, oracle, monkeypatch, size):
    probs, idx = batch(size)
    res = block_results(capi, monkeypatch, size)
    assert len(res) == size
    for k, r in zip(idx, res):
        qp, rc, n = oracle_of(oracle, k)
        assert r["status"] == qp.exitflag() == 20
        assert_same_solution(qp, r, n)                  # (status, nWSR, working sets exact; x, y within 1e-9)
        assert abs(r["obj"] - qp.objective) <= 1e-9 * max(1.0, abs(qp.objective))
    # H as its block (chunked pivots) against H in full (pair by pair): the same bits
    b, full = lane_cold(capi, monkeypatch, probs, full_H=True)
    b.close()
    for i, (a, c) in enumerate(zip(res, full)):
        for f in FIELDS:
            assert np.array_equal(np.asarray(a[f]), np.asarray(c[f])), (size, i, f, a[f], c[f])


@pytest.mark.gpu
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch):
    small, large = block_results(capi, monkeypatch, 65), block_results(capi, monkeypatch, 129)
    # (ragged wave, full wave): member 22 within the larger batch and across the two, member 100 across the two
    for rag, ful in ((large[128], large[22]), (large[128], small[22]), (small[64], large[100])):
        for f in FIELDS:
            assert np.array_equal(np.asarray(rag[f]), np.asarray(ful[f])), (f, rag[f], ful[f])


@pytest.mark.gpu
def test_hot_starts_continue_from_the_tableau_the_pivots_left(capi, oracle, monkeypatch):
    """state kept: hot starts on new vectors, then on new matrices, then on new vectors again (8-lane kernel, from the block the
    lane kernel wrote) take the oracle's number of changes exactly, member by member. (The build that keeps the state goes pair by
    pair through its pivots: this is the tableau THOSE left, through every kind of change of the members above.)"""
    probs, idx = batch(65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    orcs = []
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)              # (a handle of its own: the hot starts move it)
        assert_same_solution(qp, r, n)
        orcs.append(qp)
    rng = np.random.default_rng(SEED + 1)
    cur, changes = probs, 0
    for step in range(3):
        nxt = [problems.perturb(rng, q, 0.3) for q in cur]
        new_matrices = step == 1
        if new_matrices:
            for q in nxt:
                q.A_val = q.A_val * (1.0 + 0.02 * rng.normal(size=q.A_val.shape))
        b.set_vectors_from(nxt)
        if new_matrices:
            b.set_matrix_values(np.concatenate([q.A_val for q in nxt]), np.concatenate([q.H_val for q in nxt]))
        b.solve(capi.MODE_HOT_MATRICES if new_matrices else capi.MODE_HOT_VECTORS, 1000)
        assert b.last_kernel() == 1
        for q, qp, r in zip(nxt, orcs, b.results()):
            if new_matrices:
                qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
                rc, n = qp.hotstart_matrices(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            else:
                rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            assert r["nWSR"] == n
            assert_same_solution(qp, r, n)
            changes += n
        cur = nxt
    assert changes > 0
    b.close()
