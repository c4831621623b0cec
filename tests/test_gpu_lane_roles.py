"""The lane-per-problem kernel's ratio test (csrc/qp_lane.hip, homotopy()): the headline build -- H as its leading 4 x 4 block, no state
kept -- branches on the ROLE of a variable slot (free: two bound candidates; fixed: one multiplier candidate) where the other builds
compute both roles and select, and leaves out the re-relaxation of the limits that a cold start cannot need. Per lane the operands,
the candidate ids and the tie rule are the same, so every result bit must be the same whichever build answers, and the oracle's.

What can go wrong shows only when the lanes of ONE wave disagree on the role of the SAME slot in the same pass: then both arms run,
each under its own mask. One shape (8 x 2), one pattern, H in its leading 4 x 4 block (the batch takes `HB = 4`); the members differ in
every vector, in the matrix values and in WHICH bounds they have: a slot starts free (no bound: it pivots in during the set-up), at
its lower bound, or at its upper bound (no lower one) depending on the member, and the paths spread from there -- bounds leave (free
variables with both bounds finite), constraints enter and leave, exchanges with a bound and with a constraint as partner. A test
without a GPU reads the oracle's own paths (the working set after each change) and asserts, for every slot, a wave whose lanes hold
it in two roles at the same change count -- for the variable slots free beside at-lower and free beside at-upper --, and that no
member's answer is ambiguous (strict complementarity, no tie in a ratio test: test_gpu_lane_io.py's margin check). Batches of 65
and 129: full waves and a ragged wave of one, whose member also sits in a full wave."""
import numpy as np
import pytest

from conftest import oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc
from test_gpu_lane_io import FIELDS, _path
from test_gpu_parity import assert_same_solution

SEED, DISTINCT = 9300, 128
# batch size -> the distinct member that its ragged wave holds: one of the first wave (in both batches) and one of the second wave of
# the larger batch; both take an exchange (the CPU test below asserts it)
RAGGED = {65: 90, 129: 25}
_cache = {}


def distinct_members(seed=None):
    key = ("members", SEED if seed is None else seed)
    if key not in _cache:
        rng = np.random.default_rng(key[1])
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
            # the role a slot starts in moves with the member: slot (k mod 4) has no bound (free from the set-up on; it has curvature),
            # the slots l with (k + l) mod 3 == 0 no lower bound (they start at their upper one), the rest start at their lower bound
            # (a slot without curvature and without a lower bound: its gradient points at the upper one, the QP stays bounded)
            for l in range(8):
                if (k + l) % 3 == 0:
                    lb[l] = -np.inf
                    if l >= 4: g[l] = -abs(g[l])
            lb[k % 4] = -np.inf; ub[k % 4] = np.inf
            w = 0.3 if k % 4 == 0 else 1.0
            lbA = A @ xh - w * np.abs(rng.normal(size=2)); ubA = A @ xh + w * np.abs(rng.normal(size=2))
            out.append(QPData(8, 2, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, lbA, ubA, name="m%d" % k))
        _cache[key] = out
    return _cache[key]


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


def path_of(oracle, k):
    """the oracle's working sets of distinct member k, [bounds (8); constraints (2)] after 0 .. nWSR changes"""
    if ("path", k) not in _cache:
        qp, rc, n = oracle_of(oracle, k)
        _cache[("path", k)] = [np.array(b + c) for _, b, c in _path(oracle, distinct_members()[k], n)]
    return _cache[("path", k)]


def exchanges_of(oracle, k):
    """(exchanges with a constraint as partner, with a bound as partner) on the oracle's path of distinct member k"""
    con = bnd = 0
    ws = path_of(oracle, k)
    for a, b in zip(ws[:-1], ws[1:]):
        moved = np.nonzero(a != b)[0]
        if len(moved) == 2:
            left = [i for i in moved if a[i] != 0 and b[i] == 0]
            assert len(left) == 1, (k, a, b)
            con += left[0] >= 8; bnd += left[0] < 8
    return con, bnd


def test_the_members_share_one_pattern_with_H_in_its_leading_block():
    D = distinct_members()
    key = lambda q: (tuple(q.A_jc), tuple(q.A_ir), tuple(q.H_jc), tuple(q.H_ir))
    assert len({key(q) for q in D}) == 1
    assert int(D[0].A_jc[8]) == 16 and int(D[0].H_jc[8]) == 16 and D[0].H_ir.max() < 4 and int(D[0].H_jc[4]) == 16
    assert any(not np.array_equal(q.A_val, D[0].A_val) for q in D[1:]) and any(not np.array_equal(q.H_val, D[0].H_val) for q in D[1:])


@pytest.mark.parametrize("size", sorted(RAGGED))
def test_lanes_of_one_wave_hold_every_slot_in_different_roles_at_once(oracle, size):
    """(no GPU) from the oracle's paths, per batch: for EVERY slot a full wave in which, after the same number of changes (the pass of
    the kernel's loop that the lanes run together), two members that are both still running hold the slot in different roles -- a
    variable free in one lane beside at its lower bound in another, and free beside at its upper bound; a constraint active beside
    inactive. Members with a free variable between two finite bounds, members with a variable without bounds, and exchanges with
    a bound and with a constraint as partner, the ragged wave's member among them"""
    probs, idx = batch(size)
    for slot in range(10):
        # (a constraint slot has two roles, inactive and active on either side)
        want = [{0, -1}, {0, 1}] if slot < 8 else [{0, 2}]
        seen = [False] * len(want)
        for w0 in range(0, size - 1, 64):
            paths = [path_of(oracle, k) for k in idx[w0:w0 + 64]]
            for j in range(max(len(p) for p in paths)):
                roles = {int(p[j][slot]) if slot < 8 else 2 * int(p[j][slot] != 0) for p in paths if len(p) > j}
                seen = [s or pair <= roles for s, pair in zip(seen, want)]
        assert all(seen), (size, slot, seen)
    two_bounds = unbounded = con = bnd = 0
    for k in set(idx):
        q = distinct_members()[k]
        fin = np.isfinite(q.lb) & np.isfinite(q.ub)
        two_bounds += any(np.any((p[:8] == 0) & fin) for p in path_of(oracle, k))
        unbounded += bool(np.any(np.isinf(q.lb) & np.isinf(q.ub)))
        c, b = exchanges_of(oracle, k)
        con += c > 0; bnd += b > 0
    print(size, "members with a free variable between finite bounds", two_bounds, "without bounds", unbounded, "exchange with a constraint",
          con, "with a bound", bnd)
    assert two_bounds >= 8 and unbounded >= 8 and con >= 1 and bnd >= 1
    assert sum(exchanges_of(oracle, RAGGED[size])) >= 1


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
    assert b.lane_hblock() == (8 if full_H else 4)          # (rsqp_batch_get_lane_hblock: the build that answered)
    return b, b.results()


def block_results(capi, monkeypatch, size):
    """the batch's cold start on the HB = 4 build without its state (the build with the arms), solved once"""
    if ("results", size) not in _cache:
        b, res = lane_cold(capi, monkeypatch, batch(size)[0])
        b.close()
        _cache[("results", size)] = res
    return _cache[("results", size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(RAGGED))
def test_the_arms_give_the_oracles_answers(capi, oracle, monkeypatch, size):
    probs, idx = batch(size)
    res = block_results(capi, monkeypatch, size)
    assert len(res) == size
    for k, r in zip(idx, res):
        qp, rc, n = oracle_of(oracle, k)
        assert r["status"] == qp.exitflag() == 20
        assert_same_solution(qp, r, n)                  # (status, nWSR, working sets exact; x, y within 1e-9)
        assert abs(r["obj"] - qp.objective) <= 1e-9 * max(1.0, abs(qp.objective))


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(RAGGED))
def test_the_arms_give_the_bits_of_the_selects(capi, monkeypatch, size):
    """H as its block (arms per role) against RSQP_LANE_HBLOCK=0 (H in full: both roles computed, then selected) inside one library"""
    probs, idx = batch(size)
    res = block_results(capi, monkeypatch, size)
    b, full = lane_cold(capi, monkeypatch, probs, full_H=True)
    b.close()
    assert len(full) == len(res) == size
    for i, (a, c) in enumerate(zip(res, full)):
        for f in FIELDS:
            assert np.array_equal(np.asarray(a[f]), np.asarray(c[f])), (size, i, f, a[f], c[f])


@pytest.mark.gpu
@pytest.mark.parametrize("size", sorted(RAGGED))
def test_the_arms_agree_with_the_eight_lane_kernel(capi, monkeypatch, size):
    """against RSQP_LANE=0 as test_gpu_lane.py compares the two kernels: status, nWSR and working sets exact, x within 1e-9"""
    probs, idx = batch(size)
    res = block_results(capi, monkeypatch, size)
    monkeypatch.setenv("RSQP_LANE", "0")
    b = capi.Batch(probs)
    b.set_keep_state(False)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 1
    tiny = b.results()
    b.close()
    for r, t in zip(res, tiny):
        assert r["status"] == t["status"] and r["nWSR"] == t["nWSR"] and np.array_equal(r["ws_b"], t["ws_b"]) and np.array_equal(r["ws_c"], t["ws_c"])
        assert np.abs(r["x"] - t["x"]).max() <= 1e-9 * max(1.0, np.abs(t["x"]).max())


@pytest.mark.gpu
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch):
    small, large = block_results(capi, monkeypatch, 65), block_results(capi, monkeypatch, 129)
    a, c = RAGGED[129], RAGGED[65]
    # (ragged wave, full wave): member a within the larger batch and across the two, member c across the two
    for rag, ful in ((large[128], large[a]), (large[128], small[a]), (small[64], large[c])):
        for f in FIELDS:
            assert np.array_equal(np.asarray(rag[f]), np.asarray(ful[f])), (f, rag[f], ful[f])


@pytest.mark.gpu
def test_a_hot_start_continues_from_the_state_the_unchanged_build_kept(capi, oracle, monkeypatch):
    """state kept (the build that keeps the selects): the cold start, then a hot start on new vectors (8-lane kernel, from the block
    the lane kernel wrote) take the oracle's number of changes exactly, member by member"""
    probs, idx = batch(65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    orcs = []
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)              # (a handle of its own: the hot start moves it)
        assert_same_solution(qp, r, n)
        orcs.append(qp)
    rng = np.random.default_rng(SEED + 1)
    nxt = [problems.perturb(rng, q, 0.3) for q in probs]
    b.set_vectors_from(nxt)
    b.solve(capi.MODE_HOT_VECTORS, 1000)
    assert b.last_kernel() == 1
    changes = 0
    for q, qp, r in zip(nxt, orcs, b.results()):
        rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
        assert r["nWSR"] == n
        assert_same_solution(qp, r, n)
        changes += n
    assert changes > 0
    b.close()
