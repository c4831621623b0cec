"""The lane-per-problem kernel's way in and out (csrc/qp_lane.hip: stage, the results block): a FULL wave of 64 members moves its
inputs and results 16 bytes per lane, a ragged last wave keeps the 8-byte path. Whatever path a member takes, its answer must not
depend on where it sits in the batch:

* place independence, bit for bit: a batch of distinct members, and the same members rotated by 37 places -- np.array_equal member
  by member on x, y, working sets, status, nWSR and objective, no member exempt. Sizes 64 (one full wave), 65 and 127 (a full wave
  and a ragged one: the rotation carries members across), 1 and 129; shapes whose entry counts are even and odd (a pair of doubles
  straddling two members), every way H reaches the kernel (its leading 4 x 4 block, the table of up to 16 entries, the gather of
  a fuller H, no H at all), no constraints, and patterns of their own;
* every member against the oracle with the bar of test_gpu_lane.py: status, working sets and nWSR exact, x and y within 1e-9;
* one batch whose state is kept: the hot start that follows continues from the state this kernel wrote, nWSR as the oracle's.

The members are chosen (seeds) so that the oracle's answers are unambiguous, which a test without a GPU checks: strict
complementarity at the solution, and no tie in a ratio test -- the oracle breaks ties by the lowest id, so a tie shows as a path
(the working set after every change) that moves when the vectors move by +d or -d, |d| ~ 1e-10: the difference of two tied step
lengths is linear in d to first order and changes sign with it."""
import numpy as np
import pytest

from conftest import oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc
from test_gpu_parity import assert_same_solution

FIELDS = ("x", "y", "ws_b", "ws_c", "status", "nWSR", "obj")
NMAX, ROT = 129, 37
SIZES = (64, 65, 127, 1, 129)


def _with_H(q, Hc):
    return QPData(q.nV, q.nC, *Hc, q.A_jc, q.A_ir, q.A_val, q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name)


def _perturbations(rng, base, n, rel=0.05):
    out = []
    for _ in range(n):
        q = problems.perturb(rng, base, rel)
        q.A_val = q.A_val * (1.0 + rel * rng.normal(size=q.A_val.shape))
        out.append(q)
    return out


def _random(nV, nC, seed):
    rng = np.random.default_rng(seed)
    return _perturbations(rng, problems.random_qp(rng, nV, nC, density=0.7), NMAX)


def _hs071():
    return problems.hs071_scale_batch(NMAX)


def _hs071_outside_block():
    out = []
    for q in problems.hs071_scale_batch(NMAX):
        H = q.dense_H()
        H[4, 4] = 0.5                                   # curvature of a slack variable: 12 entries, one outside the 4 x 4 block
        out.append(_with_H(q, dense_to_csc(H)))
    return out


def _no_H():
    rng = np.random.default_rng(8200)
    empty = (np.zeros(9, np.int32), np.zeros(0, np.int32), np.zeros(0))
    return [_with_H(q, empty) for q in _perturbations(rng, problems.random_qp(rng, 8, 2, density=0.7), NMAX)]


def _own_patterns():
    rng = np.random.default_rng(8207)
    bases = [problems.random_qp(rng, 8, 2, density=d) for d in (0.3, 0.6, 1.0)]
    for k, b0 in enumerate(bases[:2]):                  # (Hessian patterns of their own too: thinned symmetrically, still positive definite)
        H = b0.dense_H()
        M = np.triu(rng.random((8, 8)) < (0.3 + 0.3 * k), 1)
        H = H * (M | M.T | np.eye(8, dtype=bool))
        H += np.diag(np.abs(H).sum(axis=1))
        b0.H_jc, b0.H_ir, b0.H_val = dense_to_csc(H)
    out = []
    for k in range(NMAX):
        q = problems.perturb(rng, bases[k % 3], 0.05)
        q.A_val = q.A_val * (1.0 + 0.05 * rng.normal(size=q.A_val.shape))
        out.append(q)
    return out


# name -> (members, the build that serves them: H as its leading block (4) or in full (8))
SHAPES = {
    "hs071": (_hs071, 4),
    "hs071_outside_block": (_hs071_outside_block, 8),
    "8x2_dense_H": (lambda: _random(8, 2, 8201), 8),
    "8x2_no_H": (_no_H, 4),
    "3x1": (lambda: _random(3, 1, 8202), 4),
    "5x2": (lambda: _random(5, 2, 8203), 8),
    "7x1": (lambda: _random(7, 1, 8204), 8),
    "8x0": (lambda: _random(8, 0, 8205), 8),
    "1x2": (lambda: _random(1, 2, 8206), 4),
    "own_patterns": (_own_patterns, 8),
}
_members, _oracles = {}, {}


def members(name):
    if name not in _members:
        _members[name] = SHAPES[name][0]()
    return _members[name]


def oracle_of(oracle, name, k):
    """the oracle's cold start of member k, computed once"""
    if (name, k) not in _oracles:
        _oracles[(name, k)] = oracle_cold(oracle, members(name)[k])
    return _oracles[(name, k)]


def test_the_shapes_are_what_they_are_named_for():
    for name, hnnz in {"hs071": 11, "hs071_outside_block": 12}.items():
        q = members(name)[0]
        assert int(q.H_jc[8]) == hnnz and int(q.A_jc[8]) == 12
    assert int(members("8x2_dense_H")[0].H_jc[8]) == 64 and int(members("8x2_no_H")[0].H_jc[8]) == 0
    own = members("own_patterns")
    assert len({(tuple(q.A_jc), tuple(q.A_ir), tuple(q.H_jc), tuple(q.H_ir)) for q in own}) == 3
    for name in SHAPES:
        if name != "own_patterns":
            qs = members(name)
            assert all(np.array_equal(q.A_ir, qs[0].A_ir) and np.array_equal(q.H_ir, qs[0].H_ir) for q in qs), name
            assert any(not np.array_equal(q.g, qs[0].g) for q in qs[1:]), name


def _path(oracle, q, n, d=None, sign=0.0):
    """the working set after each of the n changes (the oracle stopped at limits 0 .. n), vectors moved by sign * d"""
    out = []
    for limit in range(n + 1):
        if d is None:
            p = q
        else:
            mv = lambda v, dv: np.where(np.abs(v) < 1e17, v + sign * dv, v)
            both = lambda lo, hi, dl, dh: (mv(lo, dl), np.where(hi == lo, mv(lo, dl), mv(hi, dh)))      # (an equality stays one)
            p = QPData(q.nV, q.nC, q.H_jc, q.H_ir, q.H_val, q.A_jc, q.A_ir, q.A_val, q.g + sign * d[0], *both(q.lb, q.ub, d[1], d[2]),
                       *both(q.lbA, q.ubA, d[3], d[4]), name=q.name)
        qp, rc, k = oracle_cold(oracle, p, nWSR=limit)
        out.append((k, tuple(qp.ws_bounds), tuple(qp.ws_constraints)))
    return out


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_oracle_answers_are_unambiguous(oracle, name):
    """(no GPU) every member solved; strict complementarity: the multiplier of every active bound / constraint is away from zero,
    every inactive one is away from its limits; no ratio test ties (see the module's text)"""
    rng = np.random.default_rng(1)
    for k, q in enumerate(members(name)):
        qp, rc, n = oracle_of(oracle, name, k)
        assert rc == 0 and qp.exitflag() == 20, (name, k, rc)
        x, y = qp.x, qp.y
        ax = q.dense_A() @ x if q.nC else np.zeros(0)
        val = np.concatenate([x, ax]); lo = np.concatenate([q.lb, q.lbA]); hi = np.concatenate([q.ub, q.ubA])
        ws = np.concatenate([qp.ws_bounds, qp.ws_constraints])
        assert np.all(np.abs(y[ws != 0]) > 1e-6), (name, k)
        assert np.all((val - lo)[ws == 0] > 1e-6) and np.all((hi - val)[ws == 0] > 1e-6), (name, k)
        d = [1e-10 * rng.normal(size=v.shape) for v in (q.g, q.lb, q.ub, q.lbA, q.ubA)]
        ref = _path(oracle, q, n)
        assert ref[-1][0] == n
        assert _path(oracle, q, n, d, 1.0) == ref and _path(oracle, q, n, d, -1.0) == ref, (name, k)


def expected_block(probs):
    """4: one pattern and no entry of H outside its leading 4 x 4 block (none at all qualifies), else 8"""
    key = lambda q: (tuple(q.A_jc), tuple(q.A_ir), tuple(q.H_jc), tuple(q.H_ir))
    if len({key(q) for q in probs}) != 1:
        return 8
    q = probs[0]
    cols = np.repeat(np.arange(q.nV), np.diff(q.H_jc))
    return 4 if (len(q.H_ir) == 0 or (q.H_ir.max() < 4 and cols.max() < 4)) else 8


def lane_cold(capi, monkeypatch, probs, keep=False):
    monkeypatch.setenv("RSQP_LANE", "1")
    monkeypatch.delenv("RSQP_LANE_HBLOCK", raising=False)
    b = capi.Batch(probs)
    b.set_keep_state(keep)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 2
    return b, b.results(), b.lane_hblock()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_member_answers_the_same_wherever_it_sits(capi, oracle, monkeypatch, name, size):
    probs = members(name)[:size]
    b, res, hb = lane_cold(capi, monkeypatch, probs)
    b.close()
    assert hb == expected_block(probs), (hb, expected_block(probs))
    if size >= 3:                                       # (fewer members than patterns: the members left may share one)
        assert hb == SHAPES[name][1]
    for k, r in enumerate(res):
        qp, rc, n = oracle_of(oracle, name, k)
        assert_same_solution(qp, r, n)
    turned = [probs[(i + ROT) % size] for i in range(size)]
    b, res2, hb2 = lane_cold(capi, monkeypatch, turned)
    b.close()
    assert hb2 == hb
    for i in range(size):
        a, c = res[(i + ROT) % size], res2[i]
        for f in FIELDS:
            assert np.array_equal(np.asarray(a[f]), np.asarray(c[f])), (name, size, i, f, a[f], c[f])
        qp, rc, n = oracle_of(oracle, name, (i + ROT) % size)
        assert_same_solution(qp, c, n)


@pytest.mark.gpu
def test_a_hot_start_continues_from_the_state_a_full_and_a_ragged_wave_wrote(capi, oracle, monkeypatch):
    name = "8x2_dense_H"
    probs = members(name)[:65]
    b, res, hb = lane_cold(capi, monkeypatch, probs, keep=True)
    orcs = []
    for k, r in enumerate(res):
        qp, rc, n = oracle_cold(oracle, probs[k])            # (a handle of its own: the hot start below moves it)
        assert_same_solution(qp, r, n)
        orcs.append(qp)
    rng = np.random.default_rng(8210)
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
