"""What the test files of the lane-per-problem kernel (tests/test_gpu_lane*.py, csrc/qp_lane.hip) share, each stated once: the launch,
the comparisons, the oracle-side checks, the hot-start continuation and the member families that more than one file uses. No test
module of the family imports another one; a family that one file alone uses stays in that file and registers with FAMILIES, so its
members and the oracle's answers for them are computed once like everybody's.

The seeds of the families were chosen on the oracle so that every answer is unambiguous (assert_unambiguous) and every situation a
file is about occurs; a file's tests without a GPU assert both. A generator draws from its rng in a fixed order: change the order and
every batch changes."""
import json
import os
from collections import Counter

import numpy as np

from conftest import GOLDEN, oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc
from small_builds import with_H
from test_gpu_parity import assert_same_solution              # (re-exported: the lane files import from here alone)

FIELDS = ("x", "y", "ws_b", "ws_c", "status", "nWSR", "obj")
FULL = 8 * 256 + 2                                            # Batch.lane_shape() of the full-shape build
RTOL = 1e-9
SWITCHES = ("RSQP_LANE", "RSQP_LANE_HBLOCK", "RSQP_LANE_SHAPE")           # (read per batch, by rsqp_batch_create)


# ------------------------------------------------------------------------------------
# the launch
# ------------------------------------------------------------------------------------
def lane_cold(capi, monkeypatch, probs, *, keep=False, full_H=False, shape=True, lane="1"):
    """one cold start of a fresh batch -> (the open batch, its results). lane: RSQP_LANE ("0": the 8-lane kernel); full_H:
    RSQP_LANE_HBLOCK=0; shape = False: RSQP_LANE_SHAPE=0. Every switch is set or deleted on every call. Which build answered:
    b.lane_hblock(), b.lane_shape()"""
    for name, value in zip(SWITCHES, (lane, "0" if full_H else None, None if shape else "0")):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    b = capi.Batch(probs)
    b.set_keep_state(keep)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == (2 if lane != "0" else 1)
    return b, b.results()


# ------------------------------------------------------------------------------------
# the comparisons
# ------------------------------------------------------------------------------------
def assert_same_bits(a, c, tag=None):
    """every field of a result equal bit for bit (np.array_equal); one result against one, or a list against a list"""
    if isinstance(a, dict):
        a, c = [a], [c]
    assert len(a) == len(c), (tag, len(a), len(c))
    for i, (ra, rc) in enumerate(zip(a, c)):
        for f in FIELDS:
            assert np.array_equal(np.asarray(ra[f]), np.asarray(rc[f])), (tag, i, f, ra[f], rc[f])


def assert_oracle_answer(qp, r, n, tag=None):
    """the bar for a member the oracle solves: status 20, working sets and nWSR exact, x / y (assert_same_solution) and the objective
    within 1e-9 relative"""
    assert r["status"] == qp.exitflag() == 20, tag
    assert_same_solution(qp, r, n)
    assert abs(r["obj"] - qp.objective) <= RTOL * max(1.0, abs(qp.objective)), tag


def assert_eight_lane_agreement(r, t, tag=None):
    """a lane-kernel result against the 8-lane kernel's (RSQP_LANE=0): status, nWSR and working sets exact, x and y within 1e-9"""
    assert r["status"] == t["status"] and r["nWSR"] == t["nWSR"], tag
    assert np.array_equal(r["ws_b"], t["ws_b"]) and np.array_equal(r["ws_c"], t["ws_c"]), tag
    for f in ("x", "y"):
        assert np.abs(r[f] - t[f]).max() <= RTOL * max(1.0, np.abs(t[f]).max()), (tag, f)


# ------------------------------------------------------------------------------------
# on the oracle's side: needs no GPU
# ------------------------------------------------------------------------------------
def pattern(q):
    return tuple(q.A_jc), tuple(q.A_ir), tuple(q.H_jc), tuple(q.H_ir)


def expected_block(probs):
    """4: one pattern and no entry of H outside its leading 4 x 4 block (none at all qualifies), else 8"""
    if len({pattern(q) for q in probs}) != 1:
        return 8
    q = probs[0]
    cols = np.repeat(np.arange(q.nV), np.diff(q.H_jc))
    return 4 if (len(q.H_ir) == 0 or (q.H_ir.max() < 4 and cols.max() < 4)) else 8


def path(oracle, q, n, d=None, sign=0.0):
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


def working_sets(oracle, q, n):
    """path() as arrays [bounds; constraints]"""
    return [np.array(b + c) for _, b, c in path(oracle, q, n)]


def assert_unambiguous(oracle, q, qp, rc, n, rng, tag=None):
    """the oracle's answer (qp, rc, n) = oracle_cold(q) does not hang on a tie: solved; strict complementarity -- the multiplier of
    every active bound / constraint is away from zero, every inactive one away from its limits --; no tie in a ratio test. The
    oracle breaks ties by the lowest id, so a tie shows as a path that moves when the vectors move by +d or -d, |d| ~ 1e-10: the
    difference of two tied step lengths is linear in d to first order and changes sign with it. Draws d from rng"""
    assert rc == 0 and qp.exitflag() == 20, (tag, rc)
    x, y = qp.x, qp.y
    ax = q.dense_A() @ x if q.nC else np.zeros(0)
    val = np.concatenate([x, ax]); lo = np.concatenate([q.lb, q.lbA]); hi = np.concatenate([q.ub, q.ubA])
    ws = np.concatenate([qp.ws_bounds, qp.ws_constraints])
    assert np.all(np.abs(y[ws != 0]) > 1e-6), tag
    assert np.all((val - lo)[ws == 0] > 1e-6) and np.all((hi - val)[ws == 0] > 1e-6), tag
    d = [1e-10 * rng.normal(size=v.shape) for v in (q.g, q.lb, q.ub, q.lbA, q.ubA)]
    ref = path(oracle, q, n)
    assert ref[-1][0] == n, tag
    assert path(oracle, q, n, d, 1.0) == ref and path(oracle, q, n, d, -1.0) == ref, tag


def assert_family_unambiguous(oracle, family):
    """assert_unambiguous on every member of a family, d from one rng (seed 1) member after member"""
    rng = np.random.default_rng(1)
    for k, q in enumerate(members(family)):
        assert_unambiguous(oracle, q, *oracle_of(oracle, family, k), rng, (family, k))


# ------------------------------------------------------------------------------------
# the hot starts that follow a cold start whose state was kept
# ------------------------------------------------------------------------------------
def oracle_handles(oracle, probs, res):
    """the oracle's cold start of every member, on a handle of its own (the hot starts move it); res against it"""
    orcs = []
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
        orcs.append(qp)
    return orcs


def continue_hot(capi, b, probs, orcs, rng, kinds=("vectors",), rel=0.3, mat_rel=0.02):
    """hot starts of the kept batch b, one per entry of kinds: "vectors" (every vector perturbed by rel) or "matrices" (besides, the
    values of A rescaled by mat_rel). They run on the 8-lane kernel from the state the lane kernel wrote, and every member takes
    the oracle's path from orcs (oracle_handles): working sets, statuses and nWSR exact -- a hot start from a wrong tableau or slot
    state would take another one. Something must change on the way. -> the last members"""
    cur, changes = probs, 0
    for kind in kinds:
        matrices = kind == "matrices"
        assert matrices or kind == "vectors"
        nxt = [problems.perturb(rng, q, rel) for q in cur]
        if matrices:
            for q in nxt:
                q.A_val = q.A_val * (1.0 + mat_rel * rng.normal(size=q.A_val.shape))
        b.set_vectors_from(nxt)
        if matrices:
            b.set_matrix_values(np.concatenate([q.A_val for q in nxt]), np.concatenate([q.H_val for q in nxt]))
        b.solve(capi.MODE_HOT_MATRICES if matrices else capi.MODE_HOT_VECTORS, 1000)
        assert b.last_kernel() == 1 and b.lane_hblock() == 0 and b.lane_shape() == 0
        for q, qp, r in zip(nxt, orcs, b.results()):
            if matrices:
                qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
                rc, n = qp.hotstart_matrices(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            else:
                rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            assert r["nWSR"] == n
            assert_same_solution(qp, r, n)
            changes += n
        cur = nxt
    assert changes > 0
    return cur


# ------------------------------------------------------------------------------------
# generators (every one draws in the order written)
# ------------------------------------------------------------------------------------
def perturbations(rng, base, n, rel=0.05, mat_rel=None):
    """n members on the patterns of base: its vectors perturbed by rel, the values of A rescaled by mat_rel (None: rel)"""
    out = []
    for _ in range(n):
        q = problems.perturb(rng, base, rel)
        q.A_val = q.A_val * (1.0 + (rel if mat_rel is None else mat_rel) * rng.normal(size=q.A_val.shape))
        out.append(q)
    return out


def one_pattern_batch(rng, nV, nC, n, free=False, density=0.7, rel=0.05):
    base = problems.random_qp(rng, nV, nC, density=density)
    if free:
        base.lb[::2] = -np.inf; base.ub[1::3] = np.inf
        base.lb[1] = -np.inf; base.ub[1] = np.inf                  # a variable with no bound at all: it enters S in the set-up
    return perturbations(rng, base, n, rel)


def own_pattern_batch(rng, nV, nC, n):
    """members of one SHAPE whose sparsity patterns differ: three base problems of different density, interleaved member by member;
    entry counts differ as well"""
    bases = [problems.random_qp(rng, nV, nC, density=d) for d in (0.3, 0.6, 1.0)]
    for k, b0 in enumerate(bases[:2]):                  # (Hessian patterns of their own too: thinned symmetrically, still positive definite)
        H = b0.dense_H()
        M = np.triu(rng.random((nV, nV)) < (0.3 + 0.3 * k), 1)
        H = H * (M | M.T | np.eye(nV, dtype=bool))
        H += np.diag(np.abs(H).sum(axis=1))
        b0.H_jc, b0.H_ir, b0.H_val = dense_to_csc(H)
    probs = [perturbations(rng, bases[k % 3], 1)[0] for k in range(n)]
    assert len({(len(q.A_val), len(q.H_val)) for q in probs}) >= 2
    return probs


def hs071_path_batch(n):
    """The QPs of the hs071 SQP trajectory that share one sparsity pattern (tests/golden/sqp_traces.json: 5 of its 6 iterates), each
    with seeded perturbations, interleaved: neighbouring lanes of a wave take different paths of 5 changes each (entering and leaving
    bounds and constraints, exchanges)"""
    tr = json.load(open(os.path.join(GOLDEN, "sqp_traces.json")))["hs071"]["qps"]
    base = [problems.handler_qp(problems.hs071_nlp(np.array(g["x"]), np.array(g["lam"])), delta=g["delta"], rho=g["rho"]) for g in tr]
    best = Counter(pattern(q) for q in base).most_common(1)[0][0]
    base = [q for q in base if pattern(q) == best]
    assert len(base) >= 3
    rng = np.random.default_rng(20260104)
    return [problems.perturb(rng, base[k % len(base)]) for k in range(n)]


def block_members(seed, bounds):
    """128 distinct 8 x 2 members of one pattern, H in its leading 4 x 4 block and A dense, that differ in every vector and in the
    matrix values. bounds(k, g, lb, ub) takes bounds away from member k in place: which ones tells the families apart. Every fourth
    member has narrow constraints"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(4, 4))
    H0 = np.zeros((8, 8)); H0[:4, :4] = M @ M.T / 4 + np.eye(4)
    A0 = rng.normal(size=(2, 8))
    out = []
    for k in range(128):
        H = H0.copy(); H[:4, :4] *= 1.0 + 0.05 * np.abs(rng.normal())
        A = A0 * (1.0 + 0.05 * rng.normal(size=A0.shape))
        g = 3.0 * rng.normal(size=8)
        xh = rng.normal(size=8)
        lb = xh - np.abs(rng.normal(size=8)); ub = xh + np.abs(rng.normal(size=8))
        bounds(k, g, lb, ub)
        w = 0.3 if k % 4 == 0 else 1.0
        lbA = A @ xh - w * np.abs(rng.normal(size=2)); ubA = A @ xh + w * np.abs(rng.normal(size=2))
        out.append(QPData(8, 2, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, lbA, ubA, name="m%d" % k))
    return out


# ------------------------------------------------------------------------------------
# the families
# ------------------------------------------------------------------------------------
NMAX = 129


def _random(nV, nC, seed):
    rng = np.random.default_rng(seed)
    return perturbations(rng, problems.random_qp(rng, nV, nC, density=0.7), NMAX)


def _hs071_outside_block():
    out = []
    for q in problems.hs071_scale_batch(NMAX):
        H = q.dense_H()
        H[4, 4] = 0.5                                   # curvature of a slack variable: 12 entries, one outside the 4 x 4 block
        out.append(with_H(q, H))
    return out


def _no_H():
    rng = np.random.default_rng(8200)
    probs = perturbations(rng, problems.random_qp(rng, 8, 2, density=0.7), NMAX)
    return [QPData(q.nV, q.nC, np.zeros(9, np.int32), np.zeros(0, np.int32), np.zeros(0), q.A_jc, q.A_ir, q.A_val, q.g, q.lb, q.ub,
                   q.lbA, q.ubA, name=q.name) for q in probs]


# test_gpu_lane_io.py's shapes, 129 members each: name -> (members, the build that serves them: H as its leading block (4) or in
# full (8))
SHAPES = {
    "hs071": (lambda: problems.hs071_scale_batch(NMAX), 4),
    "hs071_outside_block": (_hs071_outside_block, 8),
    "8x2_dense_H": (lambda: _random(8, 2, 8201), 8),
    "8x2_no_H": (_no_H, 4),
    "3x1": (lambda: _random(3, 1, 8202), 4),
    "5x2": (lambda: _random(5, 2, 8203), 8),
    "7x1": (lambda: _random(7, 1, 8204), 8),
    "8x0": (lambda: _random(8, 0, 8205), 8),
    "1x2": (lambda: _random(1, 2, 8206), 4),
    "own_patterns": (lambda: own_pattern_batch(np.random.default_rng(8207), 8, 2, NMAX), 8),
}

ROLES_SEED, PIVOTS_SEED = 9300, 9100


def _roles_bounds(k, g, lb, ub):
    # the role a slot starts in moves with the member: slot (k mod 4) has no bound (free from the set-up on; it has curvature),
    # the slots l with (k + l) mod 3 == 0 no lower bound (they start at their upper one), the rest start at their lower bound
    # (a slot without curvature and without a lower bound: its gradient points at the upper one, the QP stays bounded)
    for l in range(8):
        if (k + l) % 3 == 0:
            lb[l] = -np.inf
            if l >= 4: g[l] = -abs(g[l])
    lb[k % 4] = -np.inf; ub[k % 4] = np.inf


def _pivots_bounds(k, g, lb, ub):
    # variable 0 has no bounds, variable 2 of every other member neither: they enter by pivots during the set-up
    lb[0] = -np.inf; ub[0] = np.inf
    if k % 2: lb[2] = -np.inf; ub[2] = np.inf
    if k % 3 == 0: lb[1] = -np.inf


ODD_INCONSISTENT, ODD_INFEASIBLE = 5, 9              # members of the odd batch


def _odd():
    """65 of the "roles" members; one gets inconsistent bounds, one constraints far from its box (test_gpu_lane.py's recipes)"""
    probs = []
    for k, q in enumerate(members("roles")[:65]):
        lb, ub, lbA, ubA = q.lb.copy(), q.ub.copy(), q.lbA.copy(), q.ubA.copy()
        if k == ODD_INCONSISTENT:
            lb[2] = 1.0; ub[2] = 0.0
        if k == ODD_INFEASIBLE:              # (every variable in a box, the constraints far from what the box allows)
            ub = np.where(np.isinf(ub), np.where(np.isinf(lb), 1.0, lb + 2.0), ub)
            lb = np.where(np.isinf(lb), ub - 2.0, lb)
            lbA = q.ubA + 500.0; ubA = lbA + 1.0
        probs.append(QPData(8, 2, q.H_jc, q.H_ir, q.H_val, q.A_jc, q.A_ir, q.A_val, q.g, lb, ub, lbA, ubA, name=q.name))
    return probs


# family -> () -> its members. "roles": test_gpu_lane_roles.py's 128 (slots of one wave in different roles), "pivots":
# test_gpu_lane_pivots.py's 128 (every kind of change), "odd": test_gpu_lane_shape.py's 65 (two of them without a solution)
FAMILIES = {name: make for name, (make, _) in SHAPES.items()}
FAMILIES.update(roles=lambda: block_members(ROLES_SEED, _roles_bounds), pivots=lambda: block_members(PIVOTS_SEED, _pivots_bounds), odd=_odd)
_members, _oracle = {}, {}


def members(family):
    """the members of a family, built once"""
    if family not in _members:
        _members[family] = FAMILIES[family]()
    return _members[family]


def oracle_of(oracle, family, k):
    """(qp, rc, nWSR): the oracle's cold start of member k of a family, computed once, left as it is"""
    if (family, k) not in _oracle:
        _oracle[(family, k)] = oracle_cold(oracle, members(family)[k])
    return _oracle[(family, k)]


# batch size -> the member of the family that the ragged wave of a "roles" / "pivots" batch holds. roles: one of the first wave (in
# both batches) and one of the second wave of the larger batch. pivots: 22 sits in the first wave of both batches as well, 100 in the
# second wave of the larger one (100 the only one with a constraint as partner). All four take an exchange (the files' CPU tests)
RAGGED = {"roles": {65: 90, 129: 25}, "pivots": {65: 100, 129: 22}}


def ragged_batch(family, size):
    """(the members, the index in the family of each): full waves of distinct members, then the ragged wave's one"""
    idx = list(range(size - 1)) + [RAGGED[family][size]]
    D = members(family)
    return [D[i] for i in idx], idx


def assert_ragged_and_full_bits(small, large, family):
    """results of the batches of 65 and of 129: a member answers the same bits in the ragged wave and in a full one -- the ragged
    member of the larger batch within it and across the two, the ragged member of the smaller one across the two"""
    a, c = RAGGED[family][129], RAGGED[family][65]
    for rag, ful in ((large[128], large[a]), (large[128], small[a]), (small[64], large[c])):
        assert_same_bits(rag, ful, family)


def assert_one_block_pattern(D):
    """the members share one pattern, A dense and H dense in its leading 4 x 4 block, and differ in the values of both"""
    assert len({pattern(q) for q in D}) == 1
    assert int(D[0].A_jc[8]) == 16 and int(D[0].H_jc[8]) == 16 and D[0].H_ir.max() < 4 and int(D[0].H_jc[4]) == 16
    assert any(not np.array_equal(q.A_val, D[0].A_val) for q in D[1:]) and any(not np.array_equal(q.H_val, D[0].H_val) for q in D[1:])
