"""The lane-per-problem kernel's overlap of work with its transfers (csrc/qp_lane.hip, the headline build: H as its leading 4 x 4
block, no state kept). A FULL wave of 16-byte aligned pools is staged in dependency order (stage_matrices, take_bounds, take_g): the
loads go out as A, H, lb, ub, lbA, ubA, g; the tableau of the empty working set is built from A and H while the vectors are still on
their way, the set-up runs from the bounds while g is, and the vectors pass through spare LDS slots behind the tableau instead of
through it. At the other end a wave none of whose lanes refines (no member with more than four pivots) issues the stores of x, y
and the working sets before it forms the exact products and the objective. A ragged wave, the build with H in full
(RSQP_LANE_HBLOCK=0) and patterns of their own stay on the earlier text -- inside the same library, so every member's answer can
be compared bit for bit between the two ways in and out, besides against the oracle. A kept state is staged in dependency order as
well and keeps the earlier order at the end (the state block goes out first).

Batches of 64, 65, 128 and 129 members (full waves; a full wave beside a ragged one, whose single member is a copy of member 5 of the
first wave). The shapes, each for the path it takes:
  hs071            8 x 2, the headline's pattern (12 entries of A, 11 of H): the ordered staging; two pivots: the results go first
  7x2, 5x1         odd nV, even and odd entry counts (a pair of doubles straddles two members; half groups of lanes)
  4x0              no constraints, no A
  outside_block    the headline's pattern with one entry of H outside the block: H in full, the earlier staging
  own_patterns     patterns of their own: every lane walks its own arrays
  free             members that lack a finite bound on some variables: the free-variable pivots of the set-up, between the passes
  inconsistent     one member of a full wave with lb > ub: the exit before any change, taken by one lane while the others set up
  mixed            members with more than four pivots beside members with none in EVERY wave: the vote keeps the earlier order
The `mixed` and `hs071` claims are asserted from the oracle's own counts in a test that needs no GPU. The launch, the comparisons
and the families that other files use as well (hs071, outside_block, own_patterns, free) are tests/lane_cases.py's."""
import numpy as np
import pytest

import lane_cases as LC
from lane_cases import assert_oracle_answer, assert_same_bits, continue_hot, lane_cold, oracle_handles
from restartsqp_amd.qpdump import QPData, dense_to_csc

SIZES = (64, 65, 128, 129)
DISTINCT, TWIN = 128, 5          # the distinct members of a shape; the one whose copy is the ragged wave of an odd-sized batch
BAD = 17                         # `inconsistent`: the member of the first wave with lb > ub


def block_members(nV, nC, seed, n=DISTINCT, quiet=0):
    """one pattern, H in its leading block (min(nV, 4) square, dense), A dense; every vector and matrix value differs by member; all
    bounds finite (the variables beyond the block have no curvature: their bounds keep the QP bounded). quiet: every quiet-th member
    is solved by its starting point (every variable at its lower bound, the gradient there pointing inwards, the constraints wide):
    no change at all beside neighbours that take many"""
    rng = np.random.default_rng(seed)
    h = min(nV, 4)
    M = rng.normal(size=(h, h))
    H0 = np.zeros((nV, nV)); H0[:h, :h] = M @ M.T / h + np.eye(h)
    A0 = rng.normal(size=(nC, nV))
    out = []
    for k in range(n):
        H = H0 * (1.0 + 0.05 * np.abs(rng.normal()))
        A = A0 * (1.0 + 0.05 * rng.normal(size=A0.shape))
        g = 3.0 * rng.normal(size=nV)
        xh = rng.normal(size=nV)
        lb = xh - np.abs(rng.normal(size=nV)); ub = xh + np.abs(rng.normal(size=nV))
        lbA = A @ xh - np.abs(rng.normal(size=nC)); ubA = A @ xh + np.abs(rng.normal(size=nC))
        if quiet and k % quiet == 0:
            g = -H @ lb + 0.5 + np.abs(rng.normal(size=nV))
            lbA = A @ lb - 1.0 - np.abs(rng.normal(size=nC)); ubA = A @ lb + 1.0 + np.abs(rng.normal(size=nC))
        Ac = dense_to_csc(A) if nC else (np.zeros(nV + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        out.append(QPData(nV, nC, *dense_to_csc(H), *Ac, g, lb, ub, lbA, ubA, name="b%dx%d_%d" % (nV, nC, k)))
    return out


def _inconsistent():
    out = list(members("mixed"))
    q = out[BAD]
    lb = q.lb.copy(); lb[2] = q.ub[2] + 1.0
    out[BAD] = QPData(q.nV, q.nC, q.H_jc, q.H_ir, q.H_val, q.A_jc, q.A_ir, q.A_val, q.g, lb, q.ub, q.lbA, q.ubA, name="bad")
    return out


# the families of this file alone
LC.FAMILIES.update({"overlap 7x2": lambda: block_members(7, 2, 9401), "overlap 5x1": lambda: block_members(5, 1, 9402),
                    "overlap 4x0": lambda: block_members(4, 0, 9403), "overlap mixed": lambda: block_members(8, 2, 9404, quiet=3),
                    "overlap inconsistent": _inconsistent})
# name -> (the family of lane_cases whose first DISTINCT members the shape takes, the build that serves them: H as its leading
# block (4) or in full (8))
SHAPES = {
    "hs071": ("hs071", 4),
    "7x2": ("overlap 7x2", 4),
    "5x1": ("overlap 5x1", 4),
    "4x0": ("overlap 4x0", 4),
    "outside_block": ("hs071_outside_block", 8),
    "own_patterns": ("own_patterns", 8),
    "free": ("roles", 4),
    "mixed": ("overlap mixed", 4),
    "inconsistent": ("overlap inconsistent", 4),
}
_cache = {}


def members(name):
    return LC.members(SHAPES[name][0])[:DISTINCT]


def batch(name, size):
    """(the members, the index among the distinct ones of each)"""
    idx = list(range(size)) if size % 2 == 0 else list(range(size - 1)) + [TWIN]
    D = members(name)
    return [D[i] for i in idx], idx


def oracle_of(oracle, name, k):
    return LC.oracle_of(oracle, SHAPES[name][0], k)


def pivots_of(oracle, name, k):
    """what the kernel counts before it decides on the refinement step: the variables without any bound (they enter by pivots of the
    set-up) + the changes of the homotopy"""
    q = members(name)[k]
    free = int(np.sum((q.lb <= -1e20) & (q.ub >= 1e20)))
    return free + oracle_of(oracle, name, k)[2]


def test_the_shapes_take_the_paths_they_are_named_for(oracle):
    """(no GPU) the build each shape is served by; the entry counts; which members have free variables; the one inconsistent member;
    per wave of every batch, whether a lane refines"""
    for name, (_, hb) in SHAPES.items():
        assert len(members(name)) == DISTINCT and LC.expected_block(members(name)) == hb, name
    q = members("hs071")[0]
    assert (q.nV, q.nC, int(q.A_jc[8]), int(q.H_jc[8])) == (8, 2, 12, 11)
    assert [int(members(n)[0].A_jc[-1]) for n in ("7x2", "5x1", "4x0")] == [14, 5, 0]
    assert sum(bool(np.any(np.isinf(q.lb) & np.isinf(q.ub))) for q in members("free")[:64]) >= 8
    bad = [k for k, q in enumerate(members("inconsistent")) if np.any(q.lb > q.ub)]
    assert bad == [BAD]
    qp, rc, n = oracle_of(oracle, "inconsistent", BAD)
    assert rc != 0 and n == 0 and qp.exitflag() != 20
    # the vote: no lane of any wave of the headline's shape refines; in `mixed` and `inconsistent` every full wave holds lanes
    # that do beside lanes that do not
    assert max(pivots_of(oracle, "hs071", k) for k in range(DISTINCT)) <= 4
    assert all(oracle_of(oracle, "mixed", k)[2] == 0 for k in range(0, DISTINCT, 3))
    for name in ("mixed", "inconsistent"):
        for w0 in (0, 64):
            p = [pivots_of(oracle, name, k) for k in range(w0, w0 + 64)]
            assert sum(v > 4 for v in p) >= 8 and sum(v <= 4 for v in p) >= 8, (name, w0, p)
    # (the ragged wave's twin: more than four pivots where the shape has such members, so both orders of the results meet in one batch)
    print({name: pivots_of(oracle, name, TWIN) for name in SHAPES})


@pytest.mark.parametrize("name", ["7x2", "5x1", "4x0", "mixed"])
def test_the_oracle_answers_are_unambiguous(oracle, name):
    """(no GPU) lane_cases.assert_unambiguous on the members generated here: solved; strict complementarity; no ratio test ties -- the
    path does not move with the vectors"""
    LC.assert_family_unambiguous(oracle, SHAPES[name][0])


def results(capi, monkeypatch, name, size):
    """the batch's cold start on the build its shape is served by, solved once"""
    if (name, size) not in _cache:
        b, res = lane_cold(capi, monkeypatch, batch(name, size)[0])
        assert b.lane_hblock() == SHAPES[name][1], (name, b.lane_hblock())
        b.close()
        assert len(res) == size
        _cache[(name, size)] = res
    return _cache[(name, size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_member_gets_the_oracles_answer(capi, oracle, monkeypatch, name, size):
    probs, idx = batch(name, size)
    res = results(capi, monkeypatch, name, size)
    for k, r in zip(idx, res):
        qp, rc, n = oracle_of(oracle, name, k)
        if name == "inconsistent" and k == BAD:
            # (infeasible before any change: no solution to compare)
            assert r["status"] == qp.exitflag() != 20 and r["nWSR"] == n == 0
            continue
        assert_oracle_answer(qp, r, n, (name, k))       # (status 20, nWSR, working sets exact; x, y, objective within 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_ordered_staging_gives_the_bits_of_the_earlier_one(capi, monkeypatch, name, size):
    """the build the shape is served by against RSQP_LANE_HBLOCK=0: H in full, the earlier staging and the earlier order of the
    results, inside one library"""
    probs, idx = batch(name, size)
    res = results(capi, monkeypatch, name, size)
    b, full = lane_cold(capi, monkeypatch, probs, full_H=True)
    assert b.lane_hblock() == 8
    b.close()
    assert len(res) == size
    assert_same_bits(res, full, (name, size))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch, name):
    r65, r129, r128 = results(capi, monkeypatch, name, 65), results(capi, monkeypatch, name, 129), results(capi, monkeypatch, name, 128)
    # (ragged wave, full wave): the twin within each odd batch and across the batches; a member of the second wave across 128 / 129
    for rag, ful in ((r65[64], r65[TWIN]), (r129[128], r129[TWIN]), (r65[64], r128[TWIN]), (r129[100], r128[100])):
        assert_same_bits(rag, ful, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hs071", "mixed"])
def test_a_hot_start_continues_from_the_kept_state(capi, oracle, monkeypatch, name):
    """state kept (staged in dependency order; the state block and the results leave in the earlier order): the cold start, then a hot
    start on new vectors (8-lane kernel, from the block the lane kernel wrote) take the oracle's number of changes exactly, member by
    member; a full wave and a ragged one"""
    probs, idx = batch(name, 65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_hblock() == 4
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), np.random.default_rng(9410))
    b.close()
