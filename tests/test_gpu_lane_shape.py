"""The lane-per-problem kernel's full-shape build (csrc/qp_lane.hip, lane_qp_shape_kernel<2, KEEP, true, 4, 8, 2>): a one-pattern batch of
8 x 2 members whose H stays inside its leading 4 x 4 block runs the text of lane_qp_kernel<2, KEEP, true, 4> with nV = 8 and nC = 2 as
compile-time constants (SmallPlan::lane_shape; RSQP_LANE_SHAPE=0, read per batch: never). The algorithm, the operands, the candidate
ids, the tie rule and the summation orders are the same text, so the requirement is THE SAME BITS as the run-time-shape build of the
same library gives (np.array_equal on x, y, both working sets, status, nWSR and the objective), and the oracle's answers by
test_gpu_parity.assert_same_solution; no tolerance of its own.

Batches of at most 129 members, RSQP_LANE=1. The members that stress the build are test_gpu_lane_roles.distinct_members(): slots
of one wave in different roles, free variables that pivot in during the set-up, exchanges with both kinds of partner; batches of 65
and 129 (full waves and a ragged wave of one, whose member also sits in a full wave). One more batch of 65 holds a member with
inconsistent bounds, one that ends infeasible and solved members whose pivots exceed 4 (finish(refine = true)); a test without a GPU
asserts from the oracle's counts that it holds each. What does NOT take the build: 7 x 2, 8 x 1, 8 x 0, patterns of their own, a
dense H."""
import numpy as np
import pytest

import small_builds as SB
import test_gpu_lane_roles as LR
from conftest import oracle_cold
from restartsqp_amd import problems
from test_gpu_lane_io import FIELDS
from test_gpu_parity import assert_same_solution

FULL = 8 * 256 + 2
ODD_INCONSISTENT, ODD_INFEASIBLE = 5, 9              # members of the odd batch (below)
_cache = {}


def lane_cold(capi, monkeypatch, probs, shape=True, keep=False):
    """one cold start of a fresh batch on the lane kernel -> (batch, results); shape = False: RSQP_LANE_SHAPE=0"""
    monkeypatch.setenv("RSQP_LANE", "1")
    monkeypatch.delenv("RSQP_LANE_HBLOCK", raising=False)
    if shape:
        monkeypatch.delenv("RSQP_LANE_SHAPE", raising=False)
    else:
        monkeypatch.setenv("RSQP_LANE_SHAPE", "0")
    b = capi.Batch(probs)
    b.set_keep_state(keep)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 2
    return b, b.results()


def odd_batch():
    """65 of the distinct members; one gets inconsistent bounds, one constraints far from its box (test_gpu_lane.py's recipes)"""
    if "odd" not in _cache:
        D = LR.distinct_members()
        probs = []
        for k in range(65):
            q = D[k]
            lb, ub, lbA, ubA = q.lb.copy(), q.ub.copy(), q.lbA.copy(), q.ubA.copy()
            if k == ODD_INCONSISTENT:
                lb[2] = 1.0; ub[2] = 0.0
            if k == ODD_INFEASIBLE:              # (every variable in a box, the constraints far from what the box allows)
                ub = np.where(np.isinf(ub), np.where(np.isinf(lb), 1.0, lb + 2.0), ub)
                lb = np.where(np.isinf(lb), ub - 2.0, lb)
                lbA = q.ubA + 500.0; ubA = lbA + 1.0
            probs.append(type(q)(8, 2, q.H_jc, q.H_ir, q.H_val, q.A_jc, q.A_ir, q.A_val, q.g, lb, ub, lbA, ubA, name=q.name))
        _cache["odd"] = probs
    return _cache["odd"]


def odd_oracle(oracle):
    if "odd oracle" not in _cache:
        _cache["odd oracle"] = [oracle_cold(oracle, q) for q in odd_batch()]
    return _cache["odd oracle"]


def batch_of(name):
    if name == "odd":
        return odd_batch()
    if name == "hs071":
        if name not in _cache:
            _cache[name] = problems.hs071_scale_batch(129)
        return _cache[name]
    return LR.batch(name)[0]


def oracle_answers(oracle, name):
    if name == "odd":
        return odd_oracle(oracle)
    if name == "hs071":
        if "hs071 oracle" not in _cache:
            _cache["hs071 oracle"] = [oracle_cold(oracle, q) for q in batch_of(name)]
        return _cache["hs071 oracle"]
    return [LR.oracle_of(oracle, k) for k in LR.batch(name)[1]]


def results(capi, monkeypatch, name, keep, shape):
    """the batch's cold start on the full-shape build (shape) or on the run-time-shape build, solved once; the getter's word checked"""
    key = ("results", name, keep, shape)
    if key not in _cache:
        b, res = lane_cold(capi, monkeypatch, batch_of(name), shape=shape, keep=bool(keep))
        assert b.lane_hblock() == 4 and b.lane_shape() == (FULL if shape else 0)
        assert capi.plan_builds(b.last_plan()) == [("lane", keep, 1, 4)]          # (the build family keeps its name)
        b.close()
        _cache[key] = res
    return _cache[key]


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_the_odd_batch_holds_each_of_its_three_kinds(oracle):
    """(no GPU) from the oracle: the member with lb > ub is infeasible before any change, the member with its constraints far from
    the box ends infeasible after some, and solved members make more than 4 pivots (free variables of the set-up + changes)"""
    probs, orc = odd_batch(), odd_oracle(oracle)
    key = lambda q: (tuple(q.A_jc), tuple(q.A_ir), tuple(q.H_jc), tuple(q.H_ir))
    assert len(probs) == 65 and len({key(q) for q in probs}) == 1
    qp, rc, n = orc[ODD_INCONSISTENT]
    assert rc != 0 and qp.exitflag() != 20 and n == 0
    qp, rc, n = orc[ODD_INFEASIBLE]
    assert rc != 0 and qp.exitflag() != 20 and n > 0
    refined = 0
    for k, (q, (qp, rc, n)) in enumerate(zip(probs, orc)):
        if k in (ODD_INCONSISTENT, ODD_INFEASIBLE):
            continue
        assert rc == 0 and qp.exitflag() == 20, k
        free = int(np.sum(np.isinf(q.lb) & np.isinf(q.ub)))
        refined += free + n > 4
    print("solved members with more than 4 pivots", refined)
    assert refined >= 8


def test_the_getter_is_declared_exported_and_bound_and_the_plan_words_stay(capi):
    """(no GPU) rsqp_batch_get_lane_shape: declared in include/rsqp_hip_lane.h, which rsqp_hip.h includes, bound in capi.LANE_SYMBOLS;
    the shape word stays out of rsqp_describe_small_launch's words: ("lane", keep, uni, hb) names the build family"""
    import os, re
    from conftest import ROOT
    main = open(os.path.join(ROOT, "include", "rsqp_hip.h")).read()
    assert re.search(r'^#include "rsqp_hip_lane.h"', main, flags=re.M)
    header = open(os.path.join(ROOT, "include", "rsqp_hip_lane.h")).read()
    declared = set(re.findall(r"^\s*int\s+(rsqp_\w+)\s*\(", header, flags=re.M))
    assert declared == set(capi.LANE_SYMBOLS) == {"rsqp_batch_get_lane_shape"} and not declared & set(capi.SYMBOLS)
    assert hasattr(capi.lib(), "rsqp_batch_get_lane_shape") and capi.lib().rsqp_batch_get_lane_shape(None) == 0
    assert "lane_shape" not in capi.SMALL_LAUNCH_OUT and len(capi.SMALL_LAUNCH_OUT) == 20


# ------------------------------------------------------------------------------------
# the same bits, and the oracle's answers
# ------------------------------------------------------------------------------------
CASES = [65, 129, "hs071", "odd"]


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_the_full_shape_build_gives_the_bits_of_the_run_time_shape(capi, monkeypatch, name, keep):
    new, old = results(capi, monkeypatch, name, keep, True), results(capi, monkeypatch, name, keep, False)
    assert len(new) == len(old) == len(batch_of(name))
    for i, (a, c) in enumerate(zip(new, old)):
        for f in FIELDS:
            assert np.array_equal(np.asarray(a[f]), np.asarray(c[f])), (name, keep, i, f, a[f], c[f])


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_the_full_shape_build_gives_the_oracles_answers(capi, oracle, monkeypatch, name, keep):
    res = results(capi, monkeypatch, name, keep, True)
    orc = oracle_answers(oracle, name)
    assert len(res) == len(orc)
    solved = 0
    for r, (qp, rc, n) in zip(res, orc):
        assert r["status"] == qp.exitflag()
        if rc == 0:
            assert_same_solution(qp, r, n)              # (status, nWSR, working sets exact; x, y within 1e-9)
            solved += 1
    assert solved == len(res) - (2 if name == "odd" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 1])
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch, keep):
    small, large = results(capi, monkeypatch, 65, keep, True), results(capi, monkeypatch, 129, keep, True)
    a, c = LR.RAGGED[129], LR.RAGGED[65]
    # (ragged wave, full wave): member a within the larger batch and across the two, member c across the two
    for rag, ful in ((large[128], large[a]), (large[128], small[a]), (small[64], large[c])):
        for f in FIELDS:
            assert np.array_equal(np.asarray(rag[f]), np.asarray(ful[f])), (f, rag[f], ful[f])


# ------------------------------------------------------------------------------------
# what does not take the build
# ------------------------------------------------------------------------------------
def block_batch(seed, nV, nC, n=65):
    """one pattern, H inside its leading 4 x 4 block (small_builds.lane_batch's recipe at another shape)"""
    rng = np.random.default_rng(seed)
    q = problems.random_qp(rng, nV, nC, density=1.0)
    H = np.zeros((nV, nV))
    H[:4, :4] = q.dense_H()[:4, :4]
    base = SB.with_H(q, H)
    out = []
    for _ in range(n):
        p = problems.perturb(rng, base, 1.0)
        p.A_val = p.A_val * (1.0 + 0.3 * rng.normal(size=p.A_val.shape))
        out.append(p)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 2), (8, 1), (8, 0)])
def test_other_shapes_stay_on_the_run_time_shape_block_build(capi, oracle, monkeypatch, shape):
    probs = block_batch(7100 + 10 * shape[0] + shape[1], *shape)
    b, res = lane_cold(capi, monkeypatch, probs)
    assert b.lane_shape() == 0 and b.lane_hblock() == 4
    b.close()
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)
        assert r["status"] == qp.exitflag()
        if rc == 0:
            assert_same_solution(qp, r, n)


@pytest.mark.gpu
@pytest.mark.parametrize("uni,hb", [(0, 8), (1, 8)], ids=["patterns of their own", "dense H"])
def test_full_shape_batches_the_block_build_does_not_serve(capi, oracle, monkeypatch, uni, hb):
    probs = SB.lane_batch(7200 + uni, 65, uni, hb)
    assert all(q.nV == 8 and q.nC == 2 for q in probs)
    b, res = lane_cold(capi, monkeypatch, probs)
    assert b.lane_shape() == 0 and b.lane_hblock() == 8
    assert capi.plan_builds(b.last_plan()) == [("lane", 0, uni, hb)]
    b.close()
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)
        assert r["status"] == qp.exitflag()
        if rc == 0:
            assert_same_solution(qp, r, n)


# ------------------------------------------------------------------------------------
# the state the KEEP build writes
# ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_hot_start_continues_from_the_state_the_full_shape_build_kept(capi, oracle, monkeypatch):
    """state kept: the cold start on the full-shape build, then a hot start on new vectors (8-lane kernel, from the block the lane
    kernel wrote) take the oracle's number of changes exactly, member by member"""
    probs, idx = LR.batch(65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_shape() == FULL
    orcs = []
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)              # (a handle of its own: the hot start moves it)
        assert_same_solution(qp, r, n)
        orcs.append(qp)
    rng = np.random.default_rng(LR.SEED + 1)
    nxt = [problems.perturb(rng, q, 0.3) for q in probs]
    b.set_vectors_from(nxt)
    b.solve(capi.MODE_HOT_VECTORS, 1000)
    assert b.last_kernel() == 1 and b.lane_shape() == 0
    changes = 0
    for q, qp, r in zip(nxt, orcs, b.results()):
        rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
        assert r["nWSR"] == n
        assert_same_solution(qp, r, n)
        changes += n
    assert changes > 0
    b.close()
