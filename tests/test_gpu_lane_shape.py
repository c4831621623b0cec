"""The lane-per-problem kernel's full-shape build (csrc/qp_lane.hip, lane_qp_shape_kernel<2, KEEP, true, 4, 8, 2>): a one-pattern batch of
8 x 2 members whose H stays inside its leading 4 x 4 block runs the text of lane_qp_kernel<2, KEEP, true, 4> with nV = 8 and nC = 2 as
compile-time constants (SmallPlan::lane_shape; RSQP_LANE_SHAPE=0, read per batch: never). The algorithm, the operands, the candidate
ids, the tie rule and the summation orders are the same text, so the requirement is THE SAME BITS as the run-time-shape build of the
same library gives (np.array_equal on x, y, both working sets, status, nWSR and the objective), and the oracle's answers by
test_gpu_parity.assert_same_solution; no tolerance of its own.

Batches of at most 129 members, RSQP_LANE=1. The members that stress the build are lane_cases' family "roles": slots
of one wave in different roles, free variables that pivot in during the set-up, exchanges with both kinds of partner; batches of 65
and 129 (full waves and a ragged wave of one, whose member also sits in a full wave). One more batch of 65 (family "odd") holds a
member with inconsistent bounds, one that ends infeasible and solved members whose pivots exceed 4 (finish(refine = true)); a test
without a GPU asserts from the oracle's counts that it holds each. What does NOT take the build: 7 x 2, 8 x 1, 8 x 0, patterns of
their own, a dense H."""
import numpy as np
import pytest

import small_builds as SB
from abi_cases import assert_entry_points
from conftest import oracle_cold
from lane_cases import (FULL, ODD_INCONSISTENT, ODD_INFEASIBLE, ROLES_SEED, assert_ragged_and_full_bits, assert_same_bits,
                        assert_same_solution, continue_hot, lane_cold, members, oracle_handles, oracle_of, pattern, perturbations, ragged_batch)
from restartsqp_amd import problems

_cache = {}


def batch_of(name):
    """(the members, the family and index in it of each) of a case: 65 / 129 of "roles", the 129 of "hs071", the 65 of "odd\""""
    if name in ("odd", "hs071"):
        return members(name), [(name, k) for k in range(len(members(name)))]
    probs, idx = ragged_batch("roles", name)
    return probs, [("roles", k) for k in idx]


def results(capi, monkeypatch, name, keep, shape):
    """the batch's cold start on the full-shape build (shape) or on the run-time-shape build, solved once; the getter's word checked"""
    key = (name, keep, shape)
    if key not in _cache:
        b, res = lane_cold(capi, monkeypatch, batch_of(name)[0], shape=shape, keep=bool(keep))
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
    probs = members("odd")
    orc = [oracle_of(oracle, "odd", k) for k in range(len(probs))]
    assert len(probs) == 65 and len({pattern(q) for q in probs}) == 1
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
    assert_entry_points(capi, "rsqp_hip_lane.h", capi.LANE_SYMBOLS, ("rsqp_batch_get_lane_shape",))
    assert capi.lib().rsqp_batch_get_lane_shape(None) == 0
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
    assert len(new) == len(batch_of(name)[0])
    assert_same_bits(new, old, (name, keep))


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("name", CASES, ids=str)
def test_the_full_shape_build_gives_the_oracles_answers(capi, oracle, monkeypatch, name, keep):
    res = results(capi, monkeypatch, name, keep, True)
    orc = [oracle_of(oracle, *key) for key in batch_of(name)[1]]
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
    assert_ragged_and_full_bits(results(capi, monkeypatch, 65, keep, True), results(capi, monkeypatch, 129, keep, True), "roles")


# ------------------------------------------------------------------------------------
# what does not take the build
# ------------------------------------------------------------------------------------
def block_batch(seed, nV, nC, n=65):
    """one pattern, H inside its leading 4 x 4 block (small_builds.lane_batch's recipe at another shape)"""
    rng = np.random.default_rng(seed)
    q = problems.random_qp(rng, nV, nC, density=1.0)
    H = np.zeros((nV, nV))
    H[:4, :4] = q.dense_H()[:4, :4]
    return perturbations(rng, SB.with_H(q, H), n, 1.0, 0.3)


def assert_oracle_where_solved(oracle, probs, res):
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)
        assert r["status"] == qp.exitflag()
        if rc == 0:
            assert_same_solution(qp, r, n)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 2), (8, 1), (8, 0)])
def test_other_shapes_stay_on_the_run_time_shape_block_build(capi, oracle, monkeypatch, shape):
    probs = block_batch(7100 + 10 * shape[0] + shape[1], *shape)
    b, res = lane_cold(capi, monkeypatch, probs)
    assert b.lane_shape() == 0 and b.lane_hblock() == 4
    b.close()
    assert_oracle_where_solved(oracle, probs, res)


@pytest.mark.gpu
@pytest.mark.parametrize("uni,hb", [(0, 8), (1, 8)], ids=["patterns of their own", "dense H"])
def test_full_shape_batches_the_block_build_does_not_serve(capi, oracle, monkeypatch, uni, hb):
    probs = SB.lane_batch(7200 + uni, 65, uni, hb)
    assert all(q.nV == 8 and q.nC == 2 for q in probs)
    b, res = lane_cold(capi, monkeypatch, probs)
    assert b.lane_shape() == 0 and b.lane_hblock() == 8
    assert capi.plan_builds(b.last_plan()) == [("lane", 0, uni, hb)]
    b.close()
    assert_oracle_where_solved(oracle, probs, res)


# ------------------------------------------------------------------------------------
# the state the KEEP build writes
# ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_hot_start_continues_from_the_state_the_full_shape_build_kept(capi, oracle, monkeypatch):
    """state kept: the cold start on the full-shape build, then a hot start on new vectors (8-lane kernel, from the block the lane
    kernel wrote) take the oracle's number of changes exactly, member by member"""
    probs, idx = ragged_batch("roles", 65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_shape() == FULL
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), np.random.default_rng(ROLES_SEED + 1))
    b.close()
