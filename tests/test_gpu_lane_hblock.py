"""The two builds of the lane-per-problem kernel (csrc/qp_lane.hip): H kept as its leading 4 x 4 block, or as the full triangle.

A batch of one sparsity pattern whose H has no entry outside the leading 4 x 4 block -- the QPhandler formulation [x u v], whose slack
variables have no curvature -- runs the block build (rsqp_batch_get_lane_hblock() == 4); every other batch, and every batch under
RSQP_LANE_HBLOCK=0, runs the full build (8). The block build leaves out only products with structural zeros, so the two give the same
BITS: np.array_equal on every result. Beside that the bar of test_gpu_lane.py: status, working sets and nWSR exact against the oracle
and the 8-lane kernel (RSQP_LANE=0), x / y within 1e-9 relative. Batches of 130-200 members: two full waves and a ragged one. The
launch and the comparisons are tests/lane_cases.py's."""
import numpy as np
import pytest

from conftest import oracle_cold
from lane_cases import (assert_eight_lane_agreement, assert_same_bits, assert_same_solution, continue_hot, hs071_path_batch, lane_cold,
                        oracle_handles, perturbations, with_H)
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc

pytestmark = pytest.mark.gpu


def cold_closed(capi, monkeypatch, probs, want, **how):
    """lane_cold on the build `want` (0: the 8-lane kernel), the batch closed -> results"""
    b, res = lane_cold(capi, monkeypatch, probs, **how)
    hb = b.lane_hblock()
    b.close()
    assert hb == want, (hb, want)
    return res


def assert_oracle_and_eight_lane(oracle, probs, res, tiny, need_solved=True):
    solved = 0
    for q, r, t in zip(probs, res, tiny):
        qp, rc, n = oracle_cold(oracle, q)
        assert r["status"] == qp.exitflag() == t["status"]
        if rc == 0:
            solved += 1
            assert_same_solution(qp, r, n)
            assert_eight_lane_agreement(r, t)
    assert not need_solved or solved == len(probs)
    return solved


def check_build(capi, oracle, monkeypatch, probs, want, keep=False):
    """the batch on the lane kernel (build `want`), against the oracle, the 8-lane kernel and -- block build -- the full build's bits"""
    res = cold_closed(capi, monkeypatch, probs, want, keep=keep)
    tiny = cold_closed(capi, monkeypatch, probs, 0, keep=keep, lane="0")
    assert_oracle_and_eight_lane(oracle, probs, res, tiny)
    if want == 4:
        assert_same_bits(res, cold_closed(capi, monkeypatch, probs, 8, keep=keep, full_H=True))
    return res


def block_batch(rng, nV, nC, n, free=False, rel=0.05):
    """perturbations of one QP whose H is dense on its first min(nV, 4) variables and zero beyond (every variable boxed, so the
    variables without curvature stay on bounds or constraints); free: variable 1 has no bound at all and enters S in the set-up"""
    base = problems.random_qp(rng, nV, nC, density=0.8)
    k = min(nV, 4)
    H = np.zeros((nV, nV))
    H[:k, :k] = base.dense_H()[:k, :k]
    base = with_H(base, H)
    if free:
        base.lb[1] = -np.inf; base.ub[1] = np.inf
    return perturbations(rng, base, n, rel)


@pytest.mark.parametrize("keep", [False, True])
def test_hs071_batch_runs_the_block_build(capi, oracle, monkeypatch, keep):
    probs = problems.hs071_scale_batch(150)
    assert max(int(q.H_ir.max()) for q in probs) < 4 and all(q.H_jc[4] == q.H_jc[8] for q in probs)
    res = check_build(capi, oracle, monkeypatch, probs, 4, keep=keep)
    assert all(r["nWSR"] == 2 for r in res)


@pytest.mark.parametrize("extra", [[(4, 4)], [(0, 7), (7, 0)]])
def test_an_entry_outside_the_block_takes_the_full_build(capi, oracle, monkeypatch, extra):
    """the hs071 batch with one more entry of H: curvature of a slack variable, or a coupling of x_0 with the last slack (and its
    mirror). The pattern decides, for the whole batch, at create"""
    probs = []
    for q in problems.hs071_scale_batch(150):
        H = q.dense_H()
        for (i, k) in extra:
            H[i, k] = 0.5 if i == k else 0.125
        probs.append(with_H(q, H))
    check_build(capi, oracle, monkeypatch, probs, 8)


@pytest.mark.parametrize("shape,free", [((3, 1), False), ((5, 2), True)])
def test_small_shapes_with_a_dense_leading_block(capi, oracle, monkeypatch, shape, free):
    nV, nC = shape
    rng = np.random.default_rng(5000 + 10 * nV + nC)
    check_build(capi, oracle, monkeypatch, block_batch(rng, nV, nC, 170, free=free), 4)


def test_patterns_of_their_own_take_the_full_build(capi, oracle, monkeypatch):
    """one shape, two sparsity patterns of A interleaved -- both with H inside the leading block: still the full build, the block
    build is the one-pattern launch's"""
    rng = np.random.default_rng(5100)
    a, b = block_batch(rng, 6, 2, 1)[0], block_batch(rng, 6, 2, 1)[0]
    A = b.dense_A(); A[0, 2] = 0.0; A[1, 4] = 0.0
    b.A_jc, b.A_ir, b.A_val = dense_to_csc(A)
    probs = [problems.perturb(rng, (a, b)[k % 2], 0.05) for k in range(160)]
    assert len({len(q.A_val) for q in probs}) == 2
    check_build(capi, oracle, monkeypatch, probs, 8)


def test_a_batch_without_H(capi, oracle, monkeypatch):
    """haveH = 0: nothing of H travels, the block holds zeros. The oracle gets the empty matrix. Members may end unsolved (no
    curvature anywhere); the kernels agree with the oracle on that too"""
    rng = np.random.default_rng(5200)
    probs = block_batch(rng, 6, 2, 140)
    zero = np.zeros(6 + 1, np.int32)
    for q in probs:
        q.H_jc = q.H_ir = q.H_val = None
    res = cold_closed(capi, monkeypatch, probs, 4)
    assert_same_bits(res, cold_closed(capi, monkeypatch, probs, 8, full_H=True))
    tiny = cold_closed(capi, monkeypatch, probs, 0, lane="0")
    oq = [QPData(q.nV, q.nC, zero, np.zeros(0, np.int32), np.zeros(0), q.A_jc, q.A_ir, q.A_val, q.g, q.lb, q.ub, q.lbA, q.ubA) for q in probs]
    assert assert_oracle_and_eight_lane(oracle, oq, res, tiny, need_solved=False) > 0


@pytest.mark.parametrize("shape", [(8, 2), (5, 2)])
def test_hot_starts_continue_from_the_state_the_block_build_wrote(capi, oracle, monkeypatch, shape):
    """the sequence of test_gpu_lane.py's hot-start test on a batch that runs the block build: the state block it writes is the full
    tableau in the 8-lane kernel's layout, and the hot starts (new vectors, new matrices, new vectors) continue from it there"""
    nV, nC = shape
    rng = np.random.default_rng(5300 + 10 * nV + nC)
    probs = block_batch(rng, nV, nC, 150)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_hblock() == 4
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), rng, ("vectors", "matrices", "vectors"))
    b.close()


def test_an_odd_member_count_and_an_odd_width(capi, oracle, monkeypatch):
    """5 x 2, 131 members: every pool's run of a wave has an odd length somewhere, and the last wave holds three members"""
    rng = np.random.default_rng(5400)
    for keep in (False, True):
        check_build(capi, oracle, monkeypatch, block_batch(rng, 5, 2, 131), 4, keep=keep)


def test_members_that_take_different_paths_on_the_block_build(capi, oracle, monkeypatch):
    """the iterates of the hs071 SQP trajectory that share one pattern, perturbed and interleaved (lane_cases.hs071_path_batch):
    neighbouring lanes take different paths of 5 changes each, exchanges among them"""
    res = check_build(capi, oracle, monkeypatch, hs071_path_batch(192), 4)
    assert len({(r["nWSR"], tuple(r["ws_b"]), tuple(r["ws_c"])) for r in res}) >= 2


def test_optimize_lp_stays_off_the_lane_kernel(capi, monkeypatch):
    """rsqp_batch_optimize_lp regularises H (hreg != 0), which the block build must never see: the LP launches of a one-shape batch
    give the same answers with RSQP_LANE=1 as with RSQP_LANE=0, and none of them is the lane kernel's"""
    rng = np.random.default_rng(5500)
    probs = block_batch(rng, 6, 2, 130)
    out = {}
    for lane in ("0", "1"):
        monkeypatch.setenv("RSQP_LANE", lane)
        b = capi.Batch(probs)
        used = b.optimize_lp()
        assert b.last_kernel() != 2 and b.lane_hblock() == 0
        out[lane] = (b.results(), used)
        b.close()
    assert_same_bits(out["0"][0], out["1"][0])
    assert np.array_equal(out["0"][1], out["1"][1])
    assert any(r["status"] == 20 for r in out["1"][0])
