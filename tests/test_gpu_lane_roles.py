"""The lane-per-problem kernel's ratio test (csrc/qp_lane.hip, homotopy()): the headline build -- H as its leading 4 x 4 block, no state
kept -- branches on the ROLE of a variable slot (free: two bound candidates; fixed: one multiplier candidate) where the other builds
compute both roles and select, and leaves out the re-relaxation of the limits that a cold start cannot need. Per lane the operands,
the candidate ids and the tie rule are the same, so every result bit must be the same whichever build answers, and the oracle's.

What can go wrong shows only when the lanes of ONE wave disagree on the role of the SAME slot in the same pass: then both arms run,
each under its own mask. One shape (8 x 2), one pattern, H in its leading 4 x 4 block (the batch takes `HB = 4`); the members
(lane_cases' family "roles") differ in every vector, in the matrix values and in WHICH bounds they have: a slot starts free (no
bound: it pivots in during the set-up), at its lower bound, or at its upper bound (no lower one) depending on the member, and the
paths spread from there -- bounds leave (free variables with both bounds finite), constraints enter and leave, exchanges with a
bound and with a constraint as partner. A test without a GPU reads the oracle's own paths (the working set after each change) and
asserts, for every slot, a wave whose lanes hold it in two roles at the same change count -- for the variable slots free beside
at-lower and free beside at-upper --, and that no member's answer is ambiguous (strict complementarity, no tie in a ratio test:
lane_cases.assert_unambiguous). Batches of 65 and 129: full waves and a ragged wave of one, whose member also sits in a full wave."""
import numpy as np
import pytest

from lane_cases import (RAGGED, assert_eight_lane_agreement, assert_family_unambiguous, assert_one_block_pattern, assert_oracle_answer,
                        assert_ragged_and_full_bits, assert_same_bits, continue_hot, lane_cold, members, oracle_handles, oracle_of,
                        ragged_batch, working_sets, ROLES_SEED)

SIZES = sorted(RAGGED["roles"])
_cache = {}


def path_of(oracle, k):
    """the oracle's working sets of distinct member k, [bounds (8); constraints (2)] after 0 .. nWSR changes"""
    if ("path", k) not in _cache:
        _cache[("path", k)] = working_sets(oracle, members("roles")[k], oracle_of(oracle, "roles", k)[2])
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
    assert_one_block_pattern(members("roles"))


@pytest.mark.parametrize("size", SIZES)
def test_lanes_of_one_wave_hold_every_slot_in_different_roles_at_once(oracle, size):
    """(no GPU) from the oracle's paths, per batch: for EVERY slot a full wave in which, after the same number of changes (the pass of
    the kernel's loop that the lanes run together), two members that are both still running hold the slot in different roles -- a
    variable free in one lane beside at its lower bound in another, and free beside at its upper bound; a constraint active beside
    inactive. Members with a free variable between two finite bounds, members with a variable without bounds, and exchanges with
    a bound and with a constraint as partner, the ragged wave's member among them"""
    probs, idx = ragged_batch("roles", size)
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
        q = members("roles")[k]
        fin = np.isfinite(q.lb) & np.isfinite(q.ub)
        two_bounds += any(np.any((p[:8] == 0) & fin) for p in path_of(oracle, k))
        unbounded += bool(np.any(np.isinf(q.lb) & np.isinf(q.ub)))
        c, b = exchanges_of(oracle, k)
        con += c > 0; bnd += b > 0
    print(size, "members with a free variable between finite bounds", two_bounds, "without bounds", unbounded, "exchange with a constraint",
          con, "with a bound", bnd)
    assert two_bounds >= 8 and unbounded >= 8 and con >= 1 and bnd >= 1
    assert sum(exchanges_of(oracle, RAGGED["roles"][size])) >= 1


def test_the_oracle_answers_are_unambiguous(oracle):
    """(no GPU) lane_cases.assert_unambiguous on every distinct member: solved; the multiplier of every active bound / constraint
    away from zero and every inactive one away from its limits; no ratio test ties -- the path does not move with the vectors"""
    assert_family_unambiguous(oracle, "roles")


def block_results(capi, monkeypatch, size):
    """the batch's cold start on the HB = 4 build without its state (the build with the arms), solved once"""
    if ("results", size) not in _cache:
        b, res = lane_cold(capi, monkeypatch, ragged_batch("roles", size)[0])
        assert b.lane_hblock() == 4                     # (rsqp_batch_get_lane_hblock: the build that answered)
        b.close()
        _cache[("results", size)] = res
    return _cache[("results", size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_arms_give_the_oracles_answers(capi, oracle, monkeypatch, size):
    probs, idx = ragged_batch("roles", size)
    res = block_results(capi, monkeypatch, size)
    assert len(res) == size
    for k, r in zip(idx, res):
        qp, rc, n = oracle_of(oracle, "roles", k)
        assert_oracle_answer(qp, r, n, k)                # (status 20, nWSR, working sets exact; x, y, objective within 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_arms_give_the_bits_of_the_selects(capi, monkeypatch, size):
    """H as its block (arms per role) against RSQP_LANE_HBLOCK=0 (H in full: both roles computed, then selected) inside one library"""
    probs, idx = ragged_batch("roles", size)
    res = block_results(capi, monkeypatch, size)
    b, full = lane_cold(capi, monkeypatch, probs, full_H=True)
    assert b.lane_hblock() == 8
    b.close()
    assert len(res) == size
    assert_same_bits(res, full, size)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_arms_agree_with_the_eight_lane_kernel(capi, monkeypatch, size):
    """against RSQP_LANE=0 as test_gpu_lane.py compares the two kernels: status, nWSR and working sets exact, x and y within 1e-9"""
    probs, idx = ragged_batch("roles", size)
    res = block_results(capi, monkeypatch, size)
    b, tiny = lane_cold(capi, monkeypatch, probs, lane="0")
    b.close()
    assert len(tiny) == len(res)
    for i, (r, t) in enumerate(zip(res, tiny)):
        assert_eight_lane_agreement(r, t, i)


@pytest.mark.gpu
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch):
    assert_ragged_and_full_bits(block_results(capi, monkeypatch, 65), block_results(capi, monkeypatch, 129), "roles")


@pytest.mark.gpu
def test_a_hot_start_continues_from_the_state_the_unchanged_build_kept(capi, oracle, monkeypatch):
    """state kept (the build that keeps the selects): the cold start, then a hot start on new vectors (8-lane kernel, from the block
    the lane kernel wrote) take the oracle's number of changes exactly, member by member"""
    probs, idx = ragged_batch("roles", 65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_hblock() == 4
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), np.random.default_rng(ROLES_SEED + 1))
    b.close()
