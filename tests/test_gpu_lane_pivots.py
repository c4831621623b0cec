"""The lane-per-problem kernel's pivots (csrc/qp_lane.hip: pivot1, pivot2, the copy of pivot1 in the set-up): the headline build
walks the tableau's stored triangle in chunks -- a chunk's LDS reads together, then its FMAs, then its stores -- where the builds
that keep the state or hold H in full go pair by pair. Only the order between independent entries differs, so every result
bit must be the same whichever build answers, and the oracle's.

One shape (8 x 2), one pattern, H in its leading 4 x 4 block (so the batch takes `HB = 4`); the members (lane_cases' family "pivots")
differ in every vector and in the matrix values, and neighbouring lanes of a wave pivot on different rows at once. Variable 0 has no
bounds (variable 2 of every other member neither): they enter by pivots during the set-up; the variables 4 .. 7 have no curvature,
so a bound of theirs that leaves with no free curvature around flips to its other side. The oracle's own paths (the working set
after each change) say which changes ran: a test without a GPU counts them per batch, and checks that the answers are unambiguous
(strict complementarity, no tie in a ratio test: lane_cases.assert_unambiguous). Batches of 65 and 129: full waves and a ragged
wave of one, whose member also sits in a full wave."""
from collections import Counter

import numpy as np
import pytest

from lane_cases import (RAGGED, assert_family_unambiguous, assert_one_block_pattern, assert_oracle_answer, assert_ragged_and_full_bits,
                        assert_same_bits, continue_hot, lane_cold, members, oracle_handles, oracle_of, ragged_batch, working_sets, PIVOTS_SEED)

SIZES = sorted(RAGGED["pivots"])
CHANGES = ("set-up pivot", "bound leaves", "constraint enters", "variable fixed", "constraint leaves", "exchange, constraint as partner",
           "exchange, bound as partner", "flip")
_cache = {}


def changes_of(oracle, k):
    """what the oracle did on distinct member k: a Counter over CHANGES, from the working set after each of its changes"""
    if ("changes", k) not in _cache:
        qp, rc, n = oracle_of(oracle, "pivots", k)
        ws = working_sets(oracle, members("pivots")[k], n)
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
    assert_one_block_pattern(members("pivots"))


@pytest.mark.parametrize("size", SIZES)
def test_the_oracle_runs_every_kind_of_change(oracle, size):
    """(no GPU) per batch: each kind of change at least once among its members -- and in the member of the ragged wave an exchange --,
    and in every full wave lanes that differ in what they do at a given change (the kinds are mixed inside the waves)"""
    probs, idx = ragged_batch("pivots", size)
    total = Counter()
    for k in idx:
        total.update(changes_of(oracle, k))
    print(size, dict(total))
    for c in CHANGES:
        assert total[c] >= 1, (size, c, dict(total))
    rag = changes_of(oracle, RAGGED["pivots"][size])
    assert rag["exchange, constraint as partner"] + rag["exchange, bound as partner"] >= 1, dict(rag)
    for w0 in range(0, size - 1, 64):
        assert len({tuple(sorted(changes_of(oracle, k).items())) for k in idx[w0:w0 + 64]}) >= 16


def test_the_oracle_answers_are_unambiguous(oracle):
    """(no GPU) lane_cases.assert_unambiguous on every distinct member: solved; the multiplier of every active bound / constraint
    away from zero and every inactive one away from its limits; no ratio test ties -- the path does not move with the vectors"""
    assert_family_unambiguous(oracle, "pivots")


def block_results(capi, monkeypatch, size):
    """the batch's cold start on the HB = 4 build, solved once"""
    if ("results", size) not in _cache:
        b, res = lane_cold(capi, monkeypatch, ragged_batch("pivots", size)[0])
        assert b.lane_hblock() == 4
        b.close()
        _cache[("results", size)] = res
    return _cache[("results", size)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_chunked_pivots_give_the_oracles_answers_and_the_full_builds_bits(capi, oracle, monkeypatch, size):
    probs, idx = ragged_batch("pivots", size)
    res = block_results(capi, monkeypatch, size)
    assert len(res) == size
    for k, r in zip(idx, res):
        qp, rc, n = oracle_of(oracle, "pivots", k)
        assert_oracle_answer(qp, r, n, k)                # (status 20, nWSR, working sets exact; x, y, objective within 1e-9)
    # H as its block (chunked pivots) against H in full (pair by pair): the same bits
    b, full = lane_cold(capi, monkeypatch, probs, full_H=True)
    assert b.lane_hblock() == 8
    b.close()
    assert_same_bits(res, full, size)


@pytest.mark.gpu
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch):
    assert_ragged_and_full_bits(block_results(capi, monkeypatch, 65), block_results(capi, monkeypatch, 129), "pivots")


@pytest.mark.gpu
def test_hot_starts_continue_from_the_tableau_the_pivots_left(capi, oracle, monkeypatch):
    """state kept: hot starts on new vectors, then on new matrices, then on new vectors again (8-lane kernel, from the block the
    lane kernel wrote) take the oracle's number of changes exactly, member by member. (The build that keeps the state goes pair by
    pair through its pivots: this is the tableau THOSE left, through every kind of change of the members above.)"""
    probs, idx = ragged_batch("pivots", 65)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_hblock() == 4
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), np.random.default_rng(PIVOTS_SEED + 1), ("vectors", "matrices", "vectors"))
    b.close()
