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

The members (lane_cases.SHAPES) are chosen (seeds) so that the oracle's answers are unambiguous, which a test without a GPU checks
(lane_cases.assert_unambiguous): strict complementarity at the solution, and no tie in a ratio test -- the oracle breaks ties by the
lowest id, so a tie shows as a path (the working set after every change) that moves when the vectors move by +d or -d, |d| ~ 1e-10:
the difference of two tied step lengths is linear in d to first order and changes sign with it."""
import numpy as np
import pytest

from lane_cases import (SHAPES, assert_family_unambiguous, assert_same_bits, assert_same_solution, continue_hot, expected_block, lane_cold,
                        members, oracle_handles, oracle_of)

ROT = 37
SIZES = (64, 65, 127, 1, 129)


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


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_oracle_answers_are_unambiguous(oracle, name):
    """(no GPU) every member solved; strict complementarity: the multiplier of every active bound / constraint is away from zero,
    every inactive one is away from its limits; no ratio test ties (see the module's text)"""
    assert_family_unambiguous(oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_member_answers_the_same_wherever_it_sits(capi, oracle, monkeypatch, name, size):
    probs = members(name)[:size]
    b, res = lane_cold(capi, monkeypatch, probs)
    hb = b.lane_hblock()
    b.close()
    assert hb == expected_block(probs), (hb, expected_block(probs))
    if size >= 3:                                       # (fewer members than patterns: the members left may share one)
        assert hb == SHAPES[name][1]
    for k, r in enumerate(res):
        qp, rc, n = oracle_of(oracle, name, k)
        assert_same_solution(qp, r, n)
    turned = [probs[(i + ROT) % size] for i in range(size)]
    b, res2 = lane_cold(capi, monkeypatch, turned)
    assert b.lane_hblock() == hb
    b.close()
    for i in range(size):
        assert_same_bits(res[(i + ROT) % size], res2[i], (name, size, i))
        qp, rc, n = oracle_of(oracle, name, (i + ROT) % size)
        assert_same_solution(qp, res2[i], n)


@pytest.mark.gpu
def test_a_hot_start_continues_from_the_state_a_full_and_a_ragged_wave_wrote(capi, oracle, monkeypatch):
    probs = members("8x2_dense_H")[:65]
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), np.random.default_rng(8210))
    b.close()
