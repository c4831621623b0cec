"""The lane-per-problem kernel's stores of results and kept state (csrc/qp_lane.hip: WaveRun, put_pairs / put_quads,
state_put_tableau / state_put_tail_half): a FULL wave whose pools are 16-byte aligned stores write-through by a buffer descriptor of
its own run of each pool, a ragged last wave (put_block, the masked state stores) keeps plain stores on flat addresses. A store
through a descriptor that is out of its range is dropped without a fault, and a line stored write-through is not in the L2 for the
kernel that reads it next -- so nothing here samples: every member of every batch is compared.

* batches of 64, 65, 128 and 129 members: one and two full waves on the write-through path; in the batches of 65 and 129 the ragged
  wave holds a copy of a member of a full wave, and the two answer the same bits (np.array_equal over lane_cases.FIELDS) -- the plain
  path is the reference for the write-through one inside one launch;
* shapes with both parities of every count the pair and quad walks see: 8 x 2 on the headline's pattern (hs071) and on the dense
  block pattern (roles: lane_cases.ragged_batch / assert_ragged_and_full_bits), 7 x 2 (odd nV and odd nV + nC), 5 x 1, 4 x 0 (no
  store of ws_c), patterns of their own, H in full (8 x 2 with a dense H; the headline's pattern with RSQP_LANE_HBLOCK=0);
* every member against the oracle (lane_cases.assert_oracle_answer);
* place independence: the same members rotated by 37 places give the same bits, member by member;
* the full-shape build against RSQP_LANE_SHAPE=0, bit for bit;
* kept state: a hot start on new vectors and one with new matrices continue, on the 8-lane kernel, from the state these stores wrote
  (lane_cases.continue_hot: every member on the oracle's path) -- the read of the dropped lines by another kernel.

No helper of the suite makes a batch whose pools are not 16-byte aligned (a batch allocates its pools itself): that arm of the
kernel's test keeps the plain stores it had and has no case here.

Which build answers: the full-shape build (hs071, roles), the one-pattern builds with H as its leading block (7 x 2 -- its H has
that block alone --, 4 x 0) and with H in full (5 x 1, 8 x 2 with a dense H, RSQP_LANE_HBLOCK=0), the builds for patterns of their
own; each of them without and with the state kept.

The new families' seeds were chosen on the oracle so that every answer is unambiguous; the test without a GPU asserts it."""
import numpy as np
import pytest

from lane_cases import (FAMILIES, FULL, assert_family_unambiguous, assert_oracle_answer, assert_ragged_and_full_bits, assert_same_bits,
                        continue_hot, lane_cold, members, oracle_handles, oracle_of, perturbations, ragged_batch)
from restartsqp_amd import problems
from small_builds import with_H

ROT = 37
SIZES = (64, 65, 128, 129)
COPY = {65: 5, 129: 70}                               # batch size -> the member of a full wave that the ragged wave repeats


def _random(nV, nC, seed, block=False):
    """128 members of one pattern; block: H keeps its leading 4 x 4 block alone, so the build with H as that block serves them"""
    rng = np.random.default_rng(seed)
    base = problems.random_qp(rng, nV, nC, density=0.7)
    if block:
        H = base.dense_H()
        H[4:, :] = 0.0; H[:, 4:] = 0.0
        base = with_H(base, H)
    return perturbations(rng, base, 128)


FAMILIES.update(store_7x2=lambda: _random(7, 2, 8301, block=True), store_5x1=lambda: _random(5, 1, 8302), store_4x0=lambda: _random(4, 0, 8303))
# family -> (H's block of the build that serves it, the full-shape build serves it)
COLD = {"hs071": (4, True), "roles": (4, True), "store_7x2": (4, False), "store_5x1": (8, False), "store_4x0": (4, False),
        "own_patterns": (8, False), "8x2_dense_H": (8, False)}
KEPT = ("roles", "store_7x2", "store_5x1", "store_4x0", "own_patterns", "8x2_dense_H")


def batch_of(name, size):
    """(the members, the index in the family of each): distinct members in the full waves; a ragged wave holds a copy of COPY[size]"""
    idx = list(range(size)) if size % 64 == 0 else list(range(size - 1)) + [COPY[size]]
    D = members(name)
    return [D[i] for i in idx], idx


def assert_oracle_answers(oracle, name, idx, res):
    assert len(res) == len(idx)
    for i, r in zip(idx, res):
        qp, rc, n = oracle_of(oracle, name, i)
        assert_oracle_answer(qp, r, n, (name, i))


@pytest.mark.parametrize("name", ["store_7x2", "store_5x1", "store_4x0"])
def test_the_oracle_answers_of_the_new_shapes_are_unambiguous(oracle, name):
    """(no GPU) every member solved, strict complementarity, no tie in a ratio test (lane_cases.assert_unambiguous)"""
    assert_family_unambiguous(oracle, name)
    q = members(name)[0]
    assert "store_%dx%d" % (q.nV, q.nC) == name and len(members(name)) == 128


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", list(COLD))
def test_full_waves_store_what_a_ragged_wave_stores(capi, oracle, monkeypatch, name, size):
    probs, idx = batch_of(name, size)
    hb, shaped = COLD[name]
    b, res = lane_cold(capi, monkeypatch, probs)
    assert b.lane_hblock() == hb and b.lane_shape() == (FULL if shaped else 0)
    b.close()
    assert_oracle_answers(oracle, name, idx, res)
    if size % 64:
        assert_same_bits(res[size - 1], res[COPY[size]], (name, size, "ragged against full"))
    # the same members 37 places on: the rotation carries members from wave to wave and into the ragged one
    b, turned = lane_cold(capi, monkeypatch, [probs[(i + ROT) % size] for i in range(size)])
    b.close()
    for i in range(size):
        assert_same_bits(res[(i + ROT) % size], turned[i], (name, size, i))
    if shaped:
        b, plain = lane_cold(capi, monkeypatch, probs, shape=False)
        assert b.lane_shape() == 0 and b.lane_hblock() == hb
        b.close()
        assert_same_bits(res, plain, (name, size, "RSQP_LANE_SHAPE=0"))


@pytest.mark.gpu
def test_the_ragged_member_of_the_block_family_answers_as_in_a_full_wave(capi, oracle, monkeypatch):
    out = {}
    for size in (65, 129):
        probs, idx = ragged_batch("roles", size)
        b, out[size] = lane_cold(capi, monkeypatch, probs)
        assert b.lane_shape() == FULL
        b.close()
        assert_oracle_answers(oracle, "roles", idx, out[size])
    assert_ragged_and_full_bits(out[65], out[129], "roles")


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_the_headline_pattern_with_H_in_full(capi, oracle, monkeypatch, size):
    probs, idx = batch_of("hs071", size)
    b, res = lane_cold(capi, monkeypatch, probs, full_H=True)
    assert b.lane_hblock() == 8
    b.close()
    assert_oracle_answers(oracle, "hs071", idx, res)
    if size % 64:
        assert_same_bits(res[size - 1], res[COPY[size]], (size, "ragged against full"))
    b, turned = lane_cold(capi, monkeypatch, [probs[(i + ROT) % size] for i in range(size)], full_H=True)
    b.close()
    for i in range(size):
        assert_same_bits(res[(i + ROT) % size], turned[i], (size, i))
    # (the products with the +0 outside H's block change no bit: the build with H as its leading block answers the same)
    b, block = lane_cold(capi, monkeypatch, probs)
    assert b.lane_hblock() == 4
    b.close()
    assert_same_bits(res, block, (size, "H as its block"))


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", KEPT)
def test_hot_starts_continue_from_the_state_the_stores_wrote(capi, oracle, monkeypatch, name, size):
    probs, idx = batch_of(name, size)
    b, res = lane_cold(capi, monkeypatch, probs, keep=True)
    assert b.lane_hblock() == COLD[name][0] and b.lane_shape() == (FULL if COLD[name][1] else 0)
    assert_oracle_answers(oracle, name, idx, res)
    if size % 64:
        assert_same_bits(res[size - 1], res[COPY[size]], (name, size, "ragged against full"))
    continue_hot(capi, b, probs, oracle_handles(oracle, probs, res), np.random.default_rng(8310 + size), ("vectors", "matrices"))
    b.close()
