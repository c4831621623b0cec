"""The lane-per-problem kernel's votes (csrc/qp_lane.hip, LaneT::VOTE): in the full-shape build without kept state the lanes of a
wave that are still in the homotopy's loop vote, by ballot, on what happens next -- whether every one of them is about to make a
working-set change of one kind, and whether none or all of them are done -- and a wave that agrees runs a text in which that is a
constant. A wave that disagrees runs the text of the other builds. Per lane every text performs the same operations on the same
operands in the same order, so the requirement is THE SAME BITS as the run-time-shape build of the same library gives
(RSQP_LANE_SHAPE=0: no votes), and the oracle's answers by test_gpu_parity.assert_same_solution.

What can go wrong depends on what the lanes of ONE wave do at the SAME change count, so the waves here are composed, lane by lane,
from the oracle's record of every member's changes (the working set after each change: kind, slot, and whether the change was
plain, a flip to the opposite side or an exchange):
  (a) every lane makes a change of kind K at one count, for K = 1 .. 4: once on the same slot in every lane, once on slots that differ;
  (b) lanes hold different kinds at one count;
  (c) every lane a kind-2 change, one lane's being a flip;
  (d) every lane a change of kind 3 or 4, some with an exchange and some without;
  (e) lanes that are done one, two and more changes before the others (the masked vote; the step's three texts in every order);
  (f) the headline's own members (two changes each, both of kind 3 by an exchange with a bound, in every lane);
  (g) a member with inconsistent bounds and a member that ends infeasible inside a full wave.
A test without a GPU asserts, from the same record, that each situation occurs in the waves built. One shape (8 x 2), one pattern, H
in its leading 4 x 4 block; the members are lane_cases' families "roles" and "pivots" (two patterns: a batch takes its waves from
one; test_gpu_lane_roles.py and test_gpu_lane_pivots.py assert that no answer of theirs is ambiguous), "odd" and "hs071". Batches
of 64, 65, 128 and 129: a full wave, a full wave beside a ragged wave of one lane, two full waves, and the ragged wave behind them;
the ragged wave's member also sits in the full wave in front of it."""
import numpy as np
import pytest

import lane_cases as LC
from lane_cases import FULL, ODD_INCONSISTENT, ODD_INFEASIBLE, assert_same_bits, assert_same_solution, lane_cold, pattern, working_sets

KINDS = {1: "constraint leaves", 2: "bound leaves", 3: "constraint enters", 4: "variable fixed"}
TWIN = 5                                     # the lane of a batch's last full wave whose member the ragged wave repeats
_cache = {}


# ------------------------------------------------------------------------------------
# the members and the oracle's record of their changes
# ------------------------------------------------------------------------------------
def member(key):
    """key: (family of lane_cases, index in it)"""
    return LC.members(key[0])[key[1]]


def oracle_of(oracle, key):
    return LC.oracle_of(oracle, *key)


def changes_of(oracle, key):
    """[(kind, slot, "plain" | "flip" | "exchange")] per change of a solved member, from the working set after each change. A flip
    is the change of kind 1 / 2 whose released direction has no curvature (the slot goes to its other side); an exchange is the
    change of kind 3 / 4 whose incoming row depends on the active ones (a partner leaves in the same change)"""
    if ("changes", key) not in _cache:
        qp, rc, n = oracle_of(oracle, key)
        assert rc == 0 and qp.exitflag() == 20, key
        ws = working_sets(oracle, member(key), n)
        ev = []
        for a, b in zip(ws[:-1], ws[1:]):
            moved = np.nonzero(a != b)[0]
            left = [i for i in moved if a[i] != 0 and b[i] == 0]
            came = [i for i in moved if a[i] == 0 and b[i] != 0]
            if len(moved) == 1 and a[moved[0]] == -b[moved[0]]:
                i, how = moved[0], "flip"
                kind = 1 if i >= 8 else 2
            elif len(moved) == 1 and left:
                i, how = left[0], "plain"
                kind = 1 if i >= 8 else 2
            elif len(moved) == 1 and came:
                i, how = came[0], "plain"
                kind = 3 if i >= 8 else 4
            else:
                assert len(moved) == 2 and len(left) == 1 and len(came) == 1, (key, a, b)
                i, how = came[0], "exchange"
                kind = 3 if i >= 8 else 4
            ev.append((kind, int(i) % 8, how))
        assert len(ev) == n and sum(e[2] == "flip" for e in ev) == qp.nflips(), key
        _cache[("changes", key)] = ev
    return _cache[("changes", key)]


def fill(cands, n=64):
    assert cands
    return [cands[j % len(cands)] for j in range(n)]


def waves(oracle):
    """{name: 64 member keys}, composed from the record; deterministic. A wave takes its members from one pool (one pattern)"""
    if "waves" in _cache:
        return _cache["waves"]
    W = {}
    pools = {p: [(p, k) for k in range(128)] for p in ("roles", "pivots")}
    ev = lambda key: changes_of(oracle, key)
    at = lambda key, i: ev(key)[i] if len(ev(key)) > i else (0, -1, "")
    best = lambda options: max(options, key=lambda o: (o[0], -o[1], o[2]))[3]          # (most distinct members; then the earliest count)
    for K in KINDS:
        same, differ = [], []
        for p, keys in pools.items():
            for i in range(16):
                plain = [key for key in keys if at(key, i)[0] == K and at(key, i)[2] == "plain"]
                for slot in sorted({at(key, i)[1] for key in plain}):
                    c = [key for key in plain if at(key, i)[1] == slot]
                    same.append((len(c), i, p, c))
                if len({at(key, i)[1] for key in plain}) >= 2:
                    differ.append((len(plain), i, p, plain))
        W["a%d same slot" % K] = fill(best(same))
        W["a%d slots differ" % K] = fill(best(differ))
    W["b kinds differ"] = pools["roles"][:64]
    flips, exch = [], []
    for p, keys in pools.items():
        for i in range(16):
            f = [key for key in keys if at(key, i) [0] == 2 and at(key, i)[2] == "flip"]
            pl = [key for key in keys if at(key, i)[0] == 2 and at(key, i)[2] == "plain"]
            if f and pl:
                flips.append((len(pl), i, p, fill(pl, 63) + f[:1]))
            for K in (3, 4):
                x = [key for key in keys if at(key, i)[0] == K and at(key, i)[2] == "exchange"]
                pl = [key for key in keys if at(key, i)[0] == K and at(key, i)[2] == "plain"]
                if x and pl:
                    xs, ps = fill(x, 16), fill(pl, 48)
                    exch.append((len(pl), i, p, [xs[j // 4] if j % 4 == 0 else ps[j - j // 4 - 1] for j in range(64)]))
    W["c one lane flips"] = best(flips)
    W["d some lanes exchange"] = best(exch)
    # (e) lanes that finish after n0, n0 + 1, n0 + 2 and n0 + 4 or more changes, lane by lane in turn
    by_len = {}
    for key in pools["pivots"]:
        by_len.setdefault(len(ev(key)), []).append(key)
    n0 = min(n for n in by_len if n + 1 in by_len and n + 2 in by_len)
    late = [key for n in sorted(by_len) if n >= n0 + 4 for key in by_len[n]]
    classes = [fill(by_len[n0], 16), fill(by_len[n0 + 1], 16), fill(by_len[n0 + 2], 16), fill(late, 16)]
    W["e done apart"] = [classes[j % 4][j // 4] for j in range(64)]
    _cache["waves"] = W
    return W


# batch -> (its full waves, whether a ragged wave of one lane follows): sizes 64, 65, 128, 129
BATCHES = {
    "64": (["a2 same slot"], False),
    "65": (["a2 slots differ"], True),
    "65 odd": (["g odd"], True),
    "128 a": (["a1 same slot", "a1 slots differ"], False),
    "128 b": (["a3 same slot", "a3 slots differ"], False),
    "129 a": (["a4 same slot", "a4 slots differ"], True),
    "129 b": (["b kinds differ", "c one lane flips"], True),
    "129 c": (["d some lanes exchange", "e done apart"], True),
    "129 hs071": (["hs071 0", "hs071 1"], True),
}


def wave_keys(oracle, name):
    if name == "g odd":
        return [("odd", k) for k in range(64)]
    if name.startswith("hs071"):
        return [("hs071", 64 * int(name[-1]) + j) for j in range(64)]
    return waves(oracle)[name]


def batch_keys(oracle, name):
    names, ragged = BATCHES[name]
    keys = [key for w in names for key in wave_keys(oracle, w)]
    if name == "129 hs071":
        return keys + [("hs071", 128)]              # (the headline's first 129 as they come)
    return keys + ([keys[-64 + TWIN]] if ragged else [])


def passes(oracle, keys):
    """what a wave's lanes do pass by pass of the kernel's loop: [(step text, {kinds}, [(kind, slot, how) of the lanes that change])].
    Lane j takes part in passes 0 .. n_j: it changes in the passes below n_j and is done in pass n_j; then it has left the loop. Step
    text: 1 no lane of those in the loop is done, 2 every one is, 0 they disagree"""
    evs = [changes_of(oracle, key) for key in keys]
    out = []
    for i in range(max(len(e) for e in evs) + 1):
        in_loop = [e for e in evs if len(e) >= i]
        done = [e for e in in_loop if len(e) == i]
        ch = [e[i] for e in in_loop if len(e) > i]
        out.append((1 if not done else (2 if len(done) == len(in_loop) else 0), {c[0] for c in ch}, ch))
    return out


# ------------------------------------------------------------------------------------
# without a GPU: the waves hold what they are named for
# ------------------------------------------------------------------------------------
def test_the_batches_have_the_four_sizes_and_one_pattern_each(oracle):
    sizes = set()
    for name in BATCHES:
        probs = [member(k) for k in batch_keys(oracle, name)]
        sizes.add(len(probs))
        assert len(probs) == int(name.split()[0])
        assert len({pattern(q) for q in probs}) == 1 and all(q.nV == 8 and q.nC == 2 and q.H_ir.max() < 4 for q in probs), name
    assert sizes == {64, 65, 128, 129}
    named = {w for names, _ in BATCHES.values() for w in names}
    assert named == set(waves(oracle)) | {"g odd", "hs071 0", "hs071 1"}              # (every wave built is in a batch)


def test_every_situation_occurs_in_the_waves_built(oracle):
    """(no GPU) from the oracle's record of each member's changes"""
    W = waves(oracle)
    P = {name: passes(oracle, keys) for name, keys in W.items()}
    for K in KINDS:
        # (a) all 64 lanes a plain change of kind K in one pass: on one slot; on slots that differ
        same = [ch for _, kinds, ch in P["a%d same slot" % K] if kinds == {K} and len(ch) == 64 and all(c[2] == "plain" for c in ch)
                and len({c[1] for c in ch}) == 1]
        differ = [ch for _, kinds, ch in P["a%d slots differ" % K] if kinds == {K} and len(ch) == 64 and all(c[2] == "plain" for c in ch)
                  and len({c[1] for c in ch}) >= 2]
        print(KINDS[K], "same slot: distinct members", len(set(W["a%d same slot" % K])), "slots differ:", len(set(W["a%d slots differ" % K])),
              sorted({c[1] for c in differ[0]}) if differ else None)
        assert same and differ, K
    # (b) lanes of one pass hold different kinds
    assert any(len(kinds) >= 2 for _, kinds, _ in P["b kinds differ"])
    # (c) every lane a kind-2 change, exactly one of them a flip
    assert any(kinds == {2} and len(ch) == 64 and sorted(c[2] for c in ch) == ["flip"] + ["plain"] * 63 for _, kinds, ch in P["c one lane flips"])
    # (d) every lane a change of one kind, 3 or 4; some with an exchange, some without
    assert any(kinds in ({3}, {4}) and len(ch) == 64 and {c[2] for c in ch} == {"exchange", "plain"} for _, kinds, ch in P["d some lanes exchange"])
    # (e) lanes done one, two and at least four changes before the last ones; every order of the step's texts among all waves
    n = sorted({len(changes_of(oracle, key)) for key in W["e done apart"]})
    assert len(n) >= 4 and n[1] == n[0] + 1 and n[2] == n[0] + 2 and n[-1] >= n[0] + 4, n
    assert {0, 1, 2} == {t for t, _, _ in P["e done apart"]}
    orders = set()
    for p in P.values():
        orders |= {(a[0], b[0]) for a, b in zip(p[:-1], p[1:])}
    print("orders of the step's texts", sorted(orders))
    assert {(1, 1), (1, 0), (0, 1), (0, 0), (0, 2), (1, 2)} <= orders          # (text 2 is a wave's last pass: nothing follows it)
    # the waves take every arm of the vote on the kind: a text of each kind, and the text by lane
    for K in KINDS:
        assert any(kinds == {K} for p in P.values() for _, kinds, _ in p)
    # (f) the headline's members: two changes each, both a constraint that enters by an exchange with a bound (kind 3, in every
    # lane); no lane done before the others
    for w in ("hs071 0", "hs071 1"):
        p = passes(oracle, wave_keys(oracle, w))
        assert [(t, kinds) for t, kinds, _ in p] == [(1, {3}), (1, {3}), (2, set())]
        assert all(c[2] == "exchange" for _, _, ch in p for c in ch)
    # (g) inside a full wave: inconsistent bounds (infeasible before any change), infeasible after some changes
    assert ODD_INCONSISTENT < 64 and ODD_INFEASIBLE < 64
    qp, rc, n0 = oracle_of(oracle, ("odd", ODD_INCONSISTENT))
    assert rc != 0 and qp.exitflag() != 20 and n0 == 0
    qp, rc, n1 = oracle_of(oracle, ("odd", ODD_INFEASIBLE))
    assert rc != 0 and qp.exitflag() != 20 and n1 > 0


# ------------------------------------------------------------------------------------
# the same bits, and the oracle's answers
# ------------------------------------------------------------------------------------
def results(capi, oracle, monkeypatch, name, shape):
    """the batch's cold start on the full-shape build (the votes) or on the run-time-shape build (none), solved once"""
    key = ("results", name, shape)
    if key not in _cache:
        b, res = lane_cold(capi, monkeypatch, [member(k) for k in batch_keys(oracle, name)], shape=shape)
        assert b.lane_hblock() == 4 and b.lane_shape() == (FULL if shape else 0)
        b.close()
        _cache[key] = res
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_the_voted_texts_give_the_oracles_answers(capi, oracle, monkeypatch, name):
    keys = batch_keys(oracle, name)
    res = results(capi, oracle, monkeypatch, name, True)
    assert len(res) == len(keys)
    solved = 0
    for key, r in zip(keys, res):
        qp, rc, n = oracle_of(oracle, key)
        assert r["status"] == qp.exitflag(), key
        if rc == 0:
            assert_same_solution(qp, r, n)              # (status, nWSR, working sets exact; x, y within 1e-9)
            solved += 1
    # (the odd wave's two members that cannot be solved; its ragged wave repeats lane TWIN, the one with inconsistent bounds)
    odd = (("odd", ODD_INCONSISTENT), ("odd", ODD_INFEASIBLE))
    assert solved == len(res) - sum(key in odd for key in keys) and (name != "65 odd" or len(res) - solved == 3)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_the_voted_texts_give_the_bits_of_the_build_without_votes(capi, oracle, monkeypatch, name):
    new, old = results(capi, oracle, monkeypatch, name, True), results(capi, oracle, monkeypatch, name, False)
    assert len(new) == len(batch_keys(oracle, name))
    assert_same_bits(new, old, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, (_, ragged) in BATCHES.items() if ragged and n != "129 hs071"])
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, oracle, monkeypatch, name):
    """the ragged wave's lanes all hold its one member: whatever the full wave in front of it voted, that wave agrees on everything"""
    res = results(capi, oracle, monkeypatch, name, True)
    assert_same_bits(res[-1], res[-65 + TWIN], name)
