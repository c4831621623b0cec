"""The exchange's votes of the lane-per-problem kernel (csrc/qp_lane.hip, change_exchange; LaneT::VOTE bits 5 .. 8): in the full-shape
build without kept state a wave whose lanes all enter a constraint (kind 3) votes again inside that change -- whether any lane needs
the sums that decide between a plain entry and an exchange (nFR - nAC <= 0 in every lane: none does) and, behind the sums, on that
decision (li) -- and a wave that agrees runs a text in which the agreed value is a constant. (The text also holds a vote on the kind
of the partner that leaves, behind the exchange's ratio test, and the ranges of the slots; the shipped build does not select them,
a tuning build does, and the waves below cover them.) Per lane every text performs the same operations on the same operands in the
same order, so the requirement is THE SAME BITS as the run-time-shape build of the same library gives (RSQP_LANE_SHAPE=0: no
votes) and the oracle's answers.

The waves are composed lane by lane from the oracle's record of each member's changes (the working set before and after each
change: kind, slot, plain / exchange, the kind of the slot that left, nFR - nAC before the change). The situations, each at ONE
change count across the lanes named:
  (a) every lane an exchange with a bound as partner while nFR - nAC <= 0: the headline's members, at both of their changes;
  (b) every lane an exchange with a constraint as partner;
  (c) every lane an exchange reached THROUGH the sums: nFR - nAC > 0, and the incoming row an exact multiple of the active one
      on the free variables (the sum over the free variables is rounding: below the band);
  (d) every lane a plain entry (li == 1);
  (e) lanes with nFR - nAC <= 0 beside lanes without;
  (f) exchanging lanes beside plain ones, once with the exchanges of (a)'s kind and once with those of (c)'s;
  (g) partners of both kinds in one wave;
  (h) a lane without a partner (infeasible) and a lane with inconsistent bounds inside a full wave of (a);
  (i) a lane that left the loop one change and a lane that left it two changes before the others: the electorate of a ballot is
      smaller than the wave.
The test without a GPU asserts from the record that every one of them occurs, and that no answer hangs on a tie.

Members: one shape (8 x 2), one pattern per batch, H in its leading 4 x 4 block -- the only batches this build serves. (a), (h), (i):
lane_cases' "hs071" family (the headline's members) and four variants of its members. (b) .. (g): four families on one dense
pattern, generated here; the existing families hold 1 to 3 exchanges per change count, so the members were searched for on the
oracle, in the streams of `candidate`, by the first two changes of their paths, and the indices found are committed (BOX, PAR, FREE,
DEP). Batches of 64, 65, 128 and 129.

The kept-state full-shape build has no votes and keeps its text, so no hot start is continued here (test_gpu_lane_shape.py does)."""
import numpy as np
import pytest

import lane_cases as LC
from lane_cases import FULL, assert_same_bits, assert_same_solution, assert_unambiguous, lane_cold, pattern, working_sets
from restartsqp_amd.qpdump import QPData, dense_to_csc

TWIN = 5                                     # the lane of a batch's last full wave whose member the ragged wave repeats
_cache = {}

# ------------------------------------------------------------------------------------
# the members
# ------------------------------------------------------------------------------------
SEED = 9500
_rng0 = np.random.default_rng(SEED)
_M = _rng0.normal(size=(4, 4))
H0 = np.zeros((8, 8)); H0[:4, :4] = _M @ _M.T / 4 + np.eye(4)
A0 = _rng0.normal(size=(2, 8))
STREAMS = {"box": 1, "free": 2, "dep": 3, "par": 4}


def candidate(kind, k):
    """member k of a stream: dense A, H dense in its 4 x 4 block, both perturbed per member. Every bounded variable starts at its
    lower bound and is held there by its gradient; the constraints lie around A x of a point inside the box, so the corner the
    cold start begins in violates them and they enter first. "box": every variable bounded (nFR = 0 at the start). "free": variables
    0 and 1 without bounds (free from the set-up on: nFR = 2). "dep": as "free", and row 1 of A twice row 0 on those two. "par":
    as "box", and row 1 half of row 0, the tighter constraint of the two: the cold start meets row 0 first, then row 1, which takes
    its place. Draws in the order written: change it and the committed indices mean other members"""
    rng = np.random.default_rng([SEED, STREAMS[kind], k])
    H = H0.copy(); H[:4, :4] *= 1.0 + 0.05 * np.abs(rng.normal())
    A = A0 * (1.0 + 0.05 * rng.normal(size=A0.shape))
    g = 3.0 + np.abs(rng.normal(size=8))
    lb = rng.normal(size=8); ub = lb + 2.0 + np.abs(rng.normal(size=8))
    if kind in ("free", "dep"):
        g[:2] = rng.normal(size=2)
        lb[:2] = -np.inf; ub[:2] = np.inf
    if kind == "dep":
        A[1, :2] = 2.0 * A[0, :2]
    xt = np.where(np.isinf(lb), rng.normal(size=8), lb) + np.where(np.isinf(lb), 0.0, rng.uniform(0.2, 0.8, size=8) * (ub - np.where(np.isinf(lb), 0.0, lb)))
    c = A @ xt
    w = 0.05 + 0.2 * np.abs(rng.normal(size=2))
    lbA = c - w; ubA = c + w
    if kind == "par":
        A[1, :] = 0.5 * A[0, :]
        f = rng.uniform(0.3, 0.7)
        lbA[1] = 0.5 * (c[0] - f * w[0]); ubA[1] = 0.5 * (c[0] + f * w[0])
    return QPData(8, 2, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, lbA, ubA, name="%s%d" % (kind, k))


# the first 64 members of each stream whose path begins as the family's name says and whose answer is unambiguous
# BOX: two exchanges with a bound (nFR - nAC = 0 both times). PAR: an exchange with a bound, then one with constraint 0
BOX = [0, 1, 4, 5, 6, 7, 8, 9, 12, 14, 15, 16, 17, 19, 20, 21, 22, 23, 24, 26, 27, 29, 30, 31, 32, 33, 35, 36, 37, 39, 40, 41, 42, 44, 46, 47,
       48, 50, 51, 52, 54, 55, 56, 57, 59, 60, 61, 66, 68, 69, 71, 74, 75, 77, 78, 79, 80, 83, 85, 87, 89, 90, 92, 93]
PAR = [0, 3, 4, 9, 10, 12, 16, 20, 24, 26, 27, 30, 31, 32, 34, 36, 37, 38, 39, 40, 43, 47, 49, 51, 52, 56, 59, 62, 67, 68, 70, 72, 79, 81, 83,
       84, 85, 87, 88, 91, 94, 100, 104, 105, 106, 109, 110, 111, 114, 121, 122, 125, 126, 129, 130, 134, 137, 140, 142, 144, 145, 146,
       147, 148]
# FREE: two plain entries (nFR - nAC = 2, then 1). DEP: a plain entry, then an exchange although nFR - nAC = 1
FREE = [5, 143, 152, 180, 223, 227, 230, 265, 369, 416, 421, 467, 519, 562, 635, 655, 671, 770, 780, 846, 863, 878, 916, 967, 974, 1048, 1060,
        1087, 1128, 1133, 1149, 1161, 1168, 1184, 1203, 1207, 1258, 1327, 1361, 1382, 1391, 1512, 1570, 1618, 1685, 1710, 1723, 1740, 1792,
        1855, 1861, 1880, 1957, 1980, 2063, 2073, 2090, 2151, 2159, 2204, 2250, 2263, 2266, 2276]
DEP = [0, 2, 3, 4, 5, 6, 9, 10, 13, 17, 18, 21, 22, 23, 27, 28, 29, 31, 34, 35, 36, 37, 39, 40, 41, 43, 44, 45, 47, 49, 50, 53, 57, 58, 59, 60,
       62, 63, 64, 66, 67, 68, 71, 72, 73, 74, 76, 78, 80, 81, 82, 84, 85, 86, 87, 88, 89, 91, 93, 96, 97, 101, 103, 104]

HS_INCONSISTENT, HS_INFEASIBLE, HS_ONE_CHANGE, HS_NO_CHANGE = range(4)       # members of "xhs"


def _hs_variants():
    """four variants of headline members: inconsistent bounds and constraints far from what the box allows (lane_cases' recipes for
    its odd batch), constraint 0 without limits (one change instead of two), both constraints without limits (none)"""
    D = LC.members("hs071")
    inf = np.inf

    def mod(q, lb=None, ub=None, lbA=None, ubA=None):
        pick = lambda new, old: old.copy() if new is None else new
        return QPData(8, 2, q.H_jc, q.H_ir, q.H_val, q.A_jc, q.A_ir, q.A_val, q.g, pick(lb, q.lb), pick(ub, q.ub), pick(lbA, q.lbA),
                      pick(ubA, q.ubA), name=q.name)
    e2 = np.arange(8) == 2
    q0, q1, q2, q3 = D[5], D[9], D[20], D[41]
    return [mod(q0, lb=np.where(e2, 1.0, q0.lb), ub=np.where(e2, 0.0, q0.ub)),
            mod(q1, lbA=q1.ubA + 500.0, ubA=q1.ubA + 501.0),
            mod(q2, lbA=np.array([-inf, q2.lbA[1]]), ubA=np.array([inf, q2.ubA[1]])),
            mod(q3, lbA=np.array([-inf, -inf]), ubA=np.array([inf, inf]))]


LC.FAMILIES.update(xbox=lambda: [candidate("box", k) for k in BOX], xpar=lambda: [candidate("par", k) for k in PAR],
                   xfree=lambda: [candidate("free", k) for k in FREE], xdep=lambda: [candidate("dep", k) for k in DEP], xhs=_hs_variants)
GENERATED = ("xbox", "xpar", "xfree", "xdep")


def member(key):
    """key: (family of lane_cases, index in it)"""
    return LC.members(key[0])[key[1]]


def oracle_of(oracle, key):
    return LC.oracle_of(oracle, *key)


def changes_of(oracle, key):
    """[(kind, slot, "plain" | "flip" | "exchange", the partner's kind -- 1 a constraint left, 2 a bound, 0 none --, nFR - nAC before
    the change)] per change of a solved member, from the working set before and after each change"""
    if ("changes", key) not in _cache:
        qp, rc, n = oracle_of(oracle, key)
        assert rc == 0 and qp.exitflag() == 20, key
        ws = working_sets(oracle, member(key), n)
        ev = []
        for a, b in zip(ws[:-1], ws[1:]):
            moved = np.nonzero(a != b)[0]
            left = [i for i in moved if a[i] != 0 and b[i] == 0]
            came = [i for i in moved if a[i] == 0 and b[i] != 0]
            d = int((a[:8] == 0).sum()) - int((a[8:] != 0).sum())
            if len(moved) == 1 and a[moved[0]] == -b[moved[0]]:
                ev.append((1 if moved[0] >= 8 else 2, int(moved[0]) % 8, "flip", 0, d))
            elif len(moved) == 1 and left:
                ev.append((1 if left[0] >= 8 else 2, int(left[0]) % 8, "plain", 0, d))
            elif len(moved) == 1 and came:
                ev.append((3 if came[0] >= 8 else 4, int(came[0]) % 8, "plain", 0, d))
            else:
                assert len(moved) == 2 and len(left) == 1 and len(came) == 1, (key, a, b)
                ev.append((3 if came[0] >= 8 else 4, int(came[0]) % 8, "exchange", 1 if left[0] >= 8 else 2, d))
        assert len(ev) == n, key
        _cache[("changes", key)] = ev
    return _cache[("changes", key)]


def _alternate(fa, fb):
    return [(fa if j % 2 == 0 else fb, j) for j in range(64)]


def _with(keys, swaps):
    keys = list(keys)
    for lane, key in swaps.items():
        keys[lane] = key
    return keys


HS0, HS1 = [("hs071", j) for j in range(64)], [("hs071", 64 + j) for j in range(64)]
WAVES = {
    "a hs071 0": HS0,
    "a hs071 1": HS1,
    "b constraint partners": [("xpar", j) for j in range(64)],
    "c through the sums": [("xdep", j) for j in range(64)],
    "d plain entries": [("xfree", j) for j in range(64)],
    "e f bound exchanges beside plain": _alternate("xbox", "xfree"),
    "f summed exchanges beside plain": _alternate("xdep", "xfree"),
    "g both partners": _alternate("xbox", "xpar"),
    "h odd lanes": _with(HS0, {5: ("xhs", HS_INCONSISTENT), 9: ("xhs", HS_INFEASIBLE)}),
    "i done apart": _with(HS1, {20: ("xhs", HS_ONE_CHANGE), 41: ("xhs", HS_NO_CHANGE)}),
}
UNSOLVED = (("xhs", HS_INCONSISTENT), ("xhs", HS_INFEASIBLE))
# batch -> (its full waves, whether a ragged wave of one lane follows): sizes 64, 65, 128, 129
BATCHES = {
    "64": (["b constraint partners"], False),
    "65": (["c through the sums"], True),
    "128": (["d plain entries", "e f bound exchanges beside plain"], False),
    "129": (["f summed exchanges beside plain", "g both partners"], True),
    "128 hs071": (["h odd lanes", "i done apart"], False),
    "129 hs071": (["a hs071 0", "a hs071 1"], True),
}


def batch_keys(name):
    names, ragged = BATCHES[name]
    keys = [key for w in names for key in WAVES[w]]
    if name == "129 hs071":
        return keys + [("hs071", 128)]              # (the headline's first 129 as they come)
    return keys + ([keys[-64 + TWIN]] if ragged else [])


def passes(oracle, keys):
    """what a wave's lanes do pass by pass of the kernel's loop: per change count, the changes of the lanes that still change"""
    evs = [changes_of(oracle, key) for key in keys if key not in UNSOLVED]
    return [[e[i] for e in evs if len(e) > i] for i in range(max(len(e) for e in evs))]


# ------------------------------------------------------------------------------------
# without a GPU: the waves hold what they are named for
# ------------------------------------------------------------------------------------
def test_the_batches_have_the_four_sizes_and_one_pattern_each():
    sizes = set()
    for name in BATCHES:
        probs = [member(k) for k in batch_keys(name)]
        sizes.add(len(probs))
        assert len(probs) == int(name.split()[0])
        assert len({pattern(q) for q in probs}) == 1 and all(q.nV == 8 and q.nC == 2 and q.H_ir.max() < 4 for q in probs), name
        assert LC.expected_block(probs) == 4
    assert sizes == {64, 65, 128, 129}
    assert {w for names, _ in BATCHES.values() for w in names} == set(WAVES)              # (every wave built is in a batch)
    for fam in GENERATED:
        assert len(LC.members(fam)) == 64 and len({q.name for q in LC.members(fam)}) == 64


def test_no_answer_of_the_generated_members_hangs_on_a_tie(oracle):
    for fam in GENERATED:
        LC.assert_family_unambiguous(oracle, fam)
    rng = np.random.default_rng(2)
    for k in (HS_ONE_CHANGE, HS_NO_CHANGE):
        assert_unambiguous(oracle, member(("xhs", k)), *oracle_of(oracle, ("xhs", k)), rng, ("xhs", k))


def test_every_situation_occurs_in_the_waves_built(oracle):
    """(no GPU) from the oracle's record of each member's changes; a situation holds at ONE change count, in all 64 lanes unless it
    says otherwise"""
    P = {name: passes(oracle, keys) for name, keys in WAVES.items()}
    full = lambda p: len(p) == 64 and all(c[0] == 3 for c in p)                 # every lane of the wave enters a constraint
    exch = lambda c: c[2] == "exchange"
    # (a) the headline's members, both changes: every lane an exchange with a bound while nFR - nAC <= 0; nothing else follows
    for w in ("a hs071 0", "a hs071 1"):
        assert len(P[w]) == 2
        for p in P[w]:
            assert full(p) and all(exch(c) and c[3] == 2 and c[4] <= 0 for c in p), w
    # (b) every lane an exchange with a constraint as partner
    assert any(full(p) and all(exch(c) and c[3] == 1 for c in p) for p in P["b constraint partners"])
    # (c) every lane an exchange although nFR - nAC > 0: li == 0 comes from the sums. The members make the sum rounding alone: the
    # free variables before that change are 0 and 1, and on them the incoming row is twice the active one, to the bit
    hit = [i for i, p in enumerate(P["c through the sums"]) if full(p) and all(exch(c) and c[4] > 0 for c in p)]
    assert hit == [1]
    for key in WAVES["c through the sums"]:
        q, (kind, slot, _, _, d) = member(key), changes_of(oracle, key)[1]
        before = working_sets(oracle, q, 1)[1]
        A = q.dense_A()
        assert list(np.nonzero(before[:8] == 0)[0]) == [0, 1] and before[8 + 1 - slot] != 0 and before[8 + slot] == 0 and d == 1, key
        assert np.array_equal(A[1, :2], 2.0 * A[0, :2]), key
    # (d) every lane a plain entry
    assert any(full(p) and all(c[2] == "plain" for c in p) for p in P["d plain entries"])
    # (e) lanes with nFR - nAC <= 0 beside lanes without, (f) exchanging lanes beside plain ones: 32 and 32
    p = P["e f bound exchanges beside plain"][0]
    assert full(p) and sorted(c[4] <= 0 for c in p) == [False] * 32 + [True] * 32
    assert all(exch(c) == (c[4] <= 0) for c in p)
    # (f) again, behind the sums: every lane nFR - nAC > 0, the sums send 32 lanes to the exchange and 32 to the plain entry
    p = P["f summed exchanges beside plain"][1]
    assert full(p) and all(c[4] > 0 for c in p) and sorted(exch(c) for c in p) == [False] * 32 + [True] * 32
    # (g) every lane an exchange while nFR - nAC <= 0, 32 partners bounds and 32 constraints
    p = P["g both partners"][1]
    assert full(p) and all(exch(c) and c[4] <= 0 for c in p) and sorted(c[3] for c in p) == [1] * 32 + [2] * 32
    # (h) inside a full wave of (a): inconsistent bounds (infeasible before any change), no partner after some changes
    p = P["h odd lanes"]
    assert len(p) == 2 and all(len(x) == 62 and all(c[0] == 3 and exch(c) and c[3] == 2 and c[4] <= 0 for c in x) for x in p)
    qp, rc, n0 = oracle_of(oracle, ("xhs", HS_INCONSISTENT))
    assert rc != 0 and qp.exitflag() != 20 and n0 == 0
    qp, rc, n1 = oracle_of(oracle, ("xhs", HS_INFEASIBLE))
    assert rc != 0 and qp.exitflag() != 20 and n1 > 0
    # (i) one lane leaves the loop two changes before the others and one lane one change before them: 63 lanes vote in the first
    # change, 62 in the second, and every vote is (a)'s
    n = sorted(len(changes_of(oracle, key)) for key in WAVES["i done apart"])
    assert n == [0, 1] + [2] * 62
    p = P["i done apart"]
    assert [len(x) for x in p] == [63, 62] and all(c[0] == 3 and exch(c) and c[3] == 2 and c[4] <= 0 for x in p for c in x)


# ------------------------------------------------------------------------------------
# the same bits, and the oracle's answers
# ------------------------------------------------------------------------------------
def results(capi, monkeypatch, name, shape):
    """the batch's cold start on the full-shape build (the votes) or on the run-time-shape build (none), solved once"""
    key = ("results", name, shape)
    if key not in _cache:
        b, res = lane_cold(capi, monkeypatch, [member(k) for k in batch_keys(name)], shape=shape)
        assert b.lane_hblock() == 4 and b.lane_shape() == (FULL if shape else 0)
        b.close()
        _cache[key] = res
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_the_exchange_texts_give_the_oracles_answers(capi, oracle, monkeypatch, name):
    keys = batch_keys(name)
    res = results(capi, monkeypatch, name, True)
    assert len(res) == len(keys)
    solved = 0
    for key, r in zip(keys, res):
        qp, rc, n = oracle_of(oracle, key)
        assert r["status"] == qp.exitflag(), key
        if rc == 0:
            assert_same_solution(qp, r, n)              # (status, nWSR, working sets exact; x, y within 1e-9)
            solved += 1
    assert solved == len(res) - sum(key in UNSOLVED for key in keys) and (name != "128 hs071" or solved == 126)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_the_exchange_texts_give_the_bits_of_the_build_without_votes(capi, monkeypatch, name):
    new, old = results(capi, monkeypatch, name, True), results(capi, monkeypatch, name, False)
    assert len(new) == len(batch_keys(name))
    assert_same_bits(new, old, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, (_, ragged) in BATCHES.items() if ragged and n != "129 hs071"])
def test_a_member_answers_the_same_bits_in_a_full_wave_and_in_the_ragged_one(capi, monkeypatch, name):
    """the ragged wave's lanes all hold its one member: whatever the full wave in front of it voted, that wave agrees on everything"""
    res = results(capi, monkeypatch, name, True)
    assert_same_bits(res[-1], res[-65 + TWIN], name)
