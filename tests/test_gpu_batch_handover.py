"""The hand-over of a batch (rsqp_batch_set_handover): the members the register-resident tableau kernels (qp_tiny.hip, qp_lane.hip)
give up on at set-up are solved by the LDS-resident Givens / TQ kernel in a masked launch right behind them, as rsqp_solve re-solves
such a call on a single handle.

The inputs are problems.stiff_free_batch: every third member has a variable without bounds and another, decoupled and pinned at a
bound, whose Hessian entry is 1e10 -- both tableau kernels refuse a free variable whose curvature is below 1e-8 of the largest
diagonal entry, the null-space engines and the CPU oracle solve the member as the well-conditioned problem it is
(tests/test_batch_handover_args.py checks the generator on the CPU). Bar as everywhere: statuses, working sets and iteration counts
exact, x / y / objective within 1e-9 relative, against the CPU oracle or, for call sequences, against one capi.Solver per member."""
import copy

import numpy as np
import pytest

from conftest import oracle_cold
from restartsqp_amd import problems
from test_gpu_parity import assert_same_solution

pytestmark = pytest.mark.gpu

RTOL = 1e-9
EVERY = 3
_cold = {}


def stiff_batch(nV, nC, n=100):
    return problems.stiff_free_batch(np.random.default_rng(5000 + 10 * nV + nC), nV, nC, n, every=EVERY)


def cold_reference(oracle, nV, nC, n=100):
    """(members, the oracle's cold solve of each), computed once per shape and size and only read afterwards"""
    key = (nV, nC, n)
    if key not in _cold:
        probs = stiff_batch(nV, nC, n)
        _cold[key] = (probs, [oracle_cold(oracle, q) for q in probs])
    return _cold[key]


def is_stiff(n):
    return np.arange(n) % EVERY == 0


def make_batch(capi, monkeypatch, probs, lane, handover, keep=True):
    monkeypatch.setenv("RSQP_LANE", lane)            # (read by rsqp_batch_create)
    b = capi.Batch(probs)
    b.set_keep_state(keep)
    b.set_handover(handover)
    return b


def assert_all_match_the_oracle(b, ref):
    res = b.results()
    ok, kkt = b.test_optimality()
    for (qp, rc, n), r, o in zip(ref, res, ok):
        assert rc == 0 and qp.exitflag() == 20
        assert_same_solution(qp, r, n)
        assert abs(r["obj"] - qp.objective) <= RTOL * max(1.0, abs(qp.objective))
        assert o == 1
    handed, count = b.handover()
    assert np.array_equal(handed, is_stiff(b.nq).astype(np.int32)) and count == int(is_stiff(b.nq).sum())


def test_off_is_todays_behaviour(capi, oracle, monkeypatch):
    """The premise: on the 8-lane tableau kernel every stiff member comes back unsolved, every other member as the oracle has it,
    and nobody is reported as handed over."""
    probs, ref = cold_reference(oracle, 8, 2)
    b = make_batch(capi, monkeypatch, probs, "0", False)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 1
    for t, ((qp, rc, n), r) in enumerate(zip(ref, b.results())):
        if t % EVERY == 0:
            assert r["status"] != 20, t
        else:
            assert_same_solution(qp, r, n)
    handed, count = b.handover()
    assert count == 0 and not handed.any()
    b.close()


@pytest.mark.parametrize("shape,mc", [((8, 2), 2), ((7, 4), 4), ((8, 8), 8)])
def test_on_eight_lane_kernel(capi, oracle, monkeypatch, shape, mc):
    """The three builds of the 8-lane kernel by the number of constraint slots (MC = 2 / 4 / 8), whose state blocks keep their ints
    at different offsets."""
    probs, ref = cold_reference(oracle, *shape)
    b = make_batch(capi, monkeypatch, probs, "0", True)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 1 and b.last_plan()["mc"] == mc
    assert_all_match_the_oracle(b, ref)
    b.close()


# (8, 2): H has entries outside its leading 4 x 4 block -- the full-triangle build (lane_hblock 8); (4, 1): all of H is that block
# -- the block build (lane_hblock 4). 131 members: two full waves and a ragged third
@pytest.mark.parametrize("shape,hblock,n,keep", [((8, 2), 8, 100, True), ((8, 2), 8, 100, False), ((4, 1), 4, 100, True),
                                                 ((4, 1), 4, 100, False), ((8, 2), 8, 131, True), ((4, 1), 4, 131, False)])
def test_on_lane_kernel(capi, oracle, monkeypatch, shape, hblock, n, keep):
    probs, ref = cold_reference(oracle, *shape, n=n)
    b = make_batch(capi, monkeypatch, probs, "1", True, keep=keep)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 2 and b.lane_hblock() == hblock
    assert_all_match_the_oracle(b, ref)
    b.close()


def repin(q):
    j = q.nV - 1
    q.lb[j] = 0.0; q.ub[j] = 1.0; q.g[j] = 100.0
    return q


def test_optimize_qp_against_single_handles(capi, monkeypatch):
    """Four optimizeQP calls -- cold, new vectors, new matrix values (a FIXED -> VARIED flip: re-initialisation from the member's own
    x, y and bounds), new vectors -- on a batch with the hand-over on and on one capi.Solver per member: status, nWSR_used, raw
    working sets, x and y agree per member and per call; the call shape agrees wherever it survives (a member handed over ran cold
    where the dispatch chose a hot start). Member 1 (ordinary) is infeasible in call 2, member 3 (stiff) in call 3: both take
    handle_error's slack-point rescue (nV = 8 >= 2 nC = 4)."""
    rng = np.random.default_rng(77)
    n = 60
    s0 = stiff_batch(8, 2, n)
    s1 = [repin(problems.perturb(rng, q, 0.05)) for q in s0]
    s2 = [copy.deepcopy(q) for q in s1]
    for q in s2:
        q.A_val = q.A_val * (1.0 + 0.05 * rng.normal(size=q.A_val.shape))
    s3 = [repin(problems.perturb(rng, q, 0.05)) for q in s2]
    steps = [s0, s1, s2, s3]
    for step, member in ((1, 1), (2, 3)):
        q = steps[step][member] = copy.deepcopy(steps[step][member])
        q.lbA = q.ubA + 50.0
    stiff = is_stiff(n)
    infeasible = np.zeros((4, n), bool)
    infeasible[1, 1] = infeasible[2, 3] = True

    b = make_batch(capi, monkeypatch, s0, "0", True)
    solvers = []
    for q in s0:
        s = capi.Solver(q.nV, q.nC, 0)
        s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        solvers.append(s)
    seen_modes, seen_rescues = [], set()
    for k, probs in enumerate(steps):
        if k > 0:
            b.set_vectors_from(probs)
        if k == 2:
            b.set_matrix_values(np.concatenate([q.A_val for q in probs]), np.concatenate([q.H_val for q in probs]))
        used = b.optimize_qp()
        assert b.last_kernel() == 1
        res = b.results()
        mode, rescue = b.dispatch()
        handed, count = b.handover()
        # a member whose bounds are inconsistent is infeasible before any set-up, in the first solve and in its rescue: it is the
        # one stiff member the tableau kernel does not give up on
        want = stiff & ~infeasible[k]
        assert np.array_equal(handed, want.astype(np.int32)) and count == int(want.sum()), k
        for t, (q, s, r) in enumerate(zip(probs, solvers, res)):
            if k == 2:
                s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
            for w, v in enumerate((q.g, q.lb, q.ub, q.lbA, q.ubA)):
                s.set_vector(w, v)
            ns = s.optimize_qp()
            wb, wc = s.working_set_raw()
            assert r["status"] == s.status and used[t] == ns, (k, t, r["status"], s.status, used[t], ns)
            assert np.array_equal(r["ws_b"], wb) and np.array_equal(r["ws_c"], wc), (k, t)
            xs, ys = s.x, s.y
            assert np.abs(r["x"] - xs).max() <= RTOL * max(1.0, np.abs(xs).max()), (k, t)
            assert np.abs(r["y"] - ys).max() <= RTOL * max(1.0, np.abs(ys).max()), (k, t)
            assert (rescue[t] == 2) == bool(infeasible[k, t]), (k, t, rescue[t])
            if rescue[t] != 0:
                continue                                     # (the handle reports the mode of the rescue solve)
            if not infeasible[:k + 1, t].any():
                assert r["status"] == 20, (k, t)
            if handed[t]:
                assert s.last_mode() == (3 if mode[t] == 3 else 0), (k, t, mode[t], s.last_mode())
            else:
                assert s.last_mode() == mode[t], (k, t, mode[t], s.last_mode())
        seen_modes.append(int(mode[2]))                      # (member 2: ordinary, never infeasible)
        seen_rescues |= set(rescue.tolist())
    assert seen_modes == [capi.MODE_COLD, capi.MODE_HOT_VECTORS, capi.MODE_WARM_REINIT, capi.MODE_HOT_VECTORS]
    assert 2 in seen_rescues
    for s in solvers:
        s.close()
    b.close()


@pytest.mark.parametrize("lane", ["0", "1"])
def test_a_handed_members_state_is_never_used_hot(capi, oracle, monkeypatch, lane):
    """Cold solve with the state kept (on the 8-lane or on the lane-per-problem kernel), then a hot start on perturbed vectors,
    which always runs on the 8-lane kernel: a stiff member finds its block "not initialised", starts cold, is given up on and
    handed over again -- the oracle's COLD count on the new data; an ordinary member continues from its state -- the count the
    same sequence gives with the hand-over off."""
    probs, _ = cold_reference(oracle, 8, 2)
    rng = np.random.default_rng(78)
    p2 = [repin(problems.perturb(rng, q, 0.3)) for q in probs]
    out = {}
    for on in (False, True):
        b = make_batch(capi, monkeypatch, probs, lane, on)
        b.solve(capi.MODE_COLD, 1000)
        assert b.last_kernel() == (2 if lane == "1" else 1)
        b.set_vectors_from(p2)
        b.solve(capi.MODE_HOT_VECTORS, 1000)
        assert b.last_kernel() == 1
        out[on] = (b.results(), b.handover())
        b.close()
    (off, (_, count_off)), (res, (handed, count)) = out[False], out[True]
    assert count_off == 0
    assert np.array_equal(handed, is_stiff(len(probs)).astype(np.int32)) and count == int(is_stiff(len(probs)).sum())
    hot_differs = 0
    for t, (q, r, o) in enumerate(zip(p2, res, off)):
        qp, rc, n = oracle_cold(oracle, q)
        if t % EVERY == 0:
            assert rc == 0
            assert_same_solution(qp, r, n)
        else:
            assert r["status"] == o["status"] == 20 and r["nWSR"] == o["nWSR"], (t, r["nWSR"], o["nWSR"])
            assert np.array_equal(r["ws_b"], o["ws_b"]) and np.array_equal(r["ws_c"], o["ws_c"])
            assert np.abs(r["x"] - o["x"]).max() <= RTOL * max(1.0, np.abs(o["x"]).max())
            assert np.abs(r["y"] - o["y"]).max() <= RTOL * max(1.0, np.abs(o["y"]).max())
            hot_differs += r["nWSR"] != n
    assert hot_differs > 0          # (the ordinary members did continue from a state: a cold start takes another count)


def test_sitters_are_untouched(capi, oracle, monkeypatch):
    """Two batches run the same three optimizeQP calls: everybody (hand-over off: the stiff members end with ret = 4); every fifth
    member sitting out, new vectors for the others -- on batch A with the hand-over ON; everybody again, new vectors, hand-over off.
    A member that sat out call 2 on A -- stiff ones with their stale ret = 4 among them -- keeps x, y, working sets, status and count
    bit for bit, is not flagged, and in call 3 does exactly what its twin on B does (its stored state was not touched)."""
    probs, _ = cold_reference(oracle, 8, 2)
    n = len(probs)
    rng = np.random.default_rng(79)
    p2 = [repin(problems.perturb(rng, q, 0.2)) for q in probs]
    p3 = [repin(problems.perturb(rng, q, 0.2)) for q in p2]
    take = (np.arange(n) % 5 != 0).astype(np.int32)
    stiff = is_stiff(n)
    assert (stiff & (take == 0)).sum() >= 3
    A = make_batch(capi, monkeypatch, probs, "0", False)
    B = make_batch(capi, monkeypatch, probs, "0", False)
    for b in (A, B):
        b.optimize_qp()
    before = A.results()
    assert all(before[t]["status"] != 20 for t in range(n) if stiff[t])
    A.set_handover(True)
    for b in (A, B):
        b.set_members(take)
        b.set_vectors_from(p2, members=take)
    usedA, usedB = A.optimize_qp(), B.optimize_qp()
    after, twin = A.results(), B.results()
    handed, count = A.handover()
    mode, _ = A.dispatch()
    assert np.array_equal(handed, (stiff & (take != 0)).astype(np.int32)) and count == int((stiff & (take != 0)).sum())
    for t in range(n):
        r, o = after[t], before[t]
        if not take[t]:
            assert usedA[t] == 0 and mode[t] == -1
            assert r["status"] == o["status"] and r["nWSR"] == o["nWSR"] and r["obj"] == o["obj"]
            for f in ("x", "y", "ws_b", "ws_c"):
                assert np.array_equal(r[f], o[f]), (t, f)
        elif stiff[t]:
            qp, rc, nn = oracle_cold(oracle, p2[t])
            assert rc == 0 and usedA[t] == nn
            assert_same_solution(qp, r, nn)
        else:
            w = twin[t]
            assert r["status"] == w["status"] == 20 and usedA[t] == usedB[t]
            for f in ("x", "y", "ws_b", "ws_c"):
                assert np.array_equal(r[f], w[f]), (t, f)
    A.set_handover(False)
    for b in (A, B):
        b.set_members(None)
        b.set_vectors_from(p3)
    usedA, usedB = A.optimize_qp(), B.optimize_qp()
    handed, count = A.handover()
    assert count == 0 and not handed.any()
    ma, mb = A.dispatch()[0], B.dispatch()[0]
    for t, (r, w) in enumerate(zip(A.results(), B.results())):
        if take[t]:
            continue
        assert ma[t] == mb[t] and usedA[t] == usedB[t] and r["status"] == w["status"], (t, ma[t], mb[t], usedA[t], usedB[t])
        for f in ("x", "y", "ws_b", "ws_c"):
            assert np.array_equal(r[f], w[f]), (t, f)
    A.close(); B.close()
