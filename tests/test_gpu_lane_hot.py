"""Hot starts on new vectors (mode 1) on the lane-per-problem kernel's WARM builds of level 2 (csrc/qp_lane.hip,
rsqp_batch_set_lane_hot beside rsqp_batch_set_lane_warm), against the CPU oracle and against the same sequence with both switches
off, where the 8-lane kernel runs these calls.

Bar as everywhere: status, nWSR and both working sets exact, x / y / objective within 1e-9 relative, against the oracle's init /
hotstart / hotstart_matrices (one OracleQP per member); against the switch-off run status, nWSR and working sets equal, for every
member of every step. Batches have 131-200 members (two or three full waves and a ragged tail) under RSQP_LANE=1; the inputs and
the oracle's answers are tests/lane_hot_cases.py's, computed once (tests/test_lane_hot_inputs.py asserts what they hold).
"""
import numpy as np
import pytest

import lane_hot_cases as C
from lane_cases import RTOL, assert_same_solution
from restartsqp_amd import problems
from test_gpu_batch_optimize import Ref, assert_member, MODES, RESCUES

pytestmark = pytest.mark.gpu

ON, WARM_ONLY, OFF = (True, True), (True, False), (False, False)


def batch(capi, monkeypatch, probs, switches):
    monkeypatch.setenv("RSQP_LANE", "1")            # (read by rsqp_batch_create)
    b = capi.Batch(probs)
    assert b.lane_hot() is False and b.lane_warm() is False          # off is the default
    switch(b, switches)
    return b


def switch(b, switches):
    warm, hot = switches
    b.set_lane_warm(warm); b.set_lane_hot(hot)
    assert b.lane_warm() is bool(warm) and b.lane_hot() is bool(hot)


def upload(b, members, matrices):
    if matrices:
        b.set_matrix_values(np.concatenate([q.A_val for q in members]), np.concatenate([q.H_val for q in members]))
    b.set_vectors_from(members)


def assert_same_path(tag, a, c):
    """status, nWSR and both working sets equal (the switch-on run against the switch-off run)"""
    assert a["status"] == c["status"] and a["nWSR"] == c["nWSR"], (tag, a["status"], c["status"], a["nWSR"], c["nWSR"])
    assert np.array_equal(a["ws_b"], c["ws_b"]) and np.array_equal(a["ws_c"], c["ws_c"]), tag


def assert_against_oracle(tag, ans, r):
    """every member, solved or not: status, nWSR, working sets exact, x / y / objective within RTOL"""
    try:
        assert_same_solution(ans, r, ans.n)
    except AssertionError as e:
        raise AssertionError("%r: status %d (oracle %d) nWSR %d (oracle %d): %s" % (tag, r["status"], ans.flag, r["nWSR"], ans.n, e))
    if ans.solved:
        assert abs(r["obj"] - ans.objective) <= RTOL * max(1.0, abs(ans.objective)), tag


def run_steps(capi, monkeypatch, steps, modes, switches, limits=None):
    """the call sequence `modes` on the members of `steps`: (results, last_kernel, last_plan) per step. switches: (lane_warm,
    lane_hot) for the whole run, or one pair per step"""
    per_step = switches if isinstance(switches, list) else [switches] * len(steps)
    b = batch(capi, monkeypatch, steps[0], per_step[0])
    out = []
    for k, (members, mode) in enumerate(zip(steps, modes)):
        if k > 0:
            switch(b, per_step[k])
            upload(b, members, mode == capi.MODE_HOT_MATRICES)
        b.solve(mode, limits[k] if limits else 1000)
        out.append((b.results(), b.last_kernel(), b.last_plan()))
    b.close()
    return out


def compare(capi, monkeypatch, steps, modes, ora, switches, kernels, limits=None):
    """a run with `switches` against the oracle's answers `ora` and against both switches off, every member of every step; returns
    the results per step"""
    on = run_steps(capi, monkeypatch, steps, modes, switches, limits)
    off = run_steps(capi, monkeypatch, steps, modes, OFF, limits)
    assert [k for _, k, _ in on] == kernels
    assert [k for _, k, _ in off] == [2 if m == capi.MODE_COLD else 1 for m in modes]
    for k, plan in enumerate(p for _, _, p in on):
        assert plan["family"] == kernels[k] and plan["mode"] == modes[k]
        if kernels[k] == 2:
            assert plan["keep"] == 1 and plan["mc"] == 2
    for k, row in enumerate(ora):
        for m, (ans, r, t) in enumerate(zip(row, on[k][0], off[k][0])):
            assert_against_oracle((k, m), ans, r)
            assert_same_path((k, m), r, t)
    return [r for r, _, _ in on]


@pytest.mark.parametrize("rel", C.RELS)
@pytest.mark.parametrize("shape", C.SHAPES)
def test_steady_state(capi, oracle, monkeypatch, shape, rel):
    """1: cold -> new vectors -> new vectors -> new matrices -> new vectors. Both switches on: every call on the lane kernel; lane_warm
    alone: the new-matrices call only; both off: the cold start only. Every new-vectors step holds members that change no working
    set and members that change it (1 x 2 at 0.02: nothing changes); the 1 x 2 batch also holds members whose previous QP ended
    infeasible, which continue from where that stopped. (6, 1): with free variables, which enter S in the set-up."""
    steps, modes, ora = C.steady_steps(shape, rel), C.modes_of(capi), C.steady_oracle(oracle, shape, rel)
    res = compare(capi, monkeypatch, steps, modes, ora, ON, [2, 2, 2, 2, 2])
    assert [k for _, k, _ in run_steps(capi, monkeypatch, steps, modes, WARM_ONLY)] == [2, 1, 1, 2, 1]
    for k, kind in enumerate(C.KINDS):
        if kind == "vectors" and (shape, rel) != ((1, 2), 0.02):
            assert sum(r["nWSR"] == 0 for r in res[k]) > 0 and sum(r["nWSR"] > 0 for r in res[k]) > 0, k
    if shape == (1, 2) and rel == 0.3:
        assert [sum(r["status"] == capi.QPERROR_INFEASIBLE for r in rows) for rows in res[:2]] == [8, 70]


def test_the_state_both_ways(capi, oracle, monkeypatch):
    """2: (a) cold and two new-vectors steps on the lane kernel, then lane_hot off and a third step on the 8-lane kernel from the state
    the mode-1 launch wrote; (b) cold and one step with the switches off, then on: a step on the lane kernel from a state
    tiny_qp_kernel wrote. From a wrong tableau or slot state either would take another path than the oracle."""
    steps, ora = C.steady_steps((8, 2), 0.3), C.steady_oracle(oracle, (8, 2), 0.3)
    kinds = C.KINDS[:3] + ("vectors",)
    modes = C.modes_of(capi, kinds)
    # (step 4 of the steady sequence brings matrices; here its vectors alone are uploaded, on the matrices of step 1)
    rng = np.random.default_rng(9900)
    steps4 = steps[:3] + [C.new_vectors(rng, steps[2], 0.3)]
    ora4 = C.oracle_sequence(oracle, steps4, kinds)
    res = compare(capi, monkeypatch, steps4, modes, ora4, [ON, ON, ON, WARM_ONLY], [2, 2, 2, 1])
    assert sum(r["nWSR"] > 0 for r in res[3]) > 0
    res = compare(capi, monkeypatch, steps[:3], modes[:3], ora[:3], [OFF, OFF, ON], [2, 1, 2])
    assert sum(r["nWSR"] > 0 for r in res[2]) > 0 and sum(r["nWSR"] == 0 for r in res[2]) > 0


def test_patterns_of_their_own(capi, oracle, monkeypatch):
    """3: members of one shape whose sparsity patterns differ: every lane walks the CSC arrays of its own problem (the build without
    the one pattern), the sequence of test 1"""
    steps, modes, ora = C.own_pattern_steps(), C.modes_of(capi), C.own_pattern_oracle(oracle)
    first = run_steps(capi, monkeypatch, steps[:1], modes[:1], ON)
    assert first[0][2]["uni"] == 0 and first[0][2]["hb"] == 8
    res = compare(capi, monkeypatch, steps, modes, ora, ON, [2, 2, 2, 2, 2])
    for k in (1, 2, 4):
        assert sum(r["nWSR"] == 0 for r in res[k]) > 0 and sum(r["nWSR"] > 0 for r in res[k]) > 0, k


@pytest.mark.parametrize("shape,limit,stopped_members", [((6, 1), 1, 150), ((4, 2), 3, 82)])
def test_a_first_launch_stopped_by_its_iteration_limit(capi, oracle, monkeypatch, shape, limit, stopped_members):
    """4a: a cold start under an iteration limit of 1 (6 x 1: it stops every member, which needs 5 or 6 changes; 4 x 2 under a limit
    of 3: stopped and solved members share the waves), then a hot start on new vectors: the members the limit stopped continue
    from the middle of their homotopy (limits that are neither the old targets nor the new ones), as the oracle's hotstart behind
    an init that hit its limit does"""
    steps = C.steady_steps(shape, 0.3)[:2]
    kinds, limits = C.KINDS[:2], [limit, 1000]
    ora = C.oracle_sequence(oracle, steps, kinds, limits)
    stopped = [m for m, a in enumerate(ora[0]) if not a.solved]
    assert len(stopped) == stopped_members
    res = compare(capi, monkeypatch, steps, C.modes_of(capi, kinds), ora, ON, [2, 2], limits)
    assert all(res[0][m]["status"] != 20 and res[0][m]["nWSR"] == limit for m in stopped)
    assert sum(res[1][m]["status"] == 20 and res[1][m]["nWSR"] > 0 for m in stopped) > 0


def test_inconsistent_new_bounds(capi, oracle, monkeypatch):
    """4b: members whose new vectors have lb > ub on one variable: infeasible before any change, the stored x, y and working sets are
    kept, and the state block is what it was -- the next hot start on new vectors continues from it on either kernel"""
    rng = np.random.default_rng(9400)
    base = C.steady_steps((8, 2), 0.3)[0]
    second = C.new_vectors(rng, base, 0.3)
    inconsistent = list(range(3, len(base), 11))
    for m in inconsistent:
        second[m].lb = second[m].lb.copy(); second[m].lb[2] = second[m].ub[2] + 1.0
    steps = [base, second, C.new_vectors(rng, base, 0.3)]
    kinds = ("cold", "vectors", "vectors")
    ora = C.oracle_sequence(oracle, steps, kinds)
    for switches, kernels in ((ON, [2, 2, 2]), ([ON, ON, OFF], [2, 2, 1])):
        res = compare(capi, monkeypatch, steps, C.modes_of(capi, kinds), ora, switches, kernels)
        for m in inconsistent:
            first, kept = res[0][m], res[1][m]
            assert kept["status"] == capi.QPERROR_INFEASIBLE and kept["nWSR"] == 0
            assert np.array_equal(kept["x"], first["x"]) and np.array_equal(kept["y"], first["y"])
            assert np.array_equal(kept["ws_b"], first["ws_b"]) and np.array_equal(kept["ws_c"], first["ws_c"])
        assert sum(res[2][m]["status"] == 20 and res[2][m]["nWSR"] > 0 for m in inconsistent) > 0


# 5: what a call of the lockstep sequence brings: (kind, who is named by the per-member mark, who sits out)
CALLS = (("cold", None, None), ("vectors", None, None), ("values_of", 3, None), ("handler", 2, None), ("vectors", None, 4),
         ("vectors", None, None))


def handler_mats(rng, q):
    """new vectors, new entries of J (the columns of A in front of the slacks' identity blocks, which stay) and a rescaled H"""
    q = problems.perturb(rng, q, 0.05)
    nj = q.A_jc[q.nV - 2 * q.nC]
    q.A_val = q.A_val.copy(); q.A_val[:nj] = q.A_val[:nj] * (1.0 + 0.01 * rng.normal(size=nj)); q.H_val = q.H_val * 1.05
    return q


def test_optimize_qp_with_per_member_marks(capi, oracle, monkeypatch):
    """5: optimize_qp call by call on an hs071-shaped batch: cold; new vectors for everybody; set_matrix_values_of for every third
    member plus new vectors; handler_set_matrices with a word per member (every second) plus new vectors; a call that a quarter of
    the members sit out; a call everybody takes again. No call carries the batch-wide update mark. With both switches on the
    first solve of every call after the first runs on the lane kernel, with the words -1, 1, 2 and 3 sharing waves; with lane_warm
    alone, and with both off, on the 8-lane kernel. dispatch(), nWSR_used and the results against the oracle-driven restatement
    of rsqp_optimize_qp and equal to the switch-off run; a member that sits out keeps its results bit for bit, and its state block
    -- which no entry point exports -- shows in the last call, where it hot-starts from it."""
    rng = np.random.default_rng(9500)
    n = 140
    steps = [problems.hs071_scale_batch(n)]
    named = [np.zeros(n, bool)]
    for kind, every, _ in CALLS[1:]:
        mark = np.zeros(n, bool)
        if every:
            mark[1::every] = True
        named.append(mark)
        steps.append([handler_mats(rng, q) if mark[m] else problems.perturb(rng, q, 0.05) for m, q in enumerate(steps[-1])])
    runs = {}
    for switches in (ON, WARM_ONLY, OFF):
        b = batch(capi, monkeypatch, steps[0], switches)
        sN, sC = b._handler_sizes()
        b.handler_set_problem(np.full(sN, -np.inf), np.full(sN, np.inf), np.full(sC, -np.inf), np.full(sC, np.inf))
        rows = []
        for k, ((kind, every, sit), members) in enumerate(zip(CALLS, steps)):
            mask = np.ones(n, np.int32)
            if sit:
                mask[2::sit] = 0
            if k > 0:
                b.set_vectors_from(members)
            if kind == "values_of":
                b.set_matrix_values(np.concatenate([q.A_val for q in members]), np.concatenate([q.H_val for q in members]),
                                    members=named[k])
            elif kind == "handler":
                jac = np.concatenate([q.A_val[:q.A_jc[q.nV - 2 * q.nC]] for q in members])
                b.handler_set_matrices(np.where(named[k], capi.HM_JAC | capi.HM_HESS, 0), jac, np.concatenate([q.H_val for q in members]))
            b.set_members(mask if sit else None)
            used = b.optimize_qp()
            mode, rescue = b.dispatch()
            rows.append(dict(used=used, mode=mode, rescue=rescue, res=b.results(), kernel=b.last_kernel(), plan=b.last_plan(), mask=mask))
        runs[switches] = rows
        b.close()
    on, off = runs[ON], runs[OFF]
    assert [r["kernel"] for r in on] == [2] * len(CALLS)
    assert [r["plan"]["family"] for r in on] == [2] * len(CALLS)
    assert [r["kernel"] for r in runs[WARM_ONLY]] == [2] + [1] * (len(CALLS) - 1)
    assert [r["kernel"] for r in off] == [2] + [1] * (len(CALLS) - 1)
    refs = [Ref(oracle, q, 1000) for q in steps[0]]
    for k, (members, row, roff) in enumerate(zip(steps, on, off)):
        assert np.array_equal(row["mode"], roff["mode"]) and np.array_equal(row["rescue"], roff["rescue"])
        assert np.array_equal(row["used"], roff["used"])
        for m, (ref, q) in enumerate(zip(refs, members)):
            if named[k][m]:
                ref.set_mats(q)
            elif k > 0:
                assert np.array_equal(q.A_val, steps[k - 1][m].A_val)
            r = row["res"][m]
            assert_same_path((k, m), r, roff["res"][m])
            if not row["mask"][m]:
                assert row["mode"][m] == -1 and row["used"][m] == 0 and row["rescue"][m] == 0
                p = on[k - 1]["res"][m]              # untouched: what the call before left, bit for bit
                assert r["status"] == p["status"] and r["nWSR"] == p["nWSR"] and r["obj"] == p["obj"], (k, m)
                assert np.array_equal(r["x"], p["x"]) and np.array_equal(r["y"], p["y"]), (k, m)
                assert np.array_equal(r["ws_b"], p["ws_b"]) and np.array_equal(r["ws_c"], p["ws_c"]), (k, m)
                continue
            used = ref.optimize(q)
            resc = [e for e in ref.log if e.startswith("rescue")]
            o = dict(used=used, mode=MODES[ref.log[0]], rescue=RESCUES[resc[0] if resc else None], flag=ref.qp.exitflag(), x=ref.qp.x,
                     y=ref.qp.y, ws_b=ref.qp.ws_bounds, ws_c=ref.qp.ws_constraints)
            assert_member((k, m), r, o, row["used"][m], row["mode"][m], row["rescue"][m])
    # the words the lane kernel's launches carried
    assert set(on[1]["mode"]) == {1}
    assert set(on[2]["mode"]) == {1, 3} and set(on[3]["mode"]) == {1, 2, 3}
    assert {-1, 1} <= set(on[4]["mode"]) and int((on[4]["mode"] == -1).sum()) == len(range(2, n, 4))
    assert 1 in set(on[5]["mode"])
    assert sum(int(u) > 0 for u in on[5]["used"]) > 0


def test_calls_that_stay_on_the_eight_lane_kernel(capi, oracle, monkeypatch):
    """6: lane_hot without lane_warm changes nothing; with both on, a hot start on new vectors stays on the 8-lane kernel while the
    hand-over is on and in the call after it, and behind set_results (pools that are not the batch's own answer); so does
    optimize_lp. The answers are the oracle's throughout."""
    rng = np.random.default_rng(9600)
    steps = [C.steady_steps((8, 2), 0.3)[0]]
    for _ in range(8):
        steps.append(C.new_vectors(rng, steps[-1], 0.3))
    kinds = ("cold",) + ("vectors",) * 8
    ora = C.oracle_sequence(oracle, steps, kinds)
    # lane_hot alone
    for r, k, plan in run_steps(capi, monkeypatch, steps[:3], C.modes_of(capi, kinds[:3]), (False, True))[1:]:
        assert k == 1 and plan["family"] == 1
    b = batch(capi, monkeypatch, steps[0], ON)
    kernels = []
    for k, members in enumerate(steps):
        if k > 0:
            upload(b, members, False)
        if k == 2:
            b.set_handover(True)
        if k == 3:
            b.set_handover(False)
        if k == 6:
            r = b.results()
            b.set_results(x=np.concatenate([np.full_like(m["x"], 7.0) for m in r]), ws_b=np.concatenate([0 * m["ws_b"] for m in r]))
        b.solve(capi.MODE_COLD if k == 0 else capi.MODE_HOT_VECTORS, 1000)
        kernels.append(b.last_kernel())
        assert b.last_plan()["family"] == kernels[-1]
        for m, (ans, r) in enumerate(zip(ora[k], b.results())):
            assert_against_oracle((k, m), ans, r)
    b.close()
    assert kernels == [2, 2, 1, 1, 2, 2, 1, 2, 2]
    # optimize_lp: every launch carries per-member modes, none goes to the lane kernel, and the answers are the switch-off run's. (Its
    # launches never take the hs071-scale tableau kernels at all -- knobs_of(b, lp) sets no_tiny, family 0 with the switches on or
    # off --, so what "stays where it is" means here is: the kernel of the switch-off run, and not kernel 2)
    out = {}
    for switches in (ON, OFF):
        b = batch(capi, monkeypatch, problems.hs071_scale_batch(131), switches)
        b.solve(capi.MODE_COLD, 1000)
        assert b.last_kernel() == 2
        used = b.optimize_lp()
        out[switches] = (b.results(), used, b.last_kernel())
        b.close()
    assert out[ON][2] == out[OFF][2] != 2
    assert np.array_equal(out[ON][1], out[OFF][1])
    for r, t in zip(out[ON][0], out[OFF][0]):
        assert_same_path("lp", r, t)
        assert np.array_equal(r["x"], t["x"]) and np.array_equal(r["y"], t["y"])
