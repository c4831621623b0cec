"""Hot starts with new matrices (mode 2) and warm re-initialisations (mode 3) on the lane-per-problem kernel's WARM builds
(csrc/qp_lane.hip, rsqp_batch_set_lane_warm), against the CPU oracle and against the same sequence with the switch off, where the
8-lane kernel runs these calls.

Bar as everywhere: status, nWSR and both working sets exact, x / y / objective within 1e-9 relative, against the oracle's
init(.., x0, y0, guess_b) / hotstart / hotstart_matrices; against the switch-off run status, nWSR and working sets equal. Batches have
131-200 members (two or three full waves and a ragged tail) under RSQP_LANE=1; the inputs are the generators of tests/lane_cases.py.
"""
import numpy as np
import pytest

from conftest import oracle_cold
from lane_cases import RTOL, assert_same_solution, one_pattern_batch, own_pattern_batch
from restartsqp_amd import problems
from test_gpu_batch_optimize import Ref, assert_member, MODES, RESCUES, newmats

pytestmark = pytest.mark.gpu


def batch(capi, monkeypatch, probs, warm):
    monkeypatch.setenv("RSQP_LANE", "1")            # (read by rsqp_batch_create)
    b = capi.Batch(probs)
    assert b.lane_warm() is False                   # off is the default
    b.set_lane_warm(warm)
    assert b.lane_warm() is bool(warm)
    return b


def upload(b, members, matrices):
    if matrices:
        b.set_matrix_values(np.concatenate([q.A_val for q in members]), np.concatenate([q.H_val for q in members]))
    b.set_vectors_from(members)


def new_vectors(rng, members):
    return [problems.perturb(rng, q, 0.3) for q in members]


def new_matrices(rng, members):
    out = new_vectors(rng, members)
    for q in out:
        q.A_val = q.A_val * (1.0 + 0.02 * rng.normal(size=q.A_val.shape))
    return out


def vecs(q):
    return q.g, q.lb, q.ub, q.lbA, q.ubA


def oracle_mats(qp, q):
    qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)


def assert_same_path(tag, a, c):
    """status, nWSR and both working sets equal (the switch-on run against the switch-off run)"""
    assert a["status"] == c["status"] and a["nWSR"] == c["nWSR"], (tag, a["status"], c["status"], a["nWSR"], c["nWSR"])
    assert np.array_equal(a["ws_b"], c["ws_b"]) and np.array_equal(a["ws_c"], c["ws_c"]), tag


def assert_against_oracle(tag, qp, r, n):
    """every member, solved or not: status, nWSR, working sets exact, x / y / objective within RTOL"""
    try:
        assert_same_solution(qp, r, n)
    except AssertionError as e:
        raise AssertionError("%r: status %d (oracle %d) nWSR %d (oracle %d): %s" % (tag, r["status"], qp.exitflag(), r["nWSR"], n, e))
    if qp.is_solved():              # (status 20 or 22, where assert_oracle_answer is for 20 alone)
        assert abs(r["obj"] - qp.objective) <= RTOL * max(1.0, abs(qp.objective)), tag


def run_steps(capi, monkeypatch, steps, modes, warm, limits=None):
    """the call sequence `modes` on the members of `steps`: (results, last_kernel, last_plan) per step"""
    b = batch(capi, monkeypatch, steps[0], warm)
    out = []
    for k, (members, mode) in enumerate(zip(steps, modes)):
        if k > 0:
            upload(b, members, mode == capi.MODE_HOT_MATRICES)
        b.solve(mode, limits[k] if limits else 1000)
        out.append((b.results(), b.last_kernel(), b.last_plan()))
    b.close()
    return out


def oracle_steps(oracle, steps, modes, capi, limits=None):
    """the same sequence per member on the oracle: [step][member] = (qp, nWSR) -- one OracleQP per member, so a row is read before the next step runs"""
    qps = []
    for q in steps[0]:
        qp = oracle.OracleQP(q.nV, q.nC)
        oracle_mats(qp, q)
        qps.append(qp)
    for k, (members, mode) in enumerate(zip(steps, modes)):
        lim = limits[k] if limits else 1000
        row = []
        for qp, q in zip(qps, members):
            if mode == capi.MODE_COLD:
                rc, n = qp.init(*vecs(q), lim)
            elif mode == capi.MODE_HOT_VECTORS:
                rc, n = qp.hotstart(*vecs(q), lim)
            else:
                oracle_mats(qp, q)
                rc, n = qp.hotstart_matrices(*vecs(q), lim)
            row.append((qp, n))
        yield row


def compare_runs(capi, oracle, monkeypatch, steps, modes, kernels_on, limits=None):
    """switch on against the oracle and against switch off, every member of every step; returns the switch-on results per step"""
    on = run_steps(capi, monkeypatch, steps, modes, True, limits)
    off = run_steps(capi, monkeypatch, steps, modes, False, limits)
    assert [k for _, k, _ in on] == kernels_on
    assert [k for _, k, _ in off] == [2 if m == capi.MODE_COLD else 1 for m in modes]
    for k, plan in enumerate(p for _, _, p in on):
        assert plan["family"] == kernels_on[k] and plan["mode"] == modes[k]
        if kernels_on[k] == 2:
            assert plan["keep"] == 1 and plan["mc"] == 2
    for k, row in enumerate(oracle_steps(oracle, steps, modes, capi, limits)):
        for m, ((qp, n), r, t) in enumerate(zip(row, on[k][0], off[k][0])):
            assert_against_oracle((k, m), qp, r, n)
            assert_same_path((k, m), r, t)
    return [r for r, _, _ in on]


@pytest.mark.parametrize("shape", [(8, 2), (6, 1), (4, 2), (8, 0), (1, 2)])
def test_new_matrices_new_vectors_new_matrices(capi, oracle, monkeypatch, shape):
    """(a) cold -> new matrices -> new vectors -> new matrices with the switch on: kernels 2, 2, 1, 2. The hot start on new vectors
    runs on the 8-lane kernel FROM the state the warm build wrote: from a wrong tableau or slot state it would take another path.
    (6, 1): with free variables, which enter S in the set-up."""
    nV, nC = shape
    rng = np.random.default_rng(7000 + 10 * nV + nC)
    steps = [one_pattern_batch(rng, nV, nC, 150, free=(nV == 6))]
    steps.append(new_matrices(rng, steps[-1]))
    steps.append(new_vectors(rng, steps[-1]))
    steps.append(new_matrices(rng, steps[-1]))
    modes = [capi.MODE_COLD, capi.MODE_HOT_MATRICES, capi.MODE_HOT_VECTORS, capi.MODE_HOT_MATRICES]
    res = compare_runs(capi, oracle, monkeypatch, steps, modes, [2, 2, 1, 2])
    hot_changes = sum(r["nWSR"] for rows in res[1:] for r in rows)
    assert hot_changes > 0
    assert sum(r["nWSR"] for r in res[1]) > 0 and sum(r["nWSR"] for r in res[3]) > 0


@pytest.mark.parametrize("shape", [(8, 2), (6, 1)])
def test_warm_reinitialisation(capi, oracle, monkeypatch, shape):
    """(b) set_warm_start with (x0, y0, guess_b), x0 alone, y0 alone, nothing -> MODE_WARM_REINIT on the lane kernel, against
    OracleQP.init(.., x0, y0, guess_b). The guess is the solution of the unperturbed members."""
    nV, nC = shape
    rng = np.random.default_rng(7100 + 10 * nV + nC)
    base = one_pattern_batch(rng, nV, nC, 140, free=(nV == 6))
    members = [problems.perturb(rng, q, 0.05) for q in base]
    runs = {}
    for warm in (True, False):
        b = batch(capi, monkeypatch, base, warm)
        b.solve(capi.MODE_COLD, 1000)
        assert b.last_kernel() == 2
        first = b.results()
        b.set_vectors_from(members)
        x0 = np.concatenate([r["x"] for r in first]); y0 = np.concatenate([r["y"] for r in first])
        gb = np.concatenate([r["ws_b"] for r in first])
        rows = []
        for given in ((x0, y0, gb), (x0, None, None), (None, y0, None), (None, None, None)):
            b.set_warm_start(*given)
            b.solve(capi.MODE_WARM_REINIT, 1000)
            assert b.last_kernel() == (2 if warm else 1)
            plan = b.last_plan()
            assert plan["mode"] == capi.MODE_WARM_REINIT and plan["family"] == (2 if warm else 1)
            rows.append(b.results())
        runs[warm] = (first, rows)
        b.close()
    first, rows = runs[True]
    for g, given in enumerate(((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 0))):
        for m, (q, f, r, t) in enumerate(zip(members, first, rows[g], runs[False][1][g])):
            qp = oracle.OracleQP(q.nV, q.nC)
            oracle_mats(qp, q)
            rc, n = qp.init(*vecs(q), 1000, x0=f["x"] if given[0] else None, y0=f["y"] if given[1] else None,
                            guess_b=f["ws_b"] if given[2] else None)
            assert_against_oracle((given, m), qp, r, n)
            assert_same_path((given, m), r, t)


def test_members_that_end_differently(capi, oracle, monkeypatch):
    """(c) one batch, one hot start with new matrices -- without an iteration limit and, from the same cold start, under a limit
    of 3, below what half of the members need (the infeasible ones among them) --, members that end differently: infeasible
    constraints; inconsistent bounds (the stored iterate is kept); a guess with a free variable that has lost its curvature and its
    column of A, so that no active constraint pairs with it (no positive definite reduced Hessian: the cold set-up in that lane);
    members that need more than 3 changes, and members that are solved."""
    rng = np.random.default_rng(7200)
    base = one_pattern_batch(rng, 6, 2, 160)
    nxt = new_matrices(rng, base)
    cold = [oracle_cold(oracle, q)[0] for q in base]
    infeasible = set(range(0, 160, 7))
    inconsistent = set(range(3, 160, 11)) - infeasible
    # a free variable j of the stored answer: row and column j of the new H and column j of the new A are zero (the patterns stay)
    flat = {}
    for m, qp in enumerate(cold):
        fr = np.flatnonzero(np.asarray(qp.ws_bounds) == 0)
        if m not in infeasible and m not in inconsistent and len(fr) and m % 5 == 1:
            flat[m] = int(fr[0])
    assert len(flat) >= 12
    for m, q in enumerate(nxt):
        if m in infeasible:
            q.lbA = q.ubA + 50.0; q.ubA = q.lbA + 1.0                     # far from the box
        if m in inconsistent:
            q.lb = q.lb.copy(); q.lb[2] = q.ub[2] + 1.0
        if m in flat:
            H = q.dense_H(); j = flat[m]
            H[j, :] = 0.0; H[:, j] = 0.0
            pattern = base[0].dense_H() != 0.0
            assert pattern.all()                                          # (a dense H: the entries keep their places)
            q.H_val = H.T[pattern.T].copy()
            assert np.array_equal(q.dense_H(), H)
            q.A_val = q.A_val.copy(); q.A_val[q.A_jc[j]:q.A_jc[j + 1]] = 0.0
    steps, modes = [base, nxt], [capi.MODE_COLD, capi.MODE_HOT_MATRICES]
    for limit in (1000, 3):
        first, second = compare_runs(capi, oracle, monkeypatch, steps, modes, [2, 2], [1000, limit])
        for m in inconsistent:
            assert second[m]["status"] == capi.QPERROR_INFEASIBLE and second[m]["nWSR"] == 0
            assert np.array_equal(second[m]["x"], first[m]["x"]) and np.array_equal(second[m]["ws_b"], first[m]["ws_b"])
        others = [second[m] for m in range(160) if m not in infeasible and m not in inconsistent]
        if limit == 1000:
            assert all(second[m]["status"] == capi.QPERROR_INFEASIBLE and second[m]["nWSR"] > 3 for m in infeasible)
            assert all(r["status"] in (20, capi.QPERROR_INFEASIBLE) for r in others) and sum(r["status"] == 20 for r in others) > 100
            assert sum(r["nWSR"] > 3 for r in others) > 0
            # the fallback: such a member takes the changes of the cold start on its new data, and ends where that ends
            for m in flat:
                qc, rc, nc = oracle_cold(oracle, nxt[m])
                assert second[m]["nWSR"] == nc and nc > 3, (m, second[m]["nWSR"], nc)
                assert_against_oracle(("cold", m), qc, second[m], nc)
        else:
            assert all(second[m]["status"] not in (20, capi.QPERROR_INFEASIBLE) and second[m]["nWSR"] == 3 for m in infeasible)
            assert sum(r["status"] == 20 for r in others) > 0 and sum(r["status"] != 20 and r["nWSR"] == 3 for r in others) > 0


@pytest.mark.parametrize("shape", [(8, 2), (5, 1)])
def test_one_shape_with_patterns_of_their_own(capi, oracle, monkeypatch, shape):
    """(d) members of one shape whose sparsity patterns differ: every lane walks the CSC arrays of its own problem (the build
    without the one pattern). cold -> new matrices -> new vectors -> new matrices"""
    nV, nC = shape
    rng = np.random.default_rng(7300 + 10 * nV + nC)
    steps = [own_pattern_batch(rng, nV, nC, 197)]
    steps.append(new_matrices(rng, steps[-1]))
    steps.append(new_vectors(rng, steps[-1]))
    steps.append(new_matrices(rng, steps[-1]))
    modes = [capi.MODE_COLD, capi.MODE_HOT_MATRICES, capi.MODE_HOT_VECTORS, capi.MODE_HOT_MATRICES]
    on = run_steps(capi, monkeypatch, steps[:1], modes[:1], True)
    assert on[0][2]["uni"] == 0 and on[0][2]["hb"] == 8
    res = compare_runs(capi, oracle, monkeypatch, steps, modes, [2, 2, 1, 2])
    assert sum(r["nWSR"] for r in res[1]) > 0


# (e): what a call of the lockstep sequence brings, and who sits out of it
CALLS = (("cold", None), ("matrices", 5), ("vectors", None), ("matrices", 3), ("vectors", None), ("vectors", None), ("matrices", 4))


def test_optimize_qp_in_lockstep(capi, oracle, monkeypatch):
    """(e) optimize_qp call by call. Call 1 is the uniform cold launch. Calls 2 and 4 follow set_matrix_values with every 5th / 3rd
    member sitting out and member 9 infeasible since call 1 (its first QP never solved: it starts cold every time): the words -1,
    0 and 2 share a wave of the lane kernel. Calls 3, 5 and 6 bring vectors only and stay on the 8-lane kernel (flips and hot starts
    on new vectors). Call 7 follows set_matrix_values with members that were FIXED in call 6: the flip, mode 3, on the lane kernel.
    dispatch(), nWSR_used and the results against the oracle-driven restatement of rsqp_optimize_qp; a member that sits out keeps
    its results bit for bit; the switch-off run takes the same decisions on the 8-lane kernel."""
    rng = np.random.default_rng(7400)
    n, bad = 140, 9
    base = one_pattern_batch(rng, 8, 2, n)

    def spoil(members):             # lbA[1] > ubA[1]: infeasible before any change, in every call
        members[bad].lbA = members[bad].lbA.copy(); members[bad].lbA[1] = members[bad].ubA[1] + 1.0
        return members

    steps = [spoil(base)]
    for kind, _ in CALLS[1:]:
        prev = steps[-1]
        steps.append(spoil([newmats(rng, q) for q in prev] if kind == "matrices" else [problems.perturb(rng, q, 0.05) for q in prev]))
    runs = {}
    for warm in (True, False):
        b = batch(capi, monkeypatch, steps[0], warm)
        rows = []
        for k, ((kind, every), members) in enumerate(zip(CALLS, steps)):
            mask = np.ones(n, np.int32)
            if every:
                mask[1::every] = 0
                mask[bad] = 1
            if k > 0:
                upload(b, members, kind == "matrices")
            b.set_members(mask if every else None)
            used = b.optimize_qp()
            mode, rescue = b.dispatch()
            rows.append(dict(used=used, mode=mode, rescue=rescue, res=b.results(), kernel=b.last_kernel(), plan=b.last_plan(), mask=mask))
        runs[warm] = rows
        b.close()
    on, off = runs[True], runs[False]
    assert [r["kernel"] for r in on] == [2, 2, 1, 2, 1, 1, 2]
    assert [r["kernel"] for r in off] == [2, 1, 1, 1, 1, 1, 1]
    refs = [Ref(oracle, q, 1000) for q in steps[0]]
    seen = set()
    for k, ((kind, every), members, row, roff) in enumerate(zip(CALLS, steps, on, off)):
        assert np.array_equal(row["mode"], roff["mode"]) and np.array_equal(row["rescue"], roff["rescue"])
        assert np.array_equal(row["used"], roff["used"])
        for m, (ref, q) in enumerate(zip(refs, members)):
            if kind == "matrices":
                ref.set_mats(q)
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
            if row["kernel"] == 2:
                seen.add((k, int(row["mode"][m])))
    # the words the lane kernel's launches carried (a member that sits out: -1)
    assert {(1, 0), (1, 2), (3, 0), (3, 2), (6, 0), (6, 3)} <= seen
    assert int((on[1]["mode"] == -1).sum()) > 0 and on[1]["mode"][bad] == 0 and on[1]["rescue"][bad] == 2
    assert int((on[6]["mode"] == 3).sum()) > 0


def test_calls_that_stay_on_the_eight_lane_kernel(capi, oracle, monkeypatch):
    """(f) with the switch on: result pools that set_results has overwritten are not the batch's own answer -- the next hot start
    with new matrices reads the stored state, on the 8-lane kernel, and the one after it is back on the lane kernel; with the
    hand-over on, these calls stay on the 8-lane kernel (and so does the call after it is switched off). The answers are the
    oracle's throughout."""
    rng = np.random.default_rng(7500)
    steps = [one_pattern_batch(rng, 8, 2, 131)]
    for _ in range(6):
        steps.append(new_matrices(rng, steps[-1]))
    b = batch(capi, monkeypatch, steps[0], True)
    qps = []
    for q in steps[0]:
        qp = oracle.OracleQP(q.nV, q.nC)
        oracle_mats(qp, q)
        qps.append(qp)
    kernels = []
    for k, members in enumerate(steps):
        if k > 0:
            upload(b, members, True)
        if k == 2:
            r = b.results()
            b.set_results(x=np.concatenate([np.full_like(m["x"], 7.0) for m in r]), ws_b=np.concatenate([0 * m["ws_b"] for m in r]))
        if k == 4:
            b.set_handover(True)
        if k == 5:
            b.set_handover(False)
        b.solve(capi.MODE_COLD if k == 0 else capi.MODE_HOT_MATRICES, 1000)
        kernels.append(b.last_kernel())
        assert b.last_plan()["family"] == kernels[-1]
        for m, (qp, q, r) in enumerate(zip(qps, members, b.results())):
            if k == 0:
                rc, n = qp.init(*vecs(q), 1000)
            else:
                oracle_mats(qp, q)
                rc, n = qp.hotstart_matrices(*vecs(q), 1000)
            assert_against_oracle((k, m), qp, r, n)
    b.close()
    assert kernels == [2, 2, 1, 2, 1, 1, 2]
