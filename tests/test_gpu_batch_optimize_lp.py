"""optimizeLP per member of a batch (rsqp_batch_optimize_lp): reference src/qpOASESInterface.cpp:227-284 and the LP branch of
handle_error (:688-717) for every member of an rsqp_batch, each in its own state, decided on the device.

Reference of every comparison: the CPU oracle, driven by lp_batch_ref.LPRef -- a restatement of rsqp_optimize_lp over
oracle.OracleQP. Members: continuous random LPs (non-degenerate: every solved member sits on a vertex, so its working set is unique),
plus members with inconsistent constraint bounds. Three batches, one per kernel family an LP call can run on; the six-step sequence
puts their members into different states within one call. x, y and the objective are compared within 1e-8 * max(1, |.|_inf), the
tolerance test_gpu_parity.test_optimize_lp uses for the x of an LP."""
import numpy as np
import pytest

from restartsqp_amd import problems
import lp_batch_ref as R
from lp_batch_ref import LPRef, STEP_KIND, FULL_BUDGET_FROM, assert_member

pytestmark = pytest.mark.gpu

KERNEL = {"tiny": 0, "mid": 0, "hbm": 3}     # LP calls stay off the tableau kernels: LDS-resident null-space kernels, or HBM-resident


def upload(b, members, matrices):
    if matrices:
        b.set_matrix_values(np.concatenate([q.A_val for q in members] + [np.zeros(0)]), None)
    b.set_vectors_from(members)


def check_step(tag, b, rows, used):
    """every member of one call against the oracle rows (all mismatches are shown together); returns the members with exit flag 20
    whose certificate does not pass"""
    mode, rescue = b.dispatch()
    res = b.results()
    ok, kkt = b.test_optimality()
    print("%s: sum nWSR_used %d (oracle %d)" % (tag, int(used.sum()), sum(o["used"] for o in rows)))
    wrong, uncertified = [], []
    for q in range(b.nq):
        try:
            assert_member(tag + (q,), res[q], rows[q], used[q], mode[q], rescue[q])
        except AssertionError as e:
            wrong.append(str(e).splitlines()[0])
        if res[q]["status"] == 20 and ok[q] != 1:
            uncertified.append(tag + (q, float(kkt[q])))
    assert not wrong, wrong
    return uncertified


@pytest.mark.parametrize("name", ["tiny", "mid", "hbm"])
def test_six_step_sequence_matches_the_oracle_and_is_certified(capi, oracle, name):
    """every member, every step: exit flag, nWSR_used, (mode, rescue) and raw working sets equal to LPRef, x, y and the objective
    within 1e-8; the certificate (H absent, no regVal term) passes for every member whose exit flag is 20. `mid` carries a random SPD
    H, which an LP call ignores."""
    steps, budget, sums, ora = R.oracle_run(oracle, name)
    R.assert_inputs_cover_the_branches(name, sums, ora)
    b = capi.Batch(steps[0])
    b.set_options(lp_maxiter=budget)
    uncertified = []
    for k, (kind, members, rows) in enumerate(zip(STEP_KIND, steps, ora)):
        if k == FULL_BUDGET_FROM:
            b.set_options(lp_maxiter=1000)
        if k > 0:
            upload(b, members, kind == "newA")
        used = b.optimize_lp()
        assert b.last_kernel() == KERNEL[name]
        uncertified += check_step((name, k + 1), b, rows, used)
    b.close()
    assert not uncertified, uncertified


@pytest.mark.parametrize("name", ["tiny", "mid", "hbm"])
def test_batch_members_match_single_handles(capi, name):
    """the same sequences through nq single handles (rsqp_optimize_lp): flag, nWSR_used and working sets equal, x and y within 1e-8
    (a handle and a batch member may run different builds of one engine, and a handle beyond the LDS fit runs the engine of
    qp_large.hip: bit-identity is not asked for). Measured before rsqp_optimize_lp left the register-resident tableau kernel: on
    `tiny` the handle's x was up to 9.1e-4 and its y up to 1.1e-6 off the oracle's, the batch member's 5.2e-12 and 6.0e-15."""
    steps, budget, sums = R.sequence(name)
    b = capi.Batch(steps[0])
    b.set_options(lp_maxiter=budget)
    hs = []
    for q in steps[0]:
        s = capi.Solver(q.nV, q.nC)
        s.set_options(lp_maxiter=budget)
        hs.append(s)
    for k, (kind, members) in enumerate(zip(STEP_KIND, steps)):
        if k == FULL_BUDGET_FROM:
            b.set_options(lp_maxiter=1000)
        if k > 0:
            upload(b, members, kind == "newA")
        used = b.optimize_lp()
        res = b.results()
        wrong = []
        for q, (s, m) in enumerate(zip(hs, members)):
            if k == FULL_BUDGET_FROM:
                s.set_options(lp_maxiter=1000)
            if k == 0 or kind == "newA":
                s.set_A_csc(m.A_jc, m.A_ir, m.A_val)
            if k == 0 and m.H_val.size:
                s.set_H_csc(m.H_jc, m.H_ir, m.H_val)
            for w, v in zip(range(5), (m.g, m.lb, m.ub, m.lbA, m.ubA)):
                s.set_vector(w, v)
            n = s.optimize_lp()
            r = res[q]
            wb, wc = s.working_set_raw()
            xs, ys = max(1.0, np.abs(s.x).max()), max(1.0, np.abs(s.y).max())
            same = (r["status"] == s.status and int(used[q]) == n and np.array_equal(r["ws_b"], wb) and np.array_equal(r["ws_c"], wc) and
                    np.abs(s.x - r["x"]).max() <= R.TOL * xs and np.abs(s.y - r["y"]).max() <= R.TOL * ys)
            if not same:
                wrong.append((name, k + 1, q, r["status"], s.status, int(used[q]), n, float(np.abs(s.x - r["x"]).max() / xs),
                              float(np.abs(s.y - r["y"]).max() / ys)))
        assert not wrong, wrong
    b.close()


def test_gradient_pool_is_restored(capi, oracle):
    """the proximal step solves on g - regVal x in a scratch pool: a second LP call with nothing uploaded again is a hot start on the
    SAME vectors for every member whose first LP is solved, as it is for LPRef"""
    steps, budget, sums = R.sequence("tiny")
    members = steps[0]
    refs = [LPRef(oracle, q, 1000) for q in members]
    b = capi.Batch(members)
    b.set_options(lp_maxiter=1000)
    for call in range(2):
        rows = [R.row_of(r, r.optimize(q), q) for r, q in zip(refs, members)]
        assert any(o["mode"] == call for o in rows)
        used = b.optimize_lp()
        assert not check_step(("same-vectors", call + 1), b, rows, used)
    b.close()


def test_qp_and_lp_calls_alternate(capi, oracle):
    """optimize_qp, optimize_lp, optimize_qp on one batch with SPD Hessians: the first call of the other kind starts every member
    over (all cold), and each call matches its reference -- Ref of test_gpu_batch_optimize for the QPs, LPRef for the LP"""
    from test_gpu_batch_optimize import Ref, MODES, RESCUES
    steps, budget, sums = R.sequence("mid")
    b = capi.Batch(steps[0])
    b.set_options(qp_maxiter=1000, lp_maxiter=1000)
    for call, members in enumerate((steps[0], steps[1], steps[0])):      # (one A: the matrices are never refreshed)
        if call > 0:
            b.set_vectors_from(members)
        if call == 1:
            refs = [LPRef(oracle, q, 1000) for q in members]
            rows = [R.row_of(r, r.optimize(q), q) for r, q in zip(refs, members)]
            used = b.optimize_lp()
        else:
            rows = []
            for q in members:
                r = Ref(oracle, q, 1000)
                n = r.optimize(q)
                resc = [e for e in r.log if e.startswith("rescue")]
                rows.append(dict(used=n, mode=MODES[r.log[0]], rescue=RESCUES[resc[0] if resc else None], flag=r.qp.exitflag(),
                                 x=r.qp.x, y=r.qp.y, ws_b=r.qp.ws_bounds, ws_c=r.qp.ws_constraints))
            used = b.optimize_qp()
        assert all(o["mode"] == 0 for o in rows)
        assert not check_step(("alternate", call + 1), b, rows, used)
    b.close()


def test_a_batch_without_state_refuses_optimize_lp(capi):
    members = R.sequence("tiny")[0][0][:4]
    b = capi.Batch(members)
    b.set_keep_state(False)
    with pytest.raises(capi.RsqpError) as e:
        b.optimize_lp()
    assert e.value.code == capi.ERR_ARG
    b.close()


def test_one_pattern_batch(capi, oracle):
    """70 members of ONE pattern (an 8 x 2 LP and its perturbations): the kernels of such a batch take sizes, offsets and -- on the
    tableau kernels -- H and hreg from batch-wide values; an LP call needs them per member. First call cold, second hot on new
    vectors, every member against the oracle."""
    first, second = R.one_pattern_members()
    refs = [LPRef(oracle, q, 1000) for q in first]
    b = capi.Batch(first)
    b.set_options(lp_maxiter=1000)
    for call, members in enumerate((first, second)):
        if call > 0:
            b.set_vectors_from(members)
        rows = [R.row_of(r, r.optimize(q), q) for r, q in zip(refs, members)]
        assert all(o["mode"] == call and o["solved"] and R.is_vertex(o) for o in rows)
        used = b.optimize_lp()
        assert b.last_kernel() == 0
        assert not check_step(("one-pattern", call + 1), b, rows, used)
    b.close()
