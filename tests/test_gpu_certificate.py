"""The device KKT certificate on points that are NOT optimal, against the long-double reference tests/kkt_ref.py (which
tests/test_certificate_reference.py checks against the oracle on the CPU).

A: points injected through rsqp_batch_set_results -- every branch of the shared code (rsqp_kkt.h, kkt_body, small_certificate_kernel).
B: points the API can reach -- iteration limits and data changed behind a solve -- on every certificate path of the single handle
   (fused into tiny_qp_kernel, speculative small_certificate_kernel, fresh launch, synchronous path, SpMV products + kkt_kernel) and
   of the batch (one batch per kernel family, the LP switch).

Bit-exact where the data makes it possible and for every discrete output; elsewhere within kkt_ref.bound, 2^-52 (n_terms + k_max + 4)
M_field. Every test prints its worst observed error / bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kkt_cases as K
import kkt_ref as R
from conftest import ROOT
from restartsqp_amd import problems

pytestmark = pytest.mark.gpu

NOT_OPTIMAL = 1.0e-5      # ten times the verdict's threshold: a case that must say "no" is at least this far from optimal


# ------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------
def compare(tag, ref, ok, values, Wb=None, Wc=None, exact=False):
    """one certificate against its reference; returns the worst error / bound over the five fields"""
    assert int(ok) == ref.ok, (tag, int(ok), ref.ok, values, ref.values)
    if Wb is not None:
        assert np.array_equal(Wb, ref.W_b), (tag, "W_b", Wb, ref.W_b)
    if Wc is not None:
        assert np.array_equal(Wc, ref.W_c), (tag, "W_c", Wc, ref.W_c)
    worst = 0.0
    for k, f in enumerate(R.FIELDS):
        if exact:
            assert values[k] == ref.values[k], (tag, f, values[k], ref.values[k])
            continue
        err, bnd = abs(float(R.LD(values[k]) - ref.fields[f])), R.bound(ref, f)
        assert err <= bnd, (tag, f, values[k], ref.values[k], err, bnd)
        worst = max(worst, err / bnd if bnd > 0.0 else 0.0)
    return worst


def guarded_reference(tag, q, x, y, ws_b, ws_c, lp=False, must_fail=False):
    """the reference of a point, with the threshold guard asserted (never a row dropped)"""
    ref = R.of_problem(q, x, y, ws_b, ws_c, lp=lp)
    m = R.guard_of_problem(q, ref, x, ws_b, ws_c)
    assert m > 1.0, (tag, "a row sits within 1e-10 of the threshold of the working-set mapping", m)
    if must_fail:
        assert ref.ok == 0 and float(ref.fields["KKT_error"]) > NOT_OPTIMAL, (tag, ref.values)
    return ref


def inject(b, cases):
    cat = lambda name, dt: np.concatenate([np.asarray(getattr(c, name), dt) for c in cases] + [np.zeros(0, dt)])
    b.set_results(cat("x", np.float64), cat("y", np.float64), cat("ws_b", np.int32), cat("ws_c", np.int32))


def batch_certificates(b):
    ok, val = b.certificates()
    W = b.mapped_working_sets()
    return ok, val, W


def check_batch(tag, b, cases, refs=None, exact=False):
    """inject the cases' points and compare every member with its own reference"""
    inject(b, cases)
    ok, val, W = batch_certificates(b)
    refs = refs or [R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c) for c in cases]
    worst = 0.0
    for k, (c, ref) in enumerate(zip(cases, refs)):
        worst = max(worst, compare("%s member %d (%s)" % (tag, k, c.q.name), ref, ok[k], val[k], W[k][0], W[k][1], exact=exact))
    return worst


# ------------------------------------------------------------------------------------
# A. injected points, batch certificate
# ------------------------------------------------------------------------------------
def test_a1_exact_data_gives_the_reference_to_the_last_bit(capi):
    cases = K.exact_cases()
    refs = [R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c) for c in cases]
    tally = {}
    for ref in refs:
        assert ref.ok == 0
        for k, v in ref.tally.items():
            tally[k] = tally.get(k, 0.0) + float(v)
    # every branch of map_bound, map_constr and kkt_terms contributes, on bounds and on constraints
    assert len(tally) == 20 and all(v > 0.0 for v in tally.values()), tally
    # the threshold probes are among the rows: distances 0, 2^-27, 2^-26 on both kinds, a negative one on a constraint
    db = np.concatenate([np.abs(c.x - np.where(c.ws_b == 1, c.q.lb, c.q.ub))[c.ws_b != 0] for c in cases])
    dc = np.concatenate([(np.asarray(r.Ax, np.float64) - np.where(c.ws_c == 1, c.q.lbA, c.q.ubA))[c.ws_c != 0] for c, r in zip(cases, refs)])
    for d in (0.0, 2.0 ** -27, 2.0 ** -26):
        assert (db == d).any() and (dc == d).any(), d
    assert (dc == -2.0 ** -27).any() and (dc == -0.5).any()
    b = capi.Batch([c.q for c in cases])
    check_batch("A1", b, cases, refs, exact=True)
    b.close()
    # and each case alone: nq = 1 is the launch shape of the single handle's LDS-scale certificate
    for c, ref in zip(cases[:5], refs):
        b = capi.Batch([c.q])
        check_batch("A1 alone", b, [c], [ref], exact=True)
        b.close()


def test_a2_one_violated_entry_wherever_it_sits(capi):
    """256 x 256, 257 x 255, 300 x 511, 511 x 300: one violated entry in each wave of the workgroup, in the first and the second pass
    of the strided loops and at the last index. The field is that one term, every other field exactly zero"""
    rng = np.random.default_rng(20261023)
    bases = [K.satisfied_qp(rng, nV, nC) for nV, nC in K.ONE_HOT_SHAPES]
    b = capi.Batch([c.q for c in bases])
    inject(b, bases)
    ok, val = b.certificates()
    assert ok.tolist() == [1] * len(bases) and not val.any()
    ncase = 0
    for kind in K.ONE_HOT_KINDS:
        sizes = [c.q.nC if kind.endswith("_c") else c.q.nV for c in bases]
        pos = [K.one_hot_positions(n) for n in sizes]
        for r in range(max(len(p) for p in pos)):
            hot = [K.one_hot(c, kind, p[min(r, len(p) - 1)]) for c, p in zip(bases, pos)]
            cases = [h[0] for h in hot]
            b.set_vectors_from([c.q for c in cases])
            inject(b, cases)
            ok, val = b.certificates()
            for k, (c, field, term) in enumerate(hot):
                want = np.zeros(5)
                want[field] = want[4] = term
                assert ok[k] == 0 and np.array_equal(val[k], want), (kind, c.q.name, pos[k][min(r, len(pos[k]) - 1)], val[k], want)
                assert np.array_equal(R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c).values, want), (kind, c.q.name)
                ncase += 1
    b.close()
    print("A2: %d one-hot cases, all exact" % ncase)


def test_a3_members_read_their_own_slices(capi):
    """a mixed batch whose members' violations are powers of ten apart, in both orders"""
    cases = K.real_cases()
    worst = 0.0
    for order in (cases, cases[::-1]):
        b = capi.Batch([c.q for c in order])
        worst = max(worst, check_batch("A3", b, order))
        b.close()
    dual = [float(R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c).fields["dual_violation"]) for c in cases]
    assert dual[-1] > 1.0e4 * max(dual[:4]) > 0.0, dual        # a neighbour's slice would swamp a small member's fields
    print("A3: %d members x 2 orders, worst error / bound = %.3f" % (len(cases), worst))


@pytest.mark.parametrize("where,entry", [("ws_b", 2), ("ws_c", -7)])
def test_a4_invalid_working_set(capi, where, entry):
    cases = K.real_cases()
    refs = [R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c) for c in cases]
    b = capi.Batch([c.q for c in cases])
    worst = 0.0
    for member, at in ((4, 0), (7, 0), (7, 280)):
        c = cases[member]
        bad = K.Case(c.q, c.x, c.y, c.ws_b.copy(), c.ws_c.copy())
        getattr(bad, where)[at] = entry
        assert R.of_problem(bad.q, bad.x, bad.y, bad.ws_b, bad.ws_c).ok == R.ERR_WORKING_SET
        inject(b, cases[:member] + [bad] + cases[member + 1:])
        ok, val, W = batch_certificates(b)
        assert ok[member] == capi.ERR_WORKING_SET == R.ERR_WORKING_SET, (member, at, ok)
        # the mapped working set marks the entry, and that entry alone, as the header says (12345)
        ref_bad = R.of_problem(bad.q, bad.x, bad.y, bad.ws_b, bad.ws_c)
        assert np.array_equal(W[member][0], ref_bad.W_b) and np.array_equal(W[member][1], ref_bad.W_c), (member, at)
        assert W[member][0 if where == "ws_b" else 1][at] == R.INVALID == 12345
        assert sum(int((w == R.INVALID).sum()) for pair in W for w in pair) == 1
        for k, ref in enumerate(refs):
            if k != member:
                worst = max(worst, compare("A4 member %d beside an invalid one" % k, ref, ok[k], val[k], W[k][0], W[k][1]))
    b.close()
    print("A4 %s = %d: 3 placements, the other members' worst error / bound = %.3f" % (where, entry, worst))


def test_a5_random_real_data_and_a_fixed_summation_tree(capi):
    worst = 0.0
    for cases in (K.real_cases(), K.real_cases(spread=False, seed=20261022)):
        b = capi.Batch([c.q for c in cases])
        worst = max(worst, check_batch("A5", b, cases))
        ok1, val1 = b.certificates()
        ok2, val2 = b.certificates()
        assert val1.tobytes() == val2.tobytes() and ok1.tobytes() == ok2.tobytes()
        b.close()
    print("A5: worst error / bound = %.3f" % worst)


def test_a6_new_matrix_values_reach_both_products(capi):
    """after rsqp_batch_set_matrix_values the certificate of an injected point uses the new values in A x (the CSR copy) and in A'y
    (the CSC pool), and in H x"""
    cases = K.real_cases()
    fresh = [K.refreshed(c) for c in cases]
    b = capi.Batch([c.q for c in cases])
    worst = check_batch("A6 before", b, cases)
    b.set_matrix_values(np.concatenate([c.q.A_val for c in fresh]), np.concatenate([c.q.H_val for c in fresh]))
    refs = [R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c) for c in fresh]
    old = [R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c) for c in cases]
    for k in (3, 7):   # the refresh moves the primal term (A x) and the stationarity (A'y, H x) far beyond the bound
        assert abs(refs[k].values[0] - old[k].values[0]) > 1.0e-3 and abs(refs[k].values[3] - old[k].values[3]) > 1.0e-3
    worst = max(worst, check_batch("A6 after", b, fresh, refs))
    b.close()
    print("A6: worst error / bound = %.3f" % worst)


# ------------------------------------------------------------------------------------
# B. points the API can reach
# ------------------------------------------------------------------------------------
VECS = ("g", "lb", "ub", "lbA", "ubA")


def make_solver(capi, q, engine=None):
    s = capi.Solver(q.nV, q.nC)
    if engine is not None:
        s.set_engine(engine)
    if q.nC > 0:
        s.set_A_csc(q.A_jc, q.A_ir, q.A_val)
    s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
    for w, name in enumerate(VECS):
        s.set_vector(w, getattr(q, name))
    return s


def copy_of(q):
    from restartsqp_amd.qpdump import QPData
    return QPData(q.nV, q.nC, q.H_jc, q.H_ir, q.H_val.copy(), q.A_jc, q.A_ir, q.A_val.copy(), q.g.copy(), q.lb.copy(), q.ub.copy(),
                  q.lbA.copy(), q.ubA.copy(), name=q.name)


def solver_certificate(tag, s, q, must_fail=False, lp=False):
    """the handle's certificate of the point it holds against the reference on the data `q`; returns (ratio, raw bytes)"""
    x, y = s.x, s.y
    wb, wc = s.working_set_raw()
    ref = guarded_reference(tag, q, x, y, wb, wc, lp=lp, must_fail=must_fail)
    try:
        ok, st, Wc, Wb = s.test_optimality()
    except Exception as e:      # RSQP_ERR_WORKING_SET comes as an error of the call
        assert ref.invalid, (tag, e)
        return 0.0, b""
    val = np.array([getattr(st, f) for f in R.FIELDS])
    return compare(tag, ref, int(ok), val, Wb, Wc), val.tobytes() + Wb.tobytes() + Wc.tobytes()


def b_problems():
    """the single-handle problems of B1 / B2: name -> convex QP"""
    rng = np.random.default_rng(20261024)
    out = {"%dx%d" % (nV, nC): problems.random_qp(rng, nV, nC, density=0.7) for nV, nC in ((8, 2), (7, 4), (8, 8), (3, 0), (1, 1), (20, 12))}
    out["hs071"] = problems.hs071_first_qp()
    return out


def changes(q, s):
    """the changes of data behind a solve, each as (name, changed copy of q, how to apply it to a handle, whether the point cannot be
    optimal any more): shift g, raise one lb above x, move one ub onto x, raise one lbA above Ax of an upper-active row (row 0 where
    there is none), scale A's values by 1.25, and H's by 1.5"""
    x = s.x
    wb, wc = s.working_set_raw()
    out = []
    q2 = copy_of(q); q2.g = q.g + 0.5
    out.append(("shift g", q2, ("vector", 0), True))
    i = int(np.argmax(wb == 0)) if (wb == 0).any() else 0
    q2 = copy_of(q); q2.lb[i] = x[i] + 0.25
    out.append(("lb above x", q2, ("entries", (1, i)), True))
    q2 = copy_of(q); q2.ub[i] = x[i]
    out.append(("ub onto x", q2, ("entries", (2, i)), False))
    if q.nC > 0:
        r = int(np.argmax(wc == -1)) if (wc == -1).any() else 0
        Ax = q.dense_A() @ x
        q2 = copy_of(q); q2.lbA[r] = Ax[r] + 0.125
        out.append(("lbA above Ax", q2, ("entries", (3, r)), True))
        q2 = copy_of(q); q2.A_val = 1.25 * q.A_val
        out.append(("A scaled", q2, ("A",), bool((wc != 0).any())))
    q2 = copy_of(q); q2.H_val = 1.5 * q.H_val
    out.append(("H scaled", q2, ("H",), False))
    return out


def apply_change(s, q2, how, by_entry):
    if how[0] == "vector":
        s.set_vector(how[1], getattr(q2, VECS[how[1]]))
    elif how[0] == "entries":
        for w, i in how[1:]:
            if by_entry:
                s.set_entry(w, i, getattr(q2, VECS[w])[i])
            else:
                s.set_vector(w, getattr(q2, VECS[w]))
    elif how[0] == "A":
        s.set_A_csc(q2.A_jc, q2.A_ir, q2.A_val)
    else:
        s.set_H_csc(q2.H_jc, q2.H_ir, q2.H_val)


def limits_and_staleness(capi, tag, q, limits, engine=None, min_unfinished=1):
    """B1 / B2 / B3 on one problem: certificates at iteration limits, at the optimum, and behind every change of data"""
    worst, n, unfinished = 0.0, 0, 0
    for lim in limits:
        s = make_solver(capi, q, engine)
        s.solve(capi.MODE_COLD, lim)
        assert s.status in (20, 28), (tag, lim, s.status)
        short = s.status == 28
        unfinished += short
        r, _ = solver_certificate("%s limit %d" % (tag, lim), s, q, must_fail=short)
        worst, n = max(worst, r), n + 1
        # a second call takes the fresh-launch path on the same point: same answer
        r2, _ = solver_certificate("%s limit %d again" % (tag, lim), s, q, must_fail=short)
        worst, n = max(worst, r2), n + 1
        s.close()
    assert unfinished >= min_unfinished, (tag, "the limits did not stop the solve short", unfinished)
    s = make_solver(capi, q, engine)
    s.optimize_qp()
    assert s.status == 20, (tag, s.status)
    r, first = solver_certificate(tag + " solved", s, q)
    assert first and np.frombuffer(first[:40])[4] <= 1.0e-6, tag       # it says "optimal"
    # the certificate that came with the solve (fused or speculative) has been handed out: from here on every call is a fresh launch
    # of small_certificate_kernel. Where the first one was fused into tiny_qp_kernel that is another kernel: the same bytes
    r2, fresh = solver_certificate(tag + " solved, fresh launch", s, q)
    assert fresh == first, (tag, "a fresh launch does not give the certificate that came with the solve",
                            np.frombuffer(first[:40]), np.frombuffer(fresh[:40]))
    worst, n = max(worst, r, r2), n + 2
    for by_entry in (False, True):
        for name, q2, how, must in changes(q, s):
            if by_entry and how[0] != "entries":
                continue
            apply_change(s, q2, how, by_entry)
            r, _ = solver_certificate("%s after '%s' (%s)" % (tag, name, "set_entry" if by_entry else "set_vector"), s, q2, must_fail=must)
            worst, n = max(worst, r), n + 1
            apply_change(s, q, how, by_entry)
            r, again = solver_certificate("%s '%s' restored" % (tag, name), s, q)
            assert again == first, (tag, name, "the restored data does not give the first certificate again",
                                    np.frombuffer(again[:40]), np.frombuffer(first[:40]))
            worst, n = max(worst, r), n + 1
    # a change BEHIND a solve whose certificate has not been asked for yet: the one launched with the solve is stale, a fresh launch is due
    for by_entry in (False, True):
        for name, q2, how, must in changes(q, s):
            if not must or by_entry != (how[0] == "entries"):
                continue
            s.optimize_qp()
            assert s.status == 20, (tag, s.status)
            apply_change(s, q2, how, by_entry)
            r, _ = solver_certificate("%s '%s' right behind the solve" % (tag, name), s, q2, must_fail=True)
            worst, n = max(worst, r), n + 1
            apply_change(s, q, how, by_entry)
    s.close()
    return worst, n


FIRST_AGAIN = {"fused": ("8x2", None), "fused hs071": ("hs071", None), "speculative": ("20x12", None), "speculative Givens": ("8x2", "0")}


@pytest.mark.parametrize("path", sorted(FIRST_AGAIN))
def test_b3_restored_data_gives_the_first_certificate_again(capi, monkeypatch, path):
    """solve, certify (the certificate that came with the solve), shift g, certify ("not optimal"), restore g, certify: the last
    certificate equals the FIRST one byte for byte, fields and working sets, although another kernel formed it -- the first is the one
    fused into tiny_qp_kernel ("fused") or the speculative small_certificate_kernel behind the solve, the last a fresh
    small_certificate_kernel. limits_and_staleness asserts the same for every change on every B1 / B2 handle; this is the property by
    itself, with both certificates printed"""
    for k in ("RSQP_SMALL_ENGINE", "RSQP_NO_SPIN"):
        monkeypatch.delenv(k, raising=False)
    name, engine = FIRST_AGAIN[path]
    if engine is not None:
        monkeypatch.setenv("RSQP_SMALL_ENGINE", engine)
    q = b_problems()[name]
    s = make_solver(capi, q)
    s.optimize_qp()
    assert s.status == 20
    _, first = solver_certificate("B3 %s first" % path, s, q)
    q2 = copy_of(q); q2.g = q.g + 0.5
    s.set_vector(0, q2.g)
    solver_certificate("B3 %s changed" % path, s, q2, must_fail=True)
    s.set_vector(0, q.g)
    _, again = solver_certificate("B3 %s restored" % path, s, q)
    s.close()
    print("B3 %s: first" % path, np.frombuffer(first[:40]), "restored", np.frombuffer(again[:40]))
    assert again[40:] == first[40:], (path, "working sets differ")
    assert again == first, (path, np.frombuffer(first[:40]), np.frombuffer(again[:40]))


def unsolvable():
    """(name, problem, status): inconsistent bounds, infeasible in the homotopy, unbounded (the constructions of
    test_gpu_parity.test_batch_edge_cases)"""
    from restartsqp_amd.qpdump import QPData, dense_to_csc
    rng = np.random.default_rng(11)
    q = problems.random_qp(rng, 5, 3); q.lbA[:] = 5.0; q.ubA[:] = 4.0
    out = [("inconsistent bounds", q, 22)]
    out.append(("infeasible", QPData(2, 1, *dense_to_csc(np.eye(2)), *dense_to_csc(np.array([[1.0, 1.0]])), np.zeros(2), -np.ones(2),
                                     np.ones(2), np.array([3.0]), np.array([np.inf]), name="infeasible"), 22))
    out.append(("unbounded", QPData(2, 0, *dense_to_csc(np.diag([1.0, -1.0])), *dense_to_csc(np.zeros((0, 2))), np.array([0.0, -1.0]),
                                    np.array([-1.0, 0.0]), np.array([1.0, np.inf]), np.zeros(0), np.zeros(0), name="unbounded"), 23))
    return out


def test_b1_certificate_fused_into_the_tableau_kernel(capi, monkeypatch):
    for k in ("RSQP_SMALL_ENGINE", "RSQP_NO_SPIN"):
        monkeypatch.delenv(k, raising=False)
    P = b_problems()
    worst, n = 0.0, 0
    for name in ("hs071", "8x2", "7x4", "8x8", "3x0", "1x1"):
        w, k = limits_and_staleness(capi, "B1 " + name, P[name], (0, 1, 2), min_unfinished=0 if name in ("3x0", "1x1") else 1)
        worst, n = max(worst, w), n + k
    for name, q, status in unsolvable():
        s = make_solver(capi, q)
        s.solve(capi.MODE_COLD, 1000)
        assert s.status == status, (name, s.status)
        r, _ = solver_certificate("B1 " + name, s, q)
        worst, n = max(worst, r), n + 1
        s.close()
    print("B1/B3 fused certificate: %d cases, worst error / bound = %.3f" % (n, worst))


def test_b2_speculative_certificate_behind_the_solve(capi, monkeypatch):
    monkeypatch.delenv("RSQP_NO_SPIN", raising=False)
    monkeypatch.delenv("RSQP_SMALL_ENGINE", raising=False)
    P = b_problems()
    worst, n = limits_and_staleness(capi, "B2 20x12", P["20x12"], (0, 1, 2, 3))
    monkeypatch.setenv("RSQP_SMALL_ENGINE", "0")      # read when the handle is created: off the tableau kernel
    for name in ("8x2", "hs071"):
        w, k = limits_and_staleness(capi, "B2 %s Givens" % name, P[name], (0, 1, 2, 3))
        worst, n = max(worst, w), n + k
    print("B2/B3 speculative certificate: %d cases, worst error / bound = %.3f" % (n, worst))


def synchronous_path_body(capi):
    """what tests/checks/certificate_no_spin.py runs in a process of its own: one B1 and one B2 problem through
    limits_and_staleness"""
    P = b_problems()
    worst, n = 0.0, 0
    for name, lim in (("8x2", (0, 1, 2)), ("20x12", (0, 1, 3))):
        w, k = limits_and_staleness(capi, "B4 " + name, P[name], lim)
        worst, n = max(worst, w), n + k
    return worst, n


def test_b4_synchronous_path():
    """RSQP_NO_SPIN=1 (read once per process, hence the child process): no doorbell, no fused and no speculative certificate -- every
    certificate is a launch followed by a blocking wait. One B1 and one B2 problem"""
    env = dict(os.environ, RSQP_NO_SPIN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "certificate_no_spin.py")], capture_output=True, text=True,
                       timeout=60, env=env, cwd=ROOT)
    assert r.returncode == 0 and "B4 synchronous path" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
    print([l for l in r.stdout.splitlines() if l.startswith("B4")])


def test_b5_spmv_products_then_kkt_kernel(capi):
    """set_engine(2): three SpMV launches and kkt_kernel. 300 x 520 has more than 256 variables and two passes of constraints"""
    rng = np.random.default_rng(20261025)
    worst, n = 0.0, 0
    for nV, nC, dens in ((40, 50, 0.5), (300, 520, 0.05), (30, 0, 0.0)):
        q = problems.random_qp(rng, nV, nC, density=dens)
        s = make_solver(capi, q, engine=2)
        s.solve(capi.MODE_COLD, 3)
        assert s.status == 28, (nV, nC, s.status)
        r, _ = solver_certificate("B5 %dx%d limit 3" % (nV, nC), s, q, must_fail=True)
        worst, n = max(worst, r), n + 1
        for by_entry in (False, True):
            for name, q2, how, must in changes(q, s):
                if by_entry and how[0] != "entries":
                    continue
                apply_change(s, q2, how, by_entry)
                r, _ = solver_certificate("B5 %dx%d after '%s'" % (nV, nC, name), s, q2, must_fail=True)
                worst, n = max(worst, r), n + 1
                apply_change(s, q, how, by_entry)
        s.close()
    print("B5 SpMV + kkt_kernel: %d cases, worst error / bound = %.3f" % (n, worst))


def batch_family_case(capi, monkeypatch, name):
    import small_builds as S
    for k in S.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if name == "lane":
        monkeypatch.setenv("RSQP_LANE", "1")
        return problems.hs071_scale_batch(64), lambda b: b.last_kernel() == 2
    if name == "tiny":
        return S.mixed(2061, 67, 8, 2), lambda b: b.last_kernel() == 1 and capi.plan_builds(b.last_plan())[0][0] == "tiny"
    if name == "mid":
        return S.mixed(1112, 5, 40, 14, one_var=False, no_con=False), lambda b: capi.plan_builds(b.last_plan())[0][0] == "qpg"
    if name == "lds":
        monkeypatch.setenv("RSQP_SMALL_ENGINE", "0")
        return S.mixed(2062, 37, 8, 8), lambda b: b.last_kernel() == 0
    return [problems.random_qp(np.random.default_rng(20261026), 120, 100, density=0.1)], lambda b: b.last_kernel() == 3


@pytest.mark.parametrize("family", ["lane", "tiny", "mid", "lds", "hbm"])
def test_b6_batch_kernels_at_iteration_limits(capi, monkeypatch, family):
    probs, ran = batch_family_case(capi, monkeypatch, family)
    b = capi.Batch(probs)
    if family == "lane":
        b.set_keep_state(False)
    worst, n, unfinished = 0.0, 0, 0
    for lim in (0, 1, 3):
        b.solve(capi.MODE_COLD, lim)
        assert ran(b), (family, b.last_kernel(), b.last_plan())
        res = b.results()
        ok, val, W = batch_certificates(b)
        for k, (q, r) in enumerate(zip(probs, res)):
            tag = "B6 %s limit %d member %d" % (family, lim, k)
            ref = guarded_reference(tag, q, r["x"], r["y"], r["ws_b"], r["ws_c"], must_fail=r["status"] == 28)
            unfinished += r["status"] == 28
            worst, n = max(worst, compare(tag, ref, ok[k], val[k], W[k][0], W[k][1])), n + 1
    assert unfinished >= len(probs), (family, unfinished)       # the limits do stop solves short
    b.close()
    print("B6 %s: %d certificates (%d of unfinished solves), worst error / bound = %.3f" % (family, n, unfinished, worst))


def test_b7_lp_calls_certify_the_lp(capi):
    """behind rsqp_batch_optimize_lp and rsqp_optimize_lp the certificate is the reference's WITHOUT H; behind a following optimize_qp
    on the same batch it is the reference's with H"""
    import lp_batch_ref as L
    steps, budget, sums = L.sequence("mid")
    probs = steps[0][:6]
    assert all(len(q.H_val) > 0 for q in probs)
    b = capi.Batch(probs)
    b.set_options(lp_maxiter=1000)
    b.optimize_lp()
    worst, n = 0.0, 0
    for lp in (True, False):
        if not lp:
            b.optimize_qp()
        res = b.results()
        ok, val, W = batch_certificates(b)
        for k, (q, r) in enumerate(zip(probs, res)):
            tag = "B7 batch %s member %d" % ("LP" if lp else "QP", k)
            ref = guarded_reference(tag, q, r["x"], r["y"], r["ws_b"], r["ws_c"], lp=lp)
            other = R.of_problem(q, r["x"], r["y"], r["ws_b"], r["ws_c"], lp=not lp)
            # the two references differ by H x, far beyond the bound: the comparison tells them apart
            assert abs(float(ref.fields["stationarity_violation"] - other.fields["stationarity_violation"])) > 1.0e-3, tag
            worst, n = max(worst, compare(tag, ref, ok[k], val[k], W[k][0], W[k][1])), n + 1
    b.close()
    for engine in (None, 2):      # the LDS-scale certificate, and the SpMV products + kkt_kernel
        for q in probs[:2]:
            s = make_solver(capi, q, engine)
            s.set_options(1000, 1000)
            s.optimize_lp()
            assert s.status == 20, (q.name, engine, s.status)
            r, _ = solver_certificate("B7 handle LP %s engine %s" % (q.name, engine), s, q, lp=True)
            worst, n = max(worst, r), n + 1
            s.close()
    # a handle beyond the LDS fit (three SpMV launches + kkt_kernel) with an H the LP ignores
    rng = np.random.default_rng(20261027)
    q = L.random_lp(rng, 120, 40, H=L.spd(rng, 120), name="lp120x40")
    s = make_solver(capi, q)
    s.set_options(1000, 1000)
    s.optimize_lp()
    assert s.status == 20 and s.large_path() >= 0, (s.status, s.large_path())     # solved, and on the HBM-resident engine
    r, _ = solver_certificate("B7 handle LP 120x40 (HBM-resident engine)", s, q, lp=True)
    worst, n = max(worst, r), n + 1
    s.close()
    print("B7 LP switch: %d certificates, worst error / bound = %.3f" % (n, worst))
