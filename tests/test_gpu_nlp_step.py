"""The decisions of a lock-step SQP loop per member of a batch on the device (rsqp_batch_handler_infeasibility / _ratio_test /
_check_optimality; restartsqp_amd/csrc/rsqp_batch_nlp.hip). Expected values come from handler.batch_ratio_test_reference and
handler.batch_check_optimality_reference, which tests/test_nlp_step_args.py pins to the committed SQP traces on the CPU, never from
the library; conditions on the inputs (which branches and verdict bits occur) are asserted from the references alone."""
import dataclasses
import os

import numpy as np
import pytest

from restartsqp_amd import handler, problems
from restartsqp_amd.handler import batch_handler_reference, batch_matrices_reference

import test_gpu_batch_handler as GH
import test_gpu_batch_members as M
import test_gpu_matrix_forms as MF
from test_gpu_batch_handler import RAGGED, Fixture, cat, synthetic_nlp          # noqa: F401  (synthetic_nlp: what Fixture builds from)
from test_nlp_step_args import NLPS, effective_flags, word_flags

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
INT_FILL = -12345
BATCHES = {"ragged": (RAGGED + [(5, 35), (70, 3)], 51, False),      # G = 64; (70, 3): a wavefront-strided walk takes a second pass
           "one_shape": ([(4, 2)] * 13, 53, True),                  # G = 8, the last wavefront ragged; CSC rows out of order
           "wide": ([(12, 1)] * 9, 57, False)}                      # G = 8 with more variables than lanes
# bound pairs, cycled over the entries of every member: every class of classify_single_constraint, with the pairs closer than
# 1e-8, -inf / +inf, +-2e19 and exactly +-1e18 (the quirk: UNBOUNDED beside a finite partner)
PAIRS = [(-2.0, 3.0), (1.0, 1.0 + 5e-9), (-np.inf, np.inf), (-1.5, 2e19), (-2e19, 2.5), (-1.0, 1e18), (-1e18, 1.0), (-1.5, np.inf),
         (-np.inf, 2.5), (-2e19, 2e19), (-1e18, 1e18)]      # (the first nine hold every case: a batch of nine (n, 1) members sees them)
# what a member's point looks like: r random (nothing engineered), o optimal, and one violation below its tolerance alone
RECIPES = {"ragged": "1r24o8r_o", "one_shape": "r1248o_r1248o", "wide": "o1_248r1r"}      # _: word 0


def make_fixture(capi, key):
    shapes, seed, shuffled = BATCHES[key]
    f = Fixture(capi, shapes, seed)
    if shuffled:      # the same members with the entries of every column of A in a random order: the batch folds them
        rng = np.random.default_rng(seed + 1)
        qs = []
        for p in f.nlps:
            q = problems.handler_qp(p, name="synthetic")
            jc, ir, val = MF._transform(rng, "shuffle", q.nC, q.nV, q.A_jc, q.A_ir, q.A_val)
            qs.append(dataclasses.replace(q, A_jc=jc, A_ir=ir, A_val=val))
        assert any(np.any(np.diff(q.A_ir[q.A_jc[c]:q.A_jc[c + 1]]) < 0) for q in qs for c in range(q.nV))
        f.b.close()
        f.b = capi.Batch(qs)
        f.b.set_vectors(*f.state)
    f.key = key
    return f


@pytest.fixture(scope="module")
def fixtures(capi):
    made = {}

    def get(key):
        if key not in made:
            made[key] = make_fixture(capi, key)
        return made[key]
    yield get
    for f in made.values():
        f.b.close()


def dense_J(p):
    J = np.zeros((p["info"].nCon, p["info"].nVar))
    for r, c, v in zip(p["J"].RowIndex, p["J"].ColIndex, p["J"].MatVal):
        J[r - 1, c - 1] += v
    return J


# ---------------------------------------------------------------------------------------------------------------------------------
# check_optimality
# ---------------------------------------------------------------------------------------------------------------------------------
def kkt_case(f):
    """bounds with every class, a point and multipliers per member as its recipe says; everything a call and the reference need"""
    rng = np.random.default_rng(BATCHES[f.key][1] + 7)
    recipe = RECIPES[f.key]
    assert len(recipe) == len(f.n)
    xl, xu, cl, cu, xk, gr, ck, lx, lc, inf, what = ([] for _ in range(11))
    for q, (n, m, p, r) in enumerate(zip(f.n, f.m, f.nlps, recipe)):
        bv = [PAIRS[(i + q) % len(PAIRS)] for i in range(n)]
        bc = [PAIRS[(i + q) % len(PAIRS)] for i in range(m)]
        lo, up = np.array([b[0] for b in bv + bc]), np.array([b[1] for b in bv + bc])
        kind = [handler.classify_single_constraint(a, b) for a, b in zip(lo, up)]
        v = rng.normal(size=n + m)
        lam = rng.uniform(0.5, 2.0, n + m) * rng.choice([-1.0, 1.0], n + m)
        above, below = np.array([k == handler.BOUNDED_ABOVE for k in kind]), np.array([k == handler.BOUNDED_BELOW for k in kind])
        unb = np.array([k == handler.UNBOUNDED for k in kind])
        infea = rng.uniform(0.5, 2.0)
        wrong = np.where(above, np.abs(lam), np.where(below, -np.abs(lam), lam))      # the signs the bounds forbid
        if r == "o":                                    # nothing violated
            lam[:] = 0.0; infea = 0.0
        elif r == "8":                                  # (stationary below; dual infeasible)
            lam = wrong
        elif r == "1":                                    # the primal violation alone is below its tolerance
            lam, infea = wrong, 0.0
        elif r == "2":                                  # dual feasible: the signs the bounds allow
            lam = np.where(above, -np.abs(lam), np.where(below, np.abs(lam), lam))
        elif r == "4":                                  # complementary: at the bound where a multiplier stands, none on free entries
            v = np.where(above, up, np.where(below, lo, v))
            lam = np.where(unb, 0.0, np.where(above, np.abs(lam), np.where(below, -np.abs(lam), lam)))
        J = dense_J(p)
        grad = rng.normal(size=n)
        if r in "o8":                                   # stationary to rounding
            grad = (J * lam[n:, None]).sum(axis=0) + lam[:n] if m else lam[:n].copy()
        hide = (lambda a: np.full(np.shape(a), np.nan)) if r == "_" else (lambda a: np.asarray(a, dtype=np.float64))
        xl.append(lo[:n]); xu.append(up[:n]); cl.append(lo[n:]); cu.append(up[n:])
        xk.append(hide(v[:n])); ck.append(hide(v[n:])); gr.append(hide(grad)); inf.append(hide([infea]))
        lx.append(lam[:n]); lc.append(lam[n:]); what.append(0 if r == "_" else 1 + q)
    c = dict(x_l=cat(xl), x_u=cat(xu), c_l=cat(cl), c_u=cat(cu), x_k=cat(xk), grad=cat(gr), c_k=cat(ck), infea=cat(inf), lam_x=cat(lx),
             lam_c=cat(lc), what=np.array(what, np.int32), J=[dense_J(p) for p in f.nlps])
    # the result pools: x anything, y member by member bounds (lam_x, then the slacks' multipliers: anything) then constraints
    c["y"] = cat([np.concatenate([a, rng.normal(size=2 * m), b]) for a, b, m in zip(lx, lc, f.m)])
    c["x"] = rng.normal(size=int(f.b.offV[-1]))
    return c


def kkt_reference(capi, f, c):
    o = capi.NlpStepOptions().as_dict()
    return handler.batch_check_optimality_reference(o, c["what"], c["x_k"], c["grad"], c["c_k"], c["infea"], c["lam_x"], c["lam_c"], c["J"],
                                                    f.n, f.m, c["x_l"], c["x_u"], c["c_l"], c["c_u"])


def assert_kkt_inputs(capi, f, c, st, verdict):
    """conditions on the input, from the reference alone"""
    o = capi.NlpStepOptions().as_dict()
    tol = np.array([o[k] for k in ("opt_prim_fea_tol", "opt_dual_fea_tol", "opt_compl_tol", "opt_stat_tol")])
    act = c["what"] != 0
    assert np.all(np.abs(st[act, :4] - tol) > 1e-9), "a violation within 1e-9 of its tolerance"
    seen = set(verdict[act].tolist())
    assert {1, 2, 4, 8} <= seen and any(v & 16 for v in seen) and 0 in seen, seen
    assert (~act).sum() >= 1 and np.isnan(c["x_k"]).any()
    for lo, up in ((c["x_l"], c["x_u"]), (c["c_l"], c["c_u"])):
        kinds = {handler.classify_single_constraint(a, b) for a, b in zip(lo, up)}
        assert kinds == {handler.EQUAL, handler.BOUNDED, handler.BOUNDED_BELOW, handler.BOUNDED_ABOVE, handler.UNBOUNDED}
        assert np.any((up == 1e18) & np.isfinite(lo) & (lo > -1e18)) and np.any((lo == -1e18) & (up < 1e18))
        assert np.any(up == 2e19) and np.any(lo == -2e19) and np.any(np.isinf(lo)) and np.any(np.isinf(up))
        assert np.any((up - lo < 1e-8) & (up > lo))
    assert (c["lam_x"] > 0).any() and (c["lam_x"] < 0).any() and (c["lam_c"] > 0).any() and (c["lam_c"] < 0).any()


def run_kkt(capi, f, c, on_device=False):
    """the call with NaN-filled outputs; returns (status, verdict) as numpy arrays"""
    nq = len(f.n)
    f.b.handler_set_problem(c["x_l"], c["x_u"], c["c_l"], c["c_u"])
    reset_matrices(capi, f)
    f.b.set_results(x=c["x"], y=c["y"])
    out, verdict = np.full((nq, 5), np.nan), np.full(nq, INT_FILL, np.int32)
    args = [c["what"], c["x_k"], c["grad"], c["c_k"], c["infea"]]
    if on_device:
        import torch
        args = [torch.as_tensor(np.ascontiguousarray(a), device="cuda") for a in args]
        out, verdict = torch.as_tensor(out, device="cuda"), torch.as_tensor(verdict, device="cuda")
        torch.cuda.synchronize()
    f.b.handler_check_optimality(*args, on_device=on_device, out=out, verdict=verdict)
    return (out.cpu().numpy(), verdict.cpu().numpy()) if on_device else (out, verdict)


def check_kkt(capi, f):
    """Each violation within (k + 4) 2^-53 S of the reference's. k: the terms of its sum; S: the sum of the absolute values of all
    products that enter it. The terms themselves are the same float64 numbers on both sides (one product, or none, per term, no
    contraction), so only the order of the additions differs. Dual and complementarity: a sum of k terms in any order is within
    (k - 1) u S of the exact sum (each of the k - 1 additions has a relative error of at most u = 2^-53 on a partial sum of at most
    S, to first order), and the reference's long-double sum rounded to float64 within u S: (k + 4) u S holds with room for the
    second-order terms. Stationarity, n columns of m products each: a column's m + 1 additions are within (m + 1) u S_j of its exact
    value (S_j: the column's |J_ij lam_i|, |lam_x|, |grad|), the sum of the n absolute values adds (n - 1) u S, the final rounding
    u S: (m + n + 1) u S, and m + n + 1 <= k = m n + 2 n for n >= 1. primal_violation is infea itself and KKT_error is the sum of
    the four in the stated order: both bit for bit."""
    c = kkt_case(f)
    st, verdict, scale = kkt_reference(capi, f, c)
    assert_kkt_inputs(capi, f, c, st, verdict)
    out, got = run_kkt(capi, f, c)
    for q in range(len(f.n)):
        if c["what"][q] == 0:
            assert np.isnan(out[q]).all() and out[q].tobytes() == np.full(5, np.nan).tobytes() and got[q] == INT_FILL, q
            continue
        assert out[q, 0].tobytes() == st[q, 0].tobytes(), q
        for col, (k, S) in zip((1, 2, 3), scale[q]):
            err, bound = abs(out[q, col] - st[q, col]), (k + 4) * U * S
            print("%s member %d %s: %.17g, reference %.17g, |difference| %.3g, bound %.3g" %
                  (f.key, q, capi.Batch.CERTIFICATE_FIELDS[col], out[q, col], st[q, col], err, bound))
            assert err <= bound, (q, col, err, bound)
        assert out[q, 4].tobytes() == np.float64(out[q, 1] + out[q, 0] + out[q, 2] + out[q, 3]).tobytes(), q
        assert got[q] == verdict[q], (q, int(got[q]), int(verdict[q]))


def test_check_optimality_ragged_batch(capi, fixtures):
    """the seven ragged members, (5, 35) and (70, 3): a wavefront per member, the member of an entry by its descriptor"""
    f = fixtures("ragged")
    check_kkt(capi, f)
    assert f.b.nV.max() + f.b.nC.max() > 16


@pytest.mark.parametrize("key", ["one_shape", "wide"])
def test_check_optimality_one_pattern_batch(capi, fixtures, key):
    """13 members of (4, 2) created with the rows of every column of A out of order -- the canonical pool is what is read, through
    member 0's pattern -- and 9 members of (12, 1): eight lanes per member"""
    f = fixtures(key)
    assert f.b.nV.max() + f.b.nC.max() <= 16
    check_kkt(capi, f)


# ---------------------------------------------------------------------------------------------------------------------------------
# ratio test
# ---------------------------------------------------------------------------------------------------------------------------------
# per member: accept + Grow / Unchanged / Shrink; pred < 0: N accepted, Z "QP is not changed"; Reject + shrink; Too small; _ word 0
BRANCHES = {"ragged": "GUSRZT_NG", "one_shape": "GUSNZRT_GUSNZ", "wide": "GUSRNZT_G"}


def reset_matrices(capi, f):
    """the members' own J and H_k back into the pools (an earlier test may have left other values there)"""
    ps = f.b.problems
    f.b.handler_set_matrices([capi.HM_JAC | capi.HM_HESS] * len(ps), cat([p.A_val[:p.A_jc[n]] for p, n in zip(ps, f.n)]),
                             cat([p.H_val for p in ps]))


def solve_for_ratio(capi, f):
    """a real handler_update + optimize_qp, so that p, norm_p and the objective are the pools' own. Members of the branches N and
    Z get a c_k far outside its bounds: their QPs pay for slack, the objective is positive, and with infea_k = 0 pred < 0"""
    nq = len(f.n)
    f.b.handler_set_problem(*f.bounds)
    delta, rho, x_k, c_k, grad = GH.solvable_iterate(f)
    reset_matrices(capi, f)
    branch = list(BRANCHES[f.key])
    assert len(branch) == nq
    oC = 0
    for q, m in enumerate(f.m):
        cl, cu = f.bounds[2][oC:oC + m], f.bounds[3][oC:oC + m]
        if branch[q] in "NZ":
            assert m and (np.isfinite(cl).any() or np.isfinite(cu).any()), q
            c_k[oC:oC + m] = np.where(np.isfinite(cl), cl - 50.0, np.where(np.isfinite(cu), cu + 50.0, 0.0))
        oC += m
    f.b.handler_update([capi.HU_SET] * nq, delta, rho, x_k, c_k, grad=grad)
    f.b.set_members(None)
    f.b.optimize_qp()
    res = f.b.results()
    assert all(r["status"] == 20 for r in res), [r["status"] for r in res]
    return branch, x_k, c_k, np.array([r["obj"] for r in res]), f.b.handler_step()


def ratio_case(capi, f):
    """inputs per member that put it on its branch -- asserted from the reference alone -- and the reference's answer"""
    rng = np.random.default_rng(BATCHES[f.key][1] + 11)
    o = capi.NlpStepOptions(refresh_ubA=1)
    branch, x_k, c_k, obj, st = solve_for_ratio(capi, f)
    nq, G = len(f.n), handler.nlp_step_lanes(f.n, f.m)
    assert G == (8 if f.b.nV.max() + f.b.nC.max() <= 16 else 64)
    rho = rng.uniform(1.0, 4.0, nq)
    c_trial = cat([rng.normal(size=m) * 2.0 for m in f.m])
    infea_k, f_k, f_t, delta = np.zeros(nq), rng.normal(size=nq), np.zeros(nq), np.ones(nq)
    oC = 0
    for q, m in enumerate(f.m):
        Cc = slice(oC, oC + m); oC += m
        it = handler.cal_infea_reference(c_trial[Cc], f.bounds[2][Cc], f.bounds[3][Cc], G)
        infea_k[q] = 0.0 if branch[q] in "NZ" else rng.uniform(0.0, 1.0)
        pred = rho[q] * infea_k[q] - obj[q]
        target = dict(G=0.9 * pred, U=0.5 * pred, S=0.125 * pred, N=0.0, Z=0.125 * pred, R=-1.0 - abs(pred), T=-1.0 - abs(pred), _=0.0)[branch[q]]
        f_t[q] = f_k[q] + rho[q] * infea_k[q] - rho[q] * it - target
        delta[q] = dict(G=st["norm_p"][q], N=st["norm_p"][q], T=1.5e-16).get(branch[q], 3.0)
    what = np.array([0 if br == "_" else 3 + q for q, br in enumerate(branch)], np.int32)
    hide = lambda a, off: cat([np.full(off[q + 1] - off[q], np.nan) if what[q] == 0 else a[off[q]:off[q + 1]] for q in range(nq)])
    one, offN, offC = np.arange(nq + 1), np.concatenate([[0], np.cumsum(f.n)]), np.concatenate([[0], np.cumsum(f.m)])
    c = dict(what=what, rho=hide(rho, one), f_trial=hide(f_t, one), c_trial=hide(c_trial, offC), x_k=hide(x_k, offN), c_k=hide(c_k, offC),
             f_k=hide(f_k, one), infea_k=hide(infea_k, one), delta=hide(delta, one))
    ref = handler.batch_ratio_test_reference(o.as_dict(), what, c["rho"], c["f_trial"], c["c_trial"], c["x_k"], c["c_k"], c["f_k"], c["infea_k"],
                                             c["delta"], st["p"], st["norm_p"], obj, f.n, f.m, f.bounds[2], f.bounds[3])
    return o, c, ref, branch, st


def assert_ratio_inputs(capi, c, ref, branch):
    """all branches in one call, from the reference alone"""
    act = c["what"] != 0
    kinds = set()
    for q in np.flatnonzero(act):
        d = int(ref["delta"][q] > c["delta"][q]) - int(ref["delta"][q] < c["delta"][q])
        kinds.add((int(ref["accept"][q]), int(d), int(ref["exitflag"][q])))
        if branch[q] in "NZ":
            assert ref["pred_reduction"][q] < 0, (q, ref["pred_reduction"][q])
        if branch[q] == "Z":
            assert (ref["accept"][q], ref["hu_word"][q], ref["hm_word"][q]) == (0, 0, 0), q
    U_, T_ = capi.EXIT_UNKNOWN, capi.EXIT_TRUST_REGION_TOO_SMALL
    assert kinds >= {(1, 1, U_), (1, 0, U_), (1, -1, U_), (0, -1, U_), (0, -1, T_), (0, 0, U_)}, kinds
    assert (~act).sum() >= 1 and any(ref["accept"][q] and ref["pred_reduction"][q] < 0 for q in np.flatnonzero(act))


def run_ratio(capi, f, o, c, on_device=False):
    """the call with NaN / INT_FILL in every output; returns every in/out array and output as numpy arrays"""
    nq = len(f.n)
    io = {k: np.array(c[k], dtype=np.float64) for k in capi.NlpTrial.INOUT}
    out = {k: (np.full(nq, INT_FILL, np.int32) if k in capi.NlpTrial.INTS else np.full(nq, np.nan)) for k in capi.NlpTrial.OUT}
    ins = {k: c[k] for k in capi.NlpTrial.IN}
    if on_device:
        import torch
        dev = lambda d: {k: torch.as_tensor(np.ascontiguousarray(a), device="cuda") for k, a in d.items()}
        io, out, ins = dev(io), dev(out), dev(ins)
        torch.cuda.synchronize()
    got = f.b.handler_ratio_test(options=o, on_device=on_device, out=out, **ins, **io)
    assert all(got[k] is out[k] for k in out)
    every = dict(io, **out)
    return {k: (a.cpu().numpy() if on_device else a) for k, a in every.items()}


def expected_ratio(capi, c, ref):
    """the reference's arrays, with what the call found where a member's word is 0"""
    act = c["what"] != 0
    exp = {}
    for k in capi.NlpTrial.INOUT:
        exp[k] = ref[k]                  # (the reference keeps a sitter's in/out entries itself)
    for k in capi.NlpTrial.OUT:
        fill = INT_FILL if k in capi.NlpTrial.INTS else np.nan
        exp[k] = np.where(act, ref[k], fill).astype(ref[k].dtype)
    return exp


def check_ratio(capi, f):
    o, c, ref, branch, st = ratio_case(capi, f)
    assert_ratio_inputs(capi, c, ref, branch)
    got = run_ratio(capi, f, o, c)
    exp = expected_ratio(capi, c, ref)
    for k in exp:
        assert got[k].tobytes() == exp[k].tobytes(), (f.key, k, np.flatnonzero(~((got[k] == exp[k]) | (got[k] != got[k]))))
    assert ref["accept"].any() and np.abs(st["p"]).max() > 0.0 and np.any(exp["x_k"] != c["x_k"])
    # the two words go straight back into the next calls: the pools equal the references' for the same words
    nq = len(f.n)
    act = c["what"] != 0
    hu, hm = np.where(act, got["hu_word"], 0).astype(np.int32), np.where(act, got["hm_word"], 0).astype(np.int32)
    assert {0, capi.HU_DELTA, capi.HU_BOUNDS | capi.HU_GRAD | capi.HU_UBA} == set(hu.tolist()) and {0, 3} == set(hm.tolist())
    before = f.b.get_vectors()
    grad = cat([f.rng.normal(size=n) for n in f.n])
    f.b.handler_update(hu, got["delta"], c["rho"], got["x_k"], got["c_k"], grad=grad, on_device=False)
    want = batch_handler_reference(before, hu, got["delta"], c["rho"], got["x_k"], got["c_k"], grad, f.n, f.m, *f.bounds)
    GH.assert_pools((f.key, "words fed back"), f.b, want, hu, before, f.b.offV, f.b.offC)
    A0, H0 = f.b.get_matrix_values()
    jac, hess = f.rng.normal(size=int(f.b.jnz.sum())), f.rng.normal(size=H0.size)
    f.b.handler_set_matrices(hm, jac, hess, on_device=False)
    A1, H1 = batch_matrices_reference(A0, H0, hm, jac, hess, f.b.nV, f.b.nC, [p.A_jc for p in f.b.problems], [p.H_jc for p in f.b.problems])
    A2, H2 = f.b.get_matrix_values()
    assert A2.tobytes() == A1.tobytes() and H2.tobytes() == H1.tobytes()
    assert np.any(A2 != A0) and np.any(A2 == A0)


@pytest.mark.parametrize("key", ["ragged", "one_shape", "wide"])
def test_ratio_test_against_the_reference(capi, fixtures, key):
    """after a real handler_update + optimize_qp: every output and every in/out array equal to the reference bit for bit (x_k += p
    included), members with word 0 keep their NaN, and the words fed back give the pools the existing references give"""
    check_ratio(capi, fixtures(key))


def test_infeasibility_and_argument_checks(capi, fixtures):
    """cal_infea for every member, bit for bit (the order of tree_sum); and with a real batch: RSQP_ERR_ARG for a missing required
    pointer, and before rsqp_batch_handler_set_problem"""
    f = fixtures("ragged")
    f.b.handler_set_problem(*f.bounds)
    c = cat([f.rng.normal(size=m) * 3.0 for m in f.m])
    got = f.b.handler_infeasibility(c)
    oC = 0
    for q, m in enumerate(f.m):
        want = handler.cal_infea_reference(c[oC:oC + m], f.bounds[2][oC:oC + m], f.bounds[3][oC:oC + m], 64)
        assert np.float64(got[q]).tobytes() == np.float64(want).tobytes(), (q, got[q], want)
        oC += m
    assert np.count_nonzero(got) >= 5
    nq, sN, sC = len(f.n), sum(f.n), sum(f.m)
    good = dict(what=np.ones(nq, np.int32), rho=np.ones(nq), f_trial=np.ones(nq), c_trial=np.ones(sC), x_k=np.ones(sN), c_k=np.ones(sC),
                f_k=np.ones(nq), infea_k=np.ones(nq), delta=np.ones(nq))
    o = capi.NlpStepOptions()
    import ctypes as C
    for missing in ("what", "rho", "f_trial", "c_trial", "x_k", "c_k", "f_k", "infea_k", "delta"):
        t = capi.NlpTrial(**{k: (None if k == missing else a.ctypes.data) for k, a in good.items()})
        assert capi.lib().rsqp_batch_handler_ratio_test(f.b._h, C.addressof(t), C.addressof(o), 0) == capi.ERR_ARG, missing
    pgood = dict(what=good["what"], x_k=good["x_k"], grad=good["x_k"], c_k=good["c_k"], infea=good["rho"])
    for missing in pgood:
        p = capi.NlpPoint(**{k: (None if k == missing else a.ctypes.data) for k, a in pgood.items()})
        assert capi.lib().rsqp_batch_handler_check_optimality(f.b._h, C.addressof(p), C.addressof(o), None, None, 0) == capi.ERR_ARG, missing
    assert capi.lib().rsqp_batch_handler_infeasibility(f.b._h, c.ctypes.data, None, 0) == capi.ERR_ARG
    fresh = Fixture(capi, RAGGED[:2], 3)
    for call in (lambda: fresh.b.handler_infeasibility(np.zeros(3)),
                 lambda: fresh.b.handler_ratio_test(np.ones(2, np.int32), np.ones(2), np.ones(2), np.ones(3), np.ones(7), np.ones(3), np.ones(2),
                                                    np.ones(2), np.ones(2)),
                 lambda: fresh.b.handler_check_optimality(np.ones(2, np.int32), np.ones(7), np.ones(7), np.ones(3), np.ones(2))):
        with pytest.raises(capi.RsqpError) as e:
            call()
        assert e.value.code == capi.ERR_ARG
    fresh.b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# trajectory replay
# ---------------------------------------------------------------------------------------------------------------------------------
def test_trajectory_replay(capi):
    """one batch holds the hs071, hs035 and hs065 runs of tests/golden/sqp_traces.json, advanced entry by entry: the pools are set
    from the trace's iterate through handler_update / handler_set_matrices with the words of its flags, solved, f and c at x + p are
    evaluated on the host, and the device ratio test decides. Bit for bit the reference's answer on the same pools; and accept, the
    new delta and the flags read off the two words are the NEXT trace entry's -- except where the reference's |pred| <= 1e-9: there
    the decision is rounding noise of the QP objective (at most four of the 23 entries)"""
    names = ("hs071", "hs035", "hs065")
    runs = {name: M.trajectory_qps(name) for name in names}
    nq = len(names)
    b = capi.Batch([runs[name][1][0] for name in names])
    nlp0 = [NLPS[name]() for name in names]
    ns, ms = [p["info"].nVar for p in nlp0], [p["info"].nCon for p in nlp0]
    offN, offC = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(ms)])
    bounds = [cat([p[k] for p in nlp0]) for k in ("x_l", "x_u", "c_l", "c_u")]
    b.handler_set_problem(*bounds)
    o = capi.NlpStepOptions(refresh_ubA=1)
    G = handler.nlp_step_lanes(ns, ms)
    pooled = lambda parts, take, off: cat([a if t else np.full(off[j + 1] - off[j], np.nan) for j, (a, t) in enumerate(zip(parts, take))])
    left_out, compared, total = [], 0, 0
    for t in range(max(len(runs[name][0]) for name in names)):
        take = np.array([t < len(runs[name][0]) for name in names])
        gold = [runs[name][0][t] if k else None for name, k in zip(names, take)]
        qps = [runs[name][1][t if k else 0] for name, k in zip(names, take)]
        nlps = [NLPS[name](np.array(g["x"]), np.array(g["lam"])) if g else None for name, g in zip(names, gold)]
        hu, hm = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
        for j, g in enumerate(gold):
            if g is None:
                continue
            fl = g["flags"]
            if fl["first"]:
                hu[j], hm[j] = capi.HU_SET, capi.HM_JAC | capi.HM_HESS
            else:
                hu[j] = (capi.HU_BOUNDS | capi.HU_UBA if fl["bounds"] else capi.HU_DELTA if fl["delta"] else 0) | \
                        (capi.HU_GRAD if fl["g"] else 0) | (capi.HU_PENALTY if fl["penalty"] else 0)
                hm[j] = (capi.HM_JAC if fl["A"] else 0) | (capi.HM_HESS if fl["H"] else 0)
            assert hu[j] != 0
        jac = cat([q.A_val[:q.A_jc[n]] for q, n in zip(qps, ns)])
        b.handler_set_matrices(hm, jac, cat([q.H_val for q in qps]))
        val = lambda key, parts: pooled([np.atleast_1d(p[key]) if p else None for p in parts], take, offN if key in ("x", "grad") else offC)
        delta, rho = [np.array([g[k] if g else np.nan for g in gold]) for k in ("delta", "rho")]
        b.handler_update(hu, delta, rho, val("x", nlps), val("c", nlps), grad=val("grad", nlps))
        b.set_members(take)
        b.optimize_qp()
        res, st = b.results(), b.handler_step()
        assert all(r["status"] == 20 for r, k in zip(res, take) if k), (t, [r["status"] for r in res])
        trial = [NLPS[name](p["x"] + st["p"][offN[j]:offN[j + 1]], np.array(g["lam"])) if g else None
                 for j, (name, p, g) in enumerate(zip(names, nlps, gold))]
        c_k = val("c", nlps)
        infea = b.handler_infeasibility(np.where(np.isnan(c_k), 0.0, c_k))
        for j in np.flatnonzero(take):
            want = handler.cal_infea_reference(nlps[j]["c"], nlps[j]["c_l"], nlps[j]["c_u"], G)
            assert np.float64(infea[j]).tobytes() == np.float64(want).tobytes(), (t, j)
        one = np.arange(nq + 1)
        c = dict(what=take.astype(np.int32), rho=rho, f_trial=pooled([[p["f"]] if p else None for p in trial], take, one), c_trial=val("c", trial),
                 x_k=val("x", nlps), c_k=c_k, f_k=pooled([[p["f"]] if p else None for p in nlps], take, one),
                 infea_k=np.where(take, infea, np.nan), delta=delta)
        obj = np.array([r["obj"] for r in res])
        ref = handler.batch_ratio_test_reference(o.as_dict(), c["what"], c["rho"], c["f_trial"], c["c_trial"], c["x_k"], c["c_k"], c["f_k"],
                                                 c["infea_k"], c["delta"], st["p"], st["norm_p"], obj, ns, ms, bounds[2], bounds[3])
        fx = type("F", (), dict(n=ns, m=ms, b=b))
        got = run_ratio(capi, fx, o, c)
        exp = expected_ratio(capi, c, ref)
        for k in exp:
            assert got[k].tobytes() == exp[k].tobytes(), (t, k)
        last_x = {}
        for j, name in enumerate(names):
            if not take[j]:
                continue
            total += 1
            tag = (name, t, float(ref["pred_reduction"][j]))
            if abs(ref["pred_reduction"][j]) <= 1e-9:
                left_out.append(tag[:2])
            elif t + 1 < len(runs[name][0]):
                nxt = runs[name][0][t + 1]
                compared += 1
                assert bool(got["accept"][j]) == bool(nxt["flags"]["A"]), tag
                assert got["delta"][j] == nxt["delta"], tag
                assert word_flags(capi, int(got["hu_word"][j]), int(got["hm_word"][j])) == effective_flags(nxt["flags"]), tag
            if name != "hs035" and (t == 0 or t + 1 == len(runs[name][0])):
                last_x[j] = t
        # check_optimality: at entry 0 the starting point, with the multipliers of its QP and the J already in the pool; at the last
        # entry of hs071 and hs065 the point the ratio test leaves, with its J brought into the pool first, as the header asks
        if last_x:
            what = np.array([1 if j in last_x else 0 for j in range(nq)], np.int32)
            pts = []
            for j, name in enumerate(names):
                if j not in last_x:
                    pts.append(None)
                elif t == 0:
                    pts.append(nlps[j])
                else:
                    lam_c = res[j]["y"][ns[j] + 2 * ms[j]:]
                    pts.append(NLPS[name](got["x_k"][offN[j]:offN[j + 1]], lam_c))
            if t > 0:
                qn = [M.full_pattern(problems.handler_qp(p, 1.0, 1.0)) if p else q for p, q in zip(pts, qps)]
                b.handler_set_matrices(what * capi.HM_JAC, cat([q.A_val[:q.A_jc[n]] for q, n in zip(qn, ns)]), None)
            sel = what != 0
            point_infea = np.where(sel, infea if t == 0 else got["infea_k"], np.nan)
            st5, verdict = b.handler_check_optimality(what, pooled([p["x"] if p else None for p in pts], sel, offN),
                                                      pooled([p["grad"] if p else None for p in pts], sel, offN),
                                                      pooled([p["c"] if p else None for p in pts], sel, offC), point_infea,
                                                      verdict=np.full(nq, INT_FILL, np.int32))
            print("entry", t, "verdicts", verdict.tolist(), "KKT errors", st5[:, 4].tolist())
            for j in range(nq):
                if j not in last_x:
                    assert verdict[j] == INT_FILL
                elif t == 0:
                    assert not verdict[j] & capi.KKT_FIRST_ORDER_OPT, (names[j], int(verdict[j]))
                else:
                    assert verdict[j] & capi.KKT_FIRST_ORDER_OPT, (names[j], int(verdict[j]), st5[j].tolist())
    print("left out of the decision comparison:", left_out, "compared:", compared, "of", total)
    assert total == 23 and len(left_out) <= 4 and compared >= 17
    b.close()


def test_device_pointers():
    """the ratio test and the KKT check with every array a device tensor give the bytes of the host-pointer calls. In a child process
    that imports torch BEFORE the library is loaded (tests/checks/handler_device_pointers.py says why)"""
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "nlp_step_device_pointers.py")], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "NLP STEP DEVICE POINTERS OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
