"""Shared by tests/test_soc_args.py, tests/test_gpu_soc.py and tests/checks/soc_device_pointers.py: the inputs of the second-order
correction per member of a batch (rsqp_batch_handler_soc_begin / _soc_end, include/rsqp_hip_soc.h), the run of
handler.batch_soc_reference over the C oracle on them, and the host-driven loop that does the same work on a second batch with the
entry points that existed before the calls, plus rsqp_batch_set_objective.

The members are those of tests/penalty_cases.py: the 70 hs071 members (8-lane group, tableau kernels) and the 40 mixed members
(wavefront group, null-space kernels). Which branches occur is a condition on the INPUTS and is asserted from the oracle run alone
(tests/test_soc_args.py), so a generator change cannot silently empty one."""
import collections

import numpy as np

import penalty_cases as PC
from restartsqp_amd import handler
from test_gpu_batch_optimize import Ref

QP_MAXITER = PC.QP_MAXITER
MARGIN = PC.MARGIN
# name -> (fields of rsqp_nlp_step_options that differ from the defaults, fields of rsqp_soc_options, qp_maxiter of the correction
# solve, infea_model given). "budget": the first solve has the full budget, the correction solve 2 iterations, so that some end
# unsolved; "delta_min": a shrunk radius falls below it; "composite": the qp_obj_ of :1198 decides, with infea_model passed in
OPTION_SETS = {"default": ({}, {}, QP_MAXITER, False), "budget": ({}, {}, 2, False), "composite": ({}, dict(composite_pred=1), QP_MAXITER, True),
               "ubA": (dict(refresh_ubA=1), {}, QP_MAXITER, False), "delta_min": (dict(delta_min=0.2), {}, QP_MAXITER, False)}
DOUBLE_FILL, INT_FILL = np.nan, -12345      # what the outputs hold before a call: a member that does not write one keeps it
# the trial values' per-member bias (objective curvature, constraint curvature): see trial_values
BIASES = ((0.0, 0.0), (-0.3, 0.3), (-0.3, 0.6), (-0.2, -0.4), (3.0, 0.0), (0.4, 0.15), (-0.6, 0.2), (-0.1, 0.8))
BIAS_SEED = 4


def members_of(batch):
    """"hs071_gpu": the 70 hs071 members of tests/penalty_cases.py; "mixed": its 40 mixed members"""
    return PC.members_of(batch)


lanes = PC.lanes
same_bytes = PC.same_bytes
raw_results = PC.raw_results


def what_of(members):
    """every seventh member sits out, every fifth takes the test alone, the others may be corrected"""
    from restartsqp_amd import capi
    return np.array([0 if q % 7 == 3 else (capi.SOC_TEST if q % 5 == 1 else capi.SOC_TEST | capi.SOC_CORRECT) for q in range(len(members))],
                    np.int32)


def biases_of(members):
    rng = np.random.default_rng(BIAS_SEED)
    return [BIASES[k] for k in rng.integers(0, len(BIASES), len(members))]


_DENSE = {}


def dense_of(d):
    """(J, H_k) of a member as dense arrays, from the QP QPhandler built: columns [0, n) of A, the leading n x n block of H"""
    key = id(d["qp"])
    if key not in _DENSE:
        qp, n, m = d["qp"], d["n"], d["m"]
        J, H = np.zeros((m, n)), np.zeros((n, n))
        for j in range(n):
            for k in range(qp.A_jc[j], qp.A_jc[j + 1]):
                J[qp.A_ir[k], j] = qp.A_val[k]
            for k in range(qp.H_jc[j], qp.H_jc[j + 1]):
                if qp.H_ir[k] < n:
                    H[qp.H_ir[k], j] = qp.H_val[k]
        _DENSE[key] = (J, H)
    return _DENSE[key]


def f_k_of(d):
    return np.float64(0.5 * float(np.dot(d["x_k"], d["x_k"])))


def trial_values(d, bias, step):
    """f and c at x_k + step by a rule both sides evaluate on their own step: the quadratic model and the linearised constraints at
    the step, plus curvature the model does not know -- the member's bias times |step|^2 / delta^2, scaled to what a step of length
    delta can change: (|grad|_1 delta + rho infea_k) for f, |J_i|_1 delta for constraint i"""
    J, H = dense_of(d)
    step = np.asarray(step, dtype=np.float64)
    grad = np.asarray(d["qp"].g, dtype=np.float64)[:d["n"]]
    ss = float(np.dot(step, step)) / d["delta"] ** 2
    infea_k = float(handler.cal_infea_reference(*d["c_infea"], 8))
    f = f_k_of(d) + float(np.dot(grad, step)) + 0.5 * float(np.dot(step, H @ step)) + \
        bias[0] * ss * (float(np.abs(grad).sum()) * d["delta"] + d["rho"] * infea_k)
    c = np.asarray(d["c_k"], dtype=np.float64) + J @ step + bias[1] * ss * np.abs(J).sum(axis=1) * d["delta"]
    return np.float64(f), c


def pooled(members, what=None):
    """the arrays of the two calls, pooled: the inputs and the in/out iterate"""
    cat = lambda k: np.concatenate([d[k] for d in members])
    return dict(what=what_of(members) if what is None else np.asarray(what, np.int32), rho=np.array([d["rho"] for d in members]),
                x_k=cat("x_k"), c_k=cat("c_k"), f_k=np.array([f_k_of(d) for d in members]), infea_k=PC.infea_k_of(members),
                delta=np.array([d["delta"] for d in members]), grad=np.concatenate([np.asarray(d["qp"].g, float)[:d["n"]] for d in members]))


ITERATE = ("x_k", "c_k", "f_k", "infea_k", "delta")


def fresh_out(capi, members):
    nq, sN = len(members), sum(d["n"] for d in members)
    return {k: (np.full(nq, INT_FILL, np.int32) if k in capi.SocTrial.INTS else np.full(sN if k == "x_trial" else nq, DOUBLE_FILL))
            for k in capi.SocTrial.OUT}


def offsets(members):
    n = np.array([d["n"] for d in members]); m = np.array([d["m"] for d in members])
    return n, m, np.concatenate([[0], np.cumsum(n)]), np.concatenate([[0], np.cumsum(m)]), np.concatenate([[0], np.cumsum(n + 2 * m)])


def member_states(members, S, model=None):
    """the per-member dicts handler.batch_soc_reference takes, from the pooled arrays"""
    return [dict(d, what=S["what"][q], f_k=S["f_k"][q], infea_k=S["infea_k"][q], grad=np.asarray(d["qp"].g, float)[:d["n"]],
                 infea_model=None if model is None else model[q]) for q, d in enumerate(members)]


_RUNS = {}


def oracle_run(O, capi, batch, option_set):
    """(members, pooled arrays, step options, soc options, rows of handler.batch_soc_reference) on the CPU oracle; computed once per
    session and shared -- nobody changes it"""
    key = (batch, option_set)
    if key not in _RUNS:
        members = members_of(batch)
        fields, soc_fields, budget, give_model = OPTION_SETS[option_set]
        o, so = capi.NlpStepOptions(**fields).as_dict(), capi.SocOptions(**soc_fields).as_dict()
        S = pooled(members)
        G = lanes(members)
        Q, model = [], []
        for d in members:
            r = Ref(O, d["qp"], QP_MAXITER)
            r.optimize(d["qp"])
            model.append(handler.tree_sum(np.abs(np.asarray(r.qp.x)[d["n"]:]), G))
            r.maxit = budget
            Q.append(PC.OracleMember(r))
        bias = biases_of(members)
        rows = handler.batch_soc_reference(Q, member_states(members, S, model if give_model else None), o, so,
                                           lambda q, step: trial_values(members[q], bias[q], step), G=G)
        _RUNS[key] = (members, S, o, so, rows)
    return _RUNS[key]


def kind_of(r):
    """the branch a row of the reference took, with what update_radius did behind it"""
    if r["branch"] is None:
        return "sits_out"
    if r["branch"] == "soc_unsolved":
        return "soc_unsolved"
    verdict = "" if r["branch"] != "no_correct" else ("_accepted" if r["accept"] else "_rejected")
    return r["branch"] + verdict + "_" + r["radius"] + ("_too_small" if r["too_small"] else "")


def census(rows):
    return collections.Counter(kind_of(r) for r in rows)


def solved_throughout(r):
    return r["branch"] in ("no_correct", "accepted", "soc_accepted", "soc_rejected") and r["x"] is not None


def assert_margins(rows):
    worst = min([m for r in rows for m in r["margins"]] or [1.0])
    assert worst >= MARGIN, worst      # (another seed or bias set if this fails, never a looser comparison)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU side: a batch with its first solve done, the two calls with the trial values between them, and the host-driven loop
# ---------------------------------------------------------------------------------------------------------------------------------
def make_batch(capi, members, budget=QP_MAXITER):
    cat = lambda k: np.concatenate([d[k] for d in members])
    b = capi.Batch([d["qp"] for d in members])
    b.handler_set_problem(cat("x_l"), cat("x_u"), cat("c_l"), cat("c_u"))
    b.optimize_qp()
    b.set_options(qp_maxiter=budget)
    return b


def snapshot(capi, b):
    """everything of a batch a call may touch and a getter shows: the result pools, the vector pools, the matrix pools, the dispatch
    of the last inner call"""
    s = dict(raw_results(b))
    for k, v in zip(("g", "lb", "ub", "lbA", "ubA"), b.get_vectors()):
        s[k] = v
    s["A"], s["H"] = b.get_matrix_values()
    s["mode"], s["rescue"] = b.dispatch()
    return s


def steps_of_pool(b, members):
    """the NLP part of every member's x in the result pools: p behind a solve, p + s behind soc_begin"""
    n, m, offN, offC, offV = offsets(members)
    x = raw_results(b)["x"]
    return [x[offV[q]:offV[q] + n[q]].copy() for q in range(len(members))]


def first_trial_values(b, members, bias):
    """f_trial, c_trial (pooled) at x_k + p of the batch's last solve, and that p per member"""
    ps = steps_of_pool(b, members)
    tv = [trial_values(d, bias[q], ps[q]) for q, d in enumerate(members)]
    return np.array([t[0] for t in tv]), np.concatenate([t[1] for t in tv]), ps


def device_route(capi, b, members, S, o, so, out, bias, on_device=False, model=None):
    """soc_begin, the evaluators at x_trial for the members that go on, soc_end -- on host arrays, or on torch tensors of the batch's
    device. S (the iterate) and out are written in place either way. Returns out as it stood between the two calls"""
    opts, sopts = capi.NlpStepOptions(**o), capi.SocOptions(**so)
    f_t, c_t, _ = first_trial_values(b, members, bias)
    n, m, offN, offC, offV = offsets(members)
    it = {k: S[k] for k in ITERATE}
    if on_device:
        torch = capi.device_torch()
        T = lambda v: None if v is None else torch.as_tensor(v, device="cuda")
        dit, dout = {k: T(v) for k, v in it.items()}, {k: T(v) for k, v in out.items()}
        torch.cuda.synchronize()
        b.handler_soc_begin(T(S["what"]), T(S["rho"]), T(f_t), T(c_t), **dit, grad=T(S["grad"]), infea_model=T(model), options=opts,
                            soc_options=sopts, on_device=True, out=dout)
        for k in out:
            out[k][:] = dout[k].cpu().numpy()
    else:
        b.handler_soc_begin(S["what"], S["rho"], f_t, c_t, **it, grad=S["grad"], infea_model=model, options=opts, soc_options=sopts, out=out)
    mid = {k: v.copy() for k, v in out.items()}
    # the driver's evaluators: f and c at x_trial, for the members with soc == 1 (the others' entries are not read)
    f_t2, c_t2 = f_t.copy(), c_t.copy()
    pool_steps = steps_of_pool(b, members)
    for q in np.flatnonzero(out["soc"] == 1):
        f_t2[q], c_t2[offC[q]:offC[q + 1]] = trial_values(members[q], bias[q], pool_steps[q])
    if on_device:
        torch.cuda.synchronize()
        b.handler_soc_end(T(S["rho"]), T(f_t2), T(c_t2), **dit, out=dout, options=opts, soc_options=sopts, on_device=True)
        for k in ITERATE:
            S[k][:] = dit[k].cpu().numpy()
        for k in out:
            out[k][:] = dout[k].cpu().numpy()
    else:
        b.handler_soc_end(S["rho"], f_t2, c_t2, **it, out=out, options=opts, soc_options=sopts)
    return mid


def host_driven(capi, hb, members, S, o, so, out, bias, model=None):
    """the same iteration on the batch hb with the entry points that existed before the calls, plus set_objective:
    handler_ratio_test for the members that need no correction; results, handler_step and get_matrix_values down; numpy float64
    scalars for H p + grad in the stated order and for the tests; handler_update, set_vectors (of the members), set_members,
    optimize_qp, set_results and set_objective up. S (the iterate) and out are written in place as the calls write them. Returns
    out as it stands between the two calls"""
    f8 = np.float64
    nq = len(members)
    n, m, offN, offC, offV = offsets(members)
    G = lanes(members)
    opts = capi.NlpStepOptions(**o)
    eta_s, tol = f8(o["eta_s"]), f8(o["tol"])
    composite = int(so.get("composite_pred", 0)) != 0
    hu_accepted = capi.HU_BOUNDS | capi.HU_GRAD | (capi.HU_UBA if o["refresh_ubA"] else 0)
    what = S["what"]
    f_t, c_t, ps = first_trial_values(hb, members, bias)
    r0 = raw_results(hb)
    step0 = hb.handler_step()
    c_l, c_u = np.concatenate([d["c_l"] for d in members]), np.concatenate([d["c_u"] for d in members])

    def test(q, ft, ct, qp_obj):
        it = handler.cal_infea_reference(ct, c_l[offC[q]:offC[q + 1]], c_u[offC[q]:offC[q + 1]], G)
        actual = (f8(S["f_k"][q]) + f8(S["rho"][q]) * f8(S["infea_k"][q])) - (f8(ft) + f8(S["rho"][q]) * it)
        pred = f8(S["rho"][q]) * f8(S["infea_k"][q]) - f8(qp_obj)
        return it, actual, pred, bool(actual >= eta_s * pred and actual >= -tol)

    # who needs a correction: the first test in numpy; everybody else takes handler_ratio_test as it was
    first, corr = {}, np.zeros(nq, np.int32)
    for q in range(nq):
        if what[q] != 0:
            first[q] = test(q, f_t[q], c_t[offC[q]:offC[q + 1]], r0["obj"][q])
            corr[q] = 1 if (not first[q][3] and (what[q] & capi.SOC_CORRECT)) else 0
    plain = ((what != 0) & (corr == 0)).astype(np.int32)
    nlp_out = {k: out[k] for k in capi.NlpTrial.OUT}
    hb.handler_ratio_test(plain, S["rho"], f_t, c_t, S["x_k"], S["c_k"], S["f_k"], S["infea_k"], S["delta"], options=opts, out=nlp_out)
    for q in np.flatnonzero(plain):
        out["soc"][q], out["nwsr_soc"][q], out["qp_obj"][q] = 0, 0, r0["obj"][q]
    if corr.any():
        # update_grad(H_k p + grad_f) and update_bounds at x_k + p with c_trial (:1181-1184)
        A, H = hb.get_matrix_values()
        offH = np.concatenate([[0], np.cumsum(hb.hnnz)])
        g, lb, ub, lbA, ubA = hb.get_vectors()
        xt = S["x_k"].copy()
        for q in np.flatnonzero(corr):
            qp = members[q]["qp"]
            pool = type("H", (), dict(H_jc=qp.H_jc, H_ir=qp.H_ir, H_val=H[offH[q]:offH[q + 1]]))
            g[offV[q]:offV[q] + n[q]] = handler.hess_times_reference(pool, n[q], ps[q]) + S["grad"][offN[q]:offN[q + 1]]
            xt[offN[q]:offN[q + 1]] = S["x_k"][offN[q]:offN[q + 1]] + ps[q]
        hb.handler_update(corr * (capi.HU_BOUNDS | (capi.HU_UBA if o["refresh_ubA"] else 0)), S["delta"], S["rho"], xt, c_t)
        _, lb, ub, lbA, ubA = hb.get_vectors()
        hb.set_vectors(g, lb, ub, lbA, ubA, members=corr)
        hb.set_members(corr)
        used = hb.optimize_qp()
        r1 = raw_results(hb)
        x_new = r1["x"].copy()
        for q in np.flatnonzero(corr):
            out["nwsr_soc"][q] = used[q]
            if r1["status"][q] != capi.QP_OPTIMAL:
                out["exitflag"][q], out["soc"][q], corr[q] = r1["status"][q], 0, 0
                continue
            step = ps[q] + r1["x"][offV[q]:offV[q] + n[q]]
            x_new[offV[q]:offV[q] + n[q]] = step
            out["x_trial"][offN[q]:offN[q + 1]] = S["x_k"][offN[q]:offN[q + 1]] + step
            mod = f8(step0["infea_model"][q]) if model is None else f8(model[q])
            out["qp_obj"][q] = f8(r1["obj"][q]) + (f8(r0["obj"][q]) - f8(S["rho"][q]) * mod)
            out["actual_reduction"][q], out["pred_reduction"][q], out["infea_trial"][q] = first[q][1], first[q][2], first[q][0]
            out["accept"][q], out["soc"][q] = 0, 1
        hb.set_results(x=x_new)
    mid = {k: v.copy() for k, v in out.items()}
    going = np.flatnonzero(corr)
    if going.size:
        # soc_end: the second test, the restore, update_radius
        r1 = raw_results(hb)
        x_back, obj_back, rejected = r1["x"].copy(), r1["obj"].copy(), np.zeros(nq, np.int32)
        for q in going:
            step = r1["x"][offV[q]:offV[q] + n[q]].copy()
            ft2, ct2 = trial_values(members[q], bias[q], step)
            it, actual, pred, acc = test(q, ft2, ct2, out["qp_obj"][q] if composite else r1["obj"][q])
            if acc:
                S["x_k"][offN[q]:offN[q + 1]] = S["x_k"][offN[q]:offN[q + 1]] + step
                S["c_k"][offC[q]:offC[q + 1]] = ct2
                S["f_k"][q], S["infea_k"][q] = ft2, it
                norm_p = f8(np.abs(step).max())
            else:
                x_back[offV[q]:offV[q + 1]] = r0["x"][offV[q]:offV[q + 1]]
                obj_back[q], rejected[q] = r0["obj"][q], 1
                out["qp_obj"][q] = r0["obj"][q]
                norm_p = f8(np.abs(ps[q]).max())
            d = f8(S["delta"][q])
            if actual < f8(o["eta_c"]) * pred:
                d = f8(o["gamma_c"]) * d
            elif actual > f8(o["eta_e"]) * pred and tol > abs(d - norm_p):
                grown = f8(o["gamma_e"]) * d
                d = f8(o["delta_max"]) if f8(o["delta_max"]) < grown else grown
            S["delta"][q] = d
            out["actual_reduction"][q], out["pred_reduction"][q], out["infea_trial"][q], out["accept"][q] = actual, pred, it, int(acc)
            out["hu_word"][q], out["hm_word"][q] = hu_accepted, (capi.HM_JAC | capi.HM_HESS) if acc else 0
            out["exitflag"][q] = capi.EXIT_TRUST_REGION_TOO_SMALL if d < f8(o["delta_min"]) else capi.EXIT_UNKNOWN
        if rejected.any():
            hb.set_results(x=x_back)
            hb.set_objective(obj_back, members=rejected)
    return mid
