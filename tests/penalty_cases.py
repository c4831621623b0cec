"""Shared by tests/test_penalty_args.py and tests/test_gpu_penalty.py: the inputs of the penalty update per member of a batch
(rsqp_batch_handler_update_penalty, include/rsqp_hip_penalty.h), the run of handler.batch_update_penalty_reference over the C oracle
on them, and the host-driven loop that does the same work on a pair of batches with the entry points that existed before the call.

Which branches occur is a condition on the INPUTS and is asserted from the oracle run alone (assert_inputs_cover_the_branches), so a
generator change cannot silently empty one."""
import collections
import functools

import numpy as np

from restartsqp_amd import handler, problems
from restartsqp_amd.qpdump import QPData, dense_to_csc
from restartsqp_amd.sqptypes import INF

from lp_batch_ref import LPRef
from test_gpu_batch_optimize import Ref

QP_MAXITER, LP_MAXITER = 1000, 100          # the defaults of a batch (rsqp_batch_set_options / rsqp_batch_set_lp_options)
EPS1 = 0.1                                  # src/Options.cpp: where the reference starts eps1
MARGIN = 1e-6                               # every float comparison that decides a branch is at least this far from a tie, relatively
# name -> (option fields that differ from the defaults, eps1 of every member, qp_maxiter of the re-solves): the sets that reach every
# branch. "budget": the first solve has the full budget, the re-solves of the loop 2 iterations, so that some end unsolved
OPTION_SETS = {"default": ({}, EPS1, QP_MAXITER), "eps2": (dict(eps2=0.9), EPS1, QP_MAXITER), "rho_max": (dict(rho_max=10.0), EPS1, QP_MAXITER),
               "eps1": ({}, 0.9, QP_MAXITER), "iter_max": (dict(penalty_iter_max=0), EPS1, QP_MAXITER), "budget": ({}, EPS1, 2)}
DOUBLE_FILL, INT_FILL = np.nan, -12345      # what the outputs hold before a call: a member that does not write one keeps it


def member_of(nlp, delta, rho, name):
    """one member: the NLP data the call reads and the QP QPhandler builds from it"""
    return dict(n=nlp["info"].nVar, m=nlp["info"].nCon, x_k=np.asarray(nlp["x"], float), c_k=np.asarray(nlp["c"], float),
                x_l=nlp["x_l"], x_u=nlp["x_u"], c_l=nlp["c_l"], c_u=nlp["c_u"], delta=float(delta), rho=float(rho),
                c_infea=(nlp["c"], nlp["c_l"], nlp["c_u"]), qp=problems.handler_qp(nlp, delta, rho, name=name))


@functools.lru_cache(maxsize=None)
def hs071_members(count=400, seed=1):
    """hs071 at random points: x uniform in [1, 5]^4, lam = 0.1 normal, delta from {0.05, 0.25, 1, 4}, rho from {1, 1, 100, 1e5, 1e6}"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        x, lam = rng.uniform(1.0, 5.0, 4), 0.1 * rng.normal(size=2)
        delta, rho = rng.choice([0.05, 0.25, 1.0, 4.0]), rng.choice([1.0, 1.0, 100.0, 1.0e5, 1.0e6])
        out.append(member_of(problems.hs071_nlp(x, lam), delta, rho, "hs071_%d" % k))
    return out


@functools.lru_cache(maxsize=None)
def mixed_members(count=40, seed=11):
    """random handler-shaped members, n in 3..12, m in 1..10 (nVmax + nCmax > 16: the wavefront group, the null-space kernels): J
    normal, H_k SPD, the box around x_k partly narrower than delta. Two members in three: constraint bounds of which about half cannot
    be met inside delta (|J_i| delta is all a step can move constraint i). Every third: bounds a step p0 inside the box meets, and a
    gradient that pulls away from it, which a small rho does not outweigh -- the LP is feasible where the QP's model is not"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n, m = int(rng.integers(3, 13)), int(rng.integers(1, 11))
        J = rng.normal(size=(m, n))
        M = rng.normal(size=(n, n))
        Hk = M @ M.T / n + np.eye(n)
        x = rng.normal(size=n)
        delta, rho = float(rng.choice([0.25, 1.0])), float(rng.choice([1.0, 1.0, 100.0, 1.0e5]))
        x_l, x_u = x - np.abs(rng.normal(size=n)) - 0.05, x + np.abs(rng.normal(size=n)) + 0.05
        c = rng.normal(size=m)
        reach = np.abs(J).sum(axis=1) * delta
        far = rng.random(m) < 0.5
        c_l = c + np.where(far, 1.0 + rng.random(m), 0.2 * rng.random(m)) * reach * np.where(rng.random(m) < 0.3, 0.02, 1.0)
        c_u = np.where(rng.random(m) < 0.4, c_l, np.where(rng.random(m) < 0.5, np.inf, c_l + 1.0 + rng.random(m)))
        grad = rng.normal(size=n)
        if k % 3 == 1:
            p0 = 0.8 * rng.uniform(np.maximum(x_l - x, -delta), np.minimum(x_u - x, delta))
            c_l = c + J @ p0
            c_u = np.where(rng.random(m) < 0.5, c_l, np.inf)
            grad, rho = -3.0 * rho * (2.0 + rng.random()) * np.sign(p0) * np.abs(J).sum(axis=0), float(rng.choice([1.0, 100.0]))
        nV = n + 2 * m
        A = np.hstack([J, np.eye(m), -np.eye(m)])
        H = np.zeros((nV, nV)); H[:n, :n] = Hk
        g = np.concatenate([grad, np.full(2 * m, rho)])
        lb = np.concatenate([np.maximum(x_l - x, -delta), np.zeros(2 * m)]); ub = np.concatenate([np.minimum(x_u - x, delta), np.full(2 * m, INF)])
        qp = QPData(nV, m, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, c_l - c, c_u - c, name="mixed_%d" % k)
        out.append(dict(n=n, m=m, x_k=x, c_k=c, x_l=x_l, x_u=x_u, c_l=c_l, c_u=c_u, delta=delta, rho=rho, c_infea=(c, c_l, c_u), qp=qp))
    return out


# the hs071 batch of the GPU tests: 70 of the 400 draws, so that a wave of the 8-lane kernels holds members of different branches --
# up to three of every branch an option set reaches (chosen from the oracle run; tests/test_penalty_args.py asserts what they
# cover), then the first draws
HS071_GPU = (15, 20, 22, 0, 37, 72, 79, 100, 116, 229, 1, 88, 119, 139, 188, 197, 298, 2, 34, 46, 54, 196, 284, 361, 3, 47, 63, 71, 238, 4,
             5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 18, 19, 21, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 35, 36, 38, 39, 40, 41, 42,
             43, 44, 45, 48, 49, 50, 51)


def members_of(batch):
    """"hs071": the 400 draws; "hs071_gpu": the 70 of them the GPU tests run; "mixed" """
    if batch == "mixed":
        return mixed_members()
    return hs071_members() if batch == "hs071" else [hs071_members()[k] for k in HS071_GPU]


def lanes(members):
    return handler.nlp_step_lanes([d["n"] for d in members], [d["m"] for d in members])


def infea_k_of(members):
    G = lanes(members)
    return np.array([handler.cal_infea_reference(*d["c_infea"], G) for d in members])


def what_of(members):
    """every seventh member sits out"""
    return np.array([0 if q % 7 == 3 else 1 for q in range(len(members))], np.int32)


def pooled(members, eps1, what=None):
    """the arrays of one call, pooled: the inputs, the in/out state (counters at 3, 2, 1: cumulative over a run)"""
    nq = len(members)
    cat = lambda k: np.concatenate([d[k] for d in members])
    return dict(what=what_of(members) if what is None else np.asarray(what, np.int32), infea_k=infea_k_of(members),
                delta=np.array([d["delta"] for d in members]), x_k=cat("x_k"), c_k=cat("c_k"), rho=np.array([d["rho"] for d in members]),
                eps1=np.full(nq, float(eps1)), trial=np.full(nq, 3, np.int32), succ=np.full(nq, 2, np.int32), fail=np.full(nq, 1, np.int32))


def fresh_out(capi, nq):
    return {k: (np.full(nq, INT_FILL, np.int32) if k in capi.PenaltyState.INTS else np.full(nq, DOUBLE_FILL)) for k in capi.PenaltyState.OUT}


def member_states(members, S):
    """the per-member dicts handler.batch_update_penalty_reference takes, from the pooled arrays"""
    return [dict(d, what=S["what"][q], infea_k=S["infea_k"][q], eps1=S["eps1"][q], trial=S["trial"][q], succ=S["succ"][q], fail=S["fail"][q])
            for q, d in enumerate(members)]


class OracleMember:
    """a member's solver object over the C oracle: Ref (optimizeQP) or LPRef (optimizeLP) with what the reference reads"""

    def __init__(s, ref):
        s.ref = ref

    def optimize(s, data, new_matrices=False):
        if new_matrices:
            s.ref.set_mats(data)
        return s.ref.optimize(data)

    x = property(lambda s: s.ref.qp.x)
    objective = property(lambda s: s.ref.qp.objective)
    status = property(lambda s: s.ref.qp.exitflag())


_RUNS = {}


def oracle_run(O, capi, batch, option_set):
    """(members, pooled arrays, options, rows of handler.batch_update_penalty_reference, the members' first QP solves as
    dict(solved, x, obj)) on the CPU oracle; computed once per session and shared -- nobody changes it"""
    key = (batch, option_set)
    if key not in _RUNS:
        members = members_of(batch)
        fields, eps1, budget = OPTION_SETS[option_set]
        o = capi.PenaltyOptions(**fields).as_dict()
        S = pooled(members, eps1)
        Q, L, first = [], [], []
        for d in members:
            r = Ref(O, d["qp"], QP_MAXITER)
            r.optimize(d["qp"])
            first.append(dict(solved=bool(r.qp.is_solved()), x=r.qp.x, obj=r.qp.objective))
            r.maxit = budget
            Q.append(OracleMember(r)); L.append(OracleMember(LPRef(O, d["qp"], LP_MAXITER)))
        rows = handler.batch_update_penalty_reference(Q, L, member_states(members, S), o, G=lanes(members))
        _RUNS[key] = (members, S, o, rows, first)
    return _RUNS[key]


def kind_of(r):
    """the branch a row of the reference took, as the issue names them"""
    if r["branch"] in (None, "qp_unsolved", "none", "lp_unsolved"):
        return {None: "sits_out", "none": "nothing"}.get(r["branch"], r["branch"])
    if r["broke"]:
        return "loop_qp_unsolved"
    if r["rounds"] == 0:
        return r["branch"] + "_no_round"
    tail = "_capped" if r["capped"] else ""
    return "%s_%s_%d%s" % (r["branch"], r["outcome"], r["rounds"], tail)


def census(rows):
    return collections.Counter(kind_of(r) for r in rows)


def solved_throughout(r):
    return r["branch"] in ("none", "A", "B") and not r["broke"]


def assert_margins(rows):
    worst = min([m for r in rows for m in r["margins"]] or [1.0])
    assert worst >= MARGIN, worst      # (another seed if this fails, never a looser comparison)


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU side: a QP batch with its first solve done and an LP batch beside it, and the host-driven loop
# ---------------------------------------------------------------------------------------------------------------------------------
def make_pair(capi, members):
    qps = [d["qp"] for d in members]
    cat = lambda k: np.concatenate([d[k] for d in members])
    pair = []
    for _ in range(2):
        b = capi.Batch(qps)
        b.handler_set_problem(cat("x_l"), cat("x_u"), cat("c_l"), cat("c_u"))
        pair.append(b)
    qp, lp = pair
    qp.optimize_qp()
    return qp, lp


def raw_results(b):
    """the result pools as they stand: x, y, the working sets, the status and the objective of every member, pooled"""
    rs = b.results()
    return dict(x=np.concatenate([r["x"] for r in rs]), y=np.concatenate([r["y"] for r in rs]), ws_b=np.concatenate([r["ws_b"] for r in rs]),
                ws_c=np.concatenate([r["ws_c"] for r in rs]), status=np.array([r["status"] for r in rs]), obj=np.array([r["obj"] for r in rs]))


def snapshot(capi, qp, lp):
    """everything of a pair a call may touch and a getter shows: the result pools, the vector pools, the A pools, the dispatch of the
    last inner calls"""
    s = {}
    for tag, b in (("qp", qp), ("lp", lp)):
        for k, v in raw_results(b).items():
            s[tag + "." + k] = v
        for k, v in zip(("g", "lb", "ub", "lbA", "ubA"), b.get_vectors()):
            s[tag + "." + k] = v
        s[tag + ".A"] = b.get_matrix_values()[0]
        try:
            s[tag + ".mode"], s[tag + ".rescue"] = b.dispatch()
        except capi.RsqpError:
            pass                       # no optimize call has run on it
    return s


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def host_driven(capi, qp, lp, members, S, o, out):
    """update_penalty_parameter on the pair (qp, lp) with the entry points that existed before rsqp_batch_handler_update_penalty:
    handler_step and results down, the decisions in numpy float64 scalars, set_members + handler_update / handler_set_matrices +
    optimize up, mask by mask. S (the in/out arrays) and out are written in place as the call writes them. Returns the x and the
    objective the QP batch's result pools must hold afterwards: its own, with the first solve's put back for the failure-path
    members (there is no setter for the objective pool, so the expectation is formed here)"""
    f8 = np.float64
    nq = len(members)
    n = np.array([d["n"] for d in members]); m = np.array([d["m"] for d in members])
    offV = np.concatenate([[0], np.cumsum(n + 2 * m)])
    tol, inc, rho_max, it_max, parm, eps2 = (f8(o["penalty_update_tol"]), f8(o["increase_parm"]), f8(o["rho_max"]), int(o["penalty_iter_max"]),
                                             f8(o["eps1_change_parm"]), f8(o["eps2"]))
    what = S["what"]
    r0 = raw_results(qp)
    model = qp.handler_step()["infea_model"].copy()
    model0 = model.copy()
    x0, obj0 = r0["x"].copy(), r0["obj"].copy()
    nw_qp, nw_lp, rounds = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    flag = np.full(nq, capi.EXIT_UNKNOWN, np.int32)
    infty = np.full(nq, np.nan)
    have_infty = np.zeros(nq, bool)
    done = np.zeros(nq, bool)            # the member writes its outputs
    take_lp = np.zeros(nq, np.int32)
    for q in range(nq):
        if what[q] == 0:
            continue
        if r0["status"][q] != capi.QP_OPTIMAL:
            out["exitflag"][q] = r0["status"][q]
        elif model[q] > tol:
            take_lp[q] = 1
        else:
            done[q] = True
    rho_trial = S["rho"].copy()
    broke = np.zeros(nq, bool)
    loop = np.zeros(nq, np.int32)
    branch = np.zeros(nq, np.int32)

    def goes_on(q):
        if branch[q] == 1:
            if not model[q] > tol:
                return False
        elif not ((S["infea_k"][q] - model[q]) < S["eps1"][q] * (S["infea_k"][q] - infty[q]) and S["trial"][q] < it_max):
            return False
        return not rho_trial[q] >= rho_max

    def start_round(q):
        nxt = rho_trial[q] * inc
        rho_trial[q] = nxt if nxt < rho_max else rho_max
        S["trial"][q] += 1
        loop[q] = 1

    if take_lp.any():
        lp.handler_update(take_lp * capi.HU_SET, S["delta"], S["rho"], S["x_k"], S["c_k"], grad=None)
        A = qp.get_matrix_values()[0]
        offA = np.concatenate([[0], np.cumsum(qp.annz)])
        jac = np.concatenate([A[offA[q]:offA[q] + qp.jnz[q]] for q in range(nq)])
        lp.handler_set_matrices(take_lp * capi.HM_JAC, jac=jac)
        lp.set_members(take_lp)
        used = lp.optimize_lp()
        rl = raw_results(lp)
        lp_model = lp.handler_step()["infea_model"]
        for q in np.flatnonzero(take_lp):
            nw_lp[q] = used[q]
            done[q] = True
            if rl["status"][q] != capi.QP_OPTIMAL:
                flag[q] = rl["status"][q]
                continue
            infty[q], have_infty[q] = lp_model[q], True
            branch[q] = 1 if infty[q] <= tol else 2
            if goes_on(q):
                start_round(q)
        while loop.any():
            qp.handler_update(loop * capi.HU_PENALTY, S["delta"], rho_trial, S["x_k"], S["c_k"])
            qp.set_members(loop)
            used = qp.optimize_qp()
            rq = raw_results(qp)
            step = qp.handler_step()["infea_model"]
            for q in np.flatnonzero(loop):
                loop[q] = 0
                rounds[q] += 1; nw_qp[q] += used[q]
                if rq["status"][q] != capi.QP_OPTIMAL:
                    flag[q], broke[q] = rq["status"][q], True
                    continue
                model[q] = step[q]
                if goes_on(q):
                    start_round(q)
    end = raw_results(qp)
    x_exp, obj_exp = end["x"].copy(), end["obj"].copy()
    for q in np.flatnonzero(done):
        hu = 0
        if rho_trial[q] > S["rho"][q]:
            ik = S["infea_k"][q]
            if not broke[q] and rho_trial[q] * ik - end["obj"][q] >= eps2 * rho_trial[q] * (ik - model[q]):
                S["succ"][q] += 1
                S["eps1"][q] = S["eps1"][q] + (1 - S["eps1"][q]) * parm
                S["rho"][q] = rho_trial[q]
            else:
                S["fail"][q] += 1
                model[q], hu = model0[q], capi.HU_PENALTY
                x_exp[offV[q]:offV[q + 1]] = x0[offV[q]:offV[q + 1]]; obj_exp[q] = obj0[q]
        out["infea_model"][q] = model[q]
        if have_infty[q]:
            out["infea_infty"][q] = infty[q]
        out["hu_word"][q], out["exitflag"][q] = hu, flag[q]
        out["nwsr_qp"][q], out["nwsr_lp"][q], out["rounds"][q] = nw_qp[q], nw_lp[q], rounds[q]
    return x_exp, obj_exp
