"""Mirror of the caller side of the boundary: ``QPhandler`` (reference ``src/QPhandler.cpp``).

In RestartSQP this class stays as it is; it is restated here only so that tests and the
replay harness can drive ``HipQPInterface`` with exactly the call sequence
``Algorithm::setupQP`` produces (``src/Algorithm.cpp:645-697``): per-element virtual setters,
``set_A`` with the ``[J I -I]`` identity descriptor, ``solveQP`` followed by the mandatory
certificate. NEW_FORMULATION=false, non-QORE branch.
"""
import numpy as np

from . import capi
from .interface import HipQPInterface
from .sqptypes import INF, QP, QP_NOT_OPTIMAL, IdentityInfo, NLPInfo, Options


class QPhandler:
    def __init__(self, nlp_info: NLPInfo, qptype=QP, jnlst=None, options=None, device=-1):
        self.nlp_info_ = nlp_info
        self.nConstr_QP_ = nlp_info.nCon                       # QPhandler.cpp:39
        self.nVar_QP_ = nlp_info.nVar + 2 * nlp_info.nCon      # :40
        n, m = nlp_info.nVar, nlp_info.nCon
        self.I_info_A_ = IdentityInfo([1, 1], [n + 1, n + m + 1], [m, m], [1.0, -1.0])  # :41-51
        self.W_b_ = np.zeros(self.nVar_QP_, np.int32)
        self.W_c_ = np.zeros(self.nConstr_QP_, np.int32)
        self.solverInterface_ = HipQPInterface(nlp_info, qptype, options or Options(), jnlst, device=device)
        self.qpOptimalStatus_ = None

    def set_bounds(self, delta, x_l, x_u, x_k, c_l, c_u, c_k):  # :167-201
        s = self.solverInterface_
        n, m = self.nlp_info_.nVar, self.nlp_info_.nCon
        for i in range(m):
            s.set_lbA(i, c_l[i] - c_k[i])
            s.set_ubA(i, c_u[i] - c_k[i])
        for i in range(n):
            s.set_lb(i, max(x_l[i] - x_k[i], -delta))
            s.set_ub(i, min(x_u[i] - x_k[i], delta))
        for i in range(2 * m):
            s.set_ub(n + i, INF)

    def update_bounds(self, delta, x_l, x_u, x_k, c_l, c_u, c_k, refresh_ubA=False):  # :342-368 (ubA is NOT refreshed)
        """refresh_ubA=True is NOT the reference's behaviour: its qpOASES branch leaves ubA stale (QPhandler.cpp:358-360),
        which turns its own run infeasible after the first accepted step when a constraint is an equality; the whole-
        trajectory replay (tests/test_sqp_trajectory.py) needs the correct value and says so."""
        s = self.solverInterface_
        n, m = self.nlp_info_.nVar, self.nlp_info_.nCon
        for i in range(m):
            s.set_lbA(i, c_l[i] - c_k[i])
            if refresh_ubA:
                s.set_ubA(i, c_u[i] - c_k[i])
        for i in range(n):
            s.set_lb(i, max(x_l[i] - x_k[i], -delta))
            s.set_ub(i, min(x_u[i] - x_k[i], delta))

    def update_delta(self, delta, x_l, x_u, x_k):  # :533-567
        s = self.solverInterface_
        for i in range(self.nlp_info_.nVar):
            s.set_lb(i, max(x_l[i] - x_k[i], -delta))
            s.set_ub(i, min(x_u[i] - x_k[i], delta))

    def set_g(self, grad, rho):  # :272-297
        s = self.solverInterface_
        for i in range(self.nVar_QP_):
            s.set_g(i, grad[i] if i < self.nlp_info_.nVar else rho)

    def update_penalty(self, rho):  # :430-441
        for i in range(self.nlp_info_.nVar, self.nVar_QP_):
            self.solverInterface_.set_g(i, rho)

    def update_grad(self, grad):  # :450-463
        for i in range(self.nlp_info_.nVar):
            self.solverInterface_.set_g(i, grad[i])

    def set_H(self, hessian):  # :310-318
        self.solverInterface_.set_H(hessian)

    update_H = set_H           # :508-517

    def set_A(self, jacobian):  # :326-334
        self.solverInterface_.set_A(jacobian, self.I_info_A_)

    update_A = set_A           # :520-530

    def solveQP(self, stats=None, options=None):  # :470-499
        self.solverInterface_.optimizeQP(stats)
        if not self.test_optimality():
            raise QP_NOT_OPTIMAL("KKT certificate failed: %g" % self.solverInterface_.get_optimality_status().KKT_error)

    def solveLP(self, stats=None):  # include/sqphot/QPhandler.hpp:66-68
        self.solverInterface_.optimizeLP(stats)

    def test_optimality(self):  # :580-587
        self.qpOptimalStatus_ = self.solverInterface_.get_optimality_status()
        return self.solverInterface_.test_optimality(self.W_c_, self.W_b_)

    def get_optimal_solution(self):
        return self.solverInterface_.get_optimal_solution()

    def get_multipliers_bounds(self):
        return self.solverInterface_.get_multipliers_bounds()

    def get_multipliers_constr(self):
        return self.solverInterface_.get_multipliers_constr()

    def get_objective(self):
        return self.solverInterface_.get_obj_value()

    def get_status(self):
        return self.solverInterface_.get_status()

    def get_infea_measure_model(self):  # :592-594, oneNorm of the slack part
        x = self.solverInterface_.get_optimal_solution()
        return float(np.abs(x[self.nlp_info_.nVar:]).sum())


# ------------------------------------------------------------------------------------
# the handler of every member of a batch (rsqp_batch_handler_* of include/rsqp_hip.h)
# ------------------------------------------------------------------------------------
def batch_handler_reference(state, what, delta, rho, x_k, c_k, grad, n, m, x_l, x_u, c_l, c_u):
    """The update rule of rsqp_batch_handler_update restated in numpy: the expected value of every test.

    state: (g, lb, ub, lbA, ubA) pooled as Batch.set_vectors takes them; a new tuple is returned. n[q], m[q]: NLP variables and
    constraints of member q (its QP has n + 2 m variables). x_k, grad, x_l, x_u: NLP layout; c_k, c_l, c_u: constraint layout;
    what, delta, rho: one entry per member. Precedence as Algorithm::setupQP (src/Algorithm.cpp:645-697): SET (set_bounds + set_g,
    src/QPhandler.cpp:167-201, 272-297) includes everything; else BOUNDS (update_bounds, :342-368; ubA only with UBA) before DELTA
    (update_delta, :533-567); PENALTY (:430-441) and GRAD (:450-463; ignored without grad) beside them."""
    g, lb, ub, lbA, ubA = (np.array(a, dtype=np.float64) for a in state)
    oN = oC = oV = 0
    for q in range(len(n)):
        nq_, mq, W = int(n[q]), int(m[q]), int(what[q])
        N, Cc, V, S = slice(oN, oN + nq_), slice(oC, oC + mq), slice(oV, oV + nq_), slice(oV + nq_, oV + nq_ + 2 * mq)
        oN, oC, oV = oN + nq_, oC + mq, oV + nq_ + 2 * mq
        if W & capi.HU_SET:
            lbA[Cc] = c_l[Cc] - c_k[Cc]; ubA[Cc] = c_u[Cc] - c_k[Cc]
            lb[V] = np.maximum(x_l[N] - x_k[N], -delta[q]); ub[V] = np.minimum(x_u[N] - x_k[N], delta[q])
            lb[S] = 0.0; ub[S] = INF
            g[V] = 0.0 if grad is None else grad[N]
            g[S] = rho[q]
            continue
        if W & capi.HU_BOUNDS:
            lbA[Cc] = c_l[Cc] - c_k[Cc]
            if W & capi.HU_UBA:
                ubA[Cc] = c_u[Cc] - c_k[Cc]
        if W & (capi.HU_BOUNDS | capi.HU_DELTA):
            lb[V] = np.maximum(x_l[N] - x_k[N], -delta[q]); ub[V] = np.minimum(x_u[N] - x_k[N], delta[q])
        if W & capi.HU_PENALTY:
            g[S] = rho[q]
        if W & capi.HU_GRAD and grad is not None:
            g[V] = grad[N]
    return g, lb, ub, lbA, ubA


def batch_matrices_reference(Aval, Hval, what, jac, hess, nV, nC, Ajc_per_member, Hjc_per_member=None):
    """The rule of rsqp_batch_handler_set_matrices restated in numpy: the expected value of every test.

    Aval, Hval: the value pools in the layout of the batch's creation (Hval None: a batch without H); new arrays are returned.
    Member q has m = nC[q] constraints and n = nV[q] - 2 m NLP variables; Ajc_per_member[q] are the column pointers of its A (and
    Hjc_per_member[q] of its H, needed with Hval). With HM_JAC its entries of columns [0, n) -- the first Ajc[n] of the member, the J
    of A = [J I -I] (src/QPhandler.cpp:326-334, 520-530) -- are the member's next Ajc[n] entries of jac; the entries of the slack
    columns are never written. With HM_HESS its H entries are those of hess, which has the layout of Hval (:310-318, 508-517). A
    member with word 0 keeps everything; every member owns its share of jac and hess whatever its word says."""
    A = np.array(Aval, dtype=np.float64)
    H = None if Hval is None else np.array(Hval, dtype=np.float64)
    oA = oJ = oH = 0
    for q in range(len(nV)):
        jc = np.asarray(Ajc_per_member[q])
        n, W = int(nV[q]) - 2 * int(nC[q]), int(what[q])
        nj, na = int(jc[n]), int(jc[int(nV[q])])
        if W & capi.HM_JAC:
            A[oA:oA + nj] = np.asarray(jac, dtype=np.float64)[oJ:oJ + nj]
        oA, oJ = oA + na, oJ + nj
        if H is not None:
            nh = int(np.asarray(Hjc_per_member[q])[int(nV[q])])
            if W & capi.HM_HESS:
                H[oH:oH + nh] = np.asarray(hess, dtype=np.float64)[oH:oH + nh]
            oH += nh
    return A, H


def nlp_step_lanes(n, m):
    """G of include/rsqp_hip_nlp_step.h: lanes per member in the kernels of the NLP step, from the batch's largest QP"""
    nV = np.asarray(n, dtype=np.int64) + 2 * np.asarray(m, dtype=np.int64)
    return 8 if int(nV.max()) + int(np.max(m)) <= 16 else 64


def tree_sum(terms, G):
    """the sum of float64 terms in the order the header fixes: lane l adds the terms l, l + G, ... in index order, starting from
    0.0; the partial sums are then added pairwise, partners G/2, G/4, ..., 1 lanes apart. Every step is one float64 addition"""
    terms = np.asarray(terms, dtype=np.float64)
    v = np.zeros(G)
    for i, t in enumerate(terms):
        v[i % G] = v[i % G] + t
    lane, o = np.arange(G), G // 2
    while o > 0:
        v = v + v[lane ^ o]
        o //= 2
    return np.float64(v[0])


def cal_infea_reference(c, c_l, c_u, G):
    """cal_infea of one member (src/Algorithm.cpp:577-602, the call without x) with the terms added as tree_sum adds them"""
    c, c_l, c_u = (np.asarray(a, dtype=np.float64) for a in (c, c_l, c_u))
    with np.errstate(invalid="ignore"):
        terms = np.where(c < c_l, c_l - c, np.where(c > c_u, c - c_u, 0.0))
    return tree_sum(terms, G)


def batch_ratio_test_reference(options, what, rho, f_trial, c_trial, x_k, c_k, f_k, infea_k, delta, p, norm_p, qp_obj, n, m, c_l, c_u):
    """ratio_test + update_radius (src/Algorithm.cpp:722-801, 820-849) as rsqp_batch_handler_ratio_test states them, in numpy
    float64 scalars (which do not contract): the expected value of every test.

    options: a mapping with eta_s, eta_c, eta_e, gamma_c, gamma_e, delta_min, delta_max, tol, refresh_ubA. p (NLP layout), norm_p and
    qp_obj (one entry per member) are those of the last solve; the other arguments are the call's. Returns a dict: the in/out
    arrays x_k, c_k, f_k, infea_k, delta as new arrays and the seven outputs; a member with word 0 keeps its in/out entries and has
    NaN (doubles) / 0 (ints) in the outputs, where the call leaves what it found."""
    f8 = np.float64
    o = {k: (int(options[k]) if k == "refresh_ubA" else f8(options[k])) for k in
         ("eta_s", "eta_c", "eta_e", "gamma_c", "gamma_e", "delta_min", "delta_max", "tol", "refresh_ubA")}
    nq, G = len(n), nlp_step_lanes(n, m)
    r = {k: np.array(a, dtype=np.float64) for k, a in (("x_k", x_k), ("c_k", c_k), ("f_k", f_k), ("infea_k", infea_k), ("delta", delta))}
    for k in ("actual_reduction", "pred_reduction", "infea_trial"):
        r[k] = np.full(nq, np.nan)
    for k in ("accept", "hu_word", "hm_word", "exitflag"):
        r[k] = np.zeros(nq, np.int32)
    c_trial, p = np.asarray(c_trial, dtype=np.float64), np.asarray(p, dtype=np.float64)
    oN = oC = 0
    for q in range(nq):
        N, Cc = slice(oN, oN + int(n[q])), slice(oC, oC + int(m[q]))
        oN, oC = oN + int(n[q]), oC + int(m[q])
        if int(what[q]) == 0:
            continue
        rho_q, fk, ik, ft = f8(rho[q]), f8(r["f_k"][q]), f8(r["infea_k"][q]), f8(f_trial[q])
        with np.errstate(all="ignore"):
            it = cal_infea_reference(c_trial[Cc], c_l[Cc], c_u[Cc], G)
            actual = (fk + rho_q * ik) - (ft + rho_q * it)
            pred = rho_q * ik - f8(qp_obj[q])
            accept = bool(actual >= o["eta_s"] * pred and actual >= -o["tol"])
            d, radius = f8(r["delta"][q]), False
            if actual < o["eta_c"] * pred:
                d, radius = o["gamma_c"] * d, True
            elif actual > o["eta_e"] * pred and o["tol"] > abs(d - f8(norm_p[q])):
                grown = o["gamma_e"] * d
                d, radius = (o["delta_max"] if o["delta_max"] < grown else grown), True
        if accept:
            r["x_k"][N] = r["x_k"][N] + p[N]
            r["c_k"][Cc] = c_trial[Cc]
            r["f_k"][q], r["infea_k"][q] = ft, it
        r["delta"][q] = d
        r["actual_reduction"][q], r["pred_reduction"][q], r["infea_trial"][q], r["accept"][q] = actual, pred, it, int(accept)
        if accept:
            r["hu_word"][q] = capi.HU_BOUNDS | capi.HU_GRAD | (capi.HU_UBA if o["refresh_ubA"] else 0)
            r["hm_word"][q] = capi.HM_JAC | capi.HM_HESS
        elif radius:
            r["hu_word"][q] = capi.HU_DELTA
        r["exitflag"][q] = capi.EXIT_TRUST_REGION_TOO_SMALL if d < o["delta_min"] else capi.EXIT_UNKNOWN
    return r


EQUAL, BOUNDED, BOUNDED_BELOW, BOUNDED_ABOVE, UNBOUNDED = "EQUAL", "BOUNDED", "BOUNDED_BELOW", "BOUNDED_ABOVE", "UNBOUNDED"


def classify_single_constraint(lower_bound, upper_bound):
    """src/Utils.cpp:29-45 exactly as written: the second branch tests upper_bound > INF, so (finite, exactly 1e18) is UNBOUNDED"""
    if lower_bound > -INF and upper_bound < INF:
        return EQUAL if (upper_bound - lower_bound) < 1.0e-8 else BOUNDED
    elif lower_bound > -INF and upper_bound > INF:
        return BOUNDED_BELOW
    elif upper_bound < INF and lower_bound < -INF:
        return BOUNDED_ABOVE
    return UNBOUNDED


def batch_check_optimality_reference(options, what, x_k, grad, c_k, infea, lam_x, lam_c, J, n, m, x_l, x_u, c_l, c_u):
    """check_optimality (src/Algorithm.cpp:170-364) as rsqp_batch_handler_check_optimality states it: the expected value of every
    test. Products and differences are float64, as the C expressions are; the four sums are taken in np.longdouble.

    lam_x (NLP layout) and lam_c (constraint layout) are the multipliers of the last solve; J[q]: member q's Jacobian as a dense
    m x n array. Returns (status, verdict, scale): status [nq, 5] float64 over (primal, dual, compl, stationarity, KKT_error) --
    NaN for a member with word 0 --, verdict the bits, and scale [nq, 3, 2] = per sum (dual, compl, stationarity) the number of
    terms that enter it and the sum of the absolute values of all products that enter it (stationarity: every |J_ij lam_i|, |lam_x|
    and |grad|), from which a test derives its rounding bound."""
    L = np.longdouble
    tol = [np.float64(options[k]) for k in ("opt_prim_fea_tol", "opt_dual_fea_tol", "opt_compl_tol", "opt_stat_tol")]
    nq = len(n)
    status, verdict, scale = np.full((nq, 5), np.nan), np.zeros(nq, np.int32), np.zeros((nq, 3, 2))
    arrs = [np.asarray(a, dtype=np.float64) for a in (x_k, grad, c_k, lam_x, lam_c, x_l, x_u, c_l, c_u)]
    x_k, grad, c_k, lam_x, lam_c, x_l, x_u, c_l, c_u = arrs
    oN = oC = 0
    for q in range(nq):
        N, Cc = slice(oN, oN + int(n[q])), slice(oC, oC + int(m[q]))
        oN, oC = oN + int(n[q]), oC + int(m[q])
        if int(what[q]) == 0:
            continue
        dual, compl, kd, kc, sd, sc = L(0), L(0), 0, 0, L(0), L(0)
        with np.errstate(all="ignore"):
            for lo, up, v, lam in list(zip(x_l[N], x_u[N], x_k[N], lam_x[N])) + list(zip(c_l[Cc], c_u[Cc], c_k[Cc], lam_c[Cc])):
                t = classify_single_constraint(lo, up)
                if t == BOUNDED_ABOVE:
                    d, c = (np.float64(0.0) if lam < 0.0 else lam), abs(lam * (up - v))
                elif t == BOUNDED_BELOW:
                    d, c = -(np.float64(0.0) if 0.0 < lam else lam), abs(lam * (v - lo))
                elif t == UNBOUNDED:
                    d, c = None, abs(lam)
                else:
                    continue
                if d is not None:
                    dual, kd, sd = dual + L(d), kd + 1, sd + L(abs(d))
                compl, kc, sc = compl + L(c), kc + 1, sc + L(c)
            Jq = np.asarray(J[q], dtype=np.float64).reshape(int(m[q]), int(n[q]))
            prod = Jq * lam_c[Cc][:, None]                                    # float64 products, as the device forms them
            col = prod.astype(L).sum(axis=0) + lam_x[N].astype(L) - grad[N].astype(L)
            stat = np.abs(col).sum()
            ks = Jq.size + 2 * int(n[q])
            ss = np.abs(prod).astype(L).sum() + np.abs(lam_x[N]).astype(L).sum() + np.abs(grad[N]).astype(L).sum()
        primal = np.float64(infea[q])
        dual, compl, stat = np.float64(dual), np.float64(compl), np.float64(stat)
        status[q] = (primal, dual, compl, stat, dual + primal + compl + stat)
        bits = [primal < tol[0], dual < tol[1], compl < tol[2], stat < tol[3]]
        verdict[q] = sum(1 << k for k, b in enumerate(bits) if b) | (16 if all(bits) else 0)
        scale[q] = ((kd, float(sd)), (kc, float(sc)), (ks, float(ss)))
    return status, verdict, scale


class BatchQPhandler:
    """QPhandler for every member of a ``capi.Batch`` whose members have the (p, u, v) shape: the reference's method names, each with
    a member mask first. A call notes its arguments for the named members and ORs bits into a pending word per member;
    ``solveQP`` / ``solveLP`` flush all words -- ONE ``Batch.handler_set_matrices`` when set_A / set_H / update_A / update_H were
    called, then ONE ``Batch.handler_update`` -- and solve for the members given.

    Arrays are pooled over the batch (x_k, grad: NLP layout; c_k: the layout of lbA); only the named members' entries are read.
    delta and rho are scalars or one entry per member. on_device: x_k, c_k and grad are torch tensors on the batch's device, the
    words and the iterate stay there, and ``step(on_device=True)`` leaves the step data there as well. handover: members the
    register-resident tableau kernels give up on are re-solved on the Givens / TQ kernel inside the call, as a single QPhandler's
    solver does (``Batch.set_handover``); off by default, it costs a kernel launch per solve."""

    def __init__(self, batch, x_l, x_u, c_l=None, c_u=None, on_device=False, handover=False):
        self.batch, self.on_device = batch, bool(on_device)
        batch.set_handover(handover)
        batch.handler_set_problem(x_l, x_u, c_l, c_u)
        self.m = np.asarray(batch.nC, dtype=np.int64)
        self.n = np.asarray(batch.nV, dtype=np.int64) - 2 * self.m
        nq = batch.nq
        self.what = np.zeros(nq, np.int32)
        self._halves = np.zeros(nq, np.int32)          # 1 set_bounds seen, 2 set_g seen: SET is both (setupQP :645-660)
        self.delta, self.rho = np.zeros(nq), np.zeros(nq)
        self.have_grad = False
        memN, memC = np.repeat(np.arange(nq), self.n), np.repeat(np.arange(nq), self.m)
        sN, sC = int(self.n.sum()), int(self.m.sum())
        if self.on_device:
            torch = capi.device_torch()
            self._xp = torch
            dev = "cuda" if getattr(batch, "device", -1) < 0 else "cuda:%d" % batch.device
            self._memN, self._memC = torch.as_tensor(memN, device=dev), torch.as_tensor(memC, device=dev)
            z = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)
            self._dev = dev
        else:
            self._xp = np
            self._memN, self._memC = memN, memC
            z = np.zeros
        self.x_k, self.grad, self.c_k = z(sN), z(sN), z(sC)
        # the matrices: pending HM_* words, the members' J and H entries (Batch.handler_set_matrices), the words of the last flush
        self.mwhat = np.zeros(nq, np.int32)
        self.matrix_words = np.zeros(nq, np.int32)
        memJ = np.repeat(np.arange(nq), batch.jnz)
        memH = np.repeat(np.arange(nq), batch.hnnz) if batch.hnnz is not None else np.zeros(0, np.int64)
        if self.on_device:
            self._memJ, self._memH = torch.as_tensor(memJ, device=dev), torch.as_tensor(memH, device=dev)
        else:
            self._memJ, self._memH = memJ, memH
        self.jac, self.hess = z(memJ.size), z(memH.size)

    # -- bookkeeping --
    def _mask(self, members):
        m = np.ones(self.batch.nq, bool) if members is None else np.asarray(members) != 0
        if m.shape != (self.batch.nq,):
            raise ValueError("the mask has %d entries, the batch has %d members" % (m.size, self.batch.nq))
        return m

    def _take(self, name, src, mask, mem):
        """the named members' entries of a pooled array into the handler's copy"""
        if self.on_device:
            sel = self._xp.as_tensor(mask, device=self._dev)[mem]
            setattr(self, name, self._xp.where(sel, src, getattr(self, name)))
        else:
            setattr(self, name, np.where(mask[mem], np.asarray(src, dtype=np.float64), getattr(self, name)))

    def _bounds(self, mask, delta, x_k, c_k=None):
        self.delta = np.where(mask, delta, self.delta)
        self._take("x_k", x_k, mask, self._memN)
        if c_k is not None:
            self._take("c_k", c_k, mask, self._memC)

    # -- the reference's setters --
    def set_bounds(self, members, delta, x_k, c_k):                                   # QPhandler.cpp:167-201
        mask = self._mask(members)
        self._bounds(mask, delta, x_k, c_k)
        self._halves[mask] |= 1

    def set_g(self, members, grad, rho):                                              # :272-297; grad None: set_g(rho), :657-660
        mask = self._mask(members)
        self.rho = np.where(mask, rho, self.rho)
        if grad is not None:
            self._take("grad", grad, mask, self._memN)
            self.have_grad = True
        self._halves[mask] |= 2

    def update_bounds(self, members, delta, x_k, c_k, refresh_ubA=False):             # :342-368 (ubA stays stale: QPhandler above)
        mask = self._mask(members)
        self._bounds(mask, delta, x_k, c_k)
        self.what[mask] |= capi.HU_BOUNDS | (capi.HU_UBA if refresh_ubA else 0)

    def update_delta(self, members, delta, x_k):                                      # :533-567
        mask = self._mask(members)
        self._bounds(mask, delta, x_k)
        self.what[mask] |= capi.HU_DELTA

    def update_penalty(self, members, rho):                                           # :430-441
        mask = self._mask(members)
        self.rho = np.where(mask, rho, self.rho)
        self.what[mask] |= capi.HU_PENALTY

    def update_grad(self, members, grad):                                             # :450-463
        mask = self._mask(members)
        self._take("grad", grad, mask, self._memN)
        self.have_grad = True
        self.what[mask] |= capi.HU_GRAD

    def set_A(self, members, jac):                                                    # :326-334; jac: Batch.handler_set_matrices
        mask = self._mask(members)
        self._take("jac", jac, mask, self._memJ)
        self.mwhat[mask] |= capi.HM_JAC

    update_A = set_A                                                                  # :520-530

    def set_H(self, members, hess):                                                   # :310-318
        mask = self._mask(members)
        self._take("hess", hess, mask, self._memH)
        self.mwhat[mask] |= capi.HM_HESS

    update_H = set_H                                                                  # :508-517

    # -- flush and solve --
    def _flush_matrices(self):
        """one handler_set_matrices for the pending matrix words, which are kept in matrix_words"""
        self.matrix_words = self.mwhat.copy()
        self.mwhat[:] = 0
        w = self.matrix_words
        if not w.any():
            return
        jac = self.jac if (w & capi.HM_JAC).any() else None
        hess = self.hess if (w & capi.HM_HESS).any() else None
        if self.on_device:
            t = self._xp
            dw = t.as_tensor(w, device=self._dev)
            t.cuda.synchronize()                       # the inputs are complete before the call, as in flush()
            self.batch.handler_set_matrices(dw, jac, hess, on_device=True)
        else:
            self.batch.handler_set_matrices(w, jac, hess)

    def flush(self):
        """the matrices first, then the vectors, as Algorithm::setupQP orders them (src/Algorithm.cpp:645-697): one
        handler_set_matrices for the pending matrix words (none without any; they stay readable as matrix_words), one handler_update
        for everything else pending; returns the vector words it sent"""
        if np.any((self._halves != 0) & (self._halves != 3)):
            raise ValueError("set_bounds and set_g go together (Algorithm::setupQP, src/Algorithm.cpp:645-660)")
        self._flush_matrices()
        what = np.where(self._halves == 3, capi.HU_SET, self.what).astype(np.int32)
        self.what[:] = 0; self._halves[:] = 0
        if not what.any():
            return what
        grad = self.grad if self.have_grad else None
        if self.on_device:
            t = self._xp
            args = (t.as_tensor(what, device=self._dev), t.as_tensor(self.delta, device=self._dev),
                    t.as_tensor(self.rho, device=self._dev), self.x_k, self.c_k, grad)
            t.cuda.synchronize()                       # the inputs are complete before the call (torch fills them on its own stream)
            self.batch.handler_update(*args, on_device=True)
        else:
            self.batch.handler_update(what, self.delta, self.rho, self.x_k, self.c_k, grad)
        return what

    def _solve(self, members, run):
        self.flush()
        self.batch.set_members(None if members is None else self._mask(members))
        used = run()
        ok, kkt = self.batch.test_optimality()
        return used, ok, kkt

    def solveQP(self, members=None):                                                  # :470-499 + the certificate (:580-587)
        """flush, then optimize_qp for the members given (None: everybody) and the certificate: (nWSR_used, ok, KKT_error)"""
        return self._solve(members, self.batch.optimize_qp)

    def solveLP(self, members=None):                                                  # include/sqphot/QPhandler.hpp:66-68
        return self._solve(members, self.batch.optimize_lp)

    def step(self, on_device=None, out=None):
        """p, lam_c, lam_x, infea_model (get_infea_measure_model, :592-594) and norm_p of the last solve (Batch.handler_step)"""
        return self.batch.handler_step(self.on_device if on_device is None else on_device, out=out)


# ------------------------------------------------------------------------------------
# update_penalty_parameter per member (rsqp_batch_handler_update_penalty of include/rsqp_hip_penalty.h)
# ------------------------------------------------------------------------------------
def penalty_lp_data(st, qp):
    """setupLP (src/Algorithm.cpp:700-704) for one member: the data of its LP from the data `qp` of the QP just solved -- set_bounds
    from the iterate, set_g(rho) (zeros, then rho on the slacks), set_A with the QP's J. H stays what `qp` has: an LP solve ignores it"""
    import copy
    n, m = int(st["n"]), int(st["m"])
    d = copy.copy(qp)
    d.g = np.concatenate([np.zeros(n), np.full(2 * m, np.float64(st["rho"]))])
    d.lb = np.concatenate([np.maximum(st["x_l"] - st["x_k"], -st["delta"]), np.zeros(2 * m)])
    d.ub = np.concatenate([np.minimum(st["x_u"] - st["x_k"], st["delta"]), np.full(2 * m, INF)])
    d.lbA, d.ubA = st["c_l"] - st["c_k"], st["c_u"] - st["c_k"]
    return d


def batch_update_penalty_reference(qp_members, lp_members, state, options, G=8):
    """Algorithm::update_penalty_parameter (src/Algorithm.cpp:886-1028) per member, in plain Python with numpy float64 scalars (which
    do not contract), as rsqp_batch_handler_update_penalty states it: the expected value of every test.

    qp_members[q] / lp_members[q]: the member's two solver objects. Each has optimize(data, new_matrices=False) -> nWSR_used of the
    call (optimizeQP / optimizeLP on the QPData-like `data`; new_matrices: set_A comes first), and x, objective, status (the exit
    flag, capi.QP_OPTIMAL when solved) of its last solve; the QP member has just solved state[q]["qp"]. state[q]: a dict with what,
    qp (the data of that solve), n, m, infea_k, delta, x_k, c_k, x_l, x_u, c_l, c_u, rho, eps1, trial, succ, fail. options: a mapping
    over the fields of rsqp_penalty_options. G: lanes of the tree sums (nlp_step_lanes over the batch).

    Returns one dict per member: the state as the call leaves it (rho, eps1, trial, succ, fail), the outputs (infea_model,
    infea_infty -- None where no LP solved --, hu_word, exitflag, nwsr_qp, nwsr_lp, rounds), x and obj as the result pools hold them
    afterwards (the first solve's on the failure path), and for the tests' own checks: branch (None sat out, "qp_unsolved", "none",
    "lp_unsolved", "A", "B"), outcome (None, "success", "failure"), broke (left the loop on an unsolved QP), capped (left it at
    rho_max) and margins, the relative distance |a - b| / max(|a|, |b|) of every float comparison that decided something."""
    import copy
    f8 = np.float64
    o = {k: (int(options[k]) if k == "penalty_iter_max" else f8(options[k])) for k in
         ("penalty_update_tol", "increase_parm", "rho_max", "penalty_iter_max", "eps1_change_parm", "eps2")}
    out = []

    def slack_sum(x, n):
        return tree_sum(np.abs(np.asarray(x, dtype=np.float64)[n:]), G)

    for q, st in enumerate(state):
        r = dict(rho=f8(st["rho"]), eps1=f8(st["eps1"]), trial=int(st["trial"]), succ=int(st["succ"]), fail=int(st["fail"]),
                 infea_model=None, infea_infty=None, hu_word=0, exitflag=None, nwsr_qp=0, nwsr_lp=0, rounds=0, branch=None, outcome=None,
                 broke=False, capped=False, margins=[], x=None, obj=None)
        out.append(r)
        if int(st["what"]) == 0:
            continue
        Q, L = qp_members[q], lp_members[q]
        margins = r["margins"]

        def cmp(a, b):
            with np.errstate(all="ignore"):
                scale = max(abs(a), abs(b))
                margins.append(float(abs(a - b) / scale) if scale > 0 and np.isfinite(scale) else 1.0)

        if Q.status != capi.QP_OPTIMAL:
            r.update(branch="qp_unsolved", exitflag=int(Q.status))
            continue
        n, m = int(st["n"]), int(st["m"])
        infea_k, rho = f8(st["infea_k"]), f8(st["rho"])
        r["exitflag"] = capi.EXIT_UNKNOWN
        model = slack_sum(Q.x, n)
        r.update(x=np.array(Q.x), obj=f8(Q.objective), infea_model=model)
        cmp(model, o["penalty_update_tol"])
        if not model > o["penalty_update_tol"]:                                          # :893
            r["branch"] = "none"
            continue
        model0, rho_trial, x0, obj0 = model, rho, np.array(Q.x), f8(Q.objective)
        r["nwsr_lp"] = int(L.optimize(penalty_lp_data(st, st["qp"]), new_matrices=True))  # setupLP + solveLP (:896-899)
        if L.status != capi.QP_OPTIMAL:                                                  # :901-904
            r.update(branch="lp_unsolved", exitflag=int(L.status))
            continue
        infty = slack_sum(L.x, n)
        r["infea_infty"] = infty
        cmp(infty, o["penalty_update_tol"])
        r["branch"] = "A" if infty <= o["penalty_update_tol"] else "B"                  # :909
        data = copy.copy(st["qp"])
        while True:
            if r["branch"] == "A":                                                       # :914
                cmp(model, o["penalty_update_tol"])
                if not model > o["penalty_update_tol"]:
                    break
            else:                                                                        # :941-944
                lhs, rhs = infea_k - model, r["eps1"] * (infea_k - infty)
                cmp(lhs, rhs)
                if not (lhs < rhs and r["trial"] < o["penalty_iter_max"]):
                    break
            if rho_trial >= o["rho_max"]:                                                # :915, :947
                r["capped"] = True
                break
            nxt = rho_trial * o["increase_parm"]
            rho_trial = nxt if nxt < o["rho_max"] else o["rho_max"]                     # min(rho_max, rho_trial * increase_parm)
            r["trial"] += 1
            data.g = np.concatenate([np.asarray(st["qp"].g, dtype=np.float64)[:n], np.full(2 * m, rho_trial)])   # update_penalty
            r["nwsr_qp"] += int(Q.optimize(data))
            r["rounds"] += 1
            if Q.status != capi.QP_OPTIMAL:                                              # :929-932, :963-966
                r.update(broke=True, exitflag=int(Q.status))
                break
            model = slack_sum(Q.x, n)
        r["infea_model"] = model
        if rho_trial > rho:                                                              # :975
            if not r["broke"]:
                lhs, rhs = rho_trial * infea_k - f8(Q.objective), o["eps2"] * rho_trial * (infea_k - model)
                cmp(lhs, rhs)
            if not r["broke"] and lhs >= rhs:                                            # :979-981
                r["succ"] += 1
                r["eps1"] = r["eps1"] + (1 - r["eps1"]) * o["eps1_change_parm"]
                r["rho"] = rho_trial
                r.update(outcome="success", x=np.array(Q.x), obj=f8(Q.objective))
            else:
                r["fail"] += 1
                r.update(outcome="failure", infea_model=model0, hu_word=capi.HU_PENALTY, x=x0, obj=obj0)
    return out


# ------------------------------------------------------------------------------------
# second_order_correction per member (rsqp_batch_handler_soc_begin / _soc_end of include/rsqp_hip_soc.h)
# ------------------------------------------------------------------------------------
def hess_times_reference(qp, n, p):
    """(H_k p)_i, i < n, as rsqp_batch_handler_soc_begin forms it: from 0.0, + H_ij * p_j (one multiplication, one addition) over the
    entries of row i of the leading n x n block of qp's H (CSC, a row at most once per column) in increasing j"""
    jc, ir, val = np.asarray(qp.H_jc), np.asarray(qp.H_ir), np.asarray(qp.H_val, dtype=np.float64)
    out = np.zeros(n)
    for j in range(n):
        for k in range(int(jc[j]), int(jc[j + 1])):
            i = int(ir[k])
            if i < n:
                out[i] = out[i] + val[k] * np.float64(p[j])
    return out


def soc_qp_data(st, qp, p, c_trial, refresh_ubA=False):
    """the correction QP of one member (src/Algorithm.cpp:1181-1184) from the data `qp` of the QP just solved: update_grad(H_k p +
    grad_f), update_bounds at x_k + p with c_trial (ubA only with refresh_ubA); the slack part of g and the matrices stay"""
    import copy
    n = int(st["n"])
    d = copy.copy(qp)
    g = np.array(qp.g, dtype=np.float64)
    g[:n] = hess_times_reference(qp, n, p) + np.asarray(st["grad"], dtype=np.float64)
    xt = np.asarray(st["x_k"], dtype=np.float64) + np.asarray(p, dtype=np.float64)
    lb, ub = np.array(qp.lb, dtype=np.float64), np.array(qp.ub, dtype=np.float64)
    lb[:n] = np.maximum(st["x_l"] - xt, -np.float64(st["delta"])); ub[:n] = np.minimum(st["x_u"] - xt, np.float64(st["delta"]))
    d.g, d.lb, d.ub = g, lb, ub
    d.lbA = np.asarray(st["c_l"], dtype=np.float64) - c_trial
    d.ubA = (np.asarray(st["c_u"], dtype=np.float64) - c_trial) if refresh_ubA else np.array(qp.ubA, dtype=np.float64)
    return d


def batch_soc_reference(qp_members, state, options, soc_options, trial, G=8):
    """ratio_test, second_order_correction and update_radius of one SQP iteration (src/Algorithm.cpp:722-801, 1144-1211, 820-849) per
    member, in plain Python with numpy float64 scalars (which do not contract), as rsqp_batch_handler_soc_begin followed by
    rsqp_batch_handler_soc_end state them: the expected value of every test.

    qp_members[q]: the member's solver object with the optimize / x / objective / status interface of
    batch_update_penalty_reference; it has just solved state[q]["qp"]. state[q]: a dict with what (SOC_* bits), qp, n, m, x_k, c_k,
    f_k, infea_k, delta, rho, grad, x_l, x_u, c_l, c_u and optionally infea_model. options: a mapping over the fields of
    rsqp_nlp_step_options the calls read; soc_options: over rsqp_soc_options. trial(q, step) -> (f, c) at x_k + step: the caller's
    evaluators. G: lanes of the tree sums (nlp_step_lanes over the batch).

    Returns one dict per member: the iterate as the calls leave it (x_k, c_k, f_k, infea_k, delta), the outputs (actual_reduction,
    pred_reduction, infea_trial, accept, hu_word, hm_word, exitflag, x_trial, soc -- as soc_begin returns it --, qp_obj, nwsr_soc;
    None where nothing is written), x and obj as the result pools hold them afterwards, and for the tests' own checks: branch (None
    sat out, "no_correct" the word lacks CORRECT, "accepted" at once, "soc_unsolved", "soc_accepted", "soc_rejected"), radius
    ("shrunk", "grown", "unchanged"; None where update_radius did not run), too_small, and margins, the relative distance
    |a - b| / max(|a|, |b|) of every float comparison that decided something."""
    f8 = np.float64
    o = {k: (int(options[k]) if k == "refresh_ubA" else f8(options[k])) for k in
         ("eta_s", "eta_c", "eta_e", "gamma_c", "gamma_e", "delta_min", "delta_max", "tol", "refresh_ubA")}
    composite = int(soc_options.get("composite_pred", 0)) != 0
    accepted_hu = capi.HU_BOUNDS | capi.HU_GRAD | (capi.HU_UBA if o["refresh_ubA"] else 0)
    out = []
    for q, st in enumerate(state):
        n, m = int(st["n"]), int(st["m"])
        r = dict(x_k=np.array(st["x_k"], dtype=np.float64), c_k=np.array(st["c_k"], dtype=np.float64), f_k=f8(st["f_k"]),
                 infea_k=f8(st["infea_k"]), delta=f8(st["delta"]), actual_reduction=None, pred_reduction=None, infea_trial=None,
                 accept=None, hu_word=None, hm_word=None, exitflag=None, x_trial=None, soc=None, qp_obj=None, nwsr_soc=None, x=None,
                 obj=None, branch=None, radius=None, too_small=False, margins=[])
        out.append(r)
        W = int(st["what"])
        if W == 0:
            continue
        Q = qp_members[q]
        margins = r["margins"]
        rho = f8(st["rho"])
        c_l, c_u = np.asarray(st["c_l"], dtype=np.float64), np.asarray(st["c_u"], dtype=np.float64)

        def cmp(a, b):
            with np.errstate(all="ignore"):
                scale = max(abs(a), abs(b))
                margins.append(float(abs(a - b) / scale) if scale > 0 and np.isfinite(scale) else 1.0)

        def test(f_t, c_t, qp_obj):
            it = cal_infea_reference(c_t, c_l, c_u, G)
            actual = (r["f_k"] + rho * r["infea_k"]) - (f8(f_t) + rho * it)
            pred = rho * r["infea_k"] - f8(qp_obj)
            cmp(actual, o["eta_s"] * pred); cmp(actual, -o["tol"])
            return it, actual, pred, bool(actual >= o["eta_s"] * pred and actual >= -o["tol"])

        def radius(actual, pred, norm_p):
            d = r["delta"]
            cmp(actual, o["eta_c"] * pred)
            if actual < o["eta_c"] * pred:
                d, r["radius"] = o["gamma_c"] * d, "shrunk"
            else:
                cmp(actual, o["eta_e"] * pred)
                if actual > o["eta_e"] * pred:
                    cmp(o["tol"], abs(d - norm_p))
                if actual > o["eta_e"] * pred and o["tol"] > abs(d - norm_p):
                    grown = o["gamma_e"] * d
                    d, r["radius"] = (o["delta_max"] if o["delta_max"] < grown else grown), "grown"
                else:
                    r["radius"] = "unchanged"
            r["delta"] = d
            cmp(d, o["delta_min"])
            r["too_small"] = bool(d < o["delta_min"])
            r["exitflag"] = capi.EXIT_TRUST_REGION_TOO_SMALL if r["too_small"] else capi.EXIT_UNKNOWN

        def accept_step(step, f_t, c_t, it):
            r["x_k"] = r["x_k"] + step
            r["c_k"], r["f_k"], r["infea_k"] = np.array(c_t, dtype=np.float64), f8(f_t), it

        x0, obj0 = np.array(Q.x, dtype=np.float64), f8(Q.objective)
        p = x0[:n]
        f_t, c_t = trial(q, p)
        c_t = np.asarray(c_t, dtype=np.float64)
        it, actual, pred, acc = test(f_t, c_t, obj0)
        r.update(x=x0, obj=obj0)
        if acc or not (W & capi.SOC_CORRECT):
            r["branch"] = "accepted" if (W & capi.SOC_CORRECT) else "no_correct"
            radius(actual, pred, f8(np.abs(p).max()) if n else f8(0.0))
            if acc:
                accept_step(p, f_t, c_t, it)
            r.update(actual_reduction=actual, pred_reduction=pred, infea_trial=it, accept=int(acc), soc=0, nwsr_soc=0, qp_obj=obj0,
                     hu_word=accepted_hu if acc else (capi.HU_DELTA if r["radius"] != "unchanged" else 0),
                     hm_word=(capi.HM_JAC | capi.HM_HESS) if acc else 0)
            continue
        data = soc_qp_data(st, st["qp"], p, c_t, bool(o["refresh_ubA"]))
        r["nwsr_soc"] = int(Q.optimize(data))
        if Q.status != capi.QP_OPTIMAL:                                                  # :1190-1193
            r.update(branch="soc_unsolved", exitflag=int(Q.status), soc=0, x=None, obj=None)
            continue
        xs, obj_soc = np.array(Q.x, dtype=np.float64), f8(Q.objective)
        model = f8(st["infea_model"]) if st.get("infea_model") is not None else tree_sum(np.abs(x0[n:]), G)
        qp_obj = obj_soc + (obj0 - rho * model)                                          # :1198
        step = p + xs[:n]
        x_pool = xs.copy(); x_pool[:n] = step
        r.update(soc=1, x_trial=r["x_k"] + step)
        f_t, c_t = trial(q, step)
        c_t = np.asarray(c_t, dtype=np.float64)
        it, actual, pred, acc = test(f_t, c_t, qp_obj if composite else obj_soc)        # :1200-1201: get_obj_QP() is the correction's
        if acc:
            r.update(branch="soc_accepted", x=x_pool, obj=obj_soc, qp_obj=qp_obj, hm_word=capi.HM_JAC | capi.HM_HESS)
            norm_p = f8(np.abs(step).max())
            accept_step(step, f_t, c_t, it)
        else:                                                                            # :1202-1208
            r.update(branch="soc_rejected", x=x0, obj=obj0, qp_obj=obj0, hm_word=0)
            norm_p = f8(np.abs(p).max())
        radius(actual, pred, norm_p)
        r.update(actual_reduction=actual, pred_reduction=pred, infea_trial=it, accept=int(acc), hu_word=accepted_hu)
    return out
