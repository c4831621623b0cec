"""A second opinion on the KKT certificate: qpOASESInterface's get_working_set and test_optimality restated in plain numpy and
evaluated in np.longdouble, with dense A and H built from the CSC arrays (repeated positions summed). Written from the behaviour that
restartsqp_amd/csrc/rsqp_kkt.h and oracle/kkt_oracle.c describe; it shares no code with either.

Besides the five fields the reference returns what a test needs to bound the rounding of another evaluation of the same sums:

  M[field]   the magnitude sum: the field's expression with every operation replaced by its absolute-value counterpart (|a||x| for a
             product, |u| + |v| for a difference). A primal term max(0, l - v) that is inactive beyond any rounding (l - v below
             -2^-30 of its own magnitude) is exactly 0 in every evaluation and adds nothing to M; that only tightens the bound
  n[field]   the number of summands
  k_max      the longest row or column dot product feeding them (stored entries, repeats counted)
  bound(f)   2^-52 (n + k_max + 4) M: the forward-error bound for two summations of the same terms in different orders, plus the dot
             products underneath
  tally      what each branch of the working-set mapping and of the per-entry rules contributed, by name
"""
import numpy as np

LD = np.longdouble
ABOVE, BELOW, BOTH, INACTIVE, INVALID = 1, -1, -99, 0, 12345
ERR_WORKING_SET = -4
EPS = LD(1.0e-8)           # sqrt_m_eps as the double constant the kernels and the oracle compare against
INFTY = 1.0e20
FIELDS = ("primal_violation", "dual_violation", "compl_violation", "stationarity_violation", "KKT_error")
U = LD(2.0) ** -52


def dense(nrow, ncol, jc, ir, val):
    """the matrix a CSC array describes, any order of rows within a column, repeated positions summed"""
    M = np.zeros((nrow, ncol), LD)
    jc = np.asarray(jc, np.int64)
    if nrow == 0 or ncol == 0 or jc[ncol] == 0:
        return M
    cols = np.repeat(np.arange(ncol), np.diff(jc[:ncol + 1]))
    np.add.at(M, (np.asarray(ir, np.int64)[:jc[ncol]], cols), np.asarray(val, np.float64)[:jc[ncol]].astype(LD))
    return M


def longest_product(nrow, ncol, jc, ir):
    """stored entries of the fullest row or column"""
    jc = np.asarray(jc, np.int64)
    nnz = int(jc[ncol])
    if nnz == 0:
        return 0
    percol = int(np.max(np.diff(jc[:ncol + 1])))
    perrow = int(np.max(np.bincount(np.asarray(ir, np.int64)[:nnz], minlength=max(nrow, 1))))
    return max(percol, perrow)


def clamp(v):
    return np.clip(np.asarray(v, np.float64), -INFTY, INFTY).astype(LD)


class Certificate:
    pass


def get_working_set(ws, val, lo, hi, signed):
    """solver +1 -> ACTIVE_ABOVE unless at (bounds: |val - lo| < eps; constraints: the SIGNED val - lo < eps) the lower side, then
    BOTH_SIDE; -1 -> ACTIVE_BELOW likewise against the upper side; 0 -> INACTIVE; anything else is invalid"""
    W = np.full(len(ws), INVALID, np.int32)
    dlo, dhi = val - lo, val - hi
    if not signed:
        dlo, dhi = np.abs(dlo), np.abs(dhi)
    for i, w in enumerate(ws):
        if w == 1:
            W[i] = BOTH if dlo[i] < EPS else ABOVE
        elif w == -1:
            W[i] = BOTH if dhi[i] < EPS else BELOW
        elif w == 0:
            W[i] = INACTIVE
    return W


def certificate(nV, nC, A, H, g, lb, ub, lbA, ubA, x, y, ws_b, ws_c):
    """A, H: (jc, ir, val), H may be None. Returns a Certificate: invalid, ok (1 / 0 / ERR_WORKING_SET), W_b, W_c, fields (dict of
    longdouble), values (the five as float64, in the order of FIELDS), M, n, k_max, bound(field), tally, Ax"""
    haveH = H is not None and H[0] is not None
    Ad = dense(nC, nV, *A)
    Hd = dense(nV, nV, *H) if haveH else np.zeros((nV, nV), LD)
    # the magnitudes take |value| entry by entry, before repeated positions are summed: the sum of a repeated position rounds too
    Aabs = dense(nC, nV, A[0], A[1], np.abs(A[2]))
    Habs = dense(nV, nV, H[0], H[1], np.abs(H[2])) if haveH else Hd
    x = np.asarray(x, np.float64).astype(LD)
    y = np.asarray(y, np.float64).astype(LD)
    g = np.asarray(g, np.float64).astype(LD)
    lb, ub, lbA, ubA = clamp(lb), clamp(ub), clamp(np.asarray(lbA, float).reshape(-1)), clamp(np.asarray(ubA, float).reshape(-1))
    ws_b, ws_c = np.asarray(ws_b, np.int64).reshape(-1), np.asarray(ws_c, np.int64).reshape(-1)
    yb, yc = y[:nV], y[nV:nV + nC]
    Ax, MAx = Ad @ x, Aabs @ np.abs(x)

    c = Certificate()
    c.Ax = Ax
    c.W_b = get_working_set(ws_b, x, lb, ub, signed=False)
    c.W_c = get_working_set(ws_c, Ax, lbA, ubA, signed=True)
    c.invalid = bool(np.any(c.W_b == INVALID) or np.any(c.W_c == INVALID))
    t = {}

    def primal_side(name, d, mag):      # d = l - v (lower side) or v - u (upper side): the term is max(0, d)
        term = np.maximum(LD(0), d)
        t[name] = term.sum()
        live = d > -(LD(2.0) ** -30) * mag
        return term.sum(), np.where(live, mag, LD(0)).sum()

    p1, m1 = primal_side("primal_lb", lb - x, np.abs(lb) + np.abs(x))
    p2, m2 = primal_side("primal_ub", x - ub, np.abs(ub) + np.abs(x))
    p3, m3 = primal_side("primal_lbA", lbA - Ax, np.abs(lbA) + MAx)
    p4, m4 = primal_side("primal_ubA", Ax - ubA, np.abs(ubA) + MAx)
    primal, Mprimal = p1 + p2 + p3 + p4, m1 + m2 + m3 + m4

    dual = compl = Mcompl = LD(0)
    for sfx, W, yv, val, mval, lo, hi in (("b", c.W_b, yb, x, np.abs(x), lb, ub), ("c", c.W_c, yc, Ax, MAx, lbA, ubA)):
        ina, bel, abv, both = W == INACTIVE, W == BELOW, W == ABOVE, W == BOTH
        neg, pos = yv < 0, yv > 0
        t["inactive_" + sfx] = np.abs(yv[ina]).sum()
        t["below_dual_" + sfx] = (-yv[bel & neg]).sum()
        t["above_dual_" + sfx] = yv[abv & pos].sum()
        t["both_ignored_" + sfx] = np.abs(yv[both]).sum()
        cb, ca = np.abs(yv * (val - lo)), np.abs(yv * (hi - val))
        t["below_compl_yneg_" + sfx] = cb[bel & neg].sum()
        t["below_compl_ypos_" + sfx] = cb[bel & pos].sum()
        t["above_compl_yneg_" + sfx] = ca[abv & neg].sum()
        t["above_compl_ypos_" + sfx] = ca[abv & pos].sum()
        dual = dual + t["inactive_" + sfx] + t["below_dual_" + sfx] + t["above_dual_" + sfx]
        compl = compl + t["inactive_" + sfx] + cb[bel].sum() + ca[abv].sum()
        Mcompl = Mcompl + np.abs(yv[ina]).sum() + (np.abs(yv) * (mval + np.abs(lo)))[bel].sum() \
            + (np.abs(yv) * (mval + np.abs(hi)))[abv].sum()

    stat = np.abs(Ad.T @ yc + yb - g - Hd @ x).sum()
    Mstat = (Aabs.T @ np.abs(yc) + np.abs(yb) + np.abs(g) + Habs @ np.abs(x)).sum()
    kkt = compl + stat + dual + primal

    c.fields = dict(zip(FIELDS, (primal, dual, compl, stat, kkt)))
    c.values = np.array([float(c.fields[f]) for f in FIELDS])
    c.M = dict(zip(FIELDS, (Mprimal, dual, Mcompl, Mstat, Mprimal + dual + Mcompl + Mstat)))
    c.n = dict(zip(FIELDS, (2 * (nV + nC), nV + nC, nV + nC, nV, 5 * (nV + nC) + 3)))
    c.k_max = max(longest_product(nC, nV, A[0], A[1]), longest_product(nV, nV, H[0], H[1]) if haveH else 0)
    c.tally = t
    c.ok = ERR_WORKING_SET if c.invalid else int(not (kkt > LD(1.0e-6)))
    return c


def bound(c, field):
    return float(U * (c.n[field] + c.k_max + 4) * c.M[field])


def of_problem(q, x, y, ws_b, ws_c, lp=False):
    """the certificate of a QPData-like problem (fields nV, nC, A_*, H_*, g, lb, ub, lbA, ubA); lp: H absent"""
    H = None if lp or getattr(q, "H_jc", None) is None else (q.H_jc, q.H_ir, q.H_val)
    return certificate(q.nV, q.nC, (q.A_jc, q.A_ir, q.A_val), H, q.g, q.lb, q.ub, q.lbA, q.ubA, x, y, ws_b, ws_c)


def guard_margin(c, nV, nC, lb, ub, lbA, ubA, x, ws_b, ws_c):
    """how far the point keeps from the thresholds of the working-set mapping, over the rows with a nonzero working-set entry: the
    smallest of | |x - side| - eps | / (1e-10 max(1, |x|)) (bounds) and |(Ax - side) - eps| / (1e-10 max(1, |Ax|)) (constraints).
    Above 1, another evaluation of Ax decides every row as the reference does; inf without such rows"""
    x = np.asarray(x, np.float64).astype(LD)
    m = LD(np.inf)
    for ws, val, lo, hi, signed in ((ws_b, x, clamp(lb), clamp(ub), False), (ws_c, c.Ax, clamp(lbA), clamp(ubA), True)):
        ws = np.asarray(ws, np.int64).reshape(-1)
        for i in np.nonzero((ws == 1) | (ws == -1))[0]:
            d = val[i] - (lo[i] if ws[i] == 1 else hi[i])
            if not signed:
                d = abs(d)
            m = min(m, abs(d - EPS) / (LD(1.0e-10) * max(LD(1), abs(val[i]))))
    return float(m)


def guard_of_problem(q, c, x, ws_b, ws_c):
    return guard_margin(c, q.nV, q.nC, q.lb, q.ub, q.lbA, q.ubA, x, ws_b, ws_c)
