"""Generated inputs of the certificate tests (test_certificate_reference.py on the CPU, test_gpu_certificate.py on the GPU): QPs with
a few entries per column and points (x, y, working set) that are NOT optimal, built so that every branch of the working-set mapping and
of the per-entry rules is taken. The GPU tests use exactly the inputs whose threshold guards the CPU test checks."""
import numpy as np

from restartsqp_amd.qpdump import QPData

A3_SHAPES = ((1, 0), (1, 3), (5, 0), (8, 2), (8, 8), (64, 64), (72, 32), (300, 511))
REF_SHAPES = ((1, 0), (1, 3), (8, 2), (8, 8), (40, 50), (300, 511))
ONE_HOT_SHAPES = ((256, 256), (257, 255), (300, 511), (511, 300))


class Case:
    def __init__(self, q, x, y, ws_b, ws_c):
        self.q, self.x, self.y, self.ws_b, self.ws_c = q, x, y, ws_b, ws_c


def sparse_csc(rng, nrow, ncol, per_col, draw, symmetric=False):
    """a CSC matrix with about per_col entries in a column (canonical: rows ascending, none repeated), values from draw(n)"""
    D = {}
    if nrow > 0:
        for c in range(ncol):
            for r in rng.choice(nrow, size=min(per_col, nrow), replace=False):
                v = float(draw(1)[0])
                D[(int(r), c)] = v
                if symmetric:
                    D[(c, int(r))] = v
    jc, ir, val = [0], [], []
    cols = {}
    for (r, c), v in D.items():
        cols.setdefault(c, []).append((r, v))
    for c in range(ncol):
        for r, v in sorted(cols.get(c, [])):
            ir.append(r); val.append(v)
        jc.append(len(ir))
    return np.array(jc, np.int32), np.array(ir, np.int32), np.array(val, np.float64)


def dense_of(nrow, ncol, jc, ir, val):
    M = np.zeros((nrow, ncol))
    for c in range(ncol):
        for k in range(jc[c], jc[c + 1]):
            M[ir[k], c] += val[k]
    return M


# distances from a side, by what they probe. Exact cases: 0, 2^-27 (below 1e-8), 2^-26 (above it), and plain gaps; a constraint's may
# be negative (the lower side shifted above Ax: BOTH_SIDE by the signed test). Real cases keep >= 1e-3 away from the threshold or sit on it
EXACT_GAPS = (0.0, 2.0 ** -27, 2.0 ** -26, 0.5, 1.25)
EXACT_NEG = (-2.0 ** -27, -2.0 ** -26, -0.5)


def make_case(rng, nV, nC, exact=False, mag=1.0, haveH=True, name=""):
    """a QP and a point for it. exact: every number is an integer or a dyadic rational small enough that every product and partial sum
    of the certificate is representable, in any order. mag scales the multipliers and the gradient (the size of the violation)"""
    if exact:
        ints = lambda n: rng.integers(-3, 4, size=n).astype(float)
        nz = lambda n: rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=n)
        real = lambda n: rng.integers(-32, 33, size=n) / 8.0
        ydraw = lambda n: rng.choice([-2.5, -1.0, -0.25, 0.0, 0.25, 1.0, 2.5], size=n)
        gaps, neg = EXACT_GAPS, EXACT_NEG
        shift = lambda: float(rng.choice([0.5, 1.25, 2.0]))
    else:
        ints = nz = lambda n: rng.normal(size=n)
        real = lambda n: rng.uniform(-4.0, 4.0, size=n)
        ydraw = lambda n: mag * rng.normal(size=n) * (rng.random(n) < 0.8)
        gaps, neg = None, None
        shift = lambda: float(rng.uniform(1.0e-3, 2.0))
    A = sparse_csc(rng, nC, nV, 3, nz)
    H = sparse_csc(rng, nV, nV, 2, nz, symmetric=True) if haveH else (None, None, None)
    x = real(nV)
    Ax = dense_of(nC, nV, *A) @ x
    g = (1.0 if exact else mag) * ints(nV)
    y = ydraw(nV + nC)

    def sides(val):
        """bounds around val and a working-set entry per row, cycling through the kinds of row"""
        n = len(val)
        lo, hi, ws = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
        kinds = rng.permutation(n) % 12
        for i, k in enumerate(kinds):
            v = val[i]
            gap = (lambda: float(rng.choice(gaps))) if exact else (lambda: 0.0 if rng.random() < 0.4 else shift())
            if k == 0:      # inactive, strictly inside
                lo[i], hi[i], ws[i] = v - shift(), v + shift(), 0
            elif k == 1:    # inactive, violated below
                lo[i], hi[i], ws[i] = v + shift(), v + 3.0, 0
            elif k == 2:    # inactive, violated above
                lo[i], hi[i], ws[i] = v - 3.0, v - shift(), 0
            elif k == 3:    # inactive, one or both sides infinite
                lo[i], hi[i], ws[i] = [(-np.inf, v + 1.0), (v - 1.0, np.inf), (-1.0e20, 1.0e20), (-np.inf, np.inf)][int(rng.integers(4))] + (0,)
            elif k in (4, 5):   # solver +1: at, near or above the lower side
                lo[i], hi[i], ws[i] = v - gap(), v + shift(), 1
            elif k in (6, 7):   # solver -1: at, near or below the upper side
                lo[i], hi[i], ws[i] = v - shift(), v + gap(), -1
            elif k == 8:    # equality / fixed variable, either sign of the entry
                lo[i] = hi[i] = v
                ws[i] = 1 if rng.random() < 0.5 else -1
            elif k == 9:    # solver +1 although the value is at the UPPER side: ACTIVE_ABOVE without a gap
                lo[i], hi[i], ws[i] = v - shift(), v, 1
            elif k == 10:   # solver -1 although the value is at the LOWER side
                lo[i], hi[i], ws[i] = v, v + shift(), -1
            else:           # a negative distance: the value beyond the side it is said to be active at (a constraint with the solver's
                            # -1 is ACTIVE_BELOW only here: the signed test calls every value at or below the upper side BOTH_SIDE)
                d = float(rng.choice(neg)) if exact else -shift()
                if rng.random() < 0.5:
                    lo[i], hi[i], ws[i] = v - d, v + 3.0, 1
                else:
                    lo[i], hi[i], ws[i] = v - 3.0, v + d, -1
        return lo, hi, ws

    lb, ub, ws_b = sides(x)
    lbA, ubA, ws_c = sides(Ax)
    q = QPData(nV, nC, H[0], H[1], H[2], A[0], A[1], A[2], g, lb, ub, lbA, ubA, name=name or "%dx%d" % (nV, nC))
    return Case(q, x, y, ws_b, ws_c)


def exact_cases():
    """the case set of the bit-exact test: small shapes, one with an empty A, one beyond 256 rows in both loops"""
    rng = np.random.default_rng(20261019)
    return [make_case(rng, nV, nC, exact=True) for nV, nC in ((1, 0), (1, 3), (8, 2), (7, 4), (8, 8), (24, 30), (64, 64), (300, 511))]


def real_cases(shapes=A3_SHAPES, seed=20261020, spread=True):
    """random real data; spread: the members' violations are powers of ten apart"""
    rng = np.random.default_rng(seed)
    return [make_case(rng, nV, nC, mag=10.0 ** (k - 2) if spread else 1.0) for k, (nV, nC) in enumerate(shapes)]


def refreshed(case):
    """the same point on the QP with new matrix values (same patterns): A scaled by 1.25, H by 0.5"""
    q = case.q
    q2 = QPData(q.nV, q.nC, q.H_jc, q.H_ir, 0.5 * q.H_val, q.A_jc, q.A_ir, 1.25 * q.A_val, q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name + "-refreshed")
    return Case(q2, case.x, case.y, case.ws_b, case.ws_c)


def noncanonical(rng, q):
    """the same QP with every column's entries reversed and some entries split in two (repeated positions)"""
    def scramble(jc, ir, val, ncol):
        njc, nir, nval = [0], [], []
        for c in range(ncol):
            ent = [(int(ir[k]), float(val[k])) for k in range(jc[c], jc[c + 1])][::-1]
            for r, v in ent:
                if rng.random() < 0.3:
                    part = float(rng.integers(-4, 5)) / 4.0
                    nir += [r, r]; nval += [part, v - part]
                else:
                    nir.append(r); nval.append(v)
            njc.append(len(nir))
        return np.array(njc, np.int32), np.array(nir, np.int32), np.array(nval, np.float64)
    A = scramble(q.A_jc, q.A_ir, q.A_val, q.nV)
    H = scramble(q.H_jc, q.H_ir, q.H_val, q.nV)
    return QPData(q.nV, q.nC, H[0], H[1], H[2], A[0], A[1], A[2], q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name + "-noncanonical")


def satisfied_qp(rng, nV, nC):
    """exact data and a point at which all four terms are exactly zero with y = 0 and an empty working set: x strictly inside its
    bounds, Ax strictly inside, g = -Hx. The one-hot test violates one entry of it at a time"""
    nz = lambda n: rng.choice([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0], size=n)
    A = sparse_csc(rng, nC, nV, 3, nz)
    H = sparse_csc(rng, nV, nV, 2, nz, symmetric=True)
    x = rng.integers(-32, 33, size=nV) / 8.0
    Ax = dense_of(nC, nV, *A) @ x
    g = -(dense_of(nV, nV, *H) @ x)
    q = QPData(nV, nC, H[0], H[1], H[2], A[0], A[1], A[2], g, x - 1.0, x + 2.0, Ax - 1.0, Ax + 2.0, name="satisfied-%dx%d" % (nV, nC))
    return Case(q, x, np.zeros(nV + nC), np.zeros(nV, np.int32), np.zeros(nC, np.int32))


ONE_HOT_KINDS = ("primal_b", "primal_c", "dual_b", "dual_c", "compl_b", "compl_c", "stat")


def one_hot(base, kind, idx):
    """a copy of a satisfied case with ONE violated entry: (case, field index 0..3, the term). idx counts variables for the _b kinds
    and stat, constraints for the _c kinds"""
    q = base.q
    g, lb, ub, lbA, ubA = (np.array(v, float) for v in (q.g, q.lb, q.ub, q.lbA, q.ubA))
    x, y, ws_b, ws_c = base.x.copy(), base.y.copy(), base.ws_b.copy(), base.ws_c.copy()
    A = dense_of(q.nC, q.nV, q.A_jc, q.A_ir, q.A_val)
    if kind == "primal_b":
        lb[idx] = x[idx] + 0.75; ub[idx] = x[idx] + 2.0
        field, term = 0, 0.75
    elif kind == "primal_c":
        ubA[idx] = A[idx] @ x - 0.5
        lbA[idx] = ubA[idx] - 1.0
        field, term = 0, 0.5
    elif kind == "dual_b":      # solver +1 with x at the UPPER side: ACTIVE_ABOVE, no gap, y > 0 is a dual violation alone
        ub[idx] = x[idx]; ws_b[idx] = 1; y[idx] = 1.5; g[idx] += 1.5
        field, term = 1, 1.5
    elif kind == "dual_c":
        ubA[idx] = A[idx] @ x; ws_c[idx] = 1; y[q.nV + idx] = 1.5; g += 1.5 * A[idx]
        field, term = 1, 1.5
    elif kind == "compl_b":     # ACTIVE_ABOVE with the right sign (y < 0) and a gap of 2 to the upper side
        ws_b[idx] = 1; y[idx] = -1.25; g[idx] -= 1.25
        field, term = 2, 2.5
    elif kind == "compl_c":
        ws_c[idx] = 1; y[q.nV + idx] = -1.25; g -= 1.25 * A[idx]
        field, term = 2, 2.5
    else:
        g[idx] += 1.5
        field, term = 3, 1.5
    q2 = QPData(q.nV, q.nC, q.H_jc, q.H_ir, q.H_val, q.A_jc, q.A_ir, q.A_val, g, lb, ub, lbA, ubA, name=q.name)
    return Case(q2, x, y, ws_b, ws_c), field, term


def one_hot_positions(n):
    """an index in each of the four waves of the first pass of the 256-thread loop, the first and one more of the second pass where
    there is one, and the last index"""
    pos = [p for p in (5, 70, 135, 200, 256, 299) if p < n]
    return sorted(set(pos + [n - 1]))
