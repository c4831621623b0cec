"""Non-canonical matrix input on the CPU side (no GPU): the contract of include/rsqp_hip.h says that a CSC array or a triplet
list describes the SUM of its entries, whatever the order of the rows within a column. The CPU oracle, its KKT certificate and
qpdump.csc_to_dense must read that matrix. The input transforms here are shared with tests/test_gpu_matrix_forms.py."""
import numpy as np

from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, csc_to_dense, dense_to_csc


# --------------------------------------------------------------------------
# the reference: the canonical form of any CSC array (rows ascending, repeats summed)
# --------------------------------------------------------------------------
def canonical_csc(nrow, ncol, jc, ir, val):
    jc = np.asarray(jc, np.int64); ir = np.asarray(ir, np.int64); val = np.asarray(val, float)
    col = np.repeat(np.arange(ncol), np.diff(jc))
    key = col * nrow + ir
    uk = np.unique(key)                       # column-major, rows ascending
    out = np.zeros(len(uk))
    np.add.at(out, np.searchsorted(uk, key), val)
    cjc = np.concatenate([[0], np.cumsum(np.bincount(uk // nrow, minlength=ncol))])
    return cjc.astype(np.int32), (uk % nrow).astype(np.int32), out


# --------------------------------------------------------------------------
# input transforms (each returns a CSC array whose canonical form is exactly the input's)
# --------------------------------------------------------------------------
def shuffle(rng, jc, ir, val):
    """the entries of every column in a random order (CSC input only: the triplet path sorts)"""
    ir = np.array(ir, np.int32); val = np.array(val, float)
    for c in range(len(jc) - 1):
        p = jc[c] + rng.permutation(jc[c + 1] - jc[c])
        ir[jc[c]:jc[c + 1]] = ir[p]; val[jc[c]:jc[c + 1]] = val[p]
    return np.array(jc, np.int32), ir, val


def split(rng, jc, ir, val, frac=1.0 / 3.0, only=None):
    """about `frac` of the entries v become two neighbouring entries 0.5 v, 0.5 v (exact in any order: the canonical form is the
    input bit for bit); `only` = list of entry indices to split instead"""
    pick = rng.random(len(val)) < frac if only is None else np.isin(np.arange(len(val)), only)
    njc, nir, nval = [0], [], []
    for c in range(len(jc) - 1):
        for k in range(jc[c], jc[c + 1]):
            if pick[k]:
                nir += [ir[k], ir[k]]; nval += [0.5 * val[k], 0.5 * val[k]]
            else:
                nir.append(ir[k]); nval.append(val[k])
        njc.append(len(nir))
    return np.array(njc, np.int32), np.array(nir, np.int32), np.array(nval, float)


def cancel(rng, nrow, jc, ir, val, t=0.75):
    """(r, c, +t), (r, c, -t) appended to a column at a position that has no entry: the canonical form stores a 0.0 there"""
    ncol = len(jc) - 1
    for c in rng.permutation(ncol):
        free = np.setdiff1d(np.arange(nrow), ir[jc[c]:jc[c + 1]])
        if len(free):
            r = int(rng.choice(free))
            e = jc[c + 1]
            nir = np.concatenate([ir[:e], [r, r], ir[e:]]).astype(np.int32)
            nval = np.concatenate([val[:e], [t, -t], val[e:]])
            njc = np.array(jc, np.int32); njc[c + 1:] += 2
            return njc, nir, nval
    raise ValueError("no free position")


def fullcount(rng, dense):
    """a dense matrix with one entry of a column dropped and another entry of the same column given twice (halves): the entry
    count is nrow * ncol, the canonical form has one entry less. Returns (jc, ir, val) and the matrix it describes."""
    nrow, ncol = dense.shape
    assert nrow >= 2 and np.all(dense != 0)
    c = int(rng.integers(ncol))
    r_drop, r_dup = rng.choice(nrow, 2, replace=False)
    M = dense.copy(); M[r_drop, c] = 0.0
    jc = np.arange(ncol + 1, dtype=np.int32) * nrow
    ir = np.tile(np.arange(nrow, dtype=np.int32), ncol)
    val = dense.T.reshape(-1).copy()
    k_drop, k_dup = c * nrow + r_drop, c * nrow + r_dup
    ir[k_drop] = r_dup
    val[k_drop] = 0.5 * dense[r_dup, c]; val[k_dup] = 0.5 * dense[r_dup, c]
    return (jc, ir, val), M


def mixed(rng, nrow, jc, ir, val):
    """split, then shuffle (the repeats land anywhere in their column)"""
    return shuffle(rng, *split(rng, jc, ir, val))


def with_matrices(q, A=None, H=None):
    A = A if A is not None else (q.A_jc, q.A_ir, q.A_val)
    H = H if H is not None else (q.H_jc, q.H_ir, q.H_val)
    return QPData(q.nV, q.nC, *H, *A, q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name)


def canonical_qp(q):
    return with_matrices(q, canonical_csc(q.nC, q.nV, q.A_jc, q.A_ir, q.A_val), canonical_csc(q.nV, q.nV, q.H_jc, q.H_ir, q.H_val))


def integer_dense(rng, nrow, ncol, density=1.0):
    M = rng.integers(-8, 9, size=(nrow, ncol)).astype(float)
    M[M == 0] = 1.0
    if density < 1.0:
        M *= rng.random((nrow, ncol)) < density
    return M


# --------------------------------------------------------------------------
def test_canonical_csc_is_the_dense_sum():
    rng = np.random.default_rng(5)
    for _ in range(20):
        nrow, ncol = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        n = int(rng.integers(0, 40))
        r = rng.integers(0, nrow, n); c = np.sort(rng.integers(0, ncol, n)); v = rng.normal(size=n)
        jc = np.concatenate([[0], np.cumsum(np.bincount(c, minlength=ncol))])
        D = np.zeros((nrow, ncol))
        np.add.at(D, (r, c), v)
        cjc, cir, cval = canonical_csc(nrow, ncol, jc, r, v)
        for col in range(ncol):
            assert np.all(np.diff(cir[cjc[col]:cjc[col + 1]]) > 0)
        assert len(cval) == len(set(zip(r.tolist(), c.tolist())))
        np.testing.assert_allclose(csc_to_dense(nrow, ncol, cjc, cir, cval), D, rtol=0, atol=1e-12)


def test_csc_to_dense_sums_repeats():
    jc = np.array([0, 3, 4]); ir = np.array([1, 0, 1, 1]); val = np.array([2.0, 5.0, 3.0, -4.0])
    assert np.array_equal(csc_to_dense(2, 2, jc, ir, val), np.array([[5.0, 0.0], [5.0, -4.0]]))


def test_transforms_keep_the_matrix():
    rng = np.random.default_rng(6)
    q = problems.random_qp(rng, 9, 7, 0.6)
    A = (q.A_jc, q.A_ir, q.A_val)
    for f in (lambda *a: shuffle(rng, *a), lambda *a: split(rng, *a)):
        jc, ir, val = f(*A)
        k = canonical_csc(q.nC, q.nV, jc, ir, val)
        assert all(np.array_equal(x, y) for x, y in zip(k, A))
    jc, ir, val = cancel(rng, q.nC, *A)
    assert len(val) == len(q.A_val) + 2
    k = canonical_csc(q.nC, q.nV, jc, ir, val)
    assert len(k[2]) == len(q.A_val) + 1 and np.count_nonzero(k[2] == 0.0) == 1
    np.testing.assert_array_equal(csc_to_dense(q.nC, q.nV, *k), q.dense_A())
    D = integer_dense(rng, 5, 4)
    (jc, ir, val), M = fullcount(rng, D)
    assert len(val) == D.size
    k = canonical_csc(5, 4, jc, ir, val)
    assert len(k[2]) == D.size - 1
    np.testing.assert_array_equal(csc_to_dense(5, 4, *k), M)


def _oracle_run(O, q, q2, A2, H2, forms):
    """init, hotstart (new vectors), hotstart_matrices (new values in the same layout) on the oracle; every step's results"""
    qp = O.OracleQP(q.nV, q.nC)
    qp.set_A_csc(*forms[0]); qp.set_H_csc(*forms[1])
    out = []
    rc, n = qp.init(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
    out.append((n, qp.exitflag(), qp.x.copy(), qp.y.copy(), qp.ws_bounds.copy(), qp.ws_constraints.copy(), qp.objective))
    rc, n = qp.hotstart(q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA, 1000)
    out.append((n, qp.exitflag(), qp.x.copy(), qp.y.copy(), qp.ws_bounds.copy(), qp.ws_constraints.copy(), qp.objective))
    qp.set_A_csc(forms[0][0], forms[0][1], A2); qp.set_H_csc(forms[1][0], forms[1][1], H2)
    rc, n = qp.hotstart_matrices(q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA, 1000)
    out.append((n, qp.exitflag(), qp.x.copy(), qp.y.copy(), qp.ws_bounds.copy(), qp.ws_constraints.copy(), qp.objective))
    return out


def _same(a, b):
    for sa, sb in zip(a, b):
        assert sa[0] == sb[0] and sa[1] == sb[1]
        for u, v in zip(sa[2:6], sb[2:6]):
            assert np.array_equal(u, v)
        assert sa[6] == sb[6]


def test_oracle_solves_the_matrix_the_input_describes(oracle):
    """about 40 seeded QPs: the oracle on the non-canonical input (shuffled rows, split entries, a cancelling pair) and on its
    canonical form -- identical x, y, working sets, status and nWSR through init, hotstart and hotstart_matrices"""
    rng = np.random.default_rng(20261016)
    for t in range(40):
        nV, nC = int(rng.integers(2, 14)), int(rng.integers(1, 12))
        q = problems.random_qp(rng, nV, nC, 0.5)
        if len(q.A_val) == 0:
            continue
        q2 = problems.perturb(rng, q, 0.05)
        A = mixed(rng, nC, q.A_jc, q.A_ir, q.A_val)
        A = cancel(rng, nC, *A) if t % 2 and len(q.A_val) < nC * nV else A
        H = mixed(rng, nV, q.H_jc, q.H_ir, q.H_val)
        # the refresh: new values in the caller's layout, and the canonical values they describe
        A2 = A[2] * (1.0 + 0.01 * rng.normal(size=len(A[2]))); H2 = H[2] * 1.05
        kA, kA2 = canonical_csc(nC, nV, *A), canonical_csc(nC, nV, A[0], A[1], A2)
        kH, kH2 = canonical_csc(nV, nV, *H), canonical_csc(nV, nV, H[0], H[1], H2)
        a = _oracle_run(oracle, q, q2, A2, H2, (A, H))
        b = _oracle_run(oracle, q, q2, kA2[2], kH2[2], (kA, kH))
        _same(a, b)
        assert a[0][1] == 20, (t, a[0][1])    # (RSQP_QP_OPTIMAL)


def test_oracle_certificate_reads_the_described_matrix(oracle):
    rng = np.random.default_rng(7)
    for t in range(20):
        nV, nC = int(rng.integers(2, 12)), int(rng.integers(1, 10))
        q = problems.random_qp(rng, nV, nC, 0.6)
        if len(q.A_val) == 0:
            continue
        qp = oracle.OracleQP(nV, nC)
        qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        qp.init(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
        A = mixed(rng, nC, q.A_jc, q.A_ir, q.A_val)
        A = cancel(rng, nC, *A) if len(q.A_val) < nC * nV else A
        H = mixed(rng, nV, q.H_jc, q.H_ir, q.H_val)
        kA, kH = canonical_csc(nC, nV, *A), canonical_csc(nV, nV, *H)
        res = []
        for AA, HH in ((A, H), (kA, kH)):
            Wb, Wc = oracle.kkt_get_working_set(nV, nC, AA, qp.x, q.lb, q.ub, q.lbA, q.ubA, qp.ws_bounds, qp.ws_constraints)
            ok, st = oracle.kkt_test_optimality(nV, nC, AA, HH, q.g, q.lb, q.ub, q.lbA, q.ubA, qp.x, qp.y, Wb, Wc)
            res.append((Wb, Wc, ok, (st.primal_violation, st.dual_violation, st.compl_violation, st.stationarity_violation,
                                     st.KKT_error)))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert res[0][2] == res[1][2] and res[0][3] == res[1][3]
        assert res[0][2]
