"""The dense f64 kernels (restartsqp_amd/csrc/dense_la.hip) in every build of k_dgemm and in the call forms the HBM-resident engine
uses, through the check entry points of include/rsqp_hip_dense_check.h: operands at an offset inside larger buffers, leading
dimensions that differ between operand and result, stale data (NaN) around the operands, in the triangle a routine does not
reference and in the workspace, one workspace over two factorisations. Every test asserts, through the plan export, which build or
variant it ran (tests/test_dense_plan.py pins the plans without a GPU).

References. Integer operands in [-8, 8] with alpha, beta powers of two: numpy's f64 product is exact, the comparison is
array_equal. Real data: a numpy.longdouble product and the entrywise bound (k + 2) 2^-53 (|alpha| |op A| |op B| + |beta| |C|), which
holds for any order of summation. Everything of a downloaded buffer that is not an addressed element (or that the contract says is
not written) holds a NaN of a fixed payload before the call and is compared as uint64 after it.

Bit-identity between layouts: the arithmetic of these kernels depends on shapes and thread indices, never on addresses or leading
dimensions, so a padded, offset, poisoned run must give the bits of the tight one."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
from restartsqp_amd import capi

pytestmark = pytest.mark.gpu

POISON = np.uint64(0x7FF80000DEADBEEF)
LAYOUTS = ("tight", "pad", "odd")
TRANS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def pad16(n):
    return (n + 15) // 16 * 16


def poisoned(n):
    return np.full(n, POISON, np.uint64).view(np.float64)


class Win:
    """a rows x cols operand inside a poisoned buffer. tight: the buffer is the operand; pad: ld = pad16(rows) + 16 (+ 16 per `which`,
    so that no two operands of a call share one), at a 16-double offset; odd: an odd ld at an odd offset (8-byte aligned only)"""

    def __init__(self, M, layout, which=0):
        rows, cols = M.shape
        self.rows, self.cols = rows, cols
        if layout == "tight":
            self.ld, self.off, tail = max(rows, 1), 0, 0
        elif layout == "pad":
            self.ld, self.off, tail = pad16(rows) + 16 * (1 + which), 16 * (1 + which), 40
        else:
            self.ld, self.off, tail = (rows | 1) + 2 * (1 + which), 2 * which + 1, 7
        self.buf = poisoned(self.off + self.ld * cols + tail + 1)
        self.window(self.buf)[...] = M
        self.before = self.buf.copy()

    def window(self, arr):
        """the operand's elements inside a buffer-sized array, as a rows x cols view (column-major, leading dimension ld)"""
        assert arr.size == self.buf.size >= self.off + self.ld * self.cols
        return np.lib.stride_tricks.as_strided(arr[self.off:], (self.rows, self.cols), (arr.itemsize, arr.itemsize * self.ld))

    def get(self):
        return self.window(self.buf).copy()

    def args(self):
        return self.buf.ctypes.data_as(capi.dp), self.buf.size, self.off, self.ld

    def assert_outside_untouched(self, written=None):
        """`written` (rows x cols, bool): the elements of the window the call may write; default all"""
        keep = np.ones(self.buf.size, bool)
        self.window(keep)[...] = False if written is None else ~written
        assert np.array_equal(self.buf.view(np.uint64)[keep], self.before.view(np.uint64)[keep])

    def assert_unchanged(self):
        assert np.array_equal(self.buf.view(np.uint64), self.before.view(np.uint64))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(float)


def run_gemm(variant, ta, tb, m, n, k, alpha, beta, A, B, C0, layout, ws_cap=0, written=None):
    """one call; A and B must come back as they went, nothing around C may change. Returns the C window"""
    wa, wc = Win(A, layout, 0), Win(C0, layout, 2)
    wb = Win(B, layout, 1) if B is not None else None
    bargs = wb.args() if wb else (None, 0, 0, 1)
    rc = capi.lib().rsqp_dense_check_gemm(variant, ta, tb, m, n, k, alpha, beta, *wa.args(), *bargs, *wc.args(), ws_cap)
    assert rc == 0, rc
    wa.assert_unchanged()
    if wb:
        wb.assert_unchanged()
    wc.assert_outside_untouched(written)
    return wc.get()


def operands(rng, ta, tb, m, n, k, gen=ints):
    A = gen(rng, (k, m) if ta else (m, k))
    B = gen(rng, (n, k) if tb else (k, n))
    return A, B, (A.T if ta else A), (B.T if tb else B)


# ---- GEMM: every build ------------------------------------------------------------------------------------------------------------

BUILD_CASES = [(bld, s) for bld, shapes in dc.GEMM_BUILD_SHAPES.items() for s in shapes]


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("bld,shape", BUILD_CASES, ids=["%dx%d-%dx%dx%d" % (b + s) for b, s in BUILD_CASES])
def test_gemm_build_is_exact_on_integers_in_every_layout(bld, shape, ta, tb):
    m, n, k = shape
    assert capi.describe_dense_gemm(m, n, k) == dict(TM=bld[0], TN=bld[1], splits=1, kc=k, skinny=0)
    rng = np.random.default_rng(m + 3 * n + 7 * k + 2 * ta + tb)
    A, B, opA, opB = operands(rng, ta, tb, m, n, k)
    C0 = ints(rng, (m, n))
    want = 0.5 * (opA @ opB) - 2.0 * C0
    tight = run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, 0.5, -2.0, A, B, C0, "tight")
    assert np.array_equal(tight, want)
    for layout in ("pad", "odd"):
        got = run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, 0.5, -2.0, A, B, C0, layout)
        assert np.array_equal(bits(got), bits(tight)), layout


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("bld", sorted(dc.GEMM_REAL_SHAPES), ids=lambda b: "%dx%d" % b)
def test_gemm_build_on_real_data_within_the_summation_bound(bld, ta, tb):
    m, n, k = dc.GEMM_REAL_SHAPES[bld]
    assert dc.build(capi.describe_dense_gemm(m, n, k)) == bld and m * n * k <= 2e7
    rng = np.random.default_rng(m + n + k + 2 * ta + tb)
    A, B, opA, opB = operands(rng, ta, tb, m, n, k, gen=lambda r, s: r.normal(size=s))
    C0 = rng.normal(size=(m, n))
    alpha, beta = 0.7, -1.3
    got = run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, alpha, beta, A, B, C0, "pad")
    ld = np.longdouble
    want = ld(alpha) * (opA.astype(ld) @ opB.astype(ld)) + ld(beta) * C0.astype(ld)
    bound = (k + 2) * 2.0 ** -53 * (abs(alpha) * (np.abs(opA) @ np.abs(opB)) + abs(beta) * np.abs(C0))
    err = np.abs(got.astype(ld) - want)
    assert np.all(err <= bound), float(np.max(err / bound))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_gemm_edge_cases(layout):
    """k = 0 gives beta C; m = 0 or n = 0 writes nothing; beta = 0 does not read C (NaN there, a finite exact result); alpha = 0"""
    rng = np.random.default_rng(11)
    m, n, k = 70, 45, 19
    A, B, opA, opB = operands(rng, 0, 0, m, n, k)
    C0 = ints(rng, (m, n))
    P = capi.DENSE_GEMM_PLAIN
    assert np.array_equal(run_gemm(P, 0, 0, m, n, 0, 0.5, -2.0, A[:, :0], B[:0, :], C0, layout), -2.0 * C0)
    assert np.array_equal(run_gemm(P, 0, 0, m, n, 0, 0.5, 0.0, A[:, :0], B[:0, :], poisoned(m * n).reshape(m, n), layout), np.zeros((m, n)))
    run_gemm(P, 0, 0, 0, n, k, 0.5, -2.0, A[:0, :], B, C0[:0, :], layout)       # (run_gemm asserts that no buffer changed)
    run_gemm(P, 0, 0, m, 0, k, 0.5, -2.0, A, B[:, :0], C0[:, :0], layout)
    got = run_gemm(P, 0, 0, m, n, k, 0.5, 0.0, A, B, poisoned(m * n).reshape(m, n), layout)
    assert np.array_equal(got, 0.5 * (opA @ opB))
    assert np.array_equal(run_gemm(P, 0, 0, m, n, k, 0.0, -2.0, A, B, C0, layout), -2.0 * C0)
    assert np.array_equal(run_gemm(P, 0, 0, m, n, k, 0.0, 0.0, A, B, poisoned(m * n).reshape(m, n), layout), np.zeros((m, n)))


# ---- split K ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ta,tb", [(1, 0), (0, 0)])
@pytest.mark.parametrize("shape", sorted(dc.SPLITK_SHAPES), ids=lambda s: "%dx%dx%d" % s)
def test_split_k_is_exact_deterministic_and_applies_beta_once(shape, ta, tb):
    """the partial products go to slabs of a workspace the entry point fills with NaN (a slab element no slice wrote, or a result
    that read C's slot of the workspace, would show), the last slice is partial, and the sum is taken in slice order"""
    m, n, k = shape
    plan, cap, last = dc.SPLITK_SHAPES[shape]
    assert capi.describe_dense_gemm(m, n, k, ws_cap=cap) == plan and k - (plan["splits"] - 1) * plan["kc"] == last
    rng = np.random.default_rng(k)
    A, B, opA, opB = operands(rng, ta, tb, m, n, k)
    C0 = ints(rng, (m, n))
    want = 0.5 * (opA @ opB) + C0
    runs = [run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, 0.5, 1.0, A, B, C0, layout, ws_cap=cap) for layout in ("tight", "tight", "pad", "odd")]
    assert np.array_equal(runs[0], want)
    for r in runs[1:]:
        assert np.array_equal(bits(r), bits(runs[0]))
    # beta = 0 under split K: C is not read
    got = run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, -2.0, 0.0, A, B, poisoned(m * n).reshape(m, n), "pad", ws_cap=cap)
    assert np.array_equal(got, -2.0 * (opA @ opB))
    # real data: the same bits twice, inside the bound
    A, B, opA, opB = operands(rng, ta, tb, m, n, k, gen=lambda r, s: r.normal(size=s))
    r1 = run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, 0.7, 1.0, A, B, C0, "tight", ws_cap=cap)
    r2 = run_gemm(capi.DENSE_GEMM_PLAIN, ta, tb, m, n, k, 0.7, 1.0, A, B, C0, "pad", ws_cap=cap)
    assert np.array_equal(bits(r1), bits(r2))
    if m * n * k <= 2e7:
        ld = np.longdouble
        want = ld(0.7) * (opA.astype(ld) @ opB.astype(ld)) + C0.astype(ld)
        bound = (k + 2) * 2.0 ** -53 * (0.7 * (np.abs(opA) @ np.abs(opB)) + np.abs(C0))
        assert np.all(np.abs(r1.astype(ld) - want) <= bound)


# ---- upper ------------------------------------------------------------------------------------------------------------------------

def skipped_tiles(n, bld):
    """elements (i, j) of an n x n result in tiles strictly below the diagonal: first row of the tile >= one past its last column"""
    i0 = (np.arange(n) // bld[0] * bld[0])[:, None]
    j0 = (np.arange(n) // bld[1] * bld[1])[None, :]
    return i0 >= j0 + bld[1]


@pytest.mark.parametrize("nk", sorted(dc.UPPER_SHAPES), ids=lambda s: "n%d-k%d" % s)
def test_upper_with_beta_1_over_a_stale_lower_triangle(nk):
    """rsqp_dgemm_upper as the Cholesky factorisation's trailing update calls it (A'B, beta = 1): entries on and above the diagonal
    exact and those of the plain product; tiles strictly below the diagonal skipped -- they keep the NaN they held; nothing outside"""
    n, k = nk
    bld = dc.UPPER_SHAPES[nk]
    assert dc.build(capi.describe_dense_gemm(n, n, k)) == bld
    rng = np.random.default_rng(n)
    A, B, opA, opB = operands(rng, 1, 0, n, n, k)
    Cup = np.triu(ints(rng, (n, n)))
    C0 = Cup.copy()
    C0[np.tril_indices(n, -1)] = poisoned(1)[0]
    want = -0.5 * (opA @ opB) + Cup
    up = np.triu(np.ones((n, n), bool))
    skip = skipped_tiles(n, bld)
    assert skip.any() and not (skip & up).any()
    plain = run_gemm(capi.DENSE_GEMM_PLAIN, 1, 0, n, n, k, -0.5, 1.0, A, B, Cup, "tight")
    assert np.array_equal(plain, want)
    for layout in LAYOUTS:
        got = run_gemm(capi.DENSE_GEMM_UPPER, 1, 0, n, n, k, -0.5, 1.0, A, B, C0, layout, written=~skip)
        assert np.array_equal(got[up], want[up]), layout
        assert np.array_equal(bits(got[up]), bits(plain[up])), layout
    # as dual_setup_blocked forms its Gram matrix: beta = 0. (Under beta = 1 a tile that was NOT skipped would leave its NaN as it was,
    # payload included: v + 1.0 * NaN is that NaN. Here it would write numbers over them.)
    got = run_gemm(capi.DENSE_GEMM_UPPER, 1, 0, n, n, k, -0.5, 0.0, A, B, poisoned(n * n).reshape(n, n), "pad", written=~skip)
    assert np.array_equal(got[up], (-0.5 * (opA @ opB))[up])


# ---- triangular operands ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sorted(dc.KTRI_SIZES))
def test_ktri_products_keep_the_bits_of_the_plain_product(n):
    """ktri = 1 (rsqp_dtrmmt_upper, X X'), 2 (A upper triangular, as setup_wz_blocked forms Wz and as the triangular inverse's second
    product) and 3 (A' with A upper triangular, its first product): the part of the inner dimension they skip multiplies exact
    zeros, so the plain product of the same operands has the same bits"""
    bld = dc.KTRI_SIZES[n]
    assert dc.build(capi.describe_dense_gemm(n, n, n)) == bld
    rng = np.random.default_rng(n)
    T = np.triu(ints(rng, (n, n)))
    Bm = ints(rng, (n, n))
    C0 = ints(rng, (n, n))
    up = np.triu(np.ones((n, n), bool))
    P, K1, K2, K3 = capi.DENSE_GEMM_PLAIN, capi.DENSE_GEMM_KTRI1, capi.DENSE_GEMM_KTRI2, capi.DENSE_GEMM_KTRI3
    # the largest size runs the engine's own transpose pairs in the padded layout only (the test stays within seconds)
    layouts, tbs = (("tight", "pad"), (1, 0)) if n < 1000 else (("pad",), (1,))
    # 1: C = alpha T T', upper tiles, beta = 0 over NaN
    skip = skipped_tiles(n, bld)
    nanC = poisoned(n * n).reshape(n, n)
    plain = run_gemm(P, 0, 1, n, n, n, 0.5, 0.0, T, T, nanC, "tight")
    assert np.array_equal(plain, 0.5 * (T @ T.T))
    for layout in layouts:
        got = run_gemm(K1, 0, 1, n, n, n, 0.5, 0.0, T, None, nanC, layout, written=~skip)
        assert np.array_equal(bits(got[up]), bits(plain[up])), layout
    # 2 as Wz = Ui Ui' is formed: both operands the same triangular matrix, beta = 0, both triangles of the result
    got = run_gemm(K2, 0, 1, n, n, n, 0.5, 0.0, T, T, nanC, "pad")
    assert np.array_equal(bits(got), bits(plain))
    # 2: C = alpha T op(B) + beta C
    for tb in tbs:
        plain = run_gemm(P, 0, tb, n, n, n, -2.0, 0.5, T, Bm, C0, "tight")
        assert np.array_equal(plain, -2.0 * (T @ (Bm.T if tb else Bm)) + 0.5 * C0)
        for layout in layouts:
            got = run_gemm(K2, 0, tb, n, n, n, -2.0, 0.5, T, Bm, C0, layout)
            assert np.array_equal(bits(got), bits(plain)), (tb, layout)
    # 3: C = alpha T' op(B) + beta C
    for tb in tbs:
        plain = run_gemm(P, 1, tb, n, n, n, 0.5, -2.0, T, Bm, C0, "tight")
        assert np.array_equal(plain, 0.5 * (T.T @ (Bm.T if tb else Bm)) - 2.0 * C0)
        for layout in layouts:
            got = run_gemm(K3, 1, tb, n, n, n, 0.5, -2.0, T, Bm, C0, layout)
            assert np.array_equal(bits(got), bits(plain)), (tb, layout)


# ---- factorisations ---------------------------------------------------------------------------------------------------------------

class Work:
    def __init__(self, mmax):
        self.h = C.c_void_p()
        assert capi.lib().rsqp_dense_check_work_create(mmax, C.byref(self.h)) == 0

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        assert capi.lib().rsqp_dense_check_work_destroy(self.h) == 0


def test_factorisation_entries_refuse_what_does_not_fit():
    """with a workspace in hand (tests/test_dense_plan.py has the refusals that need none): more rows than the workspace serves,
    m < n, a leading dimension below the rows, an operand that ends past its buffer, an unknown form -- all before anything runs"""
    L = capi.lib()
    m, n = 6, 4
    bufs = [np.zeros(k) for k in (m * n, m * m, n * n)]
    Bp, Qp, Xp = (b.ctypes.data_as(capi.dp) for b in bufs)
    f = np.full(4, 9, np.int32); fp = f.ctypes.data_as(capi.ip)
    r = C.c_int(7)
    with Work(m) as h:
        def qr(m=m, n=n, B=(Bp, m * n, 0, m), Q=(Qp, m * m, 0, m), X=(Xp, n * n, 0, n), flags=fp, ret=C.byref(r)):
            return L.rsqp_dense_check_qr(h, m, n, 1, 0, 1e-9, *B, *Q, *X, flags, ret)

        def chol(n=n, form=0, G=(Xp, n * n, 0, n), X=(Xp, n * n, 0, n), Gi=(Xp, n * n, 0, n), flags=fp):
            return L.rsqp_dense_check_chol(h, n, form, 0, 1e-10, 0.0, *G, *X, *Gi, flags)

        for kw in (dict(m=m + 1), dict(m=n - 1), dict(n=0), dict(B=(Bp, m * n, 0, m - 1)), dict(B=(Bp, m * n, 1, m)), dict(B=(None, m * n, 0, m)),
                   dict(Q=(Qp, m * m - 1, 0, m)), dict(Q=(Qp, m * m, 0, m + 1)), dict(X=(Xp, n * n, -1, n)), dict(X=(Xp, n * n, 0, n - 1)),
                   dict(flags=None), dict(ret=None)):
            assert qr(**kw) == capi.ERR_ARG, kw
        for kw in (dict(n=m + 1), dict(n=0), dict(form=-1), dict(form=3), dict(G=(Xp, n * n, 0, n - 1)), dict(X=(Xp, n * n, 1, n)),
                   dict(Gi=(None, n * n, 0, n)), dict(Gi=(Xp, n * n - 1, 0, n)), dict(flags=None)):
            assert chol(**kw) == capi.ERR_ARG, kw
    assert r.value == 7 and (f == 9).all() and not any(b.any() for b in bufs)


def run_qr(h, B0, layout, cholqr=1, poison=0, eps_li=1e-9):
    m, n = B0.shape
    wb = Win(B0, layout, 0)
    wq = Win(poisoned(m * m).reshape(m, m), layout, 1)
    wx = Win(poisoned(n * n).reshape(n, n), layout, 2)
    flags = np.full(4, -1, np.int32)
    retried = C.c_int(-1)
    rc = capi.lib().rsqp_dense_check_qr(h, m, n, cholqr, poison, eps_li, *wb.args(), *wq.args(), *wx.args(), flags.ctypes.data_as(capi.ip),
                                        C.byref(retried))
    assert rc == 0, rc
    for w in (wb, wq, wx):
        w.assert_outside_untouched()
    return wb.get(), wq.get(), wx.get(), flags.tolist(), retried.value


def qr_residuals(B0, B, Q, Ri):
    """the residual lines of tests/test_gpu_dense.py::test_blocked_qr"""
    m, n = B0.shape
    R = np.triu(B[:n, :])
    assert np.max(np.abs(Q.T @ Q - np.eye(m))) < 1e-12
    assert np.max(np.abs(Q[:, :n] @ R - B0)) < 1e-12 * max(1.0, np.abs(B0).max()) * m
    if m > n:
        assert np.max(np.abs(Q[:, n:].T @ B0)) < 1e-12 * m      # null-space basis of B0'
    assert np.max(np.abs(Ri @ R - np.eye(n))) < 1e-10
    assert np.max(np.abs(np.tril(Ri, -1))) == 0.0


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def qr_plans_equal(m, n, mmax_a, mmax_b):
    """does every product of the factorisation that is given the workspace's split-K slabs get the same plan at both workspace sizes?"""
    return all(capi.describe_dense_gemm(*s, ws_cap=4 * dc.OB * mmax_a) == capi.describe_dense_gemm(*s, ws_cap=4 * dc.OB * mmax_b)
               for s in dc.qr_ws_products(m, n))


@pytest.mark.parametrize("cholqr", [1, 0])
@pytest.mark.parametrize("m,n", dc.QR_SHAPES)
def test_qr_in_the_engines_call_form(m, n, cholqr):
    """rsqp_dgeqrf + rsqp_dtrtri_upper + rsqp_dorgqr. 128 x 64 is the smallest Cholesky-QR panel (64 columns, 128 rows below its
    diagonal: cholqr = 1 takes it there and in 200 x 130, 700 x 450, 300 x 300, 320 x 320); 320 columns are two outer blocks"""
    rng = np.random.default_rng(m + n)
    B0 = rng.normal(size=(m, n))
    with Work(m) as h:
        ref = run_qr(h, B0, "tight", cholqr)
    assert ref[3] == [0, 0, 0, 0] and ref[4] == 0
    qr_residuals(B0, *ref[:3])
    # padded, mutually different leading dimensions, offsets, NaN around the operands and in every array of the workspace
    for layout in ("pad", "odd"):
        with Work(m) as h:
            got = run_qr(h, B0, layout, cholqr, poison=1)
        assert got[3:] == ref[3:] and same_bits(got[:3], ref[:3]), layout
    # a workspace for twice the rows: other strides inside V, W, Q1 and another split-K capacity
    with Work(2 * m) as h:
        got = run_qr(h, B0, "pad", cholqr, poison=1)
    qr_residuals(B0, *got[:3])
    assert qr_plans_equal(m, n, m, 2 * m)
    assert got[3:] == ref[3:] and same_bits(got[:3], ref[:3])


def test_two_qr_factorisations_on_one_workspace():
    """the engine's dw: sized for the largest problem, reused -- the second, smaller factorisation finds the first one's reflectors,
    T factors and products in every array"""
    rng = np.random.default_rng(5)
    big, small = rng.normal(size=(700, 450)), rng.normal(size=(200, 130))
    with Work(200) as h:
        ref = run_qr(h, small, "tight")
    with Work(700) as h:
        first = run_qr(h, big, "pad", poison=1)
        second = run_qr(h, small, "pad")
        third = run_qr(h, rng.normal(size=(129, 1)), "odd")
    qr_residuals(big, *first[:3])
    qr_residuals(small, *second[:3])
    assert first[3] == second[3] == third[3] == [0, 0, 0, 0]
    assert qr_plans_equal(200, 130, 200, 700)
    assert same_bits(second[:3], ref[:3])


def run_chol(h, G, layout, form, poison=0, pd_rel=1e-10, pd_abs=1e-25):
    n = G.shape[0]
    wg = Win(G, layout, 0)
    wx = Win(poisoned(n * n).reshape(n, n), layout, 1)
    wi = Win(poisoned(n * n).reshape(n, n), layout, 2)
    flags = np.full(4, -1, np.int32)
    rc = capi.lib().rsqp_dense_check_chol(h, n, form, poison, pd_rel, pd_abs, *wg.args(), *wx.args(), *wi.args(), flags.ctypes.data_as(capi.ip))
    assert rc == 0, rc
    skip = skipped_tiles(n, dc.build(capi.describe_dense_gemm(n, n, n)))
    wg.assert_outside_untouched()
    if flags[1] != 0:
        wx.assert_unchanged()
        wi.assert_unchanged()
    else:
        wx.assert_outside_untouched()
        wi.assert_outside_untouched(~skip if form == capi.DENSE_INV_UPPER else None)      # (upper tiles only: the others keep their NaN)
    return wg.get(), wx.get(), wi.get(), flags.tolist()


FORMS = [capi.DENSE_INV_UPPER, capi.DENSE_INV_MIRROR, capi.DENSE_INV_TRI2]


def chol_residuals(G0, G, X, Gi, form):
    """the residual lines of tests/test_gpu_dense.py::test_cholesky_inverse; the lower triangles the header calls zeroed"""
    n = G0.shape[0]
    U = np.triu(G)
    assert np.max(np.abs(U.T @ U - G0)) < 1e-11 * np.abs(G0).max()
    if form == capi.DENSE_INV_UPPER:        # (upper tiles only: what the engine's dual path reads)
        Gi = np.triu(Gi) + np.triu(Gi, 1).T
    assert np.max(np.abs(Gi @ G0 - np.eye(n))) < 1e-8
    low = np.tril_indices(n, -1)
    assert not bits(G[low]).any() and not bits(X[low]).any()      # exact (+0.0) zeros


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", dc.CHOL_SIZES)
def test_cholesky_inverse_in_the_engines_call_form(n, form):
    """rsqp_dpotrf_upper + rsqp_dtrtri_upper + one of the three ways the engine forms U^-1 U^-T. For the triangular inverse: n = 65 is a
    ragged pair, 128 one batched pair (strides 2 s (ld + 1)), 192 a batched pair and a ragged level, 320 two batched pairs followed
    by ragged levels, 513 five levels. The lower triangle of G is not referenced on entry: NaN there must not change a bit"""
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n + 5, n))
    G0 = M.T @ M + 0.1 * np.eye(n)
    with Work(n) as h:
        ref = run_chol(h, G0, "tight", form)
    assert ref[3] == [0, 0, 0, 0]
    chol_residuals(G0, *ref[:3], form)
    Gn = G0.copy()
    Gn[np.tril_indices(n, -1)] = poisoned(1)[0]
    for layout, mmax in (("pad", n), ("odd", n), ("pad", 2 * n)):
        with Work(mmax) as h:
            got = run_chol(h, Gn, layout, form, poison=1)
        assert got[3] == ref[3] and same_bits(got[:3], ref[:3]), (layout, mmax)      # (no product of these three routines is given the workspace's slabs)


def test_two_cholesky_factorisations_on_one_workspace():
    rng = np.random.default_rng(6)
    mats = []
    for n in (513, 200):
        M = rng.normal(size=(n + 5, n))
        mats.append(M.T @ M + 0.1 * np.eye(n))
    with Work(200) as h:
        ref = run_chol(h, mats[1], "tight", capi.DENSE_INV_TRI2)
    with Work(513) as h:
        first = run_chol(h, mats[0], "pad", capi.DENSE_INV_TRI2, poison=1)
        second = run_chol(h, mats[1], "pad", capi.DENSE_INV_TRI2)
    chol_residuals(mats[0], *first[:3], capi.DENSE_INV_TRI2)
    chol_residuals(mats[1], *second[:3], capi.DENSE_INV_TRI2)
    assert first[3] == second[3] == [0, 0, 0, 0] and same_bits(second[:3], ref[:3])


# ---- the definiteness rule ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kcol", dc.PD_COLUMNS)
def test_definiteness_rule_two_decades_either_side_of_the_threshold(kcol):
    """p > pd_rel (|g| + max(g - p, 0)) + pd_abs at the engine's pd_rel = 1e-10 (dual_setup_blocked), pd_abs = 0: the threshold is at
    2e-10 g_kk. A pivot of 1e-8 g_kk passes, one of 1e-12 g_kk sets flag[1] -- in the first panel (column 10), the second (100), the
    second outer block (300) and the last column (319). tests/test_dense_plan.py checks the constructed ratios in longdouble"""
    with Work(dc.PD_N) as h:
        for layout in ("tight", "pad"):
            ok = run_chol(h, dc.pd_matrix(kcol, 1e-8), layout, capi.DENSE_INV_UPPER, pd_rel=1e-10, pd_abs=0.0)
            assert ok[3] == [0, 0, 0, 0], (layout, ok[3])
            G0 = dc.pd_matrix(kcol, 1e-8)
            U = np.triu(ok[0])
            assert np.max(np.abs(U.T @ U - G0)) < 1e-11 * np.abs(G0).max()
            assert abs(U[kcol, kcol] ** 2 / G0[kcol, kcol] / 1e-8 - 1.0) < 1e-2
            bad = run_chol(h, dc.pd_matrix(kcol, 1e-12), layout, capi.DENSE_INV_UPPER, pd_rel=1e-10, pd_abs=0.0)
            assert bad[3][1] != 0 and bad[3][0] == 0, (layout, bad[3])


def test_gram_matrix_of_dependent_columns_is_not_positive_definite():
    """what dual_setup_blocked's fallback hangs on: B'B with one exactly dependent column of B (column 200, in the last panel of the
    first outer block) has a pivot of rounding size there"""
    B = dc.dependent_matrix(400, 320, 200)
    with Work(320) as h:
        bad = run_chol(h, B.T @ B, "pad", capi.DENSE_INV_UPPER, poison=1, pd_rel=1e-10, pd_abs=1e-25)
        assert bad[3][1] != 0
        Bi = dc.dependent_matrix(400, 320, 200, dependent=False)
        ok = run_chol(h, Bi.T @ Bi, "pad", capi.DENSE_INV_UPPER, pd_rel=1e-10, pd_abs=1e-25)
        assert ok[3] == [0, 0, 0, 0]


# ---- dependent columns ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cholqr", [1, 0])
@pytest.mark.parametrize("m,n,col", [(300, 130, 40), (600, 300, 280)])
def test_qr_flags_dependent_columns_in_a_cholesky_qr_panel_and_in_the_second_outer_block(m, n, col, cholqr):
    """column 40 of 300 x 130 lies in a panel Cholesky-QR takes (its Gram matrix is singular: flag[2], and the repeat with the column
    kernel decides), column 280 of 600 x 300 in the second outer block. The same matrices without the dependency: 0"""
    with Work(m) as h:
        dep = run_qr(h, dc.dependent_matrix(m, n, col), "pad", cholqr, poison=1)
        assert dep[3][0] >= 1, dep[3]
        if cholqr and col == 40:
            assert dep[4] == 1          # the panel was not decided by its Gram matrix
        if not cholqr:
            assert dep[4] == 0
        B0 = dc.dependent_matrix(m, n, col, dependent=False)
        ind = run_qr(h, B0, "pad", cholqr)
        assert ind[3] == [0, 0, 0, 0] and ind[4] == 0
        qr_residuals(B0, *ind[:3])
