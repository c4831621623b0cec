"""The banded H^-1 kernels of the HBM-resident engine (k_band_apply<C>, k_band_apply_mw<C> of restartsqp_amd/csrc/qp_rs_kernels.h) in
every build C = 4, 8, 10, 12, 16 and every form the engine calls, through the check entry points of include/rsqp_hip_band_check.h, which
launch through the engine's own dispatch.

Reference and bound (tests/band_ref.py, tests/band_cases.py): x_ref is the numpy.longdouble solve from the f64 factor the library
returned, rho = |x - x_ref|_inf / |x_ref|_inf per column, rho_seq the same for the two sweeps as a sequential f64 loop. The kernels are
allowed 64 max(rho_seq, eps): a state passes through at most 6 + 15 + 15 compositions of chunk maps, each a handful of roundings.
Every case prints its figures before anything is asserted (pytest -s; collected in profiles/band_apply_check.txt).

The two kernels partition the rows identically -- a workgroup of the multi-workgroup form is a wave of the other -- and share the
chunk and scan code, so their results are compared bit for bit.

Everything of a downloaded buffer that is not an element the call writes holds a NaN of a fixed payload before the call and is
compared as uint64 after it."""
import numpy as np
import pytest

import band_cases as bc
import band_ref as br
from restartsqp_amd import capi

pytestmark = pytest.mark.gpu

POISON = np.uint64(0x7FF80000DEADBEEF)
MW, WG = capi.BAND_KERNEL_ENGINE, capi.BAND_KERNEL_1WG


def poisoned(n):
    return np.full(n, POISON, np.uint64).view(np.float64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pad16(n):
    return (n + 15) // 16 * 16


class Handle:
    def __init__(self, p):
        self.p = p

    def __enter__(self):
        self.h = capi.BandCheck(*self.p.bands)
        return self.h

    def __exit__(self, *exc):
        self.h.close()


def product(h, b, kernel, sub=None, off_sub=0, off_in=3, off_out=5):
    """one vector, in != out, both inside poisoned buffers; `in` must come back as it went and nothing around `out` may change"""
    n = b.size
    bi, bo = poisoned(off_in + n + 2), poisoned(off_out + n + 4)
    bi[off_in:off_in + n] = b
    keep_i, keep_o = bi.copy(), bo.copy()
    err = h.apply(bi, off_in, sub=sub, off_sub=off_sub, buf_out=bo, off_out=off_out, kernel=kernel)
    assert err == 0
    assert np.array_equal(bits(bi), bits(keep_i))
    assert np.array_equal(bits(bo[:off_out]), bits(keep_o[:off_out])) and np.array_equal(bits(bo[off_out + n:]), bits(keep_o[off_out + n:]))
    return bo[off_out:off_out + n].copy()


def line(n, p, rhs, rho_seq, rho_mw, rho_wg, same):
    d = max(rho_seq, bc.EPS)
    print("band_apply n=%-5d c=%-2d C=%-2d %-12s %-7s rho_seq=%.2e  mw: rho=%.2e ratio=%6.2f  1wg: rho=%.2e ratio=%6.2f  bitwise=%s"
          % (n, p.fac["c"], p.fac["build"], p.name, rhs, rho_seq, rho_mw, rho_mw / d, rho_wg, rho_wg / d, "yes" if same else "NO"))


# ---- accuracy of every build, and the two kernels against each other ---------------------------------------------------------------

@pytest.mark.parametrize("n", list(bc.SIZES), ids=["n%d-C%d" % (n, C) for n, C in bc.SIZES.items()])
def test_every_build_meets_the_bound_and_the_two_kernels_agree_bitwise(n):
    bad, differ = [], []
    for p in bc.problem_set(n):
        assert p.fac["build"] == bc.SIZES[n]
        with Handle(p) as h:
            X = {k: np.stack([product(h, p.B[:, j].copy(), k) for j in range(p.B.shape[1])], axis=1) for k in (MW, WG)}
            assert h.seq == p.B.shape[1]                    # one tag per multi-workgroup product, none for the others
        rho = {k: br.rho(X[k], p.Xref) for k in X}
        for j, rhs in enumerate(p.names):
            same = np.array_equal(bits(X[MW][:, j]), bits(X[WG][:, j]))
            line(n, p, rhs, p.rho_seq[j], rho[MW][j], rho[WG][j], same)
            if not same:
                differ.append((p.name, rhs))
            for k in X:
                if not rho[k][j] <= bc.allowed(p.rho_seq[j]):
                    bad.append((p.name, rhs, "mw" if k == MW else "1wg", rho[k][j], p.rho_seq[j]))
    assert not bad, bad
    assert not differ, differ


# ---- the engine's call forms --------------------------------------------------------------------------------------------------------

_FORMS = {}


def form_case(n):
    """the 5-band dominant Hessian of size n, 17 random columns and one vector to subtract, with the references of both (once)"""
    if n not in _FORMS:
        p = bc.problem_set(n)[2]
        assert p.name == "dominant5"
        rng = np.random.default_rng([4503, n])
        B, sub = rng.normal(size=(n, 17)), rng.normal(size=n)
        BB = np.concatenate([B, B - sub[:, None]], axis=1)
        Xref = br.solve(p.m1, p.m2, p.sinv, BB, br.LD)
        rho_seq = br.rho(br.solve(p.m1, p.m2, p.sinv, BB, np.float64), Xref)
        for a in (B, sub, Xref, rho_seq):
            a.flags.writeable = False
        _FORMS[n] = (p, B, sub, Xref, rho_seq)
    return _FORMS[n]


@pytest.mark.parametrize("with_sub", [False, True], ids=["nosub", "sub"])
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("ncols", [3, 17])
@pytest.mark.parametrize("n", bc.FORM_SIZES)
def test_column_grid_form(n, ncols, inplace, with_sub):
    """band_launch(ncols, in, sub, out, ld): ld = n rounded up to 16, plus 16; operands at an offset inside buffers poisoned with NaN.
    Every double outside the n x ncols block of `out` keeps its bits, nothing of `in` changes (or, in place -- the engine's set-up
    call -- the block is replaced and nothing else). Column j has the bits of the one-vector product of the same kernel"""
    p, B, sub, Xref, rho_seq = form_case(n)
    ld, off_in, off_out = pad16(n) + 16, 16, 32
    blk = lambda buf, off: np.lib.stride_tricks.as_strided(buf[off:], (n, ncols), (buf.itemsize, buf.itemsize * ld))
    bi, bo = poisoned(off_in + ld * ncols + 40), poisoned(off_out + ld * ncols + 7)
    blk(bi, off_in)[...] = B[:, :ncols]
    keep_i, keep_o = bi.copy(), bo.copy()
    with Handle(p) as h:
        if inplace:
            err = h.apply(bi, off_in, ncols=ncols, ld=ld, sub=sub if with_sub else None)
            got, buf, off, keep = blk(bi, off_in).copy(), bi, off_in, keep_i
        else:
            err = h.apply(bi, off_in, ncols=ncols, ld=ld, sub=sub if with_sub else None, buf_out=bo, off_out=off_out)
            got, buf, off, keep = blk(bo, off_out).copy(), bo, off_out, keep_o
            assert np.array_equal(bits(bi), bits(keep_i))
        assert err == 0 and h.seq == 0                      # the grid of one-workgroup kernels takes no tag
        outside = np.ones(buf.size, bool)
        blk(outside, off)[...] = False
        assert np.array_equal(bits(buf)[outside], bits(keep)[outside])
        one = product(h, B[:, ncols - 1].copy(), WG, sub=sub if with_sub else None)
        assert np.array_equal(bits(got[:, ncols - 1]), bits(one))
    cols = slice(17, 17 + ncols) if with_sub else slice(0, ncols)
    rho = br.rho(got, Xref[:, cols])
    print("band_apply_grid n=%d ncols=%d inplace=%d sub=%d max rho / max(rho_seq, eps) = %.2f"
          % (n, ncols, inplace, with_sub, (rho / np.maximum(rho_seq[cols], bc.EPS)).max()))
    assert np.all(rho <= bc.allowed(rho_seq[cols])), (rho, rho_seq[cols])


@pytest.mark.parametrize("kernel", [MW, WG], ids=["mw", "1wg"])
@pytest.mark.parametrize("n", bc.FORM_SIZES)
def test_one_vector_forms(n, kernel):
    """in place and with a vector subtracted, for the one-vector kernels: the bits of the plain product of in - sub"""
    p, B, sub, Xref, rho_seq = form_case(n)
    with Handle(p) as h:
        plain = product(h, B[:, 0].copy(), kernel)
        assert br.rho(plain[:, None], Xref[:, :1])[0] <= bc.allowed(rho_seq[0])
        buf = poisoned(n + 9)
        buf[4:4 + n] = B[:, 0]
        assert h.apply(buf, 4, kernel=kernel) == 0          # in == out
        assert np.array_equal(bits(buf[4:4 + n]), bits(plain))
        assert np.all(bits(buf[:4]) == POISON) and np.all(bits(buf[4 + n:]) == POISON)
        with_sub = product(h, B[:, 1].copy(), kernel, sub=np.concatenate([[np.nan], sub, [np.nan]]), off_sub=1)
        assert br.rho(with_sub[:, None], Xref[:, 18:19])[0] <= bc.allowed(rho_seq[18])
        assert np.array_equal(bits(with_sub), bits(product(h, B[:, 1] - sub, kernel)))


# ---- repeated products: the tag protocol of agg -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 10000, 16384])
def test_forty_consecutive_multi_workgroup_products(n):
    """one handle, 40 different vectors one after the other: every product reads the totals of THIS call (tag = sequence number),
    never those the call before left in agg; err stays 0. A product of the other kernel in between takes no tag"""
    p = bc.problem_set(n)[3]
    assert p.name == "biharmonic"                           # (its totals differ most from vector to vector: nothing decays)
    rng = np.random.default_rng([4504, n])
    B = rng.normal(size=(n, 40)) * 10.0 ** rng.integers(-3, 4, 40)
    Xref = br.solve(p.m1, p.m2, p.sinv, B, br.LD)
    ok = bc.allowed(br.rho(br.solve(p.m1, p.m2, p.sinv, B, np.float64), Xref))
    with Handle(p) as h:
        X = np.zeros((n, 40))
        for j in range(40):
            X[:, j] = product(h, B[:, j].copy(), MW)
            assert h.seq == j + 1
            if j == 20:
                product(h, B[:, j].copy(), WG)
                assert h.seq == j + 1
    rho = br.rho(X, Xref)
    print("band_apply_repeat n=%d max rho / allowed = %.3f" % (n, (rho / ok).max()))
    assert np.all(rho <= ok), np.nonzero(rho > ok)


# ---- the fused step-direction form --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", [MW, WG], ids=["mw", "1wg"])
@pytest.mark.parametrize("n", bc.FORM_SIZES + (16383,))
def test_fused_step_direction_form(n, kernel):
    """Hdx = (ATdy + (Sb ? dy : 0)) - (gN - g) bit for bit on every row; dx = H^-1 Hdx on the rows with Sb == 0 only, with the bits of
    the plain product of Hdx, within the bound; every other row of dx, and everything around both, keeps a sentinel's bits"""
    p = bc.problem_set(n)[2]
    rng = np.random.default_rng([4505, n])
    Sb = rng.choice(np.array([-1, 0, 0, 1], np.int32), n)
    Sb[[0, n - 1]] = (0, 1) if n > 1 else 0
    ATdy, dy, gN, g = (rng.normal(size=n) for _ in range(4))
    want_H = (ATdy + np.where(Sb != 0, dy, 0.0)) - (gN - g)
    off_h, off_x = 7, 2
    bH, bX = poisoned(off_h + n + 3), poisoned(off_x + n + 11)
    free = Sb == 0
    with Handle(p) as h:
        assert h.apply_q(Sb, ATdy, dy, gN, g, bH, off_h, bX, off_x, kernel=kernel) == 0
        assert h.seq == (1 if kernel == MW else 0)
        full = product(h, want_H.copy(), kernel)
    Hdx, dx = bH[off_h:off_h + n], bX[off_x:off_x + n]
    assert np.array_equal(bits(Hdx), bits(want_H))
    assert np.all(bits(bH[:off_h]) == POISON) and np.all(bits(bH[off_h + n:]) == POISON)
    assert np.all(bits(bX[:off_x]) == POISON) and np.all(bits(bX[off_x + n:]) == POISON)
    assert np.all(bits(dx[~free]) == POISON) and 0 < free.sum() < n
    assert np.array_equal(bits(dx[free]), bits(full[free]))
    xref = br.solve(p.m1, p.m2, p.sinv, want_H[:, None], br.LD)
    rho_seq = br.rho(br.solve(p.m1, p.m2, p.sinv, want_H[:, None], np.float64), xref)[0]
    rho = float(np.abs(np.asarray(dx[free], br.LD) - xref[free, 0]).max() / np.abs(xref).max())
    print("band_apply_q n=%d kernel=%d rho=%.2e rho_seq=%.2e" % (n, kernel, rho, rho_seq))
    assert rho <= bc.allowed(rho_seq)
