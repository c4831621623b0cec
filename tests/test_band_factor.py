"""The host side of the banded H^-1 operator of the HBM-resident engine (band_factor_host / band_build_of of
restartsqp_amd/csrc/qp_rs_path.h) through rsqp_band_check_factor, the references of tests/band_ref.py themselves, and the argument checks
of the entry points of include/rsqp_hip_band_check.h. Needs no GPU. The kernels: tests/test_gpu_band_apply.py, on the same cases
(band_cases)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import band_cases as bc
import band_ref as br
from abi_cases import assert_entry_points
from conftest import ROOT

NEW = ("rsqp_band_check_factor", "rsqp_band_check_create", "rsqp_band_check_destroy", "rsqp_band_check_apply", "rsqp_band_check_apply_q")
EPS = bc.EPS
TH = br.TH


def test_entry_points_are_declared_exported_and_bound(capi):
    header = assert_entry_points(capi, "rsqp_hip_band_check.h", capi.BAND_CHECK_SYMBOLS, NEW)
    assert int(re.search(r"#define RSQP_BAND_MAX_N (\d+)", header).group(1)) == capi.BAND_MAX_N == 16384
    assert int(re.search(r"#define RSQP_BAND_THREADS (\d+)", header).group(1)) == capi.BAND_THREADS == TH
    words = re.search(r"enum \{ (RSQP_BAND_KERNEL_ENGINE.*?) \};", header).group(1)
    assert [w.strip() for w in words.split(",")] == ["RSQP_BAND_KERNEL_ENGINE = 0", "RSQP_BAND_KERNEL_1WG = 1"]
    assert (capi.BAND_KERNEL_ENGINE, capi.BAND_KERNEL_1WG) == (0, 1)


def test_the_engine_and_the_entries_ask_the_same_host_functions():
    """the factor, the rule c -> C and the launch stand once: Impl::rs_build_band / band_launch and the check entries call them"""
    path = open(os.path.join(ROOT, "restartsqp_amd", "csrc", "qp_rs_path.h")).read()
    check = open(os.path.join(ROOT, "restartsqp_amd", "csrc", "qp_band_check.h")).read()
    assert len(re.findall(r"c <= 4 \?", path)) == 1 and "c <= 4" not in check          # the rule's only statement
    dispatch = path[path.index("static void band_dispatch("):path.index("int Impl::rs_build_band(")]
    assert dispatch.count("BAND_BUILDS(RS_MW, band.c)") == 1 and dispatch.count("BAND_BUILDS(RS_1W, band.c)") == 1
    assert len(re.findall(r"k_band_apply(?:_mw)?<", path)) == 3 and "k_band_apply" not in check       # two launches, the LDS attribute
    engine = path[path.index("int Impl::rs_build_band("):]
    assert engine.count("band_factor_host(") == 1 and engine.count("band_dispatch(") == 1 and "sqrt" not in engine[:engine.index("int Impl::rs_build_dense(")]
    assert check.count("band_factor_host(") == 2 and check.count("band_dispatch(") == 2 and check.count("band_build_of(") == 1


# ---- the reference itself -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 200])
def test_longdouble_solve_agrees_with_a_dense_solve(n):
    """band_ref.solve on the longdouble L D L' of the bands against numpy.linalg.solve on the dense f64 H, within
    n eps cond_inf(H) |x|_inf per column"""
    B = np.random.default_rng(n).normal(size=(n, 3))
    names = []
    for name, hb, bands in bc.hessians(n):
        d, l1, l2 = br.ldl(*bands)
        sq = np.sqrt(d)
        m1, m2 = l1.copy(), l2.copy()
        m1[1:] = l1[1:] * sq[:-1] / sq[1:]
        m2[2:] = l2[2:] * sq[:-2] / sq[2:]
        X = br.solve(m1, m2, 1 / sq, B)
        H = br.dense(*bands)
        Xd = np.linalg.solve(H, B)
        cond = np.linalg.norm(H, np.inf) * np.linalg.norm(np.linalg.inv(H), np.inf)
        err = np.abs(np.asarray(X, float) - Xd).max(axis=0)
        assert np.all(err <= n * EPS * cond * np.abs(Xd).max(axis=0)), (name, err)
        names.append(name)
    assert names[:4] == ["diag", "dominant3", "dominant5", "biharmonic"] and (n < 128 or "growth@64" in names)


def test_sequential_f64_loop_is_the_same_two_sweeps():
    """the yardstick differs from the reference in precision only: on integers (no rounding) both give the same numbers"""
    rng = np.random.default_rng(7)
    n = 40
    m1 = rng.integers(-2, 3, n).astype(float); m2 = rng.integers(-2, 3, n).astype(float)
    m1[:1] = 0.0; m2[:2] = 0.0
    B = rng.integers(-3, 4, (n, 4)).astype(float)
    s = 2.0 ** rng.integers(-1, 2, n)
    X = br.solve(m1, m2, s, B, np.float64)
    assert X.dtype == np.float64 and np.array_equal(X, np.asarray(br.solve(m1, m2, s, B), float))
    # ... and they solve the system: M M' (x / s) = s b
    M = np.eye(n) + np.diag(m1[1:], -1) + np.diag(m2[2:], -2)
    assert np.array_equal(M @ M.T @ (X / s[:, None]), B * s[:, None])


# ---- the factor and its chunk-interleaved image -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(bc.SIZES))
def test_rule_c_to_build(capi, n):
    fac = capi.band_factor(*bc.hessians(n)[2][2])
    c = -(-n // TH)
    assert fac["built"] and fac["c"] == c == br.chunk_rows(n)
    assert fac["build"] == bc.SIZES[n] == bc.build_of(c) and fac["build"] >= c


def test_rule_c_to_build_at_every_c(capi):
    want = {1: 4, 4: 4, 5: 8, 8: 8, 9: 10, 10: 10, 11: 12, 12: 12, 13: 16, 16: 16}
    for c in range(1, 17):
        for n in ((c - 1) * TH + 1, c * TH):
            fac = capi.band_factor(np.ones(n), np.zeros(n), np.zeros(n))
            assert (fac["c"], fac["build"]) == (c, bc.build_of(c)), n
            assert c not in want or fac["build"] == want[c]


@pytest.mark.parametrize("n", list(bc.SIZES))
def test_interleaved_layout(capi, n):
    """m1i[k 1024 + t], k <= c, and m2i[k 1024 + t], k <= c + 1, hold the factor entry of row t c + k; rows >= n and the rows without
    such a neighbour hold exact zeros; the entries stored twice (k >= c: the first rows of chunk t + 1) are bitwise equal"""
    for name, hb, bands in bc.hessians(n):
        fac = capi.band_factor(*bands)
        c = fac["c"]
        m1i, m2i = fac["m1i"], fac["m2i"]
        assert m1i.size == TH * (c + 1) and m2i.size == TH * (c + 2) and fac["sinv"].size == n
        m1, m2 = np.zeros(n + TH * c + 4), np.zeros(n + TH * c + 4)            # the plain entries, zero beyond n
        m1[:n], m2[:n] = br.plain(m1i, n, c), br.plain(m2i, n, c)
        t = np.arange(TH)
        for k in range(c + 2):
            if k <= c:
                assert np.array_equal(m1i[k * TH + t].view(np.uint64), m1[t * c + k].view(np.uint64)), (name, k)
            assert np.array_equal(m2i[k * TH + t].view(np.uint64), m2[t * c + k].view(np.uint64)), (name, k)
        z = np.zeros(1).view(np.uint64)[0]
        assert m1[0].view(np.uint64) == z and np.all(m2[:2].view(np.uint64) == z)
        # the chunks really are c consecutive rows: the k < c part, read thread by thread, is rows 0, 1, 2, ... in order
        rows = (t[:, None] * c + np.arange(c)[None, :]).ravel()
        assert np.array_equal(rows, np.arange(TH * c))
        if hb >= 1 and n > 1:
            assert np.all(m1[1:n] != 0.0)                                      # every row that has a neighbour has its entry
        if hb >= 2 and n > 2:
            assert np.all(m2[2:n] != 0.0)
        if hb < 2:
            assert not m2i.any()
        if hb < 1:
            assert not m1i.any()


@pytest.mark.parametrize("n", list(bc.SIZES))
def test_factor_reproduces_the_bands(capi, n):
    """L D L' rebuilt in longdouble from the returned m1i, m2i, sinv equals the bands within 16 eps (|L| |D| |L'|) entrywise: at most
    five operations per entry of the factorisation, plus the three roundings of the rescaling (sqrt, 1 / sqrt, m = l sq / sq)"""
    for name, hb, bands in bc.hessians(n):
        fac = capi.band_factor(*bands)
        c = fac["c"]
        got, mag = br.rebuilt_bands(br.plain(fac["m1i"], n, c), br.plain(fac["m2i"], n, c), fac["sinv"])
        for k, (g, a, want) in enumerate(zip(got, mag, bands)):
            err = np.abs(g - np.asarray(want, br.LD))[k:]
            assert np.all(err <= 16 * EPS * a[k:]), (name, k, float((err / np.maximum(a[k:], 1e-300)).max()) / EPS)


def test_the_judge_of_the_factor_holds_for_a_longdouble_factorisation():
    """band_ref.ldl and band_ref.bands_of_ldl, the two halves of the check above, against each other: the longdouble factor
    reproduces the bands within 16 longdouble eps (|L| |D| |L'|), the same count of operations in the wider format"""
    eps_ld = float(np.finfo(br.LD).eps)
    assert eps_ld < EPS / 1000
    for n in (3, 65, 4097):
        for name, hb, bands in bc.hessians(n):
            got, mag = br.bands_of_ldl(*br.ldl(*bands))
            for k, (g, a, want) in enumerate(zip(got, mag, bands)):
                assert np.all(np.abs(g - np.asarray(want, br.LD))[k:] <= 16 * eps_ld * a[k:]), (n, name, k)


def test_growth_number(capi):
    """the window rule measures what the cases are built for: 1.1^64 = 446 in the one grown window, and it restarts every 64 rows"""
    for n, start in ((200, 64), (1024, 960), (4097, 256), (16384, 15360)):
        fac = capi.band_factor(*bc.growth_window(n, start))
        assert fac["built"] and 1e2 < fac["growth"] < 1e3 and round(fac["growth"]) == 446
    # every case of the GPU test is accepted, and only the growth cases come near the rule
    for n in bc.SIZES:
        names = [name for name, _, _ in bc.hessians(n)]
        assert (n < 128) == (not any(k.startswith("growth") for k in names))
        for name, hb, bands in bc.hessians(n):
            g = capi.band_factor(*bands)["growth"]
            assert (1e2 < g < 1e3) if name.startswith("growth") else g < 1e2, (n, name, g)
    # (the first window has no incoming state -- row 0 has no neighbours --, so the rule measures nothing there: no case starts at 0)
    assert capi.band_factor(*bc.growth_window(128, 0))["growth"] <= 1.0


# ---- the rejections -----------------------------------------------------------------------------------------------------------------

def test_small_pivot_is_not_built(capi):
    for n, j in ((2, 1), (65, 64), (4097, 4095), (4097, 1)):
        d0, e1, e2 = np.ones(n), np.zeros(n), np.zeros(n)
        e1[j] = 1.0                                 # pivot j = d0[j] - 1
        for d0j, built in ((1.0 + 2.0 ** -20, True), (1.0 + 2.0 ** -39, True), (1.0 + 2.0 ** -41, False), (1.0, False), (0.5, False)):
            d0[j] = d0j                             # 2^-40 = 9.1e-13: the threshold 1e-12 |d0| lies between 2^-39 and 2^-41
            fac = capi.band_factor(d0, e1, e2)
            assert fac["built"] == built, (n, j, d0j)
            assert fac["c"] == -(-n // TH) and (built or (fac["growth"] == -1.0 and fac["m1i"] is None))
    assert not capi.band_factor(np.array([1.0, -1.0, 1.0]), np.zeros(3), np.zeros(3))["built"]
    assert not capi.band_factor(np.array([1.0, np.nan, 1.0]), np.zeros(3), np.zeros(3))["built"]


def test_growing_factor_is_not_built(capi):
    for n, start in ((128, 64), (4097, 2048), (16384, 16320)):
        for l, built in ((-1.1, True), (-1.113, True), (-1.115, False), (1.2, False)):      # 1000^(1/64) = 1.1140
            l1 = np.full(n, -0.5); l1[start:start + 64] = l; l1[0] = 0.0
            fac = capi.band_factor(1.0 + l1 * l1, l1, np.zeros(n))
            assert fac["built"] == built, (n, start, l, fac["growth"])
            assert (fac["growth"] <= 1e3) == built and fac["growth"] > 1e2
    # the second homogeneous solution counts as well: a growing l2 alone
    n = 200
    l2 = np.full(n, -0.25); l2[64:128] = -1.3; l2[:2] = 0.0           # H = L L' with only the second sub-diagonal: 1.3^32 = 4.4e3
    d0 = 1.0 + l2 * l2
    assert not capi.band_factor(d0, np.zeros(n), l2)["built"]


def test_sizes_out_of_range_are_not_built(capi):
    for n in (16385, 20000):
        fac = capi.band_factor(np.ones(n), np.zeros(n), np.zeros(n))
        assert fac == dict(built=False, c=0, build=0, growth=-1.0, m1i=None, m2i=None, sinv=None)
    assert capi.band_factor(np.ones(16384), np.zeros(16384), np.zeros(16384))["built"]
    w = [C.c_int(7) for _ in range(3)]
    g = C.c_double(7.0)
    for n in (0, -1):       # an answer, not an error, and nothing is read or written
        assert capi.lib().rsqp_band_check_factor(n, None, None, None, *[C.byref(v) for v in w], C.byref(g), None, 0, None, 0, None, 0) == 0
        assert [v.value for v in w] == [0, 0, 0] and g.value == -1.0


# ---- the argument checks ------------------------------------------------------------------------------------------------------------

def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_factor_refuses_bad_arguments(capi):
    L = capi.lib()
    n = 1500                                       # c = 2
    d0, z = np.ones(n), np.zeros(n)
    m1, m2, s = np.full(3 * TH, 7.0), np.full(4 * TH, 7.0), np.full(n, 7.0)
    w = [C.c_int(7) for _ in range(3)]
    g = C.c_double(7.0)
    outs = [C.byref(v) for v in w] + [C.byref(g)]

    def call(n=n, bands=(_p(d0), _p(z), _p(z)), outs=outs, m1=(_p(m1), m1.size), m2=(_p(m2), m2.size), s=(_p(s), s.size)):
        return L.rsqp_band_check_factor(n, *bands, *outs, *m1, *m2, *s)

    bad = [dict(bands=(None, _p(z), _p(z))), dict(bands=(_p(d0), None, _p(z))), dict(bands=(_p(d0), _p(z), None)),
           dict(m1=(None, m1.size)), dict(m2=(None, m2.size)), dict(s=(None, s.size)),
           dict(m1=(_p(m1), 3 * TH - 1)), dict(m2=(_p(m2), 4 * TH - 1)), dict(s=(_p(s), n - 1))]
    bad += [dict(outs=outs[:k] + [None] + outs[k + 1:]) for k in range(4)]
    for kw in bad:
        assert call(**kw) == capi.ERR_ARG, kw
    assert [v.value for v in w] == [7, 7, 7] and g.value == 7.0 and np.all(m1 == 7.0) and np.all(m2 == 7.0) and np.all(s == 7.0)
    assert call() == 0 and [v.value for v in w] == [1, 2, 4] and np.all(s == 1.0) and not m1.any() and not m2.any()


def test_handle_and_products_refuse_bad_arguments_on_the_host(capi):
    """every refusal answers before a device call: this test runs where there is no device. The handle is host work"""
    L = capi.lib()
    n = 70
    d0, z, neg = np.full(n, 2.0), np.zeros(n), np.full(n, -2.0)
    h = C.c_void_p()
    for args in ((n, None, _p(z), _p(z), C.byref(h)), (n, _p(d0), None, _p(z), C.byref(h)), (n, _p(d0), _p(z), None, C.byref(h)),
                 (n, _p(d0), _p(z), _p(z), None), (0, _p(d0), _p(z), _p(z), C.byref(h)), (16385, _p(d0), _p(z), _p(z), C.byref(h)),
                 (n, _p(neg), _p(z), _p(z), C.byref(h))):                      # (not positive definite: no operator, no handle)
        assert L.rsqp_band_check_create(*args) == capi.ERR_ARG
        assert h.value is None
    assert L.rsqp_band_check_destroy(None) == capi.ERR_ARG
    assert L.rsqp_band_check_create(n, _p(d0), _p(z), _p(z), C.byref(h)) == 0 and h.value
    ld, ncols, off = 80, 3, 5
    a = np.full(off + ld * (ncols - 1) + n, 3.0); o = a.copy(); sub = np.full(n + 2, 1.0)
    err, seq = C.c_int(7), C.c_longlong(7)
    tail = [C.byref(err), C.byref(seq)]

    def call(h=h, kernel=0, ncols=ncols, ld=ld, inplace=0, a=(_p(a), a.size, off), s=(_p(sub), sub.size, 2), o=(_p(o), o.size, off), tail=tail):
        return L.rsqp_band_check_apply(h, kernel, ncols, ld, inplace, *a, *s, *o, *tail)

    bad = [dict(h=None), dict(kernel=-1), dict(kernel=2), dict(ncols=0), dict(ncols=-1),
           dict(ld=n - 1), dict(ld=0), dict(ncols=1, ld=n - 1),
           dict(a=(None, a.size, off)), dict(o=(None, o.size, off)), dict(inplace=1, a=(None, a.size, off)),
           dict(a=(_p(a), a.size - 1, off)), dict(a=(_p(a), a.size, off + 1)), dict(a=(_p(a), a.size, -1)),      # the last column ends past
           dict(o=(_p(o), o.size - 1, off)), dict(o=(_p(o), o.size, off + 1)), dict(o=(_p(o), o.size, -1)),
           dict(inplace=1, a=(_p(a), a.size, off + 1)), dict(ncols=4), dict(ld=ld + 1),
           dict(s=(_p(sub), sub.size, 3)), dict(s=(_p(sub), n - 1, 0)), dict(s=(_p(sub), sub.size, -1)),
           dict(tail=[None, tail[1]]), dict(tail=[tail[0], None])]
    for kw in bad:
        assert call(**kw) == capi.ERR_ARG, kw
    # the fused form
    Sb = np.zeros(n, np.int32); v = np.ones(n)
    ipt = Sb.ctypes.data_as(capi.ip)

    def callq(h=h, kernel=0, Sb=ipt, v=(_p(v),) * 4, H=(_p(a), a.size, off), X=(_p(o), o.size, off), tail=tail):
        return L.rsqp_band_check_apply_q(h, kernel, Sb, *v, *H, *X, *tail)

    badq = [dict(h=None), dict(kernel=3), dict(Sb=None)] + [dict(v=(_p(v),) * k + (None,) + (_p(v),) * (3 - k)) for k in range(4)]
    badq += [dict(H=(None, a.size, off)), dict(X=(None, o.size, off)), dict(H=(_p(a), off + n - 1, off)), dict(X=(_p(o), o.size, o.size - n + 1)),
             dict(H=(_p(a), a.size, -1)), dict(tail=[None, tail[1]]), dict(tail=[tail[0], None])]
    for kw in badq:
        assert callq(**kw) == capi.ERR_ARG, kw
    assert np.all(a == 3.0) and np.all(o == 3.0) and np.all(sub == 1.0) and err.value == 7 and seq.value == 7
    assert L.rsqp_band_check_destroy(h) == 0


def test_binding_refuses_what_it_could_not_write_in_place(capi):
    b = capi.BandCheck(np.full(5, 2.0), np.zeros(5), np.zeros(5))
    for buf in (np.zeros(5, np.float32), np.zeros((5, 1)), np.zeros(10)[::2], [0.0] * 5):
        with pytest.raises(ValueError):
            b.apply(buf)
    with pytest.raises(ValueError):
        b.apply_q(np.zeros(4, np.int32), *[np.zeros(5)] * 4, np.zeros(5), 0, np.zeros(5), 0)
    with pytest.raises(capi.RsqpError):
        capi.BandCheck(np.full(5, -2.0), np.zeros(5), np.zeros(5))
    b.close()
