"""The launch plan of the dense GEMM (dgemm_plan of restartsqp_amd/csrc/dense_la.hip) through its host-only export
rsqp_dense_describe_gemm, and the argument checks of the check entry points of include/rsqp_hip_dense_check.h. Needs no GPU. The runs
themselves: tests/test_gpu_dense_forms.py, which takes its shapes from the same module (dense_cases)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import dense_cases as dc
from abi_cases import assert_entry_points
from conftest import ROOT

NEW = ("rsqp_dense_describe_gemm", "rsqp_dense_check_gemm", "rsqp_dense_check_work_create", "rsqp_dense_check_work_destroy",
       "rsqp_dense_check_qr", "rsqp_dense_check_chol")
SOURCE = os.path.join(ROOT, "restartsqp_amd", "csrc", "dense_la.hip")
SIZES = (1, 8, 64, 65, 128, 129, 2048, 8192, 32641, 65409, 65536)


def test_entry_points_are_declared_exported_and_bound(capi):
    header = assert_entry_points(capi, "rsqp_hip_dense_check.h", capi.DENSE_CHECK_SYMBOLS, NEW)
    assert int(re.search(r"#define RSQP_DENSE_PLAN_WORDS (\d+)", header).group(1)) == len(capi.DENSE_PLAN_OUT)
    # the header's words are the binding's, in its order
    words = re.search(r"enum \{ (RSQP_DENSE_GEMM_PLAIN.*?) \};", header).group(1)
    assert [w.strip() for w in words.split(",")] == ["RSQP_DENSE_GEMM_%s = %d" % (w, i) for i, w in enumerate(("PLAIN", "UPPER", "KTRI1", "KTRI2", "KTRI3"))]
    assert (capi.DENSE_GEMM_PLAIN, capi.DENSE_GEMM_UPPER, capi.DENSE_GEMM_KTRI1, capi.DENSE_GEMM_KTRI2, capi.DENSE_GEMM_KTRI3) == (0, 1, 2, 3, 4)
    words = re.search(r"enum \{ (RSQP_DENSE_INV_UPPER.*?) \};", header).group(1)
    assert [w.strip() for w in words.split(",")] == ["RSQP_DENSE_INV_%s = %d" % (w, i) for i, w in enumerate(("UPPER", "MIRROR", "TRI2"))]
    assert (capi.DENSE_INV_UPPER, capi.DENSE_INV_MIRROR, capi.DENSE_INV_TRI2) == (0, 1, 2)


def test_the_launcher_asks_the_plan_the_export_shows():
    """one function: dgemm_ws takes tile, splits and kc from dgemm_plan, the export calls the same one, and the tile rule stands nowhere else"""
    src = open(SOURCE).read()
    assert len(re.findall(r"\bdgemm_plan\(", src)) == 3       # definition, launcher, export
    launcher = src[src.index("static hipError_t dgemm_ws("):src.index("hipError_t rsqp_dgemm(")]
    assert "dgemm_plan(m, n, k, batch, ws != nullptr, ws_cap)" in launcher and "big" not in launcher and "skinny" not in launcher
    export = src[src.index('extern "C" int rsqp_dense_describe_gemm'):]
    assert "dgemm_plan(m, n, k, batch, have_ws != 0" in export[:export.index("\n}\n")]


def test_describe_refuses_bad_arguments(capi):
    L = capi.lib()
    o = np.zeros(5, np.int32)
    op = o.ctypes.data_as(capi.ip)
    assert L.rsqp_dense_describe_gemm(64, 64, 64, 1, 0, 0, op, 5) == 0 and o.tolist() == [64, 64, 1, 64, 0]
    for bad in ((0, 64, 64, 1, 0, 0, op, 5), (64, 0, 64, 1, 0, 0, op, 5), (64, 64, -1, 1, 0, 0, op, 5), (64, 64, 64, 0, 0, 0, op, 5),
                (64, 64, 64, 1, 1, -1, op, 5), (64, 64, 64, 1, 0, 0, None, 5), (64, 64, 64, 1, 0, 0, op, 4), (64, 64, 64, 1, 0, 0, op, 6)):
        assert L.rsqp_dense_describe_gemm(*bad) == capi.ERR_ARG, bad
    assert capi.describe_dense_gemm(64, 64, 0) == dict(TM=64, TN=64, splits=1, kc=0, skinny=0)      # (k = 0 is a product: beta C)


def _buf(n):
    a = np.zeros(max(n, 1))
    return a, a.ctypes.data_as(capi_dp)


capi_dp = C.POINTER(C.c_double)


def test_check_gemm_refuses_bad_arguments_on_the_host(capi):
    """every refusal answers before a device call: this test runs where there is no device"""
    L = capi.lib()
    m, n, k = 5, 4, 3
    A, Ap = _buf(m * k); B, Bp = _buf(k * n); Cm, Cp = _buf(m * n)

    def call(variant=0, ta=0, tb=0, m=m, n=n, k=k, A=(Ap, m * k, 0, m), B=(Bp, k * n, 0, k), Cc=(Cp, m * n, 0, m), ws=0):
        return L.rsqp_dense_check_gemm(variant, ta, tb, m, n, k, 1.0, 0.0, *A, *B, *Cc, ws)

    bad = [dict(variant=-1), dict(variant=5), dict(m=-1), dict(n=-1), dict(k=-1), dict(ws=-1),
           dict(A=(None, m * k, 0, m)), dict(B=(None, k * n, 0, k)), dict(Cc=(None, m * n, 0, m)),
           dict(A=(Ap, m * k, 0, m - 1)),                  # ld < rows
           dict(A=(Ap, m * k, 1, m)),                      # the last column ends past the buffer
           dict(A=(Ap, m * k - 1, 0, m)), dict(A=(Ap, m * k, -1, m)),
           dict(B=(Bp, k * n, 0, k - 1)), dict(B=(Bp, k * n, 1, k)), dict(Cc=(Cp, m * n, 0, m - 1)), dict(Cc=(Cp, m * n, 1, m)),
           dict(Cc=(Cp, m * n, 0, m + 1)),                 # a padded result needs the longer buffer
           dict(ta=1),                                     # A' is k x m: lda = m < k is fine, but 5 x 3 read as 3 x 5 at ld 5 ends past
           dict(variant=capi.DENSE_GEMM_UPPER),            # m != n
           dict(variant=capi.DENSE_GEMM_KTRI1), dict(variant=capi.DENSE_GEMM_KTRI2, ta=1, A=(Ap, m * k, 0, k)),
           dict(variant=capi.DENSE_GEMM_KTRI3), dict(variant=capi.DENSE_GEMM_KTRI2, ws=100), dict(ws=1 << 40)]
    for kw in bad:
        assert call(**kw) == capi.ERR_ARG, kw
    assert not A.any() and not B.any() and not Cm.any()


def test_check_factorisations_refuse_bad_arguments_on_the_host(capi):
    L = capi.lib()
    h = C.c_void_p()
    assert L.rsqp_dense_check_work_create(0, C.byref(h)) == capi.ERR_ARG
    assert L.rsqp_dense_check_work_create(64, None) == capi.ERR_ARG
    assert L.rsqp_dense_check_work_destroy(None) == capi.ERR_ARG
    assert h.value is None
    m, n = 6, 4
    B, Bp = _buf(m * n); Q, Qp = _buf(m * m); X, Xp = _buf(n * n)
    f = np.zeros(4, np.int32); fp = f.ctypes.data_as(capi.ip)
    r = C.c_int(7)
    # without a workspace nothing runs, whatever else is right
    assert L.rsqp_dense_check_qr(None, m, n, 1, 0, 1e-9, Bp, m * n, 0, m, Qp, m * m, 0, m, Xp, n * n, 0, n, fp, C.byref(r)) == capi.ERR_ARG
    assert L.rsqp_dense_check_chol(None, n, 0, 0, 1e-10, 0.0, Xp, n * n, 0, n, Xp, n * n, 0, n, Xp, n * n, 0, n, fp) == capi.ERR_ARG
    assert r.value == 7 and not f.any()


# ---- the plan --------------------------------------------------------------------------------------------------------------------

def test_every_gemm_of_test_gpu_dense_runs_the_64_x_64_build_unsplit(capi):
    """the finding behind tests/test_gpu_dense_forms.py: the six parametrised shapes and the integer case of test_gpu_dense.py -- 64 x 1000
    x 2500 and 513 x 40 x 64 among them -- all launch k_dgemm<64, 64>; rsqp_dense_gemm gives the launcher no split-K workspace"""
    shapes = dc.old_gemm_shapes()
    assert (64, 1000, 2500) in shapes and (513, 40, 64) in shapes and (150, 201, 77) in shapes
    for m, n, k in shapes:
        assert capi.describe_dense_gemm(m, n, k) == dict(TM=64, TN=64, splits=1, kc=k, skinny=0), (m, n, k)


def test_every_gpu_shape_takes_the_build_its_test_names(capi):
    for bld, shapes in dc.GEMM_BUILD_SHAPES.items():
        for m, n, k in shapes:
            assert capi.describe_dense_gemm(m, n, k) == dict(TM=bld[0], TN=bld[1], splits=1, kc=k, skinny=0), (m, n, k)
    for bld, (m, n, k) in dc.GEMM_REAL_SHAPES.items():
        assert m * n * k <= 2e7 and dc.build(capi.describe_dense_gemm(m, n, k)) == bld
    for (m, n, k), (plan, cap, last) in dc.SPLITK_SHAPES.items():
        assert capi.describe_dense_gemm(m, n, k, ws_cap=cap) == plan
        assert k - (plan["splits"] - 1) * plan["kc"] == last
        assert capi.describe_dense_gemm(m, n, k)["splits"] == 1                       # no workspace, no split
    for (n, k), bld in dc.UPPER_SHAPES.items():
        assert dc.build(capi.describe_dense_gemm(n, n, k)) == bld
    for n, bld in dc.KTRI_SIZES.items():
        assert dc.build(capi.describe_dense_gemm(n, n, n)) == bld
    # BASELINE's two configurations: the dense 2048 x 4096 one, the 7 656-column Gram matrix of the sparse one
    assert dc.build(capi.describe_dense_gemm(2048, 2048, 4096)) == (128, 64)
    assert dc.build(capi.describe_dense_gemm(7656, 7656, 9983)) == (128, 128)


def test_no_input_selects_a_64_x_128_tile_and_every_build_is_named_by_a_gpu_test(capi):
    """TM = 64 needs m <= 64 or ceil(m/64) ceil(n/128) batch < 512; TN = 128 behind TM = 64 needs that product >= 512, hence m <= 64 --
    but then it equals ceil(m/128) ceil(n/128) batch, which is < 512 on this branch. The enumeration agrees, so the build is gone"""
    seen = set()
    for m, n, batch in itertools.product(SIZES, SIZES, (1, 2, 64)):
        for k, cap in ((8, None), (4096, None), (4096, 1 << 28)):
            seen.add(dc.build(capi.describe_dense_gemm(m, n, k, batch=batch, ws_cap=cap)))
    assert (64, 128) not in seen
    assert seen == set(dc.GEMM_BUILD_SHAPES) == {(64, 64), (128, 64), (128, 128)}
    # ... and the launcher instantiates exactly these
    src = open(SOURCE).read()
    launched = {(int(a), int(b)) for a, b in re.findall(r"^\s*(?:else )?if \(TM == \d+ && TN == \d+\) GEMM_LAUNCH\((\d+), (\d+),", src, flags=re.M)}
    assert launched == seen and len(re.findall(r"\bGEMM_LAUNCH\(\d", src)) == 3


def test_split_k_slices_are_never_empty_and_start_on_multiples_of_32(capi):
    n_split = 0
    for m, n in ((1, 1), (64, 64), (65, 129), (128, 1024), (256, 7656), (512, 2048), (700, 450), (2048, 2048)):
        for k in itertools.chain(range(1024, 9000, 37), (1024, 2047, 2048, 2055, 65536)):
            for cap in (m * n, 2 * m * n, 3 * m * n + 1, 8 * m * n, 1 << 28):
                p = capi.describe_dense_gemm(m, n, k, ws_cap=cap)
                if p["splits"] == 1:
                    assert p["kc"] == k
                    continue
                n_split += 1
                assert p["kc"] % 32 == 0 and (p["splits"] - 1) * p["kc"] < k <= p["splits"] * p["kc"], (m, n, k, cap, p)
                assert p["splits"] * m * n <= cap                                      # the slabs fit the workspace
                assert capi.describe_dense_gemm(m, n, k, batch=2, ws_cap=cap)["splits"] == 1      # blockIdx.z is the batch index then
    assert n_split > 1000


def test_the_workspace_size_does_not_change_the_plans_of_the_factorisation_shapes(capi):
    """rsqp_dgeqrf / rsqp_dorgqr hand the launcher ws_cap = 4 * 256 * mmax doubles: for the shapes of the GPU tests the plan of every such
    product is the same for mmax = m, 2 m and 700 (the workspace of the back-to-back test), so those runs must agree bit for bit"""
    for m, n in dc.QR_SHAPES:
        for mm, nn, kk in dc.qr_ws_products(m, n):
            plans = [capi.describe_dense_gemm(mm, nn, kk, ws_cap=4 * dc.OB * mmax) for mmax in (m, 2 * m, 700)]
            assert plans[0] == plans[1] == plans[2] and plans[0]["splits"] == 1, (m, n, mm, nn, kk)


# ---- the constructions of the GPU tests ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", dc.PD_RATIOS)
@pytest.mark.parametrize("kcol", dc.PD_COLUMNS)
def test_constructed_pivot_has_the_ratio_asked_for(kcol, ratio):
    """a longdouble Cholesky factorisation of the f64 matrix: pivot kcol is `ratio` of its diagonal entry (two decades from the
    2e-10 the rule puts the threshold at, either side), every other pivot within a few per cent of its own"""
    G = dc.pd_matrix(kcol, ratio)
    assert np.array_equal(G, G.T)
    piv = dc.longdouble_pivots(G)
    rel = np.asarray(piv / np.diag(G).astype(np.longdouble), dtype=float)
    assert 0.99 * ratio < rel[kcol] < 1.01 * ratio
    others = np.delete(rel, kcol)
    assert others.min() > 0.9 and others.max() <= 1.0 + 1e-15
    # the rule itself, p > pd_rel (|g| + max(g - p, 0)), at pd_rel = 1e-10
    thr = 1e-10 * (2.0 - rel[kcol])
    assert (rel[kcol] > thr) == (ratio == 1e-8) and abs(np.log10(rel[kcol] / thr)) > 1.5
