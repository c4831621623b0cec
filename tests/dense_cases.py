"""The shapes the dense f64 kernels (restartsqp_amd/csrc/dense_la.hip) are tested at, shared by tests/test_dense_plan.py (no GPU:
which build of k_dgemm the launch plan gives each of them) and tests/test_gpu_dense_forms.py (the runs), and the constructions
both use."""
import ast
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# build (TM, TN) of k_dgemm -> the (m, n, k) that run it in test_gpu_dense_forms.py
GEMM_BUILD_SHAPES = {
    (128, 64): [(2048, 2048, 20), (1990, 1925, 20)],
    (128, 128): [(8065, 897, 20), (8, 65409, 8)],      # (8 rows in a 128-row tile: the clamped tile pointers)
    (64, 64): [(130, 70, 33)],
}
# real-valued data against a longdouble product: m n k <= 2e7
GEMM_REAL_SHAPES = {(64, 64): (300, 257, 129), (128, 64): (2048, 2048, 4), (128, 128): (8065, 897, 2)}
# split K: (m, n, k) -> (plan, doubles of the workspace, length of the last slice)
SPLITK_SHAPES = {
    (64, 64, 1031): (dict(TM=64, TN=64, splits=4, kc=288, skinny=0), 8 * 64 * 64, 167),
    (128, 1024, 2055): (dict(TM=128, TN=128, splits=8, kc=288, skinny=1), 8 * 128 * 1024, 39),
}
UPPER_SHAPES = {(200, 33): (64, 64), (2048, 20): (128, 64)}      # (n, k) -> build
KTRI_SIZES = {130: (64, 64), 200: (64, 64), 2048: (128, 64)}      # n (= k) -> build
QR_SHAPES = [(5, 3), (64, 64), (200, 130), (700, 450), (300, 300), (129, 1), (128, 64), (320, 320)]
CHOL_SIZES = [1, 7, 64, 65, 128, 192, 200, 320, 513]
PD_N, PD_COLUMNS, PD_RATIOS = 320, (10, 100, 300, 319), (1e-8, 1e-12)
NB, OB = 64, 256      # panel and outer block of the factorisations (dense_la.hip)


def old_gemm_shapes():
    """every (m, n, k) tests/test_gpu_dense.py gives the GEMM, read from its source"""
    src = open(os.path.join(HERE, "test_gpu_dense.py")).read()
    shapes = ast.literal_eval(re.search(r'parametrize\("m,n,k", (\[.*?\])\)', src).group(1))
    m, k, k2, n = map(int, re.search(r"size=\((\d+), (\d+)\)\).astype\(float\)\s+B = rng.integers\(-8, 9, size=\((\d+), (\d+)\)\)", src).groups())
    assert k == k2 and len(shapes) == 6
    return shapes + [(m, n, k)]


def build(plan):
    return plan["TM"], plan["TN"]


def qr_ws_products(m, n):
    """(m', n', k') of every product rsqp_dgeqrf + rsqp_dorgqr give the workspace's split-K slabs (dense_la.hip), for an m x n matrix"""
    out = []
    for K0 in range(0, n, OB):
        ob, mto = min(OB, n - K0), m - K0
        for k0 in range(K0, K0 + ob, NB):
            jb = min(NB, K0 + ob - k0)
            mt, nin = m - k0, K0 + ob - k0 - jb
            if nin > 0:
                out.append((jb, nin, mt))
        if ob > NB:
            out.append((ob, ob, mto))
        if n - K0 - ob > 0:
            out.append((ob, n - K0 - ob, mto))
        out.append((ob, mto, mto))
    return out


def pd_matrix(kcol, ratio, n=PD_N, seed=0):
    """G = U'U (f64) with U = I + a small strictly upper triangular part and U[k, k]^2 = ratio * g_kk: the pivot of column k is `ratio`
    of its diagonal entry, every other pivot close to it"""
    rng = np.random.default_rng(1000 * kcol + seed)
    U = np.eye(n) + np.triu(rng.uniform(-0.01, 0.01, size=(n, n)), 1)
    s = float(np.sum(U[:kcol, kcol] ** 2))
    U[kcol, kcol] = np.sqrt(ratio * s / (1.0 - ratio))
    return U.T @ U


def longdouble_pivots(G):
    """the pivots d_j = u_jj^2 of the Cholesky factorisation G = U'U, in longdouble"""
    A = np.array(G, dtype=np.longdouble)
    n = A.shape[0]
    piv = np.zeros(n, np.longdouble)
    for j in range(n):
        piv[j] = A[j, j]
        if j + 1 < n:
            r = A[j, j + 1:] / piv[j]
            A[j + 1:, j + 1:] -= np.outer(r, A[j, j + 1:])
    return piv


def dependent_matrix(m, n, col, dependent=True):
    rng = np.random.default_rng(m + n + col)
    B = rng.normal(size=(m, n))
    if dependent:
        B[:, col] = B[:, 3] * 2.0 - B[:, 17]
    return B
