"""References for the banded H^-1 operator of the HBM-resident engine (include/rsqp_hip_band_check.h), in numpy alone.

The operator is H^-1 = sinv M^-T M^-1 sinv with M unit lower triangular, sub-diagonals m1 (M[i][i-1]) and m2 (M[i][i-2]), and
sinv = D^-1/2 of H = L D L'. Two questions are kept apart:

  the kernels' arithmetic   solve(m1, m2, sinv, B, dtype): the two sweeps from the f64 factor values the library returned, in
                            numpy.longdouble (the reference) and in float64 (the scan un-parallelised: one row after the other, the
                            yardstick for the kernels' error). Whatever error the host's factorisation has is in both and in the
                            kernels alike.
  the host's factorisation  ldl(d0, e1, e2): L D L' of the bands in numpy.longdouble, and rebuilt_bands(m1, m2, sinv): the bands of
                            L D L' rebuilt in longdouble from what the library returned, with the entrywise |L| |D| |L'|.

Every routine takes K problems at once: the factor arrays and the right-hand sides are n x K, the Python loop runs over the rows and
each step is one numpy operation over the K columns (the columns may belong to different Hessians)."""
import numpy as np

LD = np.longdouble
TH = 1024           # threads of the kernels: thread t owns rows t c .. t c + c - 1, c = ceil(n / TH)


def chunk_rows(n):
    return (n + TH - 1) // TH


def plain(mi, n, c):
    """the factor entry of every row 0..n-1 from a chunk-interleaved image (m1i or m2i): row i = t c + k sits at [k * TH + t], k < c"""
    i = np.arange(n)
    return mi[(i % c) * TH + i // c]


def solve(m1, m2, sinv, B, dtype=LD):
    """X = sinv * M^-T M^-1 (sinv * B), columnwise; m1, m2, sinv: n or n x K, B: n x K. All arithmetic in `dtype`"""
    B = np.asarray(B)
    n, K = B.shape
    m1, m2, sinv = (np.broadcast_to(np.asarray(a, dtype).reshape(n, -1), (n, K)) for a in (m1, m2, sinv))
    Z = np.asarray(B, dtype) * sinv
    for i in range(1, n):                                   # M z = v
        if i >= 2:
            Z[i] = Z[i] - m1[i] * Z[i - 1] - m2[i] * Z[i - 2]
        else:
            Z[i] = Z[i] - m1[i] * Z[i - 1]
    for i in range(n - 2, -1, -1):                          # M' x = z
        if i + 2 < n:
            Z[i] = Z[i] - m1[i + 1] * Z[i + 1] - m2[i + 2] * Z[i + 2]
        else:
            Z[i] = Z[i] - m1[i + 1] * Z[i + 1]
    return Z * sinv


def rho(X, Xref):
    """per column: |x - x_ref|_inf / |x_ref|_inf, as float64 (0 where both vanish)"""
    num = np.abs(np.asarray(X, LD) - Xref).max(axis=0)
    den = np.abs(Xref).max(axis=0)
    out = np.zeros(num.shape)
    nz = den > 0
    out[nz] = (num[nz] / den[nz]).astype(float)
    out[~nz & (num > 0)] = np.inf
    return out


def ldl(d0, e1, e2):
    """L D L' of the symmetric pentadiagonal matrix with bands d0 (diagonal), e1 (H[i][i-1]), e2 (H[i][i-2]) in longdouble:
    (d, l1, l2), without pivoting (the caller's matrix is positive definite)"""
    n = len(d0)
    d0, e1, e2 = (np.asarray(a, LD) for a in (d0, e1, e2))
    d, l1, l2 = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    for i in range(n):
        if i >= 2:
            l2[i] = e2[i] / d[i - 2]
        if i >= 1:
            l1[i] = (e1[i] - (l2[i] * d[i - 2] * l1[i - 1] if i >= 2 else 0)) / d[i - 1]
        d[i] = d0[i] - (l1[i] * l1[i] * d[i - 1] if i >= 1 else 0) - (l2[i] * l2[i] * d[i - 2] if i >= 2 else 0)
    return d, l1, l2


def bands_of_ldl(d, l1, l2):
    """the bands of L D L' and of |L| |D| |L'| (vectorised, in the dtype of the arguments): ((d0, e1, e2), (a0, a1, a2))"""
    n = len(d)
    z = np.zeros(1, d.dtype)
    dm1 = np.concatenate([z, d[:-1]]) if n > 1 else z[:n]          # d[i-1], 0 at i = 0
    dm2 = np.concatenate([z, z, d[:-2]])[:n] if n > 2 else np.zeros(n, d.dtype)
    l1m1 = np.concatenate([z, l1[:-1]]) if n > 1 else z[:n]        # l1[i-1]
    out = []
    for f in (lambda x: x, np.abs):
        D, D1, D2, L1, L2, L11 = f(d), f(dm1), f(dm2), f(l1), f(l2), f(l1m1)
        out.append((D + L1 * L1 * D1 + L2 * L2 * D2, L1 * D1 + L2 * D2 * L11, L2 * D2))
    return out[0], out[1]


def rebuilt_bands(m1, m2, sinv):
    """the library's factor back as bands, in longdouble: d = 1 / sinv^2, L = D^1/2 M D^-1/2"""
    m1, m2, sinv = (np.asarray(a, LD) for a in (m1, m2, sinv))
    n = len(sinv)
    sq = 1 / sinv
    d = sq * sq
    l1, l2 = np.zeros(n, LD), np.zeros(n, LD)
    l1[1:] = m1[1:] * sq[1:] / sq[:-1]
    l2[2:] = m2[2:] * sq[2:] / sq[:-2]
    return bands_of_ldl(d, l1, l2)


def dense(d0, e1, e2):
    n = len(d0)
    H = np.diag(np.asarray(d0, float))
    for i in range(1, n):
        H[i, i - 1] = H[i - 1, i] = e1[i]
    for i in range(2, n):
        H[i, i - 2] = H[i - 2, i] = e2[i]
    return H
