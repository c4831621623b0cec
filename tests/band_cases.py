"""Sizes, Hessians and right-hand sides for the banded H^-1 kernels (k_band_apply<C>, k_band_apply_mw<C>), shared by
tests/test_band_factor.py (no GPU) and tests/test_gpu_band_apply.py. The references of a size are computed once (problem_set) and
never written to afterwards.

Sizes. Thread t of 1024 owns c = ceil(n / 1024) consecutive rows, and c picks the build C of the kernels: each n below is the
smallest (or largest) at which a piece of that index arithmetic changes."""
import functools

import numpy as np

import band_ref as br

EPS = float(np.finfo(np.float64).eps)
MARGIN = 64.0       # the kernels may be this many times worse than the sequential f64 loop (or than eps)

# n -> the build the engine launches
SIZES = {1: 4, 2: 4, 3: 4, 64: 4, 65: 4, 1023: 4, 1024: 4,
         1025: 4,                         # c = 2: the threads from 513 on own nothing
         2049: 4, 4096: 4,
         4097: 8,                         # c = 5 < C
         8192: 8,
         8193: 10, 10000: 10, 10240: 10,  # (10 000: the benchmark's)
         10241: 12, 12288: 12,
         12289: 16,                       # c = 13
         16383: 16,                       # the last thread owns 15 rows
         16384: 16}
FORM_SIZES = (65, 4097, 10000)            # the engine's call forms: one size of three builds, c = 1, c < C, c == C


def build_of(c):
    """the rule c -> C as the issue states it: C = 4, 8, 10, 12, 16, the smallest that holds c rows"""
    return next(C for C in (4, 8, 10, 12, 16) if c <= C)


# ---- Hessians: bands (d0, e1, e2) = (H[i][i], H[i][i-1], H[i][i-2]) ----------------------------------------------------------------

def diagonal(rng, n):
    return 10.0 ** rng.uniform(-2, 2, n), np.zeros(n), np.zeros(n)


def dominant(rng, n, hb):
    """diagonally dominant, off-diagonal entries of mixed sign in (-1, 1)"""
    e1 = rng.uniform(-1, 1, n); e1[:1] = 0.0
    e2 = rng.uniform(-1, 1, n) if hb >= 2 else np.zeros(n)
    e2[:2] = 0.0
    row = np.abs(e1) + np.abs(e2)
    row[:-1] += np.abs(e1[1:]); row[:-2] += np.abs(e2[2:])
    return row + rng.uniform(0.1, 1.0, n), e1, e2


def biharmonic(n, s=1e-4):
    """[1, -4, 6 + s, -4, 1]: the homogeneous solutions of its factor grow polynomially along the rows"""
    e1 = np.full(n, -4.0); e1[:1] = 0.0
    e2 = np.full(n, 1.0); e2[:2] = 0.0
    return np.full(n, 6.0 + s), e1, e2


def growth_window(n, start):
    """H = L L' with l1 = -1.1 on the 64 rows from `start` (a multiple of 64: one window of the build's growth rule, 1.1^64 = 446) and
    -0.5 elsewhere: the homogeneous solution grows over exactly that window and decays everywhere else"""
    assert start % 64 == 0 and 0 <= start and start + 64 <= n
    l1 = np.full(n, -0.5); l1[start:start + 64] = -1.1; l1[0] = 0.0
    return 1.0 + l1 * l1, l1.copy(), np.zeros(n)


def growth_starts(n):
    """where the growing window is put. A wave of k_band_apply is a workgroup of k_band_apply_mw: both own the 64 c rows from a
    multiple of 64 c, so their seams coincide and lie on window boundaries. 64: inside the first wave (c >= 2), across its chunk
    seams; 64 c - 64: the last window before the first wave / workgroup seam (the grown state is what the forward sweep hands over);
    the first window behind the last such seam that has 64 rows behind it (what the backward sweep hands over). Never the first
    window of the matrix: row 0 has no neighbours, no state enters it, and the growth rule measures nothing there -- so sizes below
    128 have no such case"""
    c = br.chunk_rows(n)
    last = (n - 64) // (64 * c) * 64 * c if n >= 64 else -1
    return sorted({s for s in (64, 64 * c - 64, last) if 64 <= s and s + 64 <= n})


def hessians(n):
    """[(name, half bandwidth, (d0, e1, e2))]: half bandwidth 0, 1 and 2 at every size"""
    rng = np.random.default_rng([4501, n])
    out = [("diag", 0, diagonal(rng, n)), ("dominant3", 1, dominant(rng, n, 1)), ("dominant5", 2, dominant(rng, n, 2)),
           ("biharmonic", 2, biharmonic(n))]
    return out + [("growth@%d" % s, 1, growth_window(n, s)) for s in growth_starts(n)]


def unit_rows(n):
    """columns of H^-1 that straddle the first wave seam, and the last one"""
    c = br.chunk_rows(n)
    return sorted({r for r in (64 * c - 2, 64 * c - 1, 64 * c, 64 * c + 1, n - 1) if 0 <= r < n})


def rhs(n):
    """n x R: one random vector, then the unit vectors of unit_rows(n)"""
    rng = np.random.default_rng([4502, n])
    rows = unit_rows(n)
    B = np.zeros((n, 1 + len(rows)))
    B[:, 0] = rng.normal(size=n)
    for j, r in enumerate(rows):
        B[r, 1 + j] = 1.0
    return B, ["random"] + ["e%d" % r for r in rows]


class Problem:
    """one Hessian of one size: the library's factor, the right-hand sides, the longdouble solution and rho of the sequential loop"""

    def __init__(self, n, name, hb, bands, fac):
        self.n, self.name, self.hb, self.bands, self.fac = n, name, hb, bands, fac
        c = fac["c"]
        self.m1, self.m2, self.sinv = br.plain(fac["m1i"], n, c), br.plain(fac["m2i"], n, c), fac["sinv"]


@functools.lru_cache(maxsize=None)
def problem_set(n):
    """every Hessian of size n with its factor (rsqp_band_check_factor; no GPU) and, for all of them in one pass over the rows, the
    reference solutions of rhs(n): p.B (n x R), p.names, p.Xref (longdouble), p.rho_seq (R)"""
    from restartsqp_amd import capi
    B, names = rhs(n)
    R = B.shape[1]
    ps = []
    for name, hb, bands in hessians(n):
        fac = capi.band_factor(*bands)
        assert fac["built"], (n, name, fac["growth"])
        ps.append(Problem(n, name, hb, bands, fac))
    rep = lambda key: np.repeat(np.stack([getattr(p, key) for p in ps], axis=1), R, axis=1)      # column (p, r) at p R + r
    BB = np.tile(B, (1, len(ps)))
    Xref = br.solve(rep("m1"), rep("m2"), rep("sinv"), BB, br.LD)
    Xseq = br.solve(rep("m1"), rep("m2"), rep("sinv"), BB, np.float64)
    rho_seq = br.rho(Xseq, Xref)
    for k, p in enumerate(ps):
        p.B, p.names = B, names
        p.Xref, p.rho_seq = Xref[:, k * R:(k + 1) * R], rho_seq[k * R:(k + 1) * R]
        for a in (p.B, p.Xref, p.rho_seq):
            a.flags.writeable = False
    return tuple(ps)


def allowed(rho_seq):
    return MARGIN * np.maximum(rho_seq, EPS)
