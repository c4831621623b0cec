// dense_la.hip -- dense f64 building blocks for gfx950 (see rsqp_dense.h).
//
//   * k_dgemm: LDS-tiled GEMM on v_mfma_f64_16x16x4_f64. Workgroup = 8 waves (2 x 4) on a 128 x 128
//     tile or 4 waves (2 x 2) on a 128 x 64 or 64 x 64 tile (three builds: dgemm_plan), K step 16. Both operand tiles are staged in LDS as [k][index] so that the
//     fragment of an MFMA (lane l: index l & 15, k = l >> 4) is one ds_read_b64 with 16 consecutive
//     lanes on consecutive words; the next K tile is fetched into registers while the current one
//     is multiplied. The roles of the two MFMA operands are swapped (D = B_frag x A_frag) so that
//     the 16 lanes that share a result register hold 16 consecutive ROWS of C: column-major C
//     is then written in 128-byte segments.
//   * blocked Householder QR / explicit Q / triangular inverse / Cholesky: panels of NB = 64
//     columns are factored by small kernels, everything else is rsqp_dgemm.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "rsqp_dense.h"
#include "rsqp_internal.h"

typedef double d4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int GK16 = 16;   // K step of the GEMM (32 for the 8-wave 128 x 128 tile)
#ifndef RSQP_GPAD
#define RSQP_GPAD 4
#endif
#ifndef RSQP_GEMM_GK
#define RSQP_GEMM_GK 16     // K step of the 128 x 128 tile (tuning builds: 32)
#endif
#ifndef RSQP_GEMM_DB
#define RSQP_GEMM_DB 0
#endif
constexpr int GPAD = RSQP_GPAD;   // LDS row padding (doubles): row stride = 8 words mod 64 banks (tools/gemm_pad_variants.sh builds others)

// one operand tile (GK x T) -> registers. kcontig: element (kk, t) at X[kk + t * ld], else X[t + kk * ld]
template <int T, int NTHR, int GK>
__device__ __forceinline__ void load_tile(double (&r)[GK * T / NTHR], const double *X, long long ld, bool kcontig, int k0,
                                          int t0, int kmax, int tmax) {
    constexpr int E = GK * T / NTHR;
    const int tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < E; e++) {
        int kk, t;
        if (kcontig) { kk = tid & (GK - 1); t = tid / GK + (NTHR / GK) * e; }
        else { t = tid % T; kk = tid / T + (NTHR / T) * e; }
        const int gk = k0 + kk, gt = t0 + t;
        double v = 0.0;
        if (gk < kmax && gt < tmax) v = kcontig ? X[gk + (long long)gt * ld] : X[gt + (long long)gk * ld];
        r[e] = v;
    }
}
// the same tile through per-thread pointers that step along K: one load and one 64-bit add per element instead of the index
// arithmetic, bounds tests and selects of load_tile (~350 VALU instructions per K step of a wave against its 32 MFMAs -- they
// kept the matrix pipe at 67 % busy). Valid while the whole K range of the tile is inside the slice (the last, partial step of
// a slice takes load_tile); a tile index past the edge of the matrix is CLAMPED to the last one: what it loads only reaches
// rows / columns of C that are never stored.
template <int T, int NTHR, int GK> struct TilePtr {
    static constexpr int E = GK * T / NTHR;
    const double *p[E];
    long long step;
    __device__ __forceinline__ void init(const double *X, long long ld, bool kcontig, int k0, int t0, int tmax) {
        const int tid = threadIdx.x;
#pragma unroll
        for (int e = 0; e < E; e++) {
            int kk, t;
            if (kcontig) { kk = tid & (GK - 1); t = tid / GK + (NTHR / GK) * e; }
            else { t = tid % T; kk = tid / T + (NTHR / T) * e; }
            const int gt = min(t0 + t, tmax - 1);
            p[e] = kcontig ? X + (k0 + kk) + (long long)gt * ld : X + gt + (long long)(k0 + kk) * ld;
        }
        step = kcontig ? (long long)GK : (long long)GK * ld;
    }
    __device__ __forceinline__ void load(double (&r)[E]) {
#pragma unroll
        for (int e = 0; e < E; e++) { r[e] = *p[e]; p[e] += step; }
    }
    __device__ __forceinline__ void skip() {
#pragma unroll
        for (int e = 0; e < E; e++) p[e] += step;
    }
};
template <int T, int NTHR, int GK>
__device__ __forceinline__ void store_tile(const double (&r)[GK * T / NTHR], double (*S)[T + GPAD], bool kcontig) {
    constexpr int E = GK * T / NTHR;
    const int tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < E; e++) {
        int kk, t;
        if (kcontig) { kk = tid & (GK - 1); t = tid / GK + (NTHR / GK) * e; }
        else { t = tid % T; kk = tid / T + (NTHR / T) * e; }
        S[kk][t] = r[e];
    }
}

// NW waves as 2 (rows) x NW/2 (columns); MINW = resident waves per SIMD the register budget allows
template <int TM, int TN, int NW, int MINW, int GK>
__global__ void __launch_bounds__(NW * 64, MINW)
k_dgemm(int ta, int tb, int m, int n, int kfull, int kc, double alpha, const double *__restrict__ A, long long lda,
        const double *__restrict__ B, long long ldb, double beta, double *__restrict__ C, long long ldc, int upper, int ktri,
        long long sA, long long sB, long long sC) {
    extern __shared__ __attribute__((aligned(16))) double gemm_lds[];
    // RSQP_GEMM_DB=1 (tuning build, tools/gemm_pad_variants.sh): two LDS buffers, the tiles of step i + 1 stored while step i is
    // still being multiplied, one barrier per K step instead of two -- measured SLOWER (51.3 vs 53.1 TFLOP/s on 4096^3, QR
    // 100.4 vs 97.8 ms): the barriers are not what keeps the MFMA pipe at 67 % busy. Row paddings 2 .. 20 doubles: no difference. Other tile shapes, K step 32
    // (spills), the AGPR form of the MFMAs (a 64 / 64 register split: spills, 16 TFLOP/s): all slower or equal.
    constexpr int NBUF = RSQP_GEMM_DB ? 2 : 1;
    constexpr int TILE_DOUBLES = GK * ((TM + GPAD) + (TN + GPAD));
    constexpr int NTHR = NW * 64, WN = NW / 2;
    constexpr int MI = TM / 32, NJ = TN / (16 * WN);   // 16x16 blocks per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int i0 = blockIdx.x * TM, j0 = blockIdx.y * TN;
    // upper != 0: a SYMMETRIC result of which only the upper triangle is wanted (Gram matrix, U^-1 U^-T, the trailing update of the
    // Cholesky factorisation): tiles strictly below the diagonal are not computed (half the work; what they hold is not defined)
    if (upper && i0 >= j0 + TN) return;
    const bool akc = ta != 0, bkc = tb == 0;   // k-contiguous operands
    // split K: slice blockIdx.z of the inner dimension, partial result into its own m x n slab
    // sC != 0: blockIdx.z is a BATCH index -- independent products of one shape whose operands lie sA / sB / sC doubles apart (the
    // pairs of one level of the triangular inverse in ONE launch); otherwise it is the split-K slice
    const bool batched = sC != 0;
    if (batched) { A += (long long)blockIdx.z * sA; B += (long long)blockIdx.z * sB; C += (long long)blockIdx.z * sC; }
    int kbeg = batched ? 0 : blockIdx.z * kc, k = min(kfull, kbeg + kc);
    // ktri != 0: an operand is TRIANGULAR with exact zeros in its other triangle -- the part of the inner dimension on which this
    // tile's rows or columns are zero is skipped (the skipped terms are products with 0.0: the result keeps its bits).
    //   1  C = X X' (upper tiles), X upper triangular: X[i][kk] = 0 for kk < i, so only kk >= j0 contributes
    //   2  op(A) upper triangular (A not transposed): kk >= i0        3  op(A) = A', A upper triangular: kk < i0 + TM
    if (ktri == 1) kbeg = max(kbeg, (j0 / GK) * GK);
    else if (ktri == 2) kbeg = max(kbeg, (i0 / GK) * GK);
    else if (ktri == 3) k = min(k, i0 + TM);
    if (!batched) C += (long long)blockIdx.z * m * n;
    d4 acc[NJ][MI];
#pragma unroll
    for (int a = 0; a < NJ; a++)
#pragma unroll
        for (int b = 0; b < MI; b++) acc[a][b] = (d4){0.0, 0.0, 0.0, 0.0};
    double ra[GK * TM / NTHR], rb[GK * TN / NTHR];
    TilePtr<TM, NTHR, GK> pa;
    TilePtr<TN, NTHR, GK> pb;
    pa.init(A, lda, akc, kbeg, i0, m);
    pb.init(B, ldb, bkc, kbeg, j0, n);
    if (kbeg + GK <= k) { pa.load(ra); pb.load(rb); }
    else {
        load_tile<TM, NTHR, GK>(ra, A, lda, akc, kbeg, i0, k, m);
        load_tile<TN, NTHR, GK>(rb, B, ldb, bkc, kbeg, j0, k, n);
    }
    if (NBUF == 2) {
        store_tile<TM, NTHR, GK>(ra, reinterpret_cast<double (*)[TM + GPAD]>(gemm_lds), akc);
        store_tile<TN, NTHR, GK>(rb, reinterpret_cast<double (*)[TN + GPAD]>(gemm_lds + GK * (TM + GPAD)), bkc);
        __syncthreads();
    }
    int buf = 0;
    for (int k0 = kbeg; k0 < k; k0 += GK) {
        double (*As)[TM + GPAD] = reinterpret_cast<double (*)[TM + GPAD]>(gemm_lds + buf * TILE_DOUBLES);
        double (*Bs)[TN + GPAD] = reinterpret_cast<double (*)[TN + GPAD]>(gemm_lds + buf * TILE_DOUBLES + GK * (TM + GPAD));
        if (NBUF == 1) {
            store_tile<TM, NTHR, GK>(ra, As, akc);
            store_tile<TN, NTHR, GK>(rb, Bs, bkc);
            __syncthreads();
        }
        const bool more = k0 + GK < k;
        if (more) {
            if (k0 + 2 * GK <= k) { pa.load(ra); pb.load(rb); }      // (uniform: the next tile lies inside the slice)
            else {
                load_tile<TM, NTHR, GK>(ra, A, lda, akc, k0 + GK, i0, k, m);
                load_tile<TN, NTHR, GK>(rb, B, ldb, bkc, k0 + GK, j0, k, n);
            }
        }
#pragma unroll
        for (int k4 = 0; k4 < GK; k4 += 4) {
            double af[MI], bf[NJ];
#pragma unroll
            for (int b = 0; b < MI; b++) af[b] = As[k4 + (lane >> 4)][wm * (TM / 2) + b * 16 + (lane & 15)];
#pragma unroll
            for (int a = 0; a < NJ; a++) bf[a] = Bs[k4 + (lane >> 4)][wn * (TN / WN) + a * 16 + (lane & 15)];
#pragma unroll
            for (int a = 0; a < NJ; a++)
#pragma unroll
                for (int b = 0; b < MI; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(bf[a], af[b], acc[a][b], 0, 0, 0);
        }
        if (NBUF == 2) {
            if (more) {
                buf ^= 1;
                store_tile<TM, NTHR, GK>(ra, reinterpret_cast<double (*)[TM + GPAD]>(gemm_lds + buf * TILE_DOUBLES), akc);
                store_tile<TN, NTHR, GK>(rb, reinterpret_cast<double (*)[TN + GPAD]>(gemm_lds + buf * TILE_DOUBLES + GK * (TM + GPAD)), bkc);
            }
        }
        __syncthreads();
    }
    // result register r of block (a, b): C row i = .. + (lane & 15), column j = .. + (lane >> 4) + 4 r
#pragma unroll
    for (int a = 0; a < NJ; a++)
#pragma unroll
        for (int b = 0; b < MI; b++) {
            const int i = i0 + wm * (TM / 2) + b * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = j0 + wn * (TN / WN) + a * 16 + (lane >> 4) + 4 * r;
                if (i < m && j < n) {
                    double *c = C + i + (long long)j * ldc;
                    const double v = alpha * acc[a][b][r];
                    *c = beta == 0.0 ? v : v + beta * *c;
                }
            }
        }
}

// deterministic split-K: partial products into `ws` ([split][n][m]), then summed in order
__global__ void k_splitk_reduce(int m, int n, int splits, const double *__restrict__ ws, double alpha, double beta,
                                double *__restrict__ C, long long ldc) {
    const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (e >= (long long)m * n) return;
    const int i = (int)(e % m), j = (int)(e / m);
    double s = 0.0;
    for (int z = 0; z < splits; z++) s += ws[(long long)z * m * n + e];
    double *c = C + i + (long long)j * ldc;
    *c = beta == 0.0 ? alpha * s : alpha * s + beta * *c;
}

}  // namespace

// The launch plan of one product (m, n >= 1): which build of k_dgemm (its tile TM x TN), into how many slices of kc the inner
// dimension is split (splits == 1: kc == k), and whether the forced 128 x 128 "skinny" case applies. The ONE place where this is
// decided: dgemm_ws launches what it says, rsqp_dense_describe_gemm (rsqp_hip_dense_check.h) shows it without a GPU.
// The build <64, 128> does not exist: TM = 64 needs m <= 64 (then ceil(m/64) = ceil(m/128) = 1) or ceil(m/64) ceil(n/128) batch
// < 512; TN = 128 behind it needs that same product >= 512 -- so m <= 64, and the product equals `big`, which is < 512 here
// (tests/test_dense_plan.py enumerates it).
struct DgemmPlan { int TM, TN, splits, kc, skinny; };
static DgemmPlan dgemm_plan(int m, int n, int k, int batch, bool have_ws, long long ws_cap) {
    // large tiles when they still give every CU work, small ones otherwise
    const long long big = (long long)((m + 127) / 128) * ((n + 127) / 128) * std::max(batch, 1);
    int TM = 128, TN = 128;
    if (big < 512) {
        TM = m <= 64 || (long long)((m + 63) / 64) * ((n + 127) / 128) * std::max(batch, 1) < 512 ? 64 : 128;
        TN = n <= 64 || (long long)((m + TM - 1) / TM) * ((n + 127) / 128) * std::max(batch, 1) < 512 ? 64 : 128;
    }
    // a block of reflectors against a wide matrix (W = V'C: 256 x n with an inner dimension of thousands): the large tile,
    // and K split so that the chip has work -- 64 x 64 tiles ran these at 29-35 TFLOP/s
    const bool skinny_case = have_ws && m <= 512 && m >= 128 && n >= 1024 && k >= 2048 && ws_cap >= 2LL * m * n;
    if (skinny_case) { TM = 128; TN = 128; }
    const int bx = (m + TM - 1) / TM, by = (n + TN - 1) / TN;
    // a long inner dimension over few output tiles: split K so that the chip has work
    int splits = 1;
    if (have_ws && ((long long)bx * by < 200 || skinny_case) && k >= 1024) {
        splits = (int)std::min<long long>(std::min<long long>((511 + (long long)bx * by) / ((long long)bx * by), k / 256), ws_cap / ((long long)m * n));
        if (splits < 2) splits = 1;
    }
    int kc = k;
    if (splits > 1) { kc = ((k + splits - 1) / splits + 31) / 32 * 32; splits = (k + kc - 1) / kc; }
    if (batch > 1) splits = 1;
    return DgemmPlan{TM, TN, splits, kc, skinny_case ? 1 : 0};
}

static hipError_t dgemm_ws(bool transA, bool transB, int m, int n, int k, double alpha, const double *A, long long lda,
                           const double *B, long long ldb, double beta, double *C, long long ldc, double *ws,
                           long long ws_cap, hipStream_t st, int upper = 0, int ktri = 0, int batch = 1, long long sA = 0,
                           long long sB = 0, long long sC = 0) {
    if (m <= 0 || n <= 0) return hipSuccess;
    const int ta = transA ? 1 : 0, tb = transB ? 1 : 0;
    const DgemmPlan pl = dgemm_plan(m, n, k, batch, ws != nullptr, ws_cap);
    const int TM = pl.TM, TN = pl.TN, splits = pl.splits, kc = pl.kc;
    const int bx = (m + TM - 1) / TM, by = (n + TN - 1) / TN;
    dim3 grid(bx, by, batch > 1 ? batch : splits);
    double *Cout = splits > 1 ? ws : C;
    const long long ldo = splits > 1 ? m : ldc;
    const double al = splits > 1 ? 1.0 : alpha, be = splits > 1 ? 0.0 : beta;
#define GEMM_LAUNCH(a, b, nw, mw, gk)                                                                              \
    do {                                                                                                           \
        const size_t lds_ = sizeof(double) * gk * ((a + GPAD) + (b + GPAD)) * (RSQP_GEMM_DB ? 2 : 1);               \
        static std::atomic<unsigned long long> set_{0};                                                            \
        rsqp_allow_full_lds(reinterpret_cast<const void *>(&k_dgemm<a, b, nw, mw, gk>), set_, (int)lds_);          \
        hipLaunchKernelGGL((k_dgemm<a, b, nw, mw, gk>), grid, dim3(nw * 64), lds_, st, ta, tb, m, n, k, kc, al, A, \
                           lda, B, ldb, be, Cout, ldo, upper, ktri, batch > 1 ? sA : 0LL, batch > 1 ? sB : 0LL,    \
                           batch > 1 ? sC : 0LL);                                                                  \
    } while (0)
    // measured on 4096^3: 8 waves (4 resident per SIMD, 122 VGPRs) 53.5 TFLOP/s; 4 waves x 2 resident
    // 51.5; 4 waves x 1 resident (the compiler's default allocation) 37.8; K step 32 is slower (spills)
    if (TM == 128 && TN == 128) GEMM_LAUNCH(128, 128, 8, 4, RSQP_GEMM_GK);
    else if (TM == 128 && TN == 64) GEMM_LAUNCH(128, 64, 4, 3, 16);
    else if (TM == 64 && TN == 64) GEMM_LAUNCH(64, 64, 4, 4, 16);
    else return hipErrorInvalidValue;      // (a plan no build serves: dgemm_plan yields none)
#undef GEMM_LAUNCH
    if (splits > 1) {
        const long long tot = (long long)m * n;
        hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, m, n, splits, ws, alpha, beta, C, ldc);
    }
    return hipGetLastError();
}

hipError_t rsqp_dgemm(bool transA, bool transB, int m, int n, int k, double alpha, const double *A, long long lda,
                      const double *B, long long ldb, double beta, double *C, long long ldc, hipStream_t st) {
    return dgemm_ws(transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, nullptr, 0, st);
}
// an operand triangular with exact zeros in its other triangle (ktri: see k_dgemm): the zero part of the inner dimension is skipped
hipError_t rsqp_dgemm_tri(bool transA, bool transB, int m, int n, int k, double alpha, const double *A, long long lda,
                          const double *B, long long ldb, double beta, double *C, long long ldc, int ktri, hipStream_t st) {
    return dgemm_ws(transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, nullptr, 0, st, 0, ktri);
}
// C (n x n, upper tiles) = X X' for an UPPER TRIANGULAR X (n x n; its strict lower triangle must hold zeros): U^-1 U^-T
hipError_t rsqp_dtrmmt_upper(int n, double alpha, const double *X, long long ldx, double *C, long long ldc, hipStream_t st) {
    return dgemm_ws(false, true, n, n, n, alpha, X, ldx, X, ldx, 0.0, C, ldc, nullptr, 0, st, 1, 1);
}
// the same for a symmetric n x n result of which only the UPPER triangle is wanted (tiles strictly below the diagonal are skipped)
hipError_t rsqp_dgemm_upper(bool transA, bool transB, int n, int k, double alpha, const double *A, long long lda,
                            const double *B, long long ldb, double beta, double *C, long long ldc, hipStream_t st) {
    return dgemm_ws(transA, transB, n, n, k, alpha, A, lda, B, ldb, beta, C, ldc, nullptr, 0, st, 1);
}
namespace {
// lower triangle := transpose of the upper one (32 x 32 tiles through LDS)
__global__ void k_mirror_upper(int n, double *__restrict__ M, long long ld) {
    __shared__ double tile[32][33];
    const int bi = blockIdx.x, bj = blockIdx.y;      // tile (rows bi, cols bj) of the UPPER part, bi <= bj
    if (bi > bj) return;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int i = bi * 32 + threadIdx.x, j = bj * 32 + r;
        tile[r][threadIdx.x] = (i < n && j < n) ? M[i + (long long)j * ld] : 0.0;      // tile[jj][ii] = M(i, j)
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int i2 = bj * 32 + threadIdx.x, j2 = bi * 32 + r;                         // M(i2, j2) = M(j2, i2), i2 >= j2
        if (i2 < n && j2 < n && i2 > j2) M[i2 + (long long)j2 * ld] = tile[threadIdx.x][r];
    }
}
}  // namespace
hipError_t rsqp_mirror_upper(int n, double *M, long long ld, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_mirror_upper, dim3((n + 31) / 32, (n + 31) / 32), dim3(32, 8), 0, st, n, M, ld);
    return hipGetLastError();
}

// =====================================================================================
// blocked factorisations
// =====================================================================================
namespace {

constexpr int NB = 64;
#ifndef RSQP_QR_OB
#define RSQP_QR_OB 256
#endif
constexpr int OB = RSQP_QR_OB;    // outer block of the QR: the trailing matrix is updated once per OB columns (aggregated reflector)

template <int NTHR>
__device__ __forceinline__ double block_sum(double v, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NTHR / 64; w++) s += red[w];
    return s;
}
__device__ __forceinline__ double block_sum256(double v, double *red) { return block_sum<256>(v, red); }
constexpr int QC = 1024;   // threads of the panel-column kernel (latency bound: 10 rows per thread at m = 10 000)

__global__ void __launch_bounds__(256) k_colnorm2(int m, const double *__restrict__ B, long long ldb, double *__restrict__ out) {
    __shared__ double red[4];
    const double *c = B + (long long)blockIdx.x * ldb;
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s += c[i] * c[i];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// Column j of the panel that starts at k0. Every workgroup derives the Householder reflector of
// column j (rows j..m-1) on its own -- the column is read-only during this launch -- and then
// workgroup 0 stores it (explicit, unit diagonal) in V / tau / rdiag, workgroup b > 0 applies it
// to panel column j + b.
__global__ void __launch_bounds__(QC)
k_qr_col(double *__restrict__ B, long long ldb, int m, int j, int k0, double *__restrict__ V, long long ldv,
         double *__restrict__ tau, double *__restrict__ rdiag, const double *__restrict__ norm2, double eps_li,
         int *__restrict__ flag) {
    __shared__ double red[QC / 64], red2[QC / 64];
    const double *cj = B + (long long)j * ldb;
    double *cc = B + (long long)(j + blockIdx.x) * ldb;
    // one pass: the tail of column j and of this workgroup's column stay in registers (QR_REG rows
    // per thread, i.e. m - j <= QR_REG * 1024; longer columns take the re-reading path)
    constexpr int QR_REG = 12;
    const bool inreg = m - j - 1 <= QR_REG * QC, mine = blockIdx.x != 0;
    double vj[QR_REG], vc[QR_REG];
    double s = 0.0, d = 0.0;
    if (inreg) {
#pragma unroll
        for (int u = 0; u < QR_REG; u++) {
            const int i = j + 1 + threadIdx.x + u * QC;
            vj[u] = i < m ? cj[i] : 0.0;
            vc[u] = (mine && i < m) ? cc[i] : 0.0;
            s += vj[u] * vj[u];
            d += vj[u] * vc[u];
        }
    } else {
        for (int i = j + 1 + threadIdx.x; i < m; i += QC) { const double a = cj[i]; s += a * a; if (mine) d += a * cc[i]; }
    }
    // both sums through one pair of barriers
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); d += __shfl_xor(d, o); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = s; red2[threadIdx.x >> 6] = d; }
    __syncthreads();
    double sigma = 0.0, dsum = 0.0;
#pragma unroll
    for (int w = 0; w < QC / 64; w++) { sigma += red[w]; dsum += red2[w]; }
    const double alpha = cj[j];
    double tj = 0.0, beta = alpha, scale = 0.0;
    if (sigma != 0.0) {
        const double nrm = sqrt(alpha * alpha + sigma);
        beta = alpha >= 0.0 ? -nrm : nrm;
        tj = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    if (!mine) {
        if (threadIdx.x == 0) {
            tau[j] = tj; rdiag[j] = beta;
            if (!(sqrt(alpha * alpha + sigma) > eps_li * sqrt(norm2[j]))) atomicAdd(flag, 1);
        }
        double *v = V + (long long)(j - k0) * ldv;
        for (int i = k0 + threadIdx.x; i <= j && i < m; i += QC) v[i - k0] = i < j ? 0.0 : 1.0;
        if (inreg) {
#pragma unroll
            for (int u = 0; u < QR_REG; u++) {
                const int i = j + 1 + threadIdx.x + u * QC;
                if (i < m) v[i - k0] = vj[u] * scale;
            }
        } else {
            for (int i = j + 1 + threadIdx.x; i < m; i += QC) v[i - k0] = cj[i] * scale;
        }
        return;
    }
    const double w = tj * (cc[j] + scale * dsum);
    const double sw = scale * w;
    if (inreg) {
#pragma unroll
        for (int u = 0; u < QR_REG; u++) {
            const int i = j + 1 + threadIdx.x + u * QC;
            if (i < m) cc[i] = vc[u] - vj[u] * sw;
        }
    } else {
        for (int i = j + 1 + threadIdx.x; i < m; i += QC) cc[i] -= cj[i] * sw;
    }
    __syncthreads();
    if (threadIdx.x == 0) cc[j] -= w;
}

// T factor of a panel (forward, columnwise: H_1 ... H_jb = I - V T V') from S = V'V and tau, by recursive merging
// (the block form of the column recurrence T[0:i, i] = -tau_i T[0:i, 0:i] S[0:i, i]: two reflector blocks a, b with
// factors T_a, T_b merge into [[T_a, -T_a (V_a'V_b) T_b], [0, T_b]]): blocks of 1, 2, 4, .. 32 columns, every level
// two small products in LDS over all 256 threads -- 12 barriers instead of the recurrence's 128 and no 63-term serial
// rows (100 -> ~10 us per panel).
__global__ void __launch_bounds__(256)
k_qr_T_merge(int jb, const double *__restrict__ S, const double *__restrict__ tau, double *__restrict__ T) {
    __shared__ double Ts[NB][NB + 1], Ss[NB][NB + 1], Us[NB][NB + 1];
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        const int r = e % NB, c = e / NB;
        Ts[r][c] = (r == c && r < jb) ? tau[r] : 0.0;
        Ss[r][c] = (r < jb && c < jb) ? S[r + c * jb] : 0.0;
    }
    __syncthreads();
    for (int sz = 1; sz < NB; sz *= 2) {
        // U = T_a X for every pair: element (r, c) of pair q lives at Us[base + r][base + sz + c], X = S[a rows, b cols]
        const int per = sz * sz, npair = NB / (2 * sz);
        for (int e = threadIdx.x; e < npair * per; e += 256) {
            const int q = e / per, rc = e - q * per, r = rc % sz, c = rc / sz, base = q * 2 * sz;
            double acc = 0.0;
            for (int k = r; k < sz; k++) acc += Ts[base + r][base + k] * Ss[base + k][base + sz + c];
            Us[base + r][base + sz + c] = acc;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < npair * per; e += 256) {
            const int q = e / per, rc = e - q * per, r = rc % sz, c = rc / sz, base = q * 2 * sz;
            double acc = 0.0;
            for (int k = 0; k <= c; k++) acc += Us[base + r][base + sz + k] * Ts[base + sz + k][base + sz + c];
            Ts[base + r][base + sz + c] = -acc;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < NB * NB; e += 256) T[e] = Ts[e % NB][e / NB];
}

__global__ void k_panel_writeback(double *__restrict__ B, long long ldb, int m, int k0, int jb, const double *__restrict__ V,
                                  long long ldv, const double *__restrict__ rdiag) {
    const int c = blockIdx.y;
    const int i = k0 + c + blockIdx.x * blockDim.x + threadIdx.x;   // rows from the diagonal down
    if (i >= m) return;
    B[i + (long long)(k0 + c) * ldb] = i == k0 + c ? rdiag[k0 + c] : V[(i - k0) + (long long)c * ldv];
}

// =====================================================================================
// Panel factorisation without a launch per column: Cholesky-QR twice, then the Householder representation of
// the orthonormal factor (Ballard, Demmel, Grigori, Jacquelin, Nguyen, Solomonik 2014: the LU factorisation of
// Q - [D; 0] with the signs D_k = -sgn(pivot) chosen on the way IS the set of reflectors the column-by-column
// algorithm produces: V = L, T = -U D L_1^-T, R = D R_chol -- tools/proto_qr/cholqr_hr.py checks it against LAPACK).
// All 64 x 64 work of a panel runs in two single-workgroup kernels; everything that touches the tall panel is a GEMM:
//   G1 = P'P, [R1, X1 = R1^-1] (k_cholqr_pass1), Q1 = P X1, G2 = Q1'Q1, k_cholqr_pass2 (R2, X2; Q_top = Q1_top X2;
//   L U = Q_top - D; T; M = (U R2)^-1; R = D R2 R1), V_bottom = Q1_bottom M.
// A panel whose Gram matrix loses more than ten digits in the Cholesky pivots (flag[2]) is not decided here: the
// caller repeats the factorisation with the column kernel (w->panel_cholqr = false).
//
// The 64 x 64 factorisations are ONE routine: elimination without pivoting, IN PLACE -- the row operations that turn A into
// U are the rows of L^-1, and the column a step eliminates is exactly the slot its column of L^-1 needs: afterwards the upper
// triangle holds U, the strictly lower one L^-1 (unit diagonal implied). 256 threads, a thread owning a 4 x 4 block in
// registers; per PAIR of pivots the two pivot rows and columns go through a double-buffered LDS line (one barrier, every
// thread derives the second pivot row / multipliers itself). Cholesky: R = diag(u)^-1/2 U, R^-1 = (L^-1)' diag(u)^-1/2;
// inverse of a triangular matrix: eliminate its transpose, W' -> (Lambda, F), W^-1 = F' Lambda^-1.
// (Measured: the routine is instruction-bound, one wave per SIMD -- two pivots per barrier instead of one changed nothing,
// halving the arithmetic by the in-place form did.)
constexpr int EB = 64, ES = EB + 2;     // block order; LDS row stride (even: rows 16-byte aligned, 4 consecutive rows on distinct banks)
typedef double EMat[EB][ES];
struct ElimLds { double row[2][2][EB]; double col[2][2][EB]; double dsign[EB]; double g0[EB]; int bad, skip2; };
enum { EL_PLAIN = 0, EL_CHOL = 1, EL_SIGNLU = 2 };
__device__ __forceinline__ double fast_rcp(double p) {      // v_rcp_f64 + two Newton steps (the IEEE division is ~3x the dependent chain)
    double r = __builtin_amdgcn_rcp(p), e = fma(-p, r, 1.0);
    r = fma(r, e, r);
    e = fma(-p, r, 1.0);
    return fma(r, e, r);
}
template <class F> __device__ __forceinline__ void el_init(double (&a)[4][4], F elem) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) a[r][c] = elem(4 * tr + r, 4 * tc + c);
}
__device__ __forceinline__ void el_dump(const double (&a)[4][4], EMat &Mo) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) Mo[4 * tr + r][4 * tc + c] = a[r][c];
}
// the same, split: U (zeros below the diagonal) and L^-1 (unit diagonal, zeros above) as two clean matrices
__device__ __forceinline__ void el_dump2(const double (&a)[4][4], EMat &Uo, EMat &Lo) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int row = 4 * tr + r, col = 4 * tc + c;
            Uo[row][col] = row <= col ? a[r][c] : 0.0;
            Lo[row][col] = row > col ? a[r][c] : (row == col ? 1.0 : 0.0);
        }
}
// MODE EL_CHOL: a pivot p must pass p > tol_rel (|g0| + max(g0 - p, 0)) + tol_abs, the engine's definiteness test (else E.bad); EL_SIGNLU: the pivot is shifted by D_k = -sgn(pivot) first (E.dsign)
// and the multipliers (the strictly lower triangle of L) go to Lm
template <int MODE>
__device__ __forceinline__ void elim64(double (&a)[4][4], ElimLds &E, double tol_rel, EMat *Lm, double tol_abs = 0.0) {
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    auto publish = [&](int kb, int par, int kk) {      // rows / columns k, k + 1 (k = 4 kb + kk; par, kk compile-time at the call sites)
        const bool orow = tr == kb, ocol = tc == kb;
        if (MODE == EL_SIGNLU && orow && ocol) {
            const double d = a[kk][kk] >= 0.0 ? -1.0 : 1.0;      // |pivot| = 1 + |q_kk| >= 1
            a[kk][kk] -= d;
            E.dsign[4 * kb + kk] = d;
        }
        if (orow) {
#pragma unroll
            for (int c = 0; c < 4; c++) { E.row[par][0][4 * tc + c] = a[kk][c]; E.row[par][1][4 * tc + c] = a[kk + 1][c]; }
        }
        if (ocol) {
#pragma unroll
            for (int r = 0; r < 4; r++) { E.col[par][0][4 * tr + r] = a[r][kk]; E.col[par][1][4 * tr + r] = a[r][kk + 1]; }
        }
    };
    publish(0, 0, 0);
    for (int kb = 0; kb < EB / 4; kb++) {
#pragma unroll
        for (int kk = 0; kk < 4; kk += 2) {
            const int k = 4 * kb + kk, par = kk >> 1;
            __syncthreads();
            const double p0 = E.row[par][0][k], x01 = E.row[par][0][k + 1];
            double rp0, rp1, d1 = 0.0;
            if (MODE == EL_CHOL) {
                const double g0k = E.g0[k], ex0 = g0k - p0;
                const bool ok = p0 > tol_rel * (fabs(g0k) + (ex0 > 0.0 ? ex0 : 0.0)) + tol_abs;
                if (!ok && tid == 0) E.bad = 1;
                rp0 = ok ? fast_rcp(p0) : 0.0;
            } else rp0 = fast_rcp(p0);
            const double m = E.col[par][0][k + 1] * rp0;                  // row k + 1 loses its entry in column k
            double p1 = fma(-m, x01, E.row[par][1][k + 1]);
            if (MODE == EL_SIGNLU) { d1 = p1 >= 0.0 ? -1.0 : 1.0; p1 -= d1; }
            if (MODE == EL_CHOL) {
                const double g0k = E.g0[k + 1], ex1 = g0k - p1;
                const bool ok = p1 > tol_rel * (fabs(g0k) + (ex1 > 0.0 ? ex1 : 0.0)) + tol_abs;
                if (!ok && tid == 0) E.bad = 1;
                rp1 = ok ? fast_rcp(p1) : 0.0;
            } else rp1 = fast_rcp(p1);
            double c0[4], c1[4], u0[4], u1[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = 4 * tr + r;
                c0[r] = row > k ? E.col[par][0][row] * rp0 : 0.0;
                c1[r] = row > k + 1 ? fma(-c0[r], x01, E.col[par][1][row]) * rp1 : 0.0;
            }
#pragma unroll
            for (int c = 0; c < 4; c++) {
                u0[c] = E.row[par][0][4 * tc + c];                        // (left of the pivot: the row of L^-1 built so far)
                u1[c] = fma(-m, u0[c], E.row[par][1][4 * tc + c]);
            }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) a[r][c] = fma(-c1[r], u1[c], fma(-c0[r], u0[c], a[r][c]));
            if (tc == kb) {
                // columns k, k + 1 below the pivots: the new columns of L^-1 (the identity's 1 of rows k, k + 1 took part as
                // u0[k] = 1, u1[k] = -m, u1[k + 1] = 1); the multipliers themselves are L
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int row = 4 * tr + r;
                    if (row == k + 1) { a[r][kk] = -m; if (MODE == EL_SIGNLU) (*Lm)[row][k] = m; }
                    if (row > k + 1) {
                        a[r][kk] = fma(c1[r], m, -c0[r]);
                        a[r][kk + 1] = -c1[r];
                        if (MODE == EL_SIGNLU) { (*Lm)[row][k] = c0[r]; (*Lm)[row][k + 1] = c1[r]; }
                    }
                }
                if (MODE == EL_SIGNLU && tr == kb) { a[kk + 1][kk + 1] = p1; E.dsign[k + 1] = d1; }
            }
            if (kk == 0) publish(kb, 1, 2);
            else if (kb + 1 < EB / 4) publish(kb + 1, 0, 0);
        }
    }
    __syncthreads();
}
// acc (the thread's 4 x 4 block of a 64 x 64 product) = sum_k A(i, k) B(k, j), operands through accessors. TRI: both factors
// are upper triangular (or A is and B has nothing below its block's last row): only k in [first row of the block, last
// column of the block] contributes
template <bool TRI, class FA, class FB> __device__ __forceinline__ void mm64(double (&acc)[4][4], FA A, FB B) {
    const int bi = threadIdx.x >> 4, bj = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0.0;
    const int k0 = TRI ? 4 * bi : 0, k1 = TRI ? 4 * bj + 4 : EB;
#pragma unroll 4
    for (int k = k0; k < k1; k++) {
        double ar[4], bc[4];
#pragma unroll
        for (int r = 0; r < 4; r++) ar[r] = A(4 * bi + r, k);
#pragma unroll
        for (int c = 0; c < 4; c++) bc[c] = B(k, 4 * bj + c);
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[r][c] = fma(ar[r], bc[c], acc[r][c]);
    }
}
template <class F> __device__ __forceinline__ void mm64_store(const double (&acc)[4][4], F put) {
    const int bi = threadIdx.x >> 4, bj = threadIdx.x & 15;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) put(4 * bi + r, 4 * bj + c, acc[r][c]);
}
constexpr size_t CHOLQR_LDS1 = sizeof(EMat) + sizeof(ElimLds);
constexpr size_t CHOLQR_LDS2 = 4 * sizeof(EMat) + sizeof(ElimLds);

// G (64 x 64, symmetric, column-major ld 64) = R'R:  R1 and X1 = R1^-1 (upper, ld 64)
__global__ void __launch_bounds__(256) k_cholqr_pass1(const double *__restrict__ G, double *__restrict__ X1, double *__restrict__ R1,
                                                      int *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double cq_lds[];
    EMat &U = *reinterpret_cast<EMat *>(cq_lds);
    ElimLds &E = *reinterpret_cast<ElimLds *>(cq_lds + EB * ES);
    const int tid = threadIdx.x;
    if (tid < EB) E.g0[tid] = G[tid + EB * tid];
    if (tid == 0) E.bad = 0;
    double a[4][4];
    el_init(a, [&](int r, int c) { return G[r + EB * c]; });
    __syncthreads();
    elim64<EL_CHOL>(a, E, 1e-10, nullptr);
    el_dump(a, U);
    __syncthreads();
    if (tid < EB) E.g0[tid] = 1.0 / sqrt(U[tid][tid]);      // 1 / r_kk
    __syncthreads();
    for (int e = tid; e < EB * EB; e += 256) {
        const int i = e & (EB - 1), j = e >> 6;
        R1[e] = i <= j ? U[i][j] * E.g0[i] : 0.0;
        X1[e] = i < j ? U[j][i] * E.g0[j] : (i == j ? E.g0[j] : 0.0);
    }
    if (tid == 0 && E.bad) atomicAdd(flag + 2, 1);
}

// unblocked Cholesky (upper, G = U'U) of one NB x NB diagonal block of the blocked factorisation, by the same elimination:
// the engine's definiteness test against the ORIGINAL diagonal diag0; also returns the inverse of the block's factor
__global__ void __launch_bounds__(256) k_potf2_elim(int nb, double *__restrict__ G, long long ldg, const double *__restrict__ diag0,
                                                    double pd_rel, double pd_abs, double *__restrict__ Uinv, int *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double cq_lds[];
    EMat &U = *reinterpret_cast<EMat *>(cq_lds);
    ElimLds &E = *reinterpret_cast<ElimLds *>(cq_lds + EB * ES);
    const int tid = threadIdx.x;
    if (tid < EB) E.g0[tid] = tid < nb ? diag0[tid] : 1.0;
    if (tid == 0) E.bad = 0;
    double a[4][4];
    el_init(a, [&](int r, int c) {        // (the upper triangle holds the block: mirrored)
        const int i = r < c ? r : c, j = r < c ? c : r;
        return j < nb ? G[i + (long long)j * ldg] : (r == c ? 1.0 : 0.0);
    });
    __syncthreads();
    elim64<EL_CHOL>(a, E, pd_rel, nullptr, pd_abs);
    el_dump(a, U);
    __syncthreads();
    if (tid < EB) E.g0[tid] = 1.0 / sqrt(U[tid][tid]);
    __syncthreads();
    for (int e = tid; e < EB * EB; e += 256) {
        const int i = e & (EB - 1), j = e >> 6;
        if (i < nb && j < nb) G[i + (long long)j * ldg] = i <= j ? U[i][j] * E.g0[i] : 0.0;
        Uinv[e] = i < j ? U[j][i] * E.g0[j] : (i == j ? E.g0[j] : 0.0);
    }
    if (tid == 0 && E.bad) atomicAdd(flag, 1);
}

// second pass + Householder reconstruction of one panel (see the header comment): G2 = Q1'Q1, Q1t = the first 64 rows of Q1
__global__ void __launch_bounds__(256)
k_cholqr_pass2(const double *__restrict__ G2, const double *__restrict__ Q1t, long long ldq, const double *__restrict__ R1,
               const double *__restrict__ norm2, double eps_li, double *__restrict__ Mx, double *__restrict__ Vtop, long long ldv,
               double *__restrict__ Bblk, long long ldb, double *__restrict__ rdiag, double *__restrict__ tau, double *__restrict__ Tout,
               int *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double cq_lds[];
    EMat &b0 = *reinterpret_cast<EMat *>(cq_lds), &b1 = *reinterpret_cast<EMat *>(cq_lds + EB * ES),
         &b2 = *reinterpret_cast<EMat *>(cq_lds + 2 * EB * ES), &b3 = *reinterpret_cast<EMat *>(cq_lds + 3 * EB * ES);
    ElimLds &E = *reinterpret_cast<ElimLds *>(cq_lds + 4 * EB * ES);
    const int tid = threadIdx.x;
    double a[4][4], acc[4][4];
    // 1. G2 = R2'R2. G2 = I + O(eps cond^2): a well-conditioned panel leaves nothing to correct (|G2 - I| <= 3e-14: R2 = I),
    //    and any pivot below 1/100 means the first pass was useless
    if (tid == 0) { E.bad = 0; E.skip2 = 1; }
    __syncthreads();
    {
        bool off = false;
        for (int e = tid; e < EB * EB; e += 256) { const int i = e & (EB - 1), j = e >> 6; off = off || fabs(G2[e] - (i == j ? 1.0 : 0.0)) > 3e-14; }
        if (off) E.skip2 = 0;
    }
    __syncthreads();
    const bool skip2 = E.skip2 != 0;      // (workgroup-uniform)
    if (!skip2) {
        if (tid < EB) E.g0[tid] = G2[tid + EB * tid];
        el_init(a, [&](int r, int c) { return G2[r + EB * c]; });
        __syncthreads();
        elim64<EL_CHOL>(a, E, 1e-2, nullptr);
        el_dump(a, b1);
        __syncthreads();
        if (tid < EB) E.g0[tid] = 1.0 / sqrt(b1[tid][tid]);
        __syncthreads();
        for (int e = tid; e < EB * EB; e += 256) {
            const int i = e & (EB - 1), j = e >> 6;
            b0[i][j] = i <= j ? b1[i][j] * E.g0[i] : 0.0;                                    // R2
            b3[i][j] = i < j ? b1[j][i] * E.g0[j] : (i == j ? E.g0[j] : 0.0);                // X2 = R2^-1
        }
        __syncthreads();
    }
    // 2. Q_top = Q1_top X2
    for (int e = tid; e < EB * EB; e += 256) { const int i = e & (EB - 1), j = e >> 6; (skip2 ? b2 : b1)[i][j] = Q1t[i + j * ldq]; }
    __syncthreads();
    if (!skip2) {
        mm64<false>(acc, [&](int i, int k) { return b1[i][k]; }, [&](int k, int j) { return b3[k][j]; });
        mm64_store(acc, [&](int i, int j, double v) { b2[i][j] = v; });
        __syncthreads();
    }
    // 3. L U = Q_top - D: U into b1, L^-1 into b2, the multipliers L into b3
    el_init(a, [&](int r, int c) { return b2[r][c]; });
    __syncthreads();
    elim64<EL_SIGNLU>(a, E, 0.0, &b3);
    el_dump2(a, b1, b2);
    __syncthreads();
    for (int e = tid; e < EB * EB; e += 256) {
        const int i = e & (EB - 1), j = e >> 6;
        Vtop[i + j * ldv] = i > j ? b3[i][j] : (i == j ? 1.0 : 0.0);
    }
    // T = -U D L^-T
    mm64<true>(acc, [&](int i, int k) { return b1[i][k] * E.dsign[k]; }, [&](int k, int j) { return b2[j][k]; });
    mm64_store(acc, [&](int i, int j, double v) {
        const double t = i <= j ? -v : 0.0;
        Tout[i + j * NB] = t;
        if (i == j) tau[i] = t;
    });
    __syncthreads();             // (b2, b3 are rewritten below)
    // M = (U R2)^-1: W = U R2 into b2, eliminate W'
    if (!skip2) {
        mm64<true>(acc, [&](int i, int k) { return b1[i][k]; }, [&](int k, int j) { return b0[k][j]; });
        mm64_store(acc, [&](int i, int j, double v) { b2[i][j] = i <= j ? v : 0.0; });
        __syncthreads();
    }
    el_init(a, [&](int r, int c) { return (skip2 ? b1 : b2)[c][r]; });
    // R1 into b3 meanwhile
    for (int e = tid; e < EB * EB; e += 256) { const int i = e & (EB - 1), j = e >> 6; b3[i][j] = R1[e]; }
    __syncthreads();
    elim64<EL_PLAIN>(a, E, 0.0, nullptr);
    el_dump(a, b2);               // diagonal: Lambda; strictly lower: F (unit diagonal) with F W' = Lambda
    __syncthreads();
    if (tid < EB) E.g0[tid] = 1.0 / b2[tid][tid];
    __syncthreads();
    for (int e = tid; e < EB * EB; e += 256) {
        const int i = e & (EB - 1), j = e >> 6;
        Mx[e] = i < j ? b2[j][i] * E.g0[j] : (i == j ? E.g0[j] : 0.0);
    }
    // R = D R2 R1
    auto putR = [&](int i, int j, double v) {
        const double r = E.dsign[i] * v;
        if (i < j) Bblk[i + j * ldb] = r;
        else if (i == j) {
            Bblk[i + j * ldb] = r;
            rdiag[i] = r;
            if (!(fabs(r) > eps_li * sqrt(norm2[i]))) atomicAdd(flag, 1);
        }
    };
    if (skip2) {
        for (int e = tid; e < EB * EB; e += 256) { const int i = e & (EB - 1), j = e >> 6; putR(i, j, b3[i][j]); }
    } else {
        mm64<true>(acc, [&](int i, int k) { return b0[i][k]; }, [&](int k, int j) { return b3[k][j]; });
        mm64_store(acc, putR);
    }
    if (tid == 0 && E.bad) atomicAdd(flag + 2, 1);
}

// explicit reflectors of a stored panel (for rsqp_dorgqr)
__global__ void k_build_V(const double *__restrict__ B, long long ldb, int m, int k0, int jb, double *__restrict__ V, long long ldv) {
    const int c = blockIdx.y;
    const int i = k0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    V[(i - k0) + (long long)c * ldv] = i < k0 + c ? 0.0 : (i == k0 + c ? 1.0 : B[i + (long long)(k0 + c) * ldb]);
}

__global__ void k_copy_block(int rows, int cols, const double *__restrict__ src, long long lds, double *__restrict__ dst,
                             long long ldd) {
    const int c = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows && c < cols) dst[r + (long long)c * ldd] = src[r + (long long)c * lds];
}

__global__ void k_set_identity(int m, double *__restrict__ Q, long long ldq) {
    const int j = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) Q[i + (long long)j * ldq] = i == j ? 1.0 : 0.0;
}

// inverse of every NB x NB diagonal block of the upper triangular R into X (zero elsewhere in the block)
__global__ void __launch_bounds__(64) k_trinv_diag(int n, const double *__restrict__ R, long long ldr, double *__restrict__ X, long long ldx) {
    __shared__ double Rs[NB][NB + 1], Xs[NB][NB + 1];
    const int b0 = blockIdx.x * NB, nb = min(NB, n - b0);
    const int t = threadIdx.x;
    for (int e = t; e < NB * NB; e += 64) {
        const int r = e % NB, c = e / NB;
        Rs[r][c] = (r < nb && c < nb && r <= c) ? R[(b0 + r) + (long long)(b0 + c) * ldr] : (r == c ? 1.0 : 0.0);
        Xs[r][c] = 0.0;
    }
    __syncthreads();
    // thread t solves R x = e_t by back substitution (column t of the inverse)
    if (t < nb) {
        for (int r = t; r >= 0; r--) {
            double s = r == t ? 1.0 : 0.0;
            for (int c = r + 1; c <= t; c++) s -= Rs[r][c] * Xs[c][t];
            Xs[r][t] = s / Rs[r][r];
        }
    }
    __syncthreads();
    for (int e = t; e < NB * NB; e += 64) {
        const int r = e % NB, c = e / NB;
        if (r < nb && c < nb) X[(b0 + r) + (long long)(b0 + c) * ldx] = Xs[r][c];
    }
}

__global__ void k_zero_lower(int n, double *__restrict__ X, long long ldx) {
    const int j = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && i > j) X[i + (long long)j * ldx] = 0.0;
}
__global__ void k_zero_block(int m, int n, double *__restrict__ X, long long ldx) {
    const int j = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && j < n) X[i + (long long)j * ldx] = 0.0;
}
__global__ void k_zero_block_batched(int m, int n, double *__restrict__ X, long long ldx, long long stride) {
    const int j = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m && j < n) X[(long long)blockIdx.z * stride + i + (long long)j * ldx] = 0.0;
}

__global__ void k_get_diag(int n, const double *__restrict__ G, long long ldg, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = G[i + (long long)i * ldg];
}

}  // namespace

// every double array of a workspace for mmax rows and how many doubles it holds (rsqp_dense_work_alloc allocates these; the check
// entry points at the end of this file fill them)
constexpr int DW_ARRAYS = 11;
static void dense_work_layout(RsqpDenseWork *w, long long mmax, double **(&p)[DW_ARRAYS], long long (&sz)[DW_ARRAYS]) {
    const long long np = (mmax + NB - 1) / NB;
    int a = 0;
    p[a] = &w->V; sz[a++] = mmax * OB;
    p[a] = &w->T; sz[a++] = np * NB * NB;
    p[a] = &w->W; sz[a++] = mmax * OB;
    p[a] = &w->W2; sz[a++] = mmax * OB;
    p[a] = &w->T2; sz[a++] = 2LL * OB * OB + (long long)OB * NB;      // T2, S2, tmp
    p[a] = &w->Tout; sz[a++] = ((mmax + OB - 1) / OB) * OB * OB;
    p[a] = &w->tau; sz[a++] = 2 * mmax;                                // tau, rdiag
    p[a] = &w->norm2; sz[a++] = mmax;
    p[a] = &w->dblk; sz[a++] = 66LL * NB * NB;                         // S, Uinv + split-K slabs
    p[a] = &w->ws; sz[a++] = 4LL * OB * mmax;                          // = ws_cap
    p[a] = &w->hr; sz[a++] = 3LL * NB * NB;
}

hipError_t rsqp_dense_work_alloc(RsqpDenseWork *w, long long mmax) {
    rsqp_dense_work_free(w);
    if (mmax < 1) mmax = 1;
    hipError_t e;
    double **p[DW_ARRAYS];
    long long sz[DW_ARRAYS];
    dense_work_layout(w, mmax, p, sz);
    for (int a = 0; a < DW_ARRAYS; a++)
        if ((e = hipMalloc((void **)p[a], sizeof(double) * sz[a])) != hipSuccess) return e;
    w->ws_cap = 4LL * OB * mmax;
    if ((e = hipMalloc((void **)&w->flag, sizeof(int) * 4)) != hipSuccess) return e;
    if ((e = hipMemset(w->flag, 0, sizeof(int) * 4)) != hipSuccess) return e;
    w->mmax = mmax;
    return hipSuccess;
}

void rsqp_dense_work_free(RsqpDenseWork *w) {
    double *d[] = {w->V, w->T, w->W, w->W2, w->T2, w->Tout, w->tau, w->norm2, w->dblk, w->ws, w->hr};
    for (double *p : d) if (p) (void)hipFree(p);
    if (w->flag) (void)hipFree(w->flag);
    *w = RsqpDenseWork();
}

#define DCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

hipError_t rsqp_dgeqrf(int m, int n, double *B, long long ldb, double eps_li, RsqpDenseWork *w, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (m < n || m > w->mmax) return hipErrorInvalidValue;
    double *rdiag = w->tau + w->mmax, *S = w->dblk, *ws = w->dblk + NB * NB;
    double *T2 = nullptr, *S2 = w->T2 + (long long)OB * OB, *tmp = S2 + (long long)OB * OB;
    const long long ldv = w->mmax;
    hipLaunchKernelGGL(k_colnorm2, dim3(n), dim3(256), 0, st, m, B, ldb, w->norm2);
    // Two levels. Panels of NB = 64 columns are factorised one column per launch (k_qr_col) and applied, as
    // I - V_p T_p V_p', to the rest of their OUTER block of OB = 256 columns only. The reflectors of an outer block sit
    // side by side in w->V (rows counted from the block's first row); their aggregate I - V T V' (T from the panels'
    // T_p: T_ab = -T_a (V_a'V_b) T_b) updates the trailing matrix ONCE per outer block with inner dimension 256 -- the
    // trailing matrix is streamed 3 x n/256 times instead of 3 x n/64, and those products are no longer HBM-bound.
    for (int K0 = 0, p = 0; K0 < n; K0 += OB) {
        const int ob = std::min(OB, n - K0), mto = m - K0;
        hipLaunchKernelGGL(k_zero_block, dim3((ob + 255) / 256, ob), dim3(256), 0, st, ob, ob, w->V, ldv);   // rows above a panel's first
        for (int k0 = K0; k0 < K0 + ob; k0 += NB, p++) {
            const int jb = std::min(NB, K0 + ob - k0), mt = m - k0, nin = K0 + ob - k0 - jb;
            double *Vp = w->V + (k0 - K0) + (long long)(k0 - K0) * ldv;     // panel p inside the outer block's V
            // (tried in round 3: apply a column's reflector to every remaining column of the OUTER block in the same launch -- up
            //  to 256 workgroups instead of 64 -- and drop the three small-output products below, which run at a few per cent of
            //  anything (64 x 192 results from an inner dimension of 10 000): 149 ms instead of 138 ms for 10 000 x 7 670, the
            //  column launches turn bandwidth-bound at ~15 us)
            double *Tp = w->T + (long long)p * NB * NB;
            if (w->panel_cholqr && jb == NB && mt >= 2 * NB) {
                // the panel in a dozen launches (see k_cholqr_pass2): Q1 lives in w->W (free until the panel is applied)
                double *P = B + k0 + (long long)k0 * ldb, *Q1 = w->W, *X1 = w->hr, *R1 = w->hr + NB * NB, *Mx = w->hr + 2 * NB * NB;
                const long long ldq = w->mmax;
                static std::atomic<unsigned long long> set1{0}, set2{0};
                rsqp_allow_full_lds(reinterpret_cast<const void *>(&k_cholqr_pass1), set1, (int)CHOLQR_LDS1);
                rsqp_allow_full_lds(reinterpret_cast<const void *>(&k_cholqr_pass2), set2, (int)CHOLQR_LDS2);
                DCHK(dgemm_ws(true, false, NB, NB, mt, 1.0, P, ldb, P, ldb, 0.0, S, NB, ws, 64LL * NB * NB, st));           // G1 = P'P
                hipLaunchKernelGGL(k_cholqr_pass1, dim3(1), dim3(256), CHOLQR_LDS1, st, S, X1, R1, w->flag);
                DCHK(rsqp_dgemm(false, false, mt, NB, NB, 1.0, P, ldb, X1, NB, 0.0, Q1, ldq, st));                            // Q1 = P R1^-1
                DCHK(dgemm_ws(true, false, NB, NB, mt, 1.0, Q1, ldq, Q1, ldq, 0.0, S, NB, ws, 64LL * NB * NB, st));         // G2 = Q1'Q1
                hipLaunchKernelGGL(k_cholqr_pass2, dim3(1), dim3(256), CHOLQR_LDS2, st, S, Q1, ldq, R1, w->norm2 + k0, eps_li, Mx, Vp, ldv, P,
                                   ldb, rdiag + k0, w->tau + k0, Tp, w->flag);
                DCHK(rsqp_dgemm(false, false, mt - NB, NB, NB, 1.0, Q1 + NB, ldq, Mx, NB, 0.0, Vp + NB, ldv, st));          // V below the block
            } else {
                for (int j = k0; j < k0 + jb; j++)
                    hipLaunchKernelGGL(k_qr_col, dim3(k0 + jb - j), dim3(QC), 0, st, B, ldb, m, j, k0, Vp, ldv, w->tau, rdiag,
                                       w->norm2, eps_li, w->flag);
                // S = V'V (jb x jb, long inner dimension: split K), T factor
                DCHK(dgemm_ws(true, false, jb, jb, mt, 1.0, Vp, ldv, Vp, ldv, 0.0, S, jb, ws, 64LL * NB * NB, st));
                hipLaunchKernelGGL(k_qr_T_merge, dim3(1), dim3(256), 0, st, jb, S, w->tau + k0, Tp);
            }
            // reflectors back into B
            hipLaunchKernelGGL(k_panel_writeback, dim3((mt + 255) / 256, jb), dim3(256), 0, st, B, ldb, m, k0, jb, Vp, ldv, rdiag);
            if (nin > 0) {      // the rest of the outer block
                double *Ct = B + k0 + (long long)(k0 + jb) * ldb;
                DCHK(dgemm_ws(true, false, jb, nin, mt, 1.0, Vp, ldv, Ct, ldb, 0.0, w->W, NB, w->ws, w->ws_cap, st));   // W = V'C
                DCHK(rsqp_dgemm(true, false, jb, nin, jb, 1.0, w->T + (long long)p * NB * NB, NB, w->W, NB, 0.0, w->W2, NB, st));   // T'W
                DCHK(rsqp_dgemm(false, false, mt, nin, jb, -1.0, Vp, ldv, w->W2, NB, 1.0, Ct, ldb, st));   // C -= V (T'W)
            }
        }
        const int nt = n - K0 - ob;
        // aggregated T of the outer block (kept in w->Tout for rsqp_dorgqr)
        const int p0 = p - (ob + NB - 1) / NB;          // first panel of this outer block
        T2 = w->Tout + (long long)(K0 / OB) * OB * OB;
        const double *Tagg = T2;
        const long long ldt = OB;
        {
            if (ob > NB) DCHK(dgemm_ws(true, false, ob, ob, mto, 1.0, w->V, ldv, w->V, ldv, 0.0, S2, ob, w->ws, w->ws_cap, st));   // S2 = V'V
            hipLaunchKernelGGL(k_zero_block, dim3((ob + 255) / 256, ob), dim3(256), 0, st, ob, ob, T2, (long long)OB);
            int acc = 0;
            for (int q = 0, off = 0; off < ob; q++, off += NB) {
                const int jq = std::min(NB, ob - off);
                const double *Tp = w->T + (long long)(p0 + q) * NB * NB;
                if (acc > 0) {   // T2[0:acc, off:off+jq] = -T2[0:acc,0:acc] (V_acc'V_q) T_q
                    DCHK(rsqp_dgemm(false, false, acc, jq, acc, 1.0, T2, OB, S2 + (long long)off * ob, ob, 0.0, tmp, OB, st));
                    DCHK(rsqp_dgemm(false, false, acc, jq, jq, -1.0, tmp, OB, Tp, NB, 0.0, T2 + (long long)off * OB, OB, st));
                }
                hipLaunchKernelGGL(k_copy_block, dim3(1, jq), dim3(64), 0, st, jq, jq, Tp, (long long)NB, T2 + off + (long long)off * OB, (long long)OB);
                acc += jq;
            }
        }
        if (nt <= 0) continue;
        double *Ct = B + K0 + (long long)(K0 + ob) * ldb;
        DCHK(dgemm_ws(true, false, ob, nt, mto, 1.0, w->V, ldv, Ct, ldb, 0.0, w->W, OB, w->ws, w->ws_cap, st));   // W = V'C
        DCHK(rsqp_dgemm(true, false, ob, nt, ob, 1.0, Tagg, ldt, w->W, OB, 0.0, w->W2, OB, st));                  // T'W
        DCHK(rsqp_dgemm(false, false, mto, nt, ob, -1.0, w->V, ldv, w->W2, OB, 1.0, Ct, ldb, st));               // C -= V (T'W)
    }
    return hipGetLastError();
}

hipError_t rsqp_dorgqr(int m, int n, const double *B, long long ldb, double *Q, long long ldq, RsqpDenseWork *w,
                       hipStream_t st) {
    if (m <= 0) return hipSuccess;
    if (m > w->mmax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_set_identity, dim3((m + 255) / 256, m), dim3(256), 0, st, m, Q, ldq);
    // backwards over the OUTER blocks of rsqp_dgeqrf with their aggregated factors (inner dimension 256 instead of 64:
    // Q is streamed 3 x n/256 times)
    const int nout = (n + OB - 1) / OB;
    for (int o = nout - 1; o >= 0; o--) {
        const int K0 = o * OB, ob = std::min(OB, n - K0), mto = m - K0;
        hipLaunchKernelGGL(k_build_V, dim3((mto + 255) / 256, ob), dim3(256), 0, st, B, ldb, m, K0, ob, w->V, w->mmax);
        double *Qs = Q + K0 + (long long)K0 * ldq;
        const double *To = w->Tout + (long long)o * OB * OB;
        DCHK(dgemm_ws(true, false, ob, mto, mto, 1.0, w->V, w->mmax, Qs, ldq, 0.0, w->W, OB, w->ws, w->ws_cap, st));   // W = V'Q
        DCHK(rsqp_dgemm(false, false, ob, mto, ob, 1.0, To, OB, w->W, OB, 0.0, w->W2, OB, st));                       // T W
        DCHK(rsqp_dgemm(false, false, mto, mto, ob, -1.0, w->V, w->mmax, w->W2, OB, 1.0, Qs, ldq, st));               // Q -= V (T W)
    }
    return hipGetLastError();
}

// recursive doubling: after level s every aligned diagonal block of size 2s of X is the inverse
// of the same block of R:  X12 = -X11 R12 X22
hipError_t rsqp_dtrtri_upper(int n, const double *R, long long ldr, double *X, long long ldx, RsqpDenseWork *w,
                             hipStream_t st) {
    (void)w;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_zero_block, dim3((n + 255) / 256, n), dim3(256), 0, st, n, n, X, ldx);
    hipLaunchKernelGGL(k_trinv_diag, dim3((n + NB - 1) / NB), dim3(64), 0, st, n, R, ldr, X, ldx);
    if (n <= NB) return hipGetLastError();
    // scratch for R12 X22: the strictly lower triangle of X is free; blocks of it are zeroed again afterwards.
    // All pairs of a level that have the full shape s x s run as ONE batched launch per product (round 5: at n = 7 656 the levels
    // s = 64 .. 512 were 336 launches of 12 us, 3.2 of the 8.3 ms of this routine); a ragged last pair runs on its own.
    for (int s = NB; s < n; s *= 2) {
        int nfull = 0;
        for (int a0 = 0; a0 + 2 * s <= n; a0 += 2 * s) nfull++;
        if (nfull > 0) {
            const long long stX = 2LL * s * (ldx + 1), stR = 2LL * s * (ldr + 1);
            double *tmp = X + s;                                            // pair z: X + (a0 + s) + a0 ldx, a0 = 2 s z
            DCHK(dgemm_ws(true, true, s, s, s, 1.0, X + s + (long long)s * ldx, ldx, R + (long long)s * ldr, ldr, 0.0, tmp, ldx, nullptr, 0, st, 0, 3,
                          nfull, stX, stR, stX));
            DCHK(dgemm_ws(false, true, s, s, s, -1.0, X, ldx, tmp, ldx, 0.0, X + (long long)s * ldx, ldx, nullptr, 0, st, 0, 2, nfull, stX, stX, stX));
            hipLaunchKernelGGL(k_zero_block_batched, dim3((s + 255) / 256, s, nfull), dim3(256), 0, st, s, s, tmp, ldx, stX);
        }
        const int a0 = 2 * s * nfull;
        if (a0 + s < n) {                                                  // the ragged pair behind them
            const int a1 = a0 + s, a2 = n, s2 = a2 - a1;
            double *tmp = X + a1 + (long long)a0 * ldx;     // s2 x s block (lower triangle), holds (R12 X22)'
            // (R12 X22)' = X22' R12'  ->  tmp (s2 x s) = X22' (s2 x s2) * R12' (s2 x s)
            DCHK(rsqp_dgemm_tri(true, true, s2, s, s2, 1.0, X + a1 + (long long)a1 * ldx, ldx, R + a0 + (long long)a1 * ldr, ldr, 0.0,
                                tmp, ldx, 3, st));      // (X22 upper triangular: row i of X22' ends at column i)
            // X12 (s x s2) = -X11 (s x s) * tmp' (s x s2)
            DCHK(rsqp_dgemm_tri(false, true, s, s2, s, -1.0, X + a0 + (long long)a0 * ldx, ldx, tmp, ldx, 0.0,
                                X + a0 + (long long)a1 * ldx, ldx, 2, st));      // (X11 upper triangular: row i starts at column i)
            hipLaunchKernelGGL(k_zero_block, dim3((s2 + 255) / 256, s), dim3(256), 0, st, s2, s, tmp, ldx);
        }
    }
    return hipGetLastError();
}

hipError_t rsqp_dpotrf_upper(int n, double *G, long long ldg, double pd_rel, double pd_abs, RsqpDenseWork *w, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > w->mmax) return hipErrorInvalidValue;
    double *Uinv = w->dblk;
    hipLaunchKernelGGL(k_get_diag, dim3((n + 255) / 256), dim3(256), 0, st, n, G, ldg, w->norm2);
    // Two levels (round 5). The trailing matrix is updated once per OUTER block of COB = 256 columns, with an inner dimension of
    // 256: the first version updated it behind every 64-column panel -- 120 passes over the trailing triangle at n = 7 656, each
    // with an inner dimension of 64 (8 flop per byte: HBM-bound, 2.3 TB/s measured), 12 of the 22 ms of this routine
    // (profiles/r05_j_kernel_stats_setup_full.csv). Inside an outer block the panels are right-looking on the block ROW only
    // (COB x remaining columns: a few MB).
    constexpr int COB = 256;
    for (int K0 = 0; K0 < n; K0 += COB) {
        const int ob = std::min(COB, n - K0), K1 = K0 + ob;
        for (int k0 = K0; k0 < K1; k0 += NB) {
            const int jb = std::min(NB, K1 - k0), nt = n - k0 - jb, mrest = K1 - k0 - jb;
            double *Gd = G + k0 + (long long)k0 * ldg;
            hipLaunchKernelGGL(k_potf2_elim, dim3(1), dim3(256), CHOLQR_LDS1, st, jb, Gd, ldg, w->norm2 + k0, pd_rel, pd_abs, Uinv, w->flag + 1);
            if (nt > 0) {
                double *G12 = G + k0 + (long long)(k0 + jb) * ldg;
                // U12 = Ujj^-T G12  (jb x nt): via W, then copied back
                DCHK(rsqp_dgemm(true, false, jb, nt, jb, 1.0, Uinv, NB, G12, ldg, 0.0, w->W, NB, st));
                DCHK(hipMemcpy2DAsync(G12, sizeof(double) * ldg, w->W, sizeof(double) * NB, sizeof(double) * jb, nt, hipMemcpyDeviceToDevice, st));
                // the rest of this outer block's rows: G[k0+jb .. K1, k0+jb .. n) -= U12[:, 0 .. mrest)' U12   (what lands below the
                // diagonal of the block is scratch, zeroed at the end)
                if (mrest > 0) DCHK(rsqp_dgemm(true, false, mrest, nt, jb, -1.0, w->W, NB, w->W, NB, 1.0, G + (k0 + jb) + (long long)(k0 + jb) * ldg, ldg, st));
            }
        }
        // trailing matrix (upper tiles): G22 -= U12' U12 with the whole block row, inner dimension ob
        const int nt2 = n - K1;
        if (nt2 > 0) {
            const double *U12 = G + K0 + (long long)K1 * ldg;
            DCHK(rsqp_dgemm_upper(true, false, nt2, ob, -1.0, U12, ldg, U12, ldg, 1.0, G + K1 + (long long)K1 * ldg, ldg, st));
        }
    }
    hipLaunchKernelGGL(k_zero_lower, dim3((n + 255) / 256, n), dim3(256), 0, st, n, G, ldg);
    return hipGetLastError();
}

// =====================================================================================
// host-pointer entry points (include/rsqp_hip.h): verification and benchmarking
// =====================================================================================
namespace {
struct DevMem {
    double *p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, sizeof(double) * std::max<size_t>(n, 1)); }
    ~DevMem() { if (p) (void)hipFree(p); }
};
struct Stopwatch {
    hipEvent_t a = nullptr, b = nullptr;
    Stopwatch() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    ~Stopwatch() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
    void start() { (void)hipEventRecord(a, nullptr); }
    float stop() { (void)hipEventRecord(b, nullptr); (void)hipEventSynchronize(b); float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return ms; }
};
}  // namespace

#define HCHK(call) do { if ((call) != hipSuccess) return -2; } while (0)

extern "C" int rsqp_dense_gemm(int transA, int transB, int m, int n, int k, double alpha, const double *A, int lda,
                               const double *B, int ldb, double beta, double *C, int ldc, int repeats, float *ms) {
    if (m < 0 || n < 0 || k < 0 || !A || !B || !C) return -1;
    const size_t na = (size_t)lda * (transA ? m : k), nb = (size_t)ldb * (transB ? k : n), nc = (size_t)ldc * n;
    DevMem dA, dB, dC;
    HCHK(dA.alloc(na)); HCHK(dB.alloc(nb)); HCHK(dC.alloc(nc));
    HCHK(hipMemcpy(dA.p, A, sizeof(double) * na, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(dB.p, B, sizeof(double) * nb, hipMemcpyHostToDevice));
    HCHK(hipMemcpy(dC.p, C, sizeof(double) * nc, hipMemcpyHostToDevice));
    HCHK(rsqp_dgemm(transA != 0, transB != 0, m, n, k, alpha, dA.p, lda, dB.p, ldb, beta, dC.p, ldc, nullptr));
    HCHK(hipDeviceSynchronize());
    HCHK(hipMemcpy(C, dC.p, sizeof(double) * nc, hipMemcpyDeviceToHost));
    if (ms && repeats > 0) {
        Stopwatch sw;
        sw.start();
        for (int r = 0; r < repeats; r++) HCHK(rsqp_dgemm(transA != 0, transB != 0, m, n, k, alpha, dA.p, lda, dB.p, ldb, beta, dC.p, ldc, nullptr));
        *ms = sw.stop() / repeats;
    }
    return 0;
}

extern "C" int rsqp_dense_qr(int m, int n, double *B, double *Q, double *Rinv, double eps_li, int *ndep, float *ms) {
    if (m < n || n < 0 || !B) return -1;
    DevMem dB, dQ, dX;
    RsqpDenseWork w;
    HCHK(dB.alloc((size_t)m * n)); HCHK(dQ.alloc((size_t)m * m)); HCHK(dX.alloc((size_t)n * n));
    HCHK(rsqp_dense_work_alloc(&w, m));
    HCHK(hipMemcpy(dB.p, B, sizeof(double) * (size_t)m * n, hipMemcpyHostToDevice));
    Stopwatch sw;
    sw.start();
    hipError_t e = rsqp_dgeqrf(m, n, dB.p, m, eps_li, &w, nullptr);
    {   // an ill-conditioned panel (flag[2]): once more with the column kernel, as the engine does
        int f2 = 0;
        if (e == hipSuccess) e = hipMemcpy(&f2, w.flag + 2, sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess && f2 != 0) {
            w.panel_cholqr = false;
            e = hipMemset(w.flag, 0, sizeof(int) * 4);
            if (e == hipSuccess) e = hipMemcpy(dB.p, B, sizeof(double) * (size_t)m * n, hipMemcpyHostToDevice);
            if (e == hipSuccess) e = rsqp_dgeqrf(m, n, dB.p, m, eps_li, &w, nullptr);
        }
    }
    if (e == hipSuccess) e = rsqp_dtrtri_upper(n, dB.p, m, dX.p, n, &w, nullptr);
    if (e == hipSuccess) e = rsqp_dorgqr(m, n, dB.p, m, dQ.p, m, &w, nullptr);
    const float t = sw.stop();
    if (ms) *ms = t;
    int flags[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(flags, w.flag, sizeof(flags), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(B, dB.p, sizeof(double) * (size_t)m * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && Q) e = hipMemcpy(Q, dQ.p, sizeof(double) * (size_t)m * m, hipMemcpyDeviceToHost);
    if (e == hipSuccess && Rinv) e = hipMemcpy(Rinv, dX.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost);
    rsqp_dense_work_free(&w);
    if (ndep) *ndep = flags[0];
    return e == hipSuccess ? 0 : -2;
}

extern "C" int rsqp_dense_chol_inverse(int n, double *G, double *Ginv, double pd_rel, double pd_abs, int *not_pd, float *ms) {
    if (n < 0 || !G) return -1;
    DevMem dG, dX, dI;
    RsqpDenseWork w;
    HCHK(dG.alloc((size_t)n * n)); HCHK(dX.alloc((size_t)n * n)); HCHK(dI.alloc((size_t)n * n));
    HCHK(rsqp_dense_work_alloc(&w, n));
    HCHK(hipMemcpy(dG.p, G, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice));
    Stopwatch sw;
    sw.start();
    hipError_t e = rsqp_dpotrf_upper(n, dG.p, n, pd_rel, pd_abs, &w, nullptr);
    if (e == hipSuccess) e = rsqp_dtrtri_upper(n, dG.p, n, dX.p, n, &w, nullptr);
    if (e == hipSuccess) e = rsqp_dtrmmt_upper(n, 1.0, dX.p, n, dI.p, n, nullptr);      // U^-1 U^-T: upper tiles, as the engine forms it
    if (e == hipSuccess) e = rsqp_mirror_upper(n, dI.p, n, nullptr);
    const float t = sw.stop();
    if (ms) *ms = t;
    int flags[4] = {0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpy(flags, w.flag, sizeof(flags), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(G, dG.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && Ginv) e = hipMemcpy(Ginv, dI.p, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost);
    rsqp_dense_work_free(&w);
    if (not_pd) *not_pd = flags[1];
    return e == hipSuccess ? 0 : -2;
}

// =====================================================================================
// check entry points (include/rsqp_hip_dense_check.h): the kernels called the way the engine calls them -- operands at an
// offset inside larger buffers, leading dimensions that differ between them, one workspace over several factorisations
// =====================================================================================
#include "../../include/rsqp_hip_dense_check.h"

extern "C" int rsqp_dense_describe_gemm(int m, int n, int k, int batch, int have_ws, long long ws_cap, int *out, int n_out) {
    if (m < 1 || n < 1 || k < 0 || batch < 1 || ws_cap < 0 || !out || n_out != RSQP_DENSE_PLAN_WORDS) return -1;
    const DgemmPlan pl = dgemm_plan(m, n, k, batch, have_ws != 0, have_ws ? ws_cap : 0);
    out[0] = pl.TM; out[1] = pl.TN; out[2] = pl.splits; out[3] = pl.kc; out[4] = pl.skinny;
    return 0;
}

struct rsqp_dense_check_work { RsqpDenseWork w; };

namespace {
// a rows x cols operand at `off` with leading dimension ld inside a buffer of len doubles: every element it addresses lies inside
bool window_ok(const double *buf, long long len, long long off, long long ld, long long rows, long long cols) {
    if (!buf || len < 1 || off < 0 || off > len || rows < 0 || cols < 0 || ld < std::max(1LL, rows)) return false;
    if (rows == 0 || cols == 0) return true;
    return (cols - 1) <= (len - off - rows) / ld && off + (cols - 1) * ld + rows <= len;
}
hipError_t fill_device(double *d, long long n, double v) {
    std::vector<double> h((size_t)n, v);
    return hipMemcpy(d, h.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
}
// every array of the workspace (not flag) := v
hipError_t dense_work_fill(RsqpDenseWork *w, double v) {
    double **p[DW_ARRAYS];
    long long sz[DW_ARRAYS];
    dense_work_layout(w, w->mmax, p, sz);
    for (int a = 0; a < DW_ARRAYS; a++) DCHK(fill_device(*p[a], sz[a], v));
    return hipSuccess;
}
struct HostBuf {      // a whole host buffer on the device: uploaded whole, downloaded whole
    double *host; long long len; DevMem d;
    hipError_t up() { hipError_t e = d.alloc((size_t)len); return e != hipSuccess ? e : hipMemcpy(d.p, host, sizeof(double) * (size_t)len, hipMemcpyHostToDevice); }
    hipError_t down() { return hipMemcpy(host, d.p, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost); }
};
}  // namespace

extern "C" int rsqp_dense_check_work_create(long long mmax, rsqp_dense_check_work **out) {
    if (!out || mmax < 1 || mmax > (1LL << 20)) return -1;
    rsqp_dense_check_work *h = new rsqp_dense_check_work();
    if (rsqp_dense_work_alloc(&h->w, mmax) != hipSuccess || dense_work_fill(&h->w, 0.0) != hipSuccess) {
        rsqp_dense_work_free(&h->w);
        delete h;
        return -2;
    }
    *out = h;
    return 0;
}

extern "C" int rsqp_dense_check_work_destroy(rsqp_dense_check_work *h) {
    if (!h) return -1;
    rsqp_dense_work_free(&h->w);
    delete h;
    return 0;
}

extern "C" int rsqp_dense_check_gemm(int variant, int transA, int transB, int m, int n, int k, double alpha, double beta, double *A,
                                     long long lenA, long long offA, long long lda, double *B, long long lenB, long long offB,
                                     long long ldb, double *C, long long lenC, long long offC, long long ldc, long long ws_cap) {
    if (variant < RSQP_DENSE_GEMM_PLAIN || variant > RSQP_DENSE_GEMM_KTRI3 || m < 0 || n < 0 || k < 0 || ws_cap < 0) return -1;
    if (ws_cap > 0 && (variant != RSQP_DENSE_GEMM_PLAIN || ws_cap > (1LL << 28))) return -1;      // split-K belongs to the plain product
    if (variant == RSQP_DENSE_GEMM_UPPER && m != n) return -1;
    if (variant == RSQP_DENSE_GEMM_KTRI1 && (m != n || k != n || transA || !transB)) return -1;      // C = alpha A A'
    if (variant == RSQP_DENSE_GEMM_KTRI2 && transA) return -1;
    if (variant == RSQP_DENSE_GEMM_KTRI3 && !transA) return -1;
    if (!window_ok(A, lenA, offA, lda, transA ? k : m, transA ? m : k)) return -1;
    if (variant != RSQP_DENSE_GEMM_KTRI1 && !window_ok(B, lenB, offB, ldb, transB ? n : k, transB ? k : n)) return -1;
    if (!window_ok(C, lenC, offC, ldc, m, n)) return -1;
    const bool haveB = variant != RSQP_DENSE_GEMM_KTRI1;
    HostBuf a{A, lenA}, b{B, lenB}, c{C, lenC};
    DevMem ws;
    HCHK(a.up()); if (haveB) HCHK(b.up()); HCHK(c.up());
    if (ws_cap > 0) { HCHK(ws.alloc((size_t)ws_cap)); HCHK(fill_device(ws.p, ws_cap, std::numeric_limits<double>::quiet_NaN())); }
    const double *dA = a.d.p + offA, *dB = haveB ? b.d.p + offB : nullptr;
    double *dC = c.d.p + offC;
    const bool ta = transA != 0, tb = transB != 0;
    hipError_t e = hipSuccess;
    switch (variant) {
    case RSQP_DENSE_GEMM_PLAIN:
        e = ws_cap > 0 ? dgemm_ws(ta, tb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, ws.p, ws_cap, nullptr)
                       : rsqp_dgemm(ta, tb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, nullptr);
        break;
    case RSQP_DENSE_GEMM_UPPER: e = rsqp_dgemm_upper(ta, tb, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, nullptr); break;
    case RSQP_DENSE_GEMM_KTRI1: e = rsqp_dtrmmt_upper(n, alpha, dA, lda, dC, ldc, nullptr); break;
    case RSQP_DENSE_GEMM_KTRI2: e = rsqp_dgemm_tri(ta, tb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, 2, nullptr); break;
    default: e = rsqp_dgemm_tri(ta, tb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, 3, nullptr); break;
    }
    HCHK(e);
    HCHK(hipDeviceSynchronize());
    HCHK(a.down()); if (haveB) HCHK(b.down()); HCHK(c.down());
    return 0;
}

extern "C" int rsqp_dense_check_qr(rsqp_dense_check_work *h, int m, int n, int panel_cholqr, int poison, double eps_li, double *B,
                                   long long lenB, long long offB, long long ldb, double *Q, long long lenQ, long long offQ,
                                   long long ldq, double *X, long long lenX, long long offX, long long ldx, int *flags, int *retried) {
    if (!h || !flags || !retried || n < 1 || m < n || m > h->w.mmax) return -1;
    if (!window_ok(B, lenB, offB, ldb, m, n) || !window_ok(Q, lenQ, offQ, ldq, m, m) || !window_ok(X, lenX, offX, ldx, n, n)) return -1;
    RsqpDenseWork &w = h->w;
    HostBuf b{B, lenB}, q{Q, lenQ}, x{X, lenX};
    HCHK(b.up()); HCHK(q.up()); HCHK(x.up());
    if (poison) HCHK(dense_work_fill(&w, std::numeric_limits<double>::quiet_NaN()));
    *retried = 0;
    w.panel_cholqr = panel_cholqr != 0;
    hipError_t e = hipSuccess;
    for (int attempt = 0; attempt < 2 && e == hipSuccess; attempt++) {      // (setup_tq_blocked of qp_large.hip)
        e = hipMemset(w.flag, 0, sizeof(int) * 4);
        if (e == hipSuccess && attempt) e = b.up();
        if (e == hipSuccess) e = rsqp_dgeqrf(m, n, b.d.p + offB, ldb, eps_li, &w, nullptr);
        if (e == hipSuccess) e = hipMemcpy(flags, w.flag, sizeof(int) * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess || flags[2] == 0 || !w.panel_cholqr) break;
        w.panel_cholqr = false;
        *retried = 1;
    }
    w.panel_cholqr = true;
    if (e == hipSuccess) e = rsqp_dtrtri_upper(n, b.d.p + offB, ldb, x.d.p + offX, ldx, &w, nullptr);
    if (e == hipSuccess) e = rsqp_dorgqr(m, n, b.d.p + offB, ldb, q.d.p + offQ, ldq, &w, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    HCHK(e);
    HCHK(b.down()); HCHK(q.down()); HCHK(x.down());
    return 0;
}

extern "C" int rsqp_dense_check_chol(rsqp_dense_check_work *h, int n, int form, int poison, double pd_rel, double pd_abs, double *G,
                                     long long lenG, long long offG, long long ldg, double *X, long long lenX, long long offX,
                                     long long ldx, double *Gi, long long lenI, long long offI, long long ldi, int *flags) {
    if (!h || !flags || n < 1 || n > h->w.mmax || form < RSQP_DENSE_INV_UPPER || form > RSQP_DENSE_INV_TRI2) return -1;
    if (!window_ok(G, lenG, offG, ldg, n, n) || !window_ok(X, lenX, offX, ldx, n, n) || !window_ok(Gi, lenI, offI, ldi, n, n)) return -1;
    RsqpDenseWork &w = h->w;
    HostBuf g{G, lenG}, x{X, lenX}, gi{Gi, lenI};
    HCHK(g.up()); HCHK(x.up()); HCHK(gi.up());
    if (poison) HCHK(dense_work_fill(&w, std::numeric_limits<double>::quiet_NaN()));
    HCHK(hipMemset(w.flag, 0, sizeof(int) * 4));
    HCHK(rsqp_dpotrf_upper(n, g.d.p + offG, ldg, pd_rel, pd_abs, &w, nullptr));
    HCHK(hipMemcpy(flags, w.flag, sizeof(int) * 4, hipMemcpyDeviceToHost));
    if (flags[1] == 0) {      // (not positive definite: the engine stops here as well)
        double *dX = x.d.p + offX, *dI = gi.d.p + offI;
        HCHK(rsqp_dtrtri_upper(n, g.d.p + offG, ldg, dX, ldx, &w, nullptr));
        if (form == RSQP_DENSE_INV_TRI2) HCHK(rsqp_dgemm_tri(false, true, n, n, n, 1.0, dX, ldx, dX, ldx, 0.0, dI, ldi, 2, nullptr));
        else HCHK(rsqp_dtrmmt_upper(n, 1.0, dX, ldx, dI, ldi, nullptr));
        if (form == RSQP_DENSE_INV_MIRROR) HCHK(rsqp_mirror_upper(n, dI, ldi, nullptr));
    }
    HCHK(hipDeviceSynchronize());
    HCHK(g.down()); HCHK(x.down()); HCHK(gi.down());
    return 0;
}
