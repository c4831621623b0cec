/* rsqp_hip_dense_check.h -- the dense f64 building blocks (rsqp_dense_* of rsqp_hip.h) called the way the HBM-resident engine calls
 * them, for verification: an extension of the C ABI of rsqp_hip.h, which includes this header (so `#include "rsqp_hip.h"` declares
 * everything); exported by the same library. The Python binding lists these entry points in capi.DENSE_CHECK_SYMBOLS, beside the
 * table of rsqp_hip.h's own.
 *
 * rsqp_dense_gemm / _qr / _chol_inverse pass tight leading dimensions, offset 0 and a fresh workspace of exactly the problem's size.
 * The engine passes leading dimensions padded to 16 doubles that differ between operand and result, addresses operands inside
 * buffers it reuses (so what lies around an operand, and in a triangle the routine "does not reference", is stale data), and keeps
 * ONE workspace, sized for its largest problem, over all factorisations. The entries below take every matrix as a WHOLE host buffer
 * of `len` doubles, upload it whole, address the operand at (off, ld) inside it (column-major: element (i, j) at off + i + j ld)
 * and download the whole buffer again: the caller sees every double around the operand.
 * All return 0, -1 on a bad argument (decided on the host before any device call: a null buffer, a negative size, ld < rows, or an
 * operand that does not lie inside its buffer), -2 on a device error. */
#ifndef RSQP_HIP_DENSE_CHECK_H
#define RSQP_HIP_DENSE_CHECK_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The launch plan of the GEMM for an m x n result (m, n >= 1) with inner dimension k >= 0, `batch` >= 1 products in one launch,
 * and a split-K workspace of ws_cap doubles (have_ws != 0) or none: out[0], out[1] = the tile TM, TN of the build of k_dgemm that
 * runs -- (64, 64), (128, 64) or (128, 128) --, out[2] = the slices the inner dimension is split into (1: not split), out[3] = the
 * inner dimension of a slice (k when not split), out[4] = 1 when the forced 128 x 128 case of a few rows against a wide matrix
 * applies. The launcher asks the same function; needs no GPU. n_out must be RSQP_DENSE_PLAN_WORDS. */
#define RSQP_DENSE_PLAN_WORDS 5
int rsqp_dense_describe_gemm(int m, int n, int k, int batch, int have_ws, long long ws_cap, int *out, int n_out);

/* C = alpha op(A) op(B) + beta C through the entry the engine uses for the variant:
 *   RSQP_DENSE_GEMM_PLAIN  rsqp_dgemm; with ws_cap > 0 the launcher is given a split-K workspace of ws_cap doubles, filled with NaN
 *   RSQP_DENSE_GEMM_UPPER  rsqp_dgemm_upper (m == n): tiles strictly below the diagonal are skipped
 *   RSQP_DENSE_GEMM_KTRI1  rsqp_dtrmmt_upper: C = alpha A A' for an upper triangular A (m == n == k, transA == 0, transB != 0;
 *                          B and beta are not used, B may be NULL)
 *   RSQP_DENSE_GEMM_KTRI2  rsqp_dgemm_tri(ktri = 2): op(A) = A upper triangular (transA == 0)
 *   RSQP_DENSE_GEMM_KTRI3  rsqp_dgemm_tri(ktri = 3): op(A) = A', A upper triangular (transA != 0)
 * A, B, C are downloaded again after the call. */
enum { RSQP_DENSE_GEMM_PLAIN = 0, RSQP_DENSE_GEMM_UPPER = 1, RSQP_DENSE_GEMM_KTRI1 = 2, RSQP_DENSE_GEMM_KTRI2 = 3, RSQP_DENSE_GEMM_KTRI3 = 4 };
int rsqp_dense_check_gemm(int variant, int transA, int transB, int m, int n, int k, double alpha, double beta, double *A,
                          long long lenA, long long offA, long long lda, double *B, long long lenB, long long offB, long long ldb,
                          double *C, long long lenC, long long offC, long long ldc, long long ws_cap);

/* A workspace of the factorisations for up to mmax rows (RsqpDenseWork), zero-filled; it lives over as many calls of the two
 * entries below as the caller makes, as the engine's does. */
typedef struct rsqp_dense_check_work rsqp_dense_check_work;
int rsqp_dense_check_work_create(long long mmax, rsqp_dense_check_work **out);
int rsqp_dense_check_work_destroy(rsqp_dense_check_work *w);

/* setup_tq_blocked's sequence on B (m x n, 1 <= n <= m <= mmax): rsqp_dgeqrf -- once more with the column kernel when it sets
 * flag[2] and panel_cholqr != 0; *retried says so --, X (n x n) = R^-1 by rsqp_dtrtri_upper, Q (m x m) by rsqp_dorgqr.
 * poison != 0: every array of the workspace (not its flags) is filled with NaN first. flags[4] = the workspace's flags after the
 * last rsqp_dgeqrf (see rsqp_dense_qr: [0] dependent columns, [2] a panel too ill-conditioned for Cholesky-QR). */
int rsqp_dense_check_qr(rsqp_dense_check_work *w, int m, int n, int panel_cholqr, int poison, double eps_li, double *B,
                        long long lenB, long long offB, long long ldb, double *Q, long long lenQ, long long offQ, long long ldq,
                        double *X, long long lenX, long long offX, long long ldx, int *flags, int *retried);

/* setup_wz_blocked's / dual_setup_blocked's sequence on the upper triangle of G (n x n, 1 <= n <= mmax): rsqp_dpotrf_upper,
 * flags[4] = the workspace's flags ([1] != 0: not positive definite -- nothing more runs, X and Ginv keep what they held), X = U^-1
 * by rsqp_dtrtri_upper, then Ginv = U^-1 U^-T by
 *   RSQP_DENSE_INV_UPPER   rsqp_dtrmmt_upper (upper tiles only)      RSQP_DENSE_INV_MIRROR  the same + rsqp_mirror_upper
 *   RSQP_DENSE_INV_TRI2    rsqp_dgemm_tri(ktri = 2), both triangles. */
enum { RSQP_DENSE_INV_UPPER = 0, RSQP_DENSE_INV_MIRROR = 1, RSQP_DENSE_INV_TRI2 = 2 };
int rsqp_dense_check_chol(rsqp_dense_check_work *w, int n, int form, int poison, double pd_rel, double pd_abs, double *G,
                          long long lenG, long long offG, long long ldg, double *X, long long lenX, long long offX, long long ldx,
                          double *Ginv, long long lenI, long long offI, long long ldi, int *flags);

#ifdef __cplusplus
}
#endif
#endif
