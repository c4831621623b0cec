/* rsqp_hip_band_check.h -- the banded H^-1 operator of the HBM-resident engine's general range-space path (DESIGN 4.5:
 * k_band_apply<C>, k_band_apply_mw<C>) called the way the engine calls it, for verification: an extension of the C ABI of
 * rsqp_hip.h, which includes this header (so `#include "rsqp_hip.h"` declares everything); exported by the same library. The Python
 * binding lists these entry points in capi.BAND_CHECK_SYMBOLS, beside the table of rsqp_hip.h's own.
 *
 * The operator. H is symmetric with half bandwidth <= 2, given by three bands of n doubles each: d0[i] = H[i][i] (any
 * regularisation already added), e1[i] = H[i][i-1] (e1[0] is not read), e2[i] = H[i][i-2] (e2[0], e2[1] are not read). The host
 * factors H = L D L', rescales to M = D^-1/2 L D^1/2 (unit lower, sub-diagonals m1, m2) and sinv = D^-1/2, so that
 * H^-1 = sinv M^-T M^-1 sinv. Thread t of 1024 owns the c = ceil(n / 1024) rows t c .. t c + c - 1 and reads its factor entries
 * from a chunk-interleaved image: m1i[k * 1024 + t] = m1 of row t c + k for k = 0..c, m2i[k * 1024 + t] = m2 of row t c + k for
 * k = 0..c + 1 (the entries k >= c belong to the next chunk as well: they are stored twice), zero for rows >= n and for the rows
 * that have no such neighbour. The kernels are built for C = 4, 8, 10, 12, 16 rows per chunk; c picks the build.
 *
 * Every function here and the engine ask the same three host functions (qp_rs_path.h): the factor and its image, the rule c -> C,
 * and the launch. Vectors and matrices are taken as WHOLE host buffers of `len` doubles, uploaded whole, addressed at `off` inside
 * (column j of a matrix at off + j ld) and downloaded whole again: the caller sees every double around the operand.
 * All return 0, -1 on a bad argument (decided on the host before any device call: a null pointer, ld < n, an operand that does not
 * lie inside its buffer, a Hessian the engine would not build the operator for), -2 on a device error. */
#ifndef RSQP_HIP_BAND_CHECK_H
#define RSQP_HIP_BAND_CHECK_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RSQP_BAND_MAX_N 16384
#define RSQP_BAND_THREADS 1024

/* The host side alone; needs no GPU. *built = 1 when the engine would take the banded operator for these bands: 1 <= n <=
 * RSQP_BAND_MAX_N, every pivot d of the L D L' above 1e-12 |d0[i]|, and no entry of the two homogeneous solutions of the forward
 * recurrence, restarted every 64 rows, above 1e3 in magnitude. *growth = the largest such entry (-1 when a pivot failed first or
 * n is out of range), *c = rows per chunk and *build = the C of the kernels the engine would launch (both 0 when n is out of
 * range). When built, m1i (len1 >= 1024 (c + 1)), m2i (len2 >= 1024 (c + 2)) and sinv (lens >= n) receive the image exactly as
 * it is uploaded; otherwise they keep what they held. n out of range is an answer (built = 0, return 0), not a bad argument. */
int rsqp_band_check_factor(int n, const double *d0, const double *e1, const double *e2, int *built, int *c, int *build,
                           double *growth, double *m1i, long long len1, double *m2i, long long len2, double *sinv, long long lens);

/* The factor of one Hessian with the words the engine keeps beside it: the totals `agg` of the multi-workgroup form (zero-filled),
 * the `err` word (0) and the sequence number of the last multi-workgroup product (0; every such product takes the next one as its
 * tag). -1 as well when the operator is not built for these bands. Creating the handle is host work: the image goes to the device,
 * once, with the first product, so the argument checks of the two calls below answer on a machine without a device too. */
typedef struct rsqp_band_check rsqp_band_check;
int rsqp_band_check_create(int n, const double *d0, const double *e1, const double *e2, rsqp_band_check **out);
int rsqp_band_check_destroy(rsqp_band_check *h);

/* out(:, j) = H^-1 (in(:, j) - sub) for j < ncols (1 <= ncols, ld >= n) through the engine's dispatch. kernel:
 *   RSQP_BAND_KERNEL_ENGINE  what the engine launches: k_band_apply_mw (16 single-wave workgroups) for one column, a grid of
 *                            k_band_apply (one workgroup of 1024 threads per column) for more
 *   RSQP_BAND_KERNEL_1WG     k_band_apply for one column as well (the engine under RSQP_LARGE_BAND_1WG)
 * sub is ONE vector of n doubles at off_sub, subtracted from every column, or NULL (then len_sub, off_sub are not looked at).
 * inplace != 0: `out` of the launch is the device address of `in` (the engine's set-up call on the unit matrix); out, len_out,
 * off_out are not looked at and the result comes back in `in`. Otherwise in and out are two device buffers and both come back.
 * *err = the handle's err word after the call (set when a bounded spin of the multi-workgroup form ran out; it is never cleared),
 * *seq = the handle's sequence number after the call. */
enum { RSQP_BAND_KERNEL_ENGINE = 0, RSQP_BAND_KERNEL_1WG = 1 };
int rsqp_band_check_apply(rsqp_band_check *h, int kernel, int ncols, long long ld, int inplace, double *in, long long len_in,
                          long long off_in, const double *sub, long long len_sub, long long off_sub, double *out,
                          long long len_out, long long off_out, int *err, long long *seq);

/* The step direction's product of ONE vector in one launch: Hdx[i] = (ATdy[i] + (Sb[i] != 0 ? dy[i] : 0)) - (gN[i] - g[i]) for
 * every row, dx[i] = (H^-1 Hdx)[i] on the rows with Sb[i] == 0 only. Sb, ATdy, dy, gN, g: n entries each; Hdx and dx are whole
 * buffers, uploaded before and downloaded after the call. kernel, *err, *seq as above. */
int rsqp_band_check_apply_q(rsqp_band_check *h, int kernel, const int *Sb, const double *ATdy, const double *dy, const double *gN,
                            const double *g, double *Hdx, long long len_h, long long off_h, double *dx, long long len_x,
                            long long off_x, int *err, long long *seq);

#ifdef __cplusplus
}
#endif
#endif
