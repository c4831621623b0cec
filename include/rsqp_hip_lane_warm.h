/* rsqp_hip_lane_warm.h -- hot starts with new matrices and warm re-initialisations of a batch on the lane-per-problem kernel: an
 * extension of the C ABI of rsqp_hip.h, which includes this header (so `#include "rsqp_hip.h"` declares everything); exported by the
 * same library. The Python binding lists these entry points in capi.LANE_WARM_SYMBOLS, beside the table of rsqp_hip.h's own. */
#ifndef RSQP_HIP_LANE_WARM_H
#define RSQP_HIP_LANE_WARM_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The lane-per-problem kernel (kernel 2 of rsqp_batch_get_last_kernel) takes the uniform cold start of the batches it serves: one
 * shape of at most 8 x 2, one sparsity pattern or patterns of their own, RSQP_LANE members or more. on != 0: such a batch, while it
 * keeps its state (rsqp_batch_set_keep_state), also runs on that kernel
 *   - rsqp_batch_solve(b, RSQP_MODE_HOT_MATRICES, n) and rsqp_batch_solve(b, RSQP_MODE_WARM_REINIT, n);
 *   - the first solve of an rsqp_batch_optimize_qp call that follows rsqp_batch_set_matrix_values: every member then starts cold, as
 *     a hot start with new matrices or as a FIXED <-> VARIED flip, never as a hot start on new vectors; members that sit out
 *     (rsqp_batch_set_members) are left untouched.
 * Both call shapes build their tableau from the new matrices and take nothing from the stored state but the previous x, y and
 * working sets, which a batch holds in its result pools. The answers are those of the 8-lane kernel: status, nWSR and working sets
 * equal, x, y and the objective to rounding; rsqp_batch_get_dispatch, nWSR_used and the stored state's layout do not change, and a
 * later hot start on new vectors continues from the state on the 8-lane kernel. rsqp_batch_get_last_plan reports family 2 with the
 * mode of the launch.
 * These calls stay on the 8-lane kernel with the switch on: a hot start on new vectors and an optimize call without
 * rsqp_batch_set_matrix_values before it (marks of rsqp_batch_set_matrix_values_of and rsqp_batch_handler_set_matrices alone
 * included) -- both unless rsqp_batch_set_lane_hot of rsqp_hip_lane_hot.h is on as well --; the rescue solve of an optimize call
 * and rsqp_batch_optimize_lp; a hot start whose result pools
 * rsqp_batch_set_results has written since the last solve; every call while the hand-over is on (rsqp_batch_set_handover), and the
 * call after it. on == 0 (default): every entry point launches what it launched before there was a switch. */
int rsqp_batch_set_lane_warm(rsqp_batch *b, int on);
/* the switch: 1 on, 0 off */
int rsqp_batch_get_lane_warm(const rsqp_batch *b);

#ifdef __cplusplus
}
#endif
#endif
