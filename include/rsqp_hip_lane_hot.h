/* rsqp_hip_lane_hot.h -- hot starts on new vectors of a batch on the lane-per-problem kernel: an extension of the C ABI of rsqp_hip.h,
 * which includes this header (so `#include "rsqp_hip.h"` declares everything); exported by the same library. The Python binding
 * lists these entry points in capi.LANE_HOT_SYMBOLS, beside the table of rsqp_hip.h's own. */
#ifndef RSQP_HIP_LANE_HOT_H
#define RSQP_HIP_LANE_HOT_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rsqp_batch_set_lane_warm (rsqp_hip_lane_warm.h) brings a batch's hot starts with new matrices and its warm re-initialisations to
 * the lane-per-problem kernel (kernel 2 of rsqp_batch_get_last_kernel) and leaves one call shape on the 8-lane kernel: the hot start
 * on new vectors, hotstart(g, lb, ub, lbA, ubA). This switch brings that one too. It has an effect only WHILE
 * rsqp_batch_set_lane_warm IS ON AS WELL and under that switch's conditions (a batch the lane-per-problem kernel serves, which keeps
 * its state; no hand-over; result pools that are the batch's own); alone it changes nothing. With both on, such a batch also runs on
 * that kernel
 *   - rsqp_batch_solve(b, RSQP_MODE_HOT_VECTORS, n);
 *   - the first solve of every rsqp_batch_optimize_qp call that goes through the plan kernel, whether its update mark is batch-wide
 *     (rsqp_batch_set_matrix_values), per member (rsqp_batch_set_matrix_values_of, rsqp_batch_handler_set_matrices) or absent: each
 *     member starts as its own word says -- cold, hot on new vectors, hot with new matrices, FIXED <-> VARIED flip --, and members
 *     that sit out (rsqp_batch_set_members) keep every byte.
 * A hot start on new vectors there takes the previous x, y and working sets from the batch's result pools and the limits the
 * previous homotopy ended on from the members' state blocks; it builds its tableau from the matrices instead of reading the stored
 * one. The answers are those of the 8-lane kernel: status, nWSR and working sets equal, x, y and the objective to rounding. A member
 * without a solved or stopped QP behind it starts cold; one whose new bounds are inconsistent reports infeasibility and keeps its
 * stored iterate, working sets and state block. rsqp_batch_get_dispatch, nWSR_used and the layout of the state block do not change:
 * the next hot start continues from it on either kernel. rsqp_batch_get_last_plan reports family 2 with the mode of the launch.
 * These stay where they are with both switches on: the rescue solve of an optimize call and rsqp_batch_optimize_lp; the uniform
 * cold first call; a call whose result pools rsqp_batch_set_results has written; every call while the hand-over is on
 * (rsqp_batch_set_handover), and the call after it; batches that do not keep their state or that the lane-per-problem kernel does
 * not serve. on == 0 (default): every entry point launches what it launched before there was a switch. */
int rsqp_batch_set_lane_hot(rsqp_batch *b, int on);
/* the switch: 1 on, 0 off */
int rsqp_batch_get_lane_hot(const rsqp_batch *b);

#ifdef __cplusplus
}
#endif
#endif
