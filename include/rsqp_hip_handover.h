/* rsqp_hip_handover.h -- the hand-over of a single handle, for the members of a batch: an extension of the C ABI of rsqp_hip.h, which
 * includes this header (so `#include "rsqp_hip.h"` declares everything); exported by the same library. The Python binding lists these
 * entry points in capi.HANDOVER_SYMBOLS, beside the table of rsqp_hip.h's own. */
#ifndef RSQP_HIP_HANDOVER_H
#define RSQP_HIP_HANDOVER_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The hand-over a single handle has inside rsqp_solve, for the members of a batch. The register-resident tableau kernels (kernels 1
 * and 2 of rsqp_batch_get_last_kernel) give up on a member at set-up when a pivot falls into their rounding band -- or, without any
 * rounding, when a free variable's curvature is below 1e-8 of the LARGEST diagonal entry of H -- and leave it unsolved; a handle
 * runs the call again on the LDS-resident Givens / TQ kernel. on != 0: every launch of the batch on kernel 1 or 2 (rsqp_batch_solve,
 * both solves of rsqp_batch_optimize_qp) is followed on the same stream by one masked launch of that kernel, which takes over exactly
 * the members the first launch gave up on: cold where the call shape was a hot start, the warm re-initialisation inputs kept, the
 * iteration budget afresh. status, nWSR (hence nWSR_used, handle_error's decision) and the results of such a member are the second
 * kernel's, as on a handle. Its stored state is left "not initialised": its next hot start runs cold, on the tableau kernel first
 * again. rsqp_batch_get_last_kernel, _get_lane_hblock, _get_last_plan and _get_dispatch report the tableau launch and the call shape
 * the dispatch chose. Launches on kernels 0 and 3 and rsqp_batch_optimize_lp add nothing.
 * on == 0 (default): no such launch; the masked launch costs one kernel boundary behind every tableau launch, needed or not. */
int rsqp_batch_set_handover(rsqp_batch *b, int on);
/* which members the last rsqp_batch_solve / rsqp_batch_optimize_qp / _lp handed over -- handed[q] = 1 (in the first solve or in the
 * rescue solve of an optimize call) or 0, nq entries, may be NULL -- and how many (*count, may be NULL). All zero when the call ran
 * with the switch off. Waits for the batch's stream, as rsqp_batch_get_results does. */
int rsqp_batch_get_handover(rsqp_batch *b, int *handed, int *count);

#ifdef __cplusplus
}
#endif
#endif
