/* rsqp_hip_lane.h -- which build of the lane-per-problem kernel a batch's last launch took, beyond rsqp_batch_get_lane_hblock: an
 * extension of the C ABI of rsqp_hip.h, which includes this header (so `#include "rsqp_hip.h"` declares everything); exported by the
 * same library. The Python binding lists the entry point in capi.LANE_SYMBOLS, beside the table of rsqp_hip.h's own. */
#ifndef RSQP_HIP_LANE_H
#define RSQP_HIP_LANE_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the shape the lane-per-problem build of the launch rsqp_batch_get_last_kernel reports was compiled for: 8 * 256 + 2 = the full-shape
 * build (a batch of one sparsity pattern, every member 8 x 2, H inside its leading 4 x 4 block: nV and nC are compile-time constants
 * of the kernel), 0 = the shape was a run-time value of that launch (RSQP_LANE_SHAPE=0, read when the batch is created, forces it)
 * or another kernel ran. Both builds give the same bits. The word is not among those of rsqp_describe_small_launch /
 * rsqp_batch_get_last_plan: (keep, uni, hb) keep naming the build family. */
int rsqp_batch_get_lane_shape(const rsqp_batch *b);

#ifdef __cplusplus
}
#endif
#endif
