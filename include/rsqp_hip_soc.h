/* rsqp_hip_soc.h -- Algorithm::second_order_correction (src/Algorithm.cpp:1144-1211, called at :91) for every member of a batch, with
 * every decision taken on the device, and the setter of the objective pool. An extension of the C ABI of rsqp_hip.h, which includes
 * this header (so `#include "rsqp_hip.h"` declares everything); exported by the same library. The Python binding lists these entry
 * points in capi.SOC_SYMBOLS, beside the table of rsqp_hip.h's own.
 *
 * In the reference the correction runs BETWEEN ratio_test and update_radius: it reads the unchanged delta_, and update_radius then
 * reads the reductions of the correction's own ratio test. rsqp_batch_handler_ratio_test fuses the two, so a driver with the
 * correction on calls rsqp_batch_handler_soc_begin INSTEAD OF it, evaluates f and c at x_trial for the members with soc[q] == 1, and
 * calls rsqp_batch_handler_soc_end with those values in f_trial / c_trial. A driver that never calls these launches what it launched
 * before. The conventions are those of rsqp_hip_nlp_step.h and rsqp_hip_penalty.h: layouts, on_device, the pinned block of a
 * host-pointer call (one copy each way), the G-lane groups and the fixed tree order of the sums, scalar formulas that give the
 * host's bits without contraction; a member whose word is 0 keeps every byte of every in/out and out array and of the batch's
 * pools; the mask of rsqp_batch_set_members plays no role and is what it was when a call returns; each call returns when its outputs
 * are written, and every launch goes on the batch's stream.
 * RSQP_ERR_ARG before any device call: a null batch, trial or options, a missing required pointer, no
 * rsqp_batch_handler_set_problem, a batch without H, a batch that does not keep its state (rsqp_batch_set_keep_state). */
#ifndef RSQP_HIP_SOC_H
#define RSQP_HIP_SOC_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { RSQP_SOC_TEST = 1, RSQP_SOC_CORRECT = 2 };     /* bits of what[q]; any non-zero word runs the test */

/* composite_pred = 0 (the default) is the reference as found, see rsqp_batch_handler_soc_end */
typedef struct {
    int composite_pred;
} rsqp_soc_options;
/* composite_pred = 0. Host only. RSQP_ERR_ARG for a null pointer */
int rsqp_soc_default_options(rsqp_soc_options *o);

typedef struct {
    /* the fields of rsqp_nlp_trial, same meaning */
    const int *what;                          /* nq: 0 = the member sits out; RSQP_SOC_* bits (soc_end reads `soc` instead)  */
    const double *rho, *f_trial;              /* nq: the penalty parameter; f at the trial point                          */
    const double *c_trial;                    /* constraint layout: c at the trial point (may be NULL without constraints) */
    double *x_k;                              /* in / out, NLP layout                                                      */
    double *c_k;                              /* in / out, constraint layout (may be NULL without constraints)             */
    double *f_k, *infea_k, *delta;            /* in / out, nq: obj_value_, infea_measure_, delta_                          */
    double *actual_reduction, *pred_reduction, *infea_trial;     /* out, nq each, any may be NULL                          */
    int *accept;                              /* out: 1 accepted, 0 rejected                                               */
    int *hu_word, *hm_word;                   /* out: the words of the next rsqp_batch_handler_update / _set_matrices      */
    int *exitflag;                            /* out: RSQP_EXIT_*, or the status of a correction QP that ended unsolved    */
    /* plus: */
    const double *grad;                       /* NLP layout: grad_f at x_k (required when some word has CORRECT)           */
    const double *infea_model;                /* nq, may be NULL: infea_measure_model_ as the penalty call left it         */
    double *x_trial;                          /* out, NLP layout: x_k + (p + s) of the members that go on                  */
    int *soc;                                 /* out (begin) / in (end), nq: 1 = the member awaits its second trial point  */
    double *qp_obj;                           /* out, nq, may be NULL: the reference's qp_obj_ (:1198 / :1204)             */
    int *nwsr_soc;                            /* out, nq, may be NULL: what the member adds to Stats::qp_iter              */
} rsqp_soc_trial;

/* Per member q with t->what[q] != 0, on the result pools of the batch's last solve:
 *   1. ratio_test (:722-801) exactly as rsqp_batch_handler_ratio_test states it.
 *   2. The step is accepted, or the word lacks RSQP_SOC_CORRECT: every in/out and out field gets, bit for bit, what
 *      rsqp_batch_handler_ratio_test writes for the member -- the radius update, both words and the exit flag included --, and
 *      soc[q] = 0, nwsr_soc[q] = 0, qp_obj[q] = the objective pool.
 *   3. The step is rejected and the word has CORRECT (:1172-1185). The member's x (ALL nV ENTRIES) AND OBJECTIVE ARE SAVED in buffers
 *      of the call, as the penalty call saves them. g[i < n] = (H_k p)_i + grad_i, where (H_k p)_i starts from 0 and adds H_ij * p_j
 *      (one multiplication, one addition) over the entries of row i of the leading n x n block in increasing j, THE VALUES
 *      READ IN PLACE from the batch's canonical H pool; the slack part of g is untouched. update_bounds(delta, x_l, x_u, x_k + p, c_l, c_u,
 *      c_trial) by the formulas (and the device functions) of RSQP_HU_BOUNDS, x_k + p one addition per entry, ubA written only with
 *      refresh_ubA. delta, x_k, c_k, f_k, infea_k are NOT changed.
 *   4. ONE rsqp_batch_optimize_qp for exactly the members of 3, with the mask read from device memory; skipped when the decision
 *      kernel reports nobody.
 *   5. Per member that was solved. The solve ends unsolved: exitflag = its status as rsqp_batch_get_results maps it (:1190-1193),
 *      soc[q] = 0, nwsr_soc = the solve's iterations, nothing else is written. Otherwise: s = x[0..n) of the solve, the x pool gets
 *      x[i < n] = p_i + s_i (its slack entries stay the correction's), x_trial = x_k + (p + s), soc[q] = 1, nwsr_soc as above,
 *      qp_obj = obj_soc + (qp_obj_first - rho * infea_model) (:1198; with infea_model == NULL the tree sum of the saved slacks, as
 *      rsqp_batch_handler_get_step forms it); actual_reduction, pred_reduction, infea_trial and accept hold the first test's values
 *      until soc_end; the words, the exit flag and the in/out fields are not written.
 * The decisions are two kernels of 8 lanes per member when nVmax + nCmax <= 16, else one wavefront, one before the solve and one
 * behind it; the first fuses the test, the save, the product, the vector writes, the member's word in the mask of the inner solve
 * and the outputs, and tells the host ONE number, how many members go on, through a host-mapped word. A lane owns the rows
 * lane, lane + G, ... of H_k and finds a row's entry in each column of the sorted canonical pattern, so the product needs neither
 * atomics nor a second buffer. rsqp_batch_get_dispatch reports the inner call.
 * Required: t, o, so, what, rho, f_trial, x_k, f_k, infea_k, delta, x_trial, soc (and c_trial, c_k when the batch has constraints);
 * grad when a word has CORRECT (a host-pointer call checks the words; with device pointers grad is required). */
int rsqp_batch_handler_soc_begin(rsqp_batch *b, const rsqp_soc_trial *t, const rsqp_nlp_step_options *o, const rsqp_soc_options *so,
                                 int on_device);

/* Per member q with t->soc[q] != 0 that the batch's last soc_begin set going (any other member is ignored, with every byte kept;
 * what and grad are not read): the second ratio test (:1200-1201) with f_trial / c_trial at x_trial and p + s read from the x pool.
 *   pred = rho * infea_k - get_obj_QP(), and get_obj_QP() is the objective pool, i.e. THE CORRECTION QP'S OWN OBJECTIVE: that is
 *   what the reference's ratio_test reads (:729, :1219-1221); the composite qp_obj_ of :1198 is never read by a decision there.
 *   so->composite_pred != 0 is the opt-in that uses the qp_obj of :1198 instead, in the manner of refresh_ubA.
 *   accepted: the writes of an accepted ratio test -- x_k += p + s, c_k = c_trial, f_k, infea_k, hu_word = BOUNDS | GRAD (| UBA),
 *     hm_word = JAC | HESS. THE POOLS KEEP p + s, the correction's slacks, y, working sets, status and objective: get_multipliers
 *     reads myQP_, the asymmetry of the penalty call.
 *   rejected (:1202-1208): THE x POOL (ALL nV ENTRIES) AND THE OBJECTIVE ARE PUT BACK TO THE SAVED FIRST SOLVE'S, qp_obj = the first
 *     solve's; hu_word = BOUNDS | GRAD (| UBA) and hm_word = 0: the reference's update_grad(grad_f_) + update_bounds(.., x_k, c_k),
 *     left to the next rsqp_batch_handler_update as words -- nothing reads g or the bounds before it.
 *   then update_radius (:820-849) with THIS test's reductions, whether or not it accepted, and norm_p = max |p_i| of the x pool as it
 *     now stands: delta, exitflag (TRUST_REGION_TOO_SMALL or UNKNOWN), actual_reduction, pred_reduction, infea_trial and accept.
 * One launch. RSQP_ERR_ARG as above, and for a batch on which no rsqp_batch_handler_soc_begin has run.
 * Required: t, o, so, soc, rho, f_trial, x_k, f_k, infea_k, delta (and c_trial, c_k when the batch has constraints). */
int rsqp_batch_handler_soc_end(rsqp_batch *b, const rsqp_soc_trial *t, const rsqp_nlp_step_options *o, const rsqp_soc_options *so,
                               int on_device);

/* the objective pool of the members named in `members` (nq ints, NULL = everybody) := obj (nq doubles, host memory); nothing else is
 * touched. With rsqp_batch_set_results it lets a host-driven driver reproduce the restore of a failure path */
int rsqp_batch_set_objective(rsqp_batch *b, const int *members, const double *obj);

#ifdef __cplusplus
}
#endif
#endif
