/* rsqp_hip_nlp_step.h -- the decisions of a lock-step SQP loop for every member of a batch, on the device: the infeasibility measure,
 * the ratio test with the radius update, and the NLP's KKT check (src/Algorithm.cpp). An extension of the C ABI of rsqp_hip.h, which
 * includes this header (so `#include "rsqp_hip.h"` declares everything); exported by the same library. The Python binding lists
 * these entry points in capi.NLP_STEP_SYMBOLS, beside the table of rsqp_hip.h's own.
 *
 * With rsqp_batch_handler_update, rsqp_batch_handler_set_matrices, the optimize calls and rsqp_batch_handler_get_step these close
 * the loop: a caller whose NLP evaluators run on the device moves no per-member data through the host between iteration 0 and
 * convergence. The conventions are the handler layer's: "NLP layout", "constraint layout" and on_device mean what they mean for
 * rsqp_batch_handler_update; a host-pointer call packs its arrays into the pinned block and crosses in one copy each way;
 * rsqp_batch_handler_set_problem must have been called (it holds x_l, x_u, c_l, c_u), else RSQP_ERR_ARG before any device call, as
 * for a null batch or a missing required pointer. A member whose word in `what` is 0 keeps every byte of every in/out array and of
 * every output; the mask of rsqp_batch_set_members plays no role. Each call returns when its outputs are written.
 *
 * Every scalar formula gives the bits the same C expression gives on the host without contraction (the kernels are compiled with
 * floating-point contraction off). Sums over a member's entries are tree sums over G lanes, G = 8 when nVmax + nCmax <= 16 over the
 * batch, else 64: lane l adds the terms of the entries i = l, l + G, ... in index order, starting from 0, and the lanes' partial sums
 * are then added pairwise, partners G/2, G/4, ..., 1 lanes apart. That order is fixed, so a result is reproducible bit for bit; it
 * differs from the index-order sum by rounding. */
#ifndef RSQP_HIP_NLP_STEP_H
#define RSQP_HIP_NLP_STEP_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the options the three calls read (src/Options.cpp:28-42), and refresh_ubA: the RSQP_HU_UBA bit in the word of an accepted step */
typedef struct {
    double active_set_tol;
    double opt_prim_fea_tol, opt_dual_fea_tol, opt_compl_tol, opt_stat_tol;
    double eta_s, eta_c, eta_e;
    double gamma_c, gamma_e;
    double delta_min, delta_max;
    double tol;
    int refresh_ubA;
} rsqp_nlp_step_options;
/* the values of src/Options.cpp:28-42, refresh_ubA = 0. Host only. RSQP_ERR_ARG for a null pointer */
int rsqp_nlp_step_default_options(rsqp_nlp_step_options *o);

/* cal_infea(c, c_l, c_u) of every member (src/Algorithm.cpp:577-602 without the x part: the NEW_FORMULATION=false call at :427): the
 * sum over the member's constraints of c_l - c where c < c_l, else of c - c_u where c > c_u. c: constraint layout (may be NULL when
 * the batch has no constraints); infea: nq entries. Every member is written. A driver needs it once, for infea_measure_ at the
 * starting point; the ratio test applies the same device function to c_trial. */
int rsqp_batch_handler_infeasibility(rsqp_batch *b, const double *c, double *infea, int on_device);

#define RSQP_EXIT_UNKNOWN (-99)               /* include/sqphot/Types.hpp:57: UNKNOWN                  */
#define RSQP_EXIT_TRUST_REGION_TOO_SMALL 4    /*                              TRUST_REGION_TOO_SMALL   */
typedef struct {
    /* in */
    const int *what;                          /* nq: != 0 = the member takes part                                        */
    const double *rho, *f_trial;              /* nq: the penalty parameter; f at x_k + p                                  */
    const double *c_trial;                    /* constraint layout: c at x_k + p (may be NULL without constraints)        */
    /* in / out: the member's iterate */
    double *x_k;                              /* NLP layout                                                              */
    double *c_k;                              /* constraint layout (may be NULL without constraints)                      */
    double *f_k, *infea_k, *delta;            /* nq: obj_value_, infea_measure_, delta_                                  */
    /* out, nq each, any may be NULL */
    double *actual_reduction, *pred_reduction, *infea_trial;
    int *accept;                              /* 1 accepted, 0 rejected                                                  */
    int *hu_word, *hm_word;                   /* the words of the next rsqp_batch_handler_update / _set_matrices         */
    int *exitflag;                            /* RSQP_EXIT_*                                                             */
} rsqp_nlp_trial;
/* ratio_test (src/Algorithm.cpp:722-801) followed by update_radius (:820-849) for every member q with t->what[q] != 0. The two are
 * fused: check_optimality, which the reference runs between them, reads neither delta nor the flags, and a member it declares OPTIMAL
 * leaves the loop. From the result pools of the last solve, as rsqp_batch_handler_get_step and rsqp_batch_get_results report them:
 * p = x[0..n), norm_p = max |p_i|, qp_obj = the objective (get_obj_QP, :1219). Per member:
 *   infea_trial = cal_infea(c_trial)                                   (rsqp_batch_handler_infeasibility)
 *   actual = (f_k + rho*infea_k) - (f_trial + rho*infea_trial);  pred = rho*infea_k - qp_obj
 *   accept iff actual >= eta_s*pred && actual >= -tol                  (the `#if 1` branch, :768-769)
 *   accepted: x_k += p (one addition per entry, :416-417), c_k = c_trial, f_k = f_trial, infea_k = infea_trial
 *   radius:   actual < eta_c*pred: delta *= gamma_c; else actual > eta_e*pred && tol > fabs(delta - norm_p):
 *             delta = min(gamma_e*delta, delta_max)
 *   exitflag = RSQP_EXIT_TRUST_REGION_TOO_SMALL when delta < delta_min afterwards, else RSQP_EXIT_UNKNOWN
 * and the words are the reference's dirty flags in the form the next calls take, with the precedence of Algorithm::setupQP (:672-695):
 *   accepted:                 hu_word = RSQP_HU_BOUNDS | RSQP_HU_GRAD (| RSQP_HU_UBA with refresh_ubA), hm_word = RSQP_HM_JAC | RSQP_HM_HESS
 *                             (update_bounds covers a changed radius: no RSQP_HU_DELTA beside BOUNDS)
 *   rejected, a radius branch taken: hu_word = RSQP_HU_DELTA, hm_word = 0
 *   otherwise:                both 0 -- the reference's "QP is not changed" state (:652-671), which the caller sees as two zero
 *                             words beside a non-zero `what`.
 * The penalty bit stays with the caller, who ORs it in: update_penalty_parameter solves QPs and LPs and is not part of this call but
 * of rsqp_hip_penalty.h's rsqp_batch_handler_update_penalty, which runs before it and returns that bit as its own hu_word.
 * Required: t, o, what, rho, f_trial, x_k, f_k, infea_k, delta (and c_trial, c_k when the batch has constraints). */
int rsqp_batch_handler_ratio_test(rsqp_batch *b, const rsqp_nlp_trial *t, const rsqp_nlp_step_options *o, int on_device);

typedef struct {
    const int *what;                          /* nq: != 0 = the member takes part                                        */
    const double *x_k, *grad;                 /* NLP layout                                                              */
    const double *c_k;                        /* constraint layout (may be NULL without constraints)                      */
    const double *infea;                      /* nq: the member's infea_measure_                                         */
} rsqp_nlp_point;
/* verdict bits */
enum { RSQP_KKT_PRIMAL = 1, RSQP_KKT_DUAL = 2, RSQP_KKT_COMPL = 4, RSQP_KKT_STAT = 8, RSQP_KKT_FIRST_ORDER_OPT = 16 };
/* check_optimality (src/Algorithm.cpp:170-364) for every member q with pt->what[q] != 0. The multipliers are those get_multipliers
 * takes (:619-622), from the result pools of the last solve: lam_x = y[0..n), lam_c = y[nV..nV+m). THE JACOBIAN IS READ IN PLACE: the
 * columns [0, n) of the member's A as they stand in the batch's canonical CSC pool. A driver therefore calls
 * rsqp_batch_handler_set_matrices with the accepted point's J BEFORE this call; setupQP would make the same call one step later, and
 * nothing solves in between. Per member:
 *   every bound pair is classified by classify_single_constraint (src/Utils.cpp:29-45) exactly as written, INF = 1e18 -- its second
 *     branch tests upper > INF, so an upper bound of exactly 1e18 beside a finite lower bound is UNBOUNDED (as is a lower bound of
 *     exactly -1e18 beside a finite upper bound), and only an upper bound above 1e18 (2e19, +inf) gives BOUNDED_BELOW;
 *   primal_violation = infea;
 *   dual_violation: over BOUNDED_ABOVE entries max(lam, 0), over BOUNDED_BELOW entries -min(lam, 0) (:251-269);
 *   compl_violation (:277-306): BOUNDED_ABOVE |lam*(u - v)|, BOUNDED_BELOW |lam*(v - l)|, UNBOUNDED |lam|; EQUAL and BOUNDED
 *     contribute nothing, as in the reference;
 *   stationarity_violation = || J' lam_c + lam_x - grad ||_1 (:329-333): a column's entries in index order, then + lam_x, - grad;
 *   KKT_error = dual + primal + compl + stationarity, in this order (:346-347);
 *   verdict: RSQP_KKT_PRIMAL / _DUAL / _COMPL / _STAT where the violation < its tolerance, RSQP_KKT_FIRST_ORDER_OPT with all four
 *     (:354-362).
 * The sums over variables and constraints are tree sums (above). The W_constr_ / W_bounds_ identification of :189-229 is not built:
 * the verdict never reads it (options->active_set_tol is carried for a caller that builds it). out (nq records) and verdict (nq) may
 * each be NULL. Required: pt, o, what, x_k, grad, infea (and c_k when the batch has constraints). */
int rsqp_batch_handler_check_optimality(rsqp_batch *b, const rsqp_nlp_point *pt, const rsqp_nlp_step_options *o,
                                        rsqp_optimality_status *out, int *verdict, int on_device);

#ifdef __cplusplus
}
#endif
#endif
