/* rsqp_hip_penalty.h -- Algorithm::update_penalty_parameter (src/Algorithm.cpp:886-1028) for every member of a batch, with every
 * decision taken on the device. An extension of the C ABI of rsqp_hip.h, which includes this header (so `#include "rsqp_hip.h"`
 * declares everything); exported by the same library. The Python binding lists these entry points in capi.PENALTY_SYMBOLS, beside
 * the table of rsqp_hip.h's own.
 *
 * The reference keeps two handler objects, myQP_ and myLP_ (:561-562); here a QP batch has an LP batch paired with it
 * (rsqp_batch_handler_pair_lp). The call runs between the QP solve and the ratio test of an SQP iteration (:81): it reads the result
 * pools of the QP batch's last solve, solves the LP of the members whose model is infeasible, re-solves their QP with larger penalty
 * parameters and decides who keeps the new one. Between the launches the host learns ONE number, how many members still take part,
 * from a host-mapped word the decision kernel writes; no per-member data crosses with on_device != 0. The conventions are those of
 * rsqp_hip_nlp_step.h's rsqp_batch_handler_ratio_test: layouts, on_device, the pinned block of a host-pointer call (one copy each
 * way), the fixed tree order of the sums, scalar formulas that give the host's bits without contraction. */
#ifndef RSQP_HIP_PENALTY_H
#define RSQP_HIP_PENALTY_H
#include "rsqp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the options the call reads (src/Options.cpp:43-52). eps1 is not among them: the reference changes it during a run (:984), so it
 * is state of each member (rsqp_penalty_state::eps1; the reference starts it at 0.1) */
typedef struct {
    double penalty_update_tol;
    double increase_parm;
    double rho_max;
    int penalty_iter_max;
    double eps1_change_parm;
    double eps2;
} rsqp_penalty_options;
/* 1e-8, 10, 1e6, 200, 0.1, 1e-6. Host only. RSQP_ERR_ARG for a null pointer */
int rsqp_penalty_default_options(rsqp_penalty_options *o);

/* lp becomes the LP handler of qp (myLP_ beside myQP_); lp == NULL unpairs. Checked on the host before any device call, RSQP_ERR_ARG
 * otherwise: both on the same device, the same number of members, nV[q] and nC[q] of every member equal, the same canonical A
 * pattern member by member, both keep their state (rsqp_batch_set_keep_state), rsqp_batch_handler_set_problem called on both -- with
 * the same bounds, which is the caller's promise. A BATCH WHOSE A WAS CREATED IN A NON-CANONICAL LAYOUT (rows out of order within a
 * column, repeated positions) IS REFUSED: the call copies J slot by slot between the canonical pools. The pair holds until it is
 * replaced or undone; destroy neither batch while it is paired. */
int rsqp_batch_handler_pair_lp(rsqp_batch *qp, rsqp_batch *lp);

typedef struct {
    /* in */
    const int *what;                          /* nq: 0 = the member keeps every byte of everything                        */
    const double *infea_k, *delta;            /* nq: infea_measure_, delta_                                                */
    const double *x_k;                        /* NLP layout                                                               */
    const double *c_k;                        /* constraint layout (may be NULL without constraints): setupLP's set_bounds */
    /* in / out, nq each */
    double *rho, *eps1;                       /* rho_, options_->eps1                                                      */
    int *trial, *succ, *fail;                 /* Stats::penalty_change_trial / _Succ / _Fail, cumulative over a run (:943) */
    /* out, nq each, any may be NULL */
    double *infea_model, *infea_infty;        /* infea_measure_model_ as the call leaves it; the LP's (where its LP solved) */
    int *hu_word;                             /* RSQP_HU_PENALTY or 0: QPinfoFlag_.Update_penalty (:1001)                  */
    int *exitflag;                            /* RSQP_EXIT_UNKNOWN, or the status of the solve that ended unsolved         */
    int *nwsr_qp, *nwsr_lp;                   /* what the member adds to Stats::qp_iter                                    */
    int *rounds;                              /* QP re-solves of this call                                                 */
} rsqp_penalty_state;
/* update_penalty_parameter for every member q with s->what[q] != 0, on qp and the LP batch paired with it. The reads are those of
 * rsqp_batch_handler_get_step: infea_model = the tree sum of |x_i|, i >= n, by the same device function; qp_obj = the objective pool.
 * Per member, with the reference's conditions in the reference's order:
 *   1. the last QP solve is not solved: exitflag = its status as rsqp_batch_get_results maps it, nothing else is written.
 *   2. infea_model <= penalty_update_tol: nothing happens (:893); the outputs say so (rounds = 0, both counts 0, hu_word = 0).
 *   3. setupLP on the LP batch (:700-704): set_bounds + set_g(rho) -- the RSQP_HU_SET word of rsqp_batch_handler_update with
 *      grad == NULL --, and set_A: J IS READ IN PLACE from the columns [0, n) of the member's A in qp's canonical CSC pool, the
 *      matrix the QP was just solved with, and written into the LP batch's CSC pool and its CSR copy by one launch, which raises the
 *      member's update mark as rsqp_batch_handler_set_matrices would.
 *   4. rsqp_batch_optimize_lp for exactly these members. An LP that ends unsolved: exitflag = its status, nothing of the QP side is
 *      touched (:901-904). infea_infty = the same tree sum over the LP's x.
 *   5. infea_infty <= tol: `while (infea_model > tol)` (:914); else `while (infea_k - infea_model < eps1 * (infea_k - infea_infty)
 *      && trial < penalty_iter_max)` (:941-944); in both the first statement is `if (rho_trial >= rho_max) break`. A round:
 *      rho_trial = min(rho_max, rho_trial * increase_parm), trial++, g[n..) = rho_trial (update_penalty), rsqp_batch_optimize_qp for
 *      the members still looping, infea_model anew. A QP that ends unsolved leaves the loop with exitflag = its status (:929-932).
 *   6. rho_trial > rho (:975): rho_trial * infea_k - qp_obj >= eps2 * rho_trial * (infea_k - infea_model) (:979-981) is a success:
 *      rho = rho_trial, eps1 += (1 - eps1) * eps1_change_parm, succ++; the result pools keep the new solve, so the caller's next
 *      rsqp_batch_handler_get_step gives the new p (get_search_direction, :988) and the caller evaluates f_trial / c_trial as before.
 *      Otherwise a failure: fail++, infea_model = the value from before the loop, hu_word = RSQP_HU_PENALTY, rho unchanged -- and
 *      THE MEMBER'S x (ALL nV ENTRIES) AND OBJECTIVE IN THE RESULT POOLS ARE PUT BACK TO THE FIRST SOLVE'S, which the call saved
 *      when the member entered the loop: the reference's p_k_ and qp_obj_ keep those values there. THE ASYMMETRY: y, the working
 *      sets, the status and the stored hot-start state stay those of the LAST solve, as the reference's get_multipliers (:619-622)
 *      reads myQP_, which holds the last solve. The g pool keeps the last rho_trial, which is why the word asks for update_penalty.
 *      One stated deviation: a member that left the loop on an unsolved QP takes the failure path whatever the inequality says (the
 *      reference evaluates :979 with the objective of an unsolved QP there).
 *   7. exitflag = RSQP_EXIT_UNKNOWN wherever nothing above set it.
 * The decisions are kernels with 8 lanes per member when nVmax + nCmax <= 16, else one wavefront (the groups and the tree order of
 * rsqp_hip_nlp_step.h); each fuses the slack sum, the branch and loop tests, the g write, the save or restore of x and the
 * objective, the member's word in the mask of the next launch and the outputs. The inner optimize calls read those masks from device
 * memory; the mask of rsqp_batch_set_members of either batch plays no role and is what it was when the call returns. When nobody
 * (or nobody any more) takes part, the LP solve, the loop or the rest of it is skipped: a call in which no member exceeds the
 * tolerance costs one launch. Every launch goes on qp's stream, which the LP batch's work is ordered against by an event, without a
 * device-wide wait. rsqp_batch_get_dispatch of either batch reports its last inner call.
 * RSQP_ERR_ARG before any device call: a null batch, state or options, a missing required pointer (everything but the outputs, and
 * c_k when the batch has constraints), no LP batch paired, increase_parm <= 1 (the first loop would not end). */
int rsqp_batch_handler_update_penalty(rsqp_batch *qp, const rsqp_penalty_state *s, const rsqp_penalty_options *o, int on_device);

#ifdef __cplusplus
}
#endif
#endif
