// rsqp_batch_penalty.hip -- Algorithm::update_penalty_parameter (src/Algorithm.cpp:886-1028) for every member of a QP batch and the
// LP batch paired with it (rsqp_batch_handler_pair_lp / rsqp_batch_handler_update_penalty of include/rsqp_hip_penalty.h): the
// decision kernels between the inner optimize calls, the launch that carries J from the QP batch's A pool into the LP batch's, and
// the host side that strings them together and learns one number per round.
#include "rsqp_batch_decide.h"

// Every scalar formula here must give the bits the same C expression gives on the host without contraction (rsqp_batch_decide.h)
#pragma clang fp contract(off)

namespace {
// the call's per-member work (rsqp_batch::pen)
enum { PI_PHASE = 0, PI_TAKE_LP, PI_TAKE_QP, PI_HU_LP, PI_ROUNDS, PI_NWSR_QP, PI_NWSR_LP, PEN_INTS };
enum { PD_RHO_TRIAL = 0, PD_MODEL, PD_MODEL0, PD_INFTY, PD_OBJ0, PEN_DOUBLES };
// PI_PHASE: where the member stands between two launches
enum { PH_DONE = 0, PH_LP, PH_LOOP_A, PH_LOOP_B };
// what lane 0 of a member's group tells the other lanes to do behind the decision
enum { ACT_ROUND = 1, ACT_SAVE = 2, ACT_RESTORE = 4 };

struct PenaltyArgs {
    DecisionView w;                           // nq, and the work: PEN_INTS x nq ints, PEN_DOUBLES x nq doubles
    int uniV, uniC;
    const QPDesc *desc;
    rsqp_penalty_state s;                     // device addresses
    rsqp_penalty_options o;
    // the QP batch: the result pools of its last solve, the g pool, the counts of the last inner call (host-mapped)
    double *x, *obj, *g;
    const int *status, *used;
    // the LP batch
    const double *lp_x;
    const int *lp_status, *lp_used;
};

// the loop conditions of :914-917 and :941-949 before a round: the while test, then `if (rho_trial >= rho_max) break`
__device__ inline bool loop_goes_on(const PenaltyArgs &a, int q, int phase, double model, double infty, double rho_trial) {
    const rsqp_penalty_options &o = a.o;
    if (phase == PH_LOOP_A) {
        if (!(model > o.penalty_update_tol)) return false;
    } else {
        const double infea_k = a.s.infea_k[q];
        if (!((infea_k - model) < a.s.eps1[q] * (infea_k - infty) && (a.s.trial[q] < o.penalty_iter_max))) return false;
    }
    return !(rho_trial >= o.rho_max);
}
// the head of a round (:919-924): the new rho_trial, trial++; the g write and the mask word follow
__device__ inline double start_round(const PenaltyArgs &a, int q, double rho_trial) {
    const double next = rho_trial * a.o.increase_parm;
    rho_trial = (next < a.o.rho_max) ? next : a.o.rho_max;        // min(rho_max, rho_trial * increase_parm)
    a.s.trial[q] = a.s.trial[q] + 1;
    a.w.wd(PD_RHO_TRIAL, q) = rho_trial;
    a.w.wi(PI_TAKE_QP, q) = 1;
    return rho_trial;
}
// where a member leaves the call (:975-1004, and the outputs). broke: it left the loop on an unsolved QP, `flag` its status.
// Returns ACT_RESTORE on the failure path
__device__ inline int leave(const PenaltyArgs &a, int q, double model, double rho_trial, bool have_infty, bool broke, int flag) {
    const rsqp_penalty_options &o = a.o;
    const double rho = a.s.rho[q];
    int act = 0, hu = 0;
    if (rho_trial > rho) {
        const double infea_k = a.s.infea_k[q];
        if (!broke && rho_trial * infea_k - a.obj[q] >= o.eps2 * rho_trial * (infea_k - model)) {
            a.s.succ[q] = a.s.succ[q] + 1;
            const double eps1 = a.s.eps1[q];
            a.s.eps1[q] = eps1 + (1 - eps1) * o.eps1_change_parm;
            a.s.rho[q] = rho_trial;
        } else {
            a.s.fail[q] = a.s.fail[q] + 1;
            model = a.w.wd(PD_MODEL0, q);
            hu = RSQP_HU_PENALTY;
            a.obj[q] = a.w.wd(PD_OBJ0, q);
            act = ACT_RESTORE;
        }
    }
    if (a.s.infea_model) a.s.infea_model[q] = model;
    if (a.s.infea_infty && have_infty) a.s.infea_infty[q] = a.w.wd(PD_INFTY, q);
    if (a.s.hu_word) a.s.hu_word[q] = hu;
    if (a.s.exitflag) a.s.exitflag[q] = flag;
    if (a.s.nwsr_qp) a.s.nwsr_qp[q] = a.w.wi(PI_NWSR_QP, q);
    if (a.s.nwsr_lp) a.s.nwsr_lp[q] = a.w.wi(PI_NWSR_LP, q);
    if (a.s.rounds) a.s.rounds[q] = a.w.wi(PI_ROUNDS, q);
    a.w.wi(PI_PHASE, q) = PH_DONE;
    a.w.wi(PI_TAKE_QP, q) = 0;
    return act;
}

// The decision kernels, G lanes per member (batch_nlp_ratio_kernel): STAGE 0 penalty_begin, behind the QP solve of the iteration;
// STAGE 1 penalty_after_lp, behind the LP solve; STAGE 2 penalty_round, behind a QP re-solve -- a member that leaves takes
// penalty_finish (leave) in the same launch. Lanes past the last member, and those of a member the stage does not concern, skip the
// loops and stay in the shuffles. The last block to finish reports the number of members that go on through the mapped word
template <int G, int STAGE>
__global__ void __launch_bounds__(256) batch_penalty_kernel(PenaltyArgs a) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    const bool in = q < a.w.nq;
    int phase = PH_DONE;
    bool act = false;
    if (in) {
        if (STAGE == 0) act = a.s.what[q] != 0 && a.status[q] == QPS_SOLVED;
        else {
            phase = a.w.wi(PI_PHASE, q);
            act = STAGE == 1 ? phase == PH_LP : (phase == PH_LOOP_A || phase == PH_LOOP_B);
        }
    }
    // a QP that ended unsolved inside the loop has no model to sum; its lanes stay in the shuffle
    const bool solved = act && (STAGE == 0 || (STAGE == 1 ? a.lp_status[q] : a.status[q]) == QPS_SOLVED);
    MemberShape sh{0, 0, 0, 0};
    int n = 0;
    double sm = 0.0;
    if (act) {
        sh = shape_of(a.desc, a.uniV, a.uniC, q);
        n = sh.nV - 2 * sh.nC;
        if (solved) {
            const double *const src = STAGE == 1 ? a.lp_x : a.x;
            for (int i = n + lane; i < sh.nV; i += G) sm += fabs(src[sh.offV + i]);      // get_infea_measure_model (QPhandler.cpp:592-594)
        }
    }
    sm = group_sum<G>(sm);
    int todo = 0, goes_on = 0;
    double rho_trial = 0.0;
    if (in && lane == 0) {
        if (STAGE == 0) {
            int lp = 0;
            if (act) {
                a.w.wi(PI_ROUNDS, q) = 0; a.w.wi(PI_NWSR_QP, q) = 0; a.w.wi(PI_NWSR_LP, q) = 0;
                if (sm > a.o.penalty_update_tol) {                                       // :893
                    a.w.wd(PD_MODEL, q) = sm; a.w.wd(PD_MODEL0, q) = sm;
                    lp = 1;
                } else {
                    (void)leave(a, q, sm, a.s.rho[q], false, false, RSQP_EXIT_UNKNOWN);
                }
            } else if (a.s.what[q] != 0 && a.s.exitflag) {
                a.s.exitflag[q] = dev_exitflag(a.status[q]);                             // the QP of this iteration is unsolved
            }
            a.w.wi(PI_PHASE, q) = lp ? PH_LP : PH_DONE;
            a.w.wi(PI_TAKE_LP, q) = lp; a.w.wi(PI_HU_LP, q) = lp ? RSQP_HU_SET : 0;
            a.w.wi(PI_TAKE_QP, q) = 0;
            goes_on = lp;
        } else if (act && STAGE == 1) {
            a.w.wi(PI_NWSR_LP, q) = a.lp_used[q];
            if (!solved) {                                                                // :901-904
                (void)leave(a, q, a.w.wd(PD_MODEL0, q), a.s.rho[q], false, false, dev_exitflag(a.lp_status[q]));
            } else {
                a.w.wd(PD_INFTY, q) = sm;
                phase = (sm <= a.o.penalty_update_tol) ? PH_LOOP_A : PH_LOOP_B;          // :909
                rho_trial = a.s.rho[q];
                const double model = a.w.wd(PD_MODEL, q);
                if (loop_goes_on(a, q, phase, model, sm, rho_trial)) {
                    a.w.wi(PI_PHASE, q) = phase;
                    a.w.wd(PD_OBJ0, q) = a.obj[q];
                    rho_trial = start_round(a, q, rho_trial);
                    todo = ACT_SAVE | ACT_ROUND; goes_on = 1;
                } else {
                    (void)leave(a, q, model, rho_trial, true, false, RSQP_EXIT_UNKNOWN);
                }
            }
        } else if (act) {
            a.w.wi(PI_ROUNDS, q) = a.w.wi(PI_ROUNDS, q) + 1;
            a.w.wi(PI_NWSR_QP, q) = a.w.wi(PI_NWSR_QP, q) + a.used[q];
            rho_trial = a.w.wd(PD_RHO_TRIAL, q);
            if (!solved) {                                                                // :929-932, :963-966
                todo = leave(a, q, a.w.wd(PD_MODEL, q), rho_trial, true, true, dev_exitflag(a.status[q]));
            } else {
                a.w.wd(PD_MODEL, q) = sm;
                if (loop_goes_on(a, q, phase, sm, a.w.wd(PD_INFTY, q), rho_trial)) {
                    rho_trial = start_round(a, q, rho_trial);
                    todo = ACT_ROUND; goes_on = 1;
                } else {
                    todo = leave(a, q, sm, rho_trial, true, false, RSQP_EXIT_UNKNOWN);
                }
            }
        }
    }
    todo = __shfl(todo, 0, G);
    rho_trial = __shfl(rho_trial, 0, G);
    if (todo & ACT_SAVE)
        for (int i = lane; i < sh.nV; i += G) a.w.x0[sh.offV + i] = a.x[sh.offV + i];
    if (todo & ACT_ROUND)
        for (int i = n + lane; i < sh.nV; i += G) a.g[sh.offV + i] = rho_trial;          // update_penalty (QPhandler.cpp:430-441)
    if (todo & ACT_RESTORE)
        for (int i = lane; i < sh.nV; i += G) a.x[sh.offV + i] = a.w.x0[sh.offV + i];
    // how many go on: added per member, reported by the block that finishes last
    report_live(goes_on, a.w.cnt, a.w.live);
}

// set_A of setupLP (:703) for the members penalty_begin named: the entries of columns [0, n) of the member's A, slot by slot from the
// QP batch's canonical CSC pool into the LP batch's and, through the inverse of perm, into its CSR copy; the update mark as
// batch_handler_matrices_kernel raises it. Both batches have one pattern member by member (rsqp_batch_handler_pair_lp), so a slot
// is the same number in both pools. uni_pat: member 0's column pointers, as the solve kernels read them
template <int G>
__global__ void __launch_bounds__(256)
batch_penalty_jacobian_kernel(int nq, int uni_pat, int uni_annz, const QPDesc *__restrict__ desc, const int *__restrict__ take,
                              const int *__restrict__ Ajc, const double *__restrict__ src, double *__restrict__ Aval,
                              double *__restrict__ Arv, const int *__restrict__ inv, int *__restrict__ mark, const int *__restrict__ first) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    if (q >= nq || take[q] == 0) return;
    const int n = desc[q].nV - 2 * desc[q].nC;
    const int jn = Ajc[(uni_pat ? 0 : desc[q].offAjc) + n];
    const long long base = uni_pat ? (long long)q * uni_annz : (long long)desc[q].offAnz;
    for (int k = lane; k < jn; k += G) {
        const double v = src[base + k];
        Aval[base + k] = v;
        Arv[inv[base + k]] = v;
    }
    if (lane == 0 && first[q] != 0) mark[q] = 1;
}

template <int STAGE>
int decide(rsqp_batch *b, const PenaltyArgs &a, int *live) {
    return launch_decision(b, b->pen, live, [](auto g) { return batch_penalty_kernel<decltype(g)::value, STAGE>; }, a);
}

// while the call runs: the LP batch launches on the QP batch's stream, and an inner optimize call of either batch reads the mask a
// decision kernel wrote where it reads the mask of rsqp_batch_set_members (MaskLoan). Both are put back when the call ends, however
// it ends
struct Loan {
    MaskLoan qp_mask, lp_mask;
    rsqp_batch *lp;
    hipStream_t lp_stream;
    Loan(rsqp_batch *q, rsqp_batch *l) : qp_mask(q), lp_mask(l), lp(l), lp_stream(l->stream) { lp->stream = q->stream; }
    static void lend(rsqp_batch *b, int *mask, int live) { MaskLoan::lend(b, mask, live); }
    ~Loan() { lp->stream = lp_stream; }
};
}  // namespace

extern "C" int rsqp_penalty_default_options(rsqp_penalty_options *o) {
    if (!o) return fail(RSQP_ERR_ARG, "rsqp_penalty_default_options: null pointer");
    o->penalty_update_tol = 1.0e-8;
    o->increase_parm = 10;
    o->rho_max = 1.0e6;
    o->penalty_iter_max = 200;
    o->eps1_change_parm = 0.1;
    o->eps2 = 1.0e-6;
    return RSQP_OK;
}

extern "C" int rsqp_batch_handler_pair_lp(rsqp_batch *qp, rsqp_batch *lp) {
    if (!qp) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_pair_lp: null batch");
    if (!lp) { qp->lp_pair = nullptr; return RSQP_OK; }
    const char *why = nullptr;
    if (lp == qp) why = "a batch cannot be its own LP batch";
    else if (lp->device != qp->device) why = "the batches are on different devices";
    else if (lp->nq != qp->nq) why = "the batches have different numbers of members";
    else if (!qp->keep_state || !lp->keep_state) why = "both batches must keep their state";
    else if (!qp->have_problem || !lp->have_problem) why = "rsqp_batch_handler_set_problem has not been called on both";
    else if (!qp->Afold.canon || !lp->Afold.canon) why = "a batch whose A was created in a non-canonical layout cannot be paired";
    for (int q = 0; !why && q < qp->nq; q++)
        if (qp->desc[q].nV != lp->desc[q].nV || qp->desc[q].nC != lp->desc[q].nC) why = "a member has different sizes in the two batches";
    if (!why && (qp->h_Ajc != lp->h_Ajc || qp->h_Air != lp->h_Air)) why = "a member has different A patterns in the two batches";
    if (why) return fail(RSQP_ERR_ARG, std::string("rsqp_batch_handler_pair_lp: ") + why);
    qp->lp_pair = lp;
    return RSQP_OK;
}

extern "C" int rsqp_batch_handler_update_penalty(rsqp_batch *b, const rsqp_penalty_state *s, const rsqp_penalty_options *o, int on_device) {
    if (!b || !s || !o || !s->what || !s->infea_k || !s->delta || !s->x_k || !s->rho || !s->eps1 || !s->trial || !s->succ || !s->fail ||
        (b->sumC > 0 && !s->c_k))
        return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update_penalty: what, infea_k, delta, x_k (and c_k), rho, eps1, trial, succ, fail and the options are required");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update_penalty: rsqp_batch_handler_set_problem has not been called");
    rsqp_batch *const lp = b->lp_pair;
    if (!lp) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update_penalty: no LP batch is paired (rsqp_batch_handler_pair_lp)");
    if (!(o->increase_parm > 1.0)) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update_penalty: increase_parm must exceed 1");
    if (!b->keep_state || !lp->keep_state) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update_penalty: both batches must keep their state");
    HIPCHK(hipSetDevice(b->device));
    const size_t nq = (size_t)b->nq;
    int rc;
    if ((rc = b->pen.ensure(PEN_INTS * nq, PEN_DOUBLES * nq, (size_t)b->sumV)) != RSQP_OK) return rc;
    if ((rc = ensure_opt(lp)) != RSQP_OK || (rc = ensure_handler_matrices(lp)) != RSQP_OK) return rc;
    if (!b->used.p) HIPCHK(b->used.alloc(nq, true));
    if (!lp->used.p) HIPCHK(lp->used.alloc(nq, true));
    // the LP batch's earlier work on its own stream comes first (a solve may still run there): an event, no device-wide wait. Behind
    // the call both streams are idle: the call waits for qp's, which has carried everything
    HIPCHK(hipEventRecord(lp->ev3, lp->stream));
    HIPCHK(hipStreamWaitEvent(b->stream, lp->ev3, 0));
    Loan loan(b, lp);

    PenaltyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.s = *s; a.o = *o;
    Staging st(b, on_device);
    if (st.active) stage_penalty(st, a.s, stage_sizes(b));
    if ((rc = st.up()) != RSQP_OK) return rc;
    a.w = b->pen.view(b->nq); a.uniV = uni_shape(b); a.uniC = a.uniV > 0 ? b->uniC : 0; a.desc = b->d_desc.p;
    a.x = b->x.p; a.obj = b->obj.p; a.g = b->g.p; a.status = b->status.p; a.used = b->used.dev;
    a.lp_x = lp->x.p; a.lp_status = lp->status.p; a.lp_used = lp->used.dev;
    int *const take_lp = b->pen.i.p + (size_t)PI_TAKE_LP * nq, *const take_qp = b->pen.i.p + (size_t)PI_TAKE_QP * nq;

    int live = 0;
    if ((rc = decide<0>(b, a, &live)) != RSQP_OK) return rc;                   // penalty_begin
    if (live > 0) {
        // setupLP (:700-704): set_bounds + set_g(rho) by the SET word penalty_begin wrote, then set_A from the QP batch's pool
        rsqp_handler_iterate it;
        std::memset(&it, 0, sizeof(it));
        it.what = b->pen.i.p + (size_t)PI_HU_LP * nq; it.delta = a.s.delta; it.rho = a.s.rho; it.x_k = a.s.x_k; it.c_k = a.s.c_k;
        if ((rc = rsqp_batch_handler_update(lp, &it, 1)) != RSQP_OK) return rc;
        int *const mark = lp->opt.p + (size_t)OPT_UPD * nq;
        const int *const first = lp->opt.p + (size_t)OPT_FIRST * nq;
        rc = launch_groups(b, [](auto g) { return batch_penalty_jacobian_kernel<decltype(g)::value>; }, b->nq, b->uni_pat ? 1 : 0, b->uni_annz,
                           b->d_desc.p, take_lp, b->Ajc.p, b->Aval.p, lp->Aval.p, lp->Arv.p, lp->hm_inv.p, mark, first);
        if (rc != RSQP_OK) return rc;
        Loan::lend(lp, take_lp, live);
        if ((rc = rsqp_batch_optimize_lp(lp, nullptr)) != RSQP_OK) return rc;
        if ((rc = decide<1>(b, a, &live)) != RSQP_OK) return rc;               // penalty_after_lp
        while (live > 0) {
            Loan::lend(b, take_qp, live);
            if ((rc = rsqp_batch_optimize_qp(b, nullptr)) != RSQP_OK) return rc;
            if ((rc = decide<2>(b, a, &live)) != RSQP_OK) return rc;           // penalty_round (+ penalty_finish)
        }
    }
    return on_device ? RSQP_OK : st.down();      // (every decision has waited for the stream)
}
