// rsqp_batch_soc.hip -- Algorithm::second_order_correction (src/Algorithm.cpp:1144-1211) for every member of a batch
// (rsqp_batch_handler_soc_begin / _soc_end of include/rsqp_hip_soc.h): the decision kernels around the one masked inner solve, the
// host side that strings them together and learns one number, and rsqp_batch_set_objective.
#include "rsqp_batch_decide.h"

// Every scalar formula here must give the bits the same C expression gives on the host without contraction (rsqp_batch_decide.h)
#pragma clang fp contract(off)

namespace {
// the calls' per-member work (rsqp_batch::soc)
// SI_TAKE: the member's word in the mask of the inner solve; SI_PEND: soc_begin set it going and soc_end has not seen it yet
enum { SI_TAKE = 0, SI_PEND, SOC_INTS };
// the objective of the first solve, the composite qp_obj_ of :1198, and the first test's outputs (written once the correction solved)
enum { SD_OBJ0 = 0, SD_QPOBJ, SD_ACTUAL, SD_PRED, SD_INFEA, SOC_DOUBLES };
// what lane 0 of a member's group tells the other lanes to do behind the decision
enum { ACT_ACCEPT = 1, ACT_CORRECT = 2, ACT_RESTORE = 4 };

struct SocArgs {
    DecisionView w;                           // nq, and the work: SOC_INTS x nq ints, SOC_DOUBLES x nq doubles
    int uniV, uniC;
    const QPDesc *desc;
    rsqp_soc_trial t;                         // device addresses
    rsqp_nlp_step_options o;
    rsqp_soc_options so;
    const double *x_l, *x_u, *c_l, *c_u;      // rsqp_batch_handler_set_problem
    // the batch: the result pools of its last solve, the vector pools, the counts of the last inner call (host-mapped), the
    // canonical CSC pool of H
    double *x, *obj, *g, *lb, *ub, *lbA, *ubA;
    const int *status, *used;
    const int *Hjc, *Hir;
    const double *Hval;
};

// (H_k p)_i over the leading n x n block: from 0, + H_ij * p_j over the entries of row i in increasing j. The canonical pattern holds
// a row at most once per column, rows ascending: the entry of row i in column j by bisection, no atomics
__device__ inline double hess_row_times(const int *__restrict__ jc, const int *__restrict__ ir, const double *__restrict__ val,
                                        const double *__restrict__ p, int n, int i) {
    double s = 0.0;
    for (int j = 0; j < n; j++) {
        int lo = jc[j], hi = jc[j + 1];
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ir[mid] < i) lo = mid + 1; else hi = mid;
        }
        if (lo < jc[j + 1] && ir[lo] == i) s += val[lo] * p[j];
    }
    return s;
}

// soc_test, behind the QP solve of the iteration: the ratio test of every member that takes part; who is accepted, or may not be
// corrected, gets what batch_nlp_ratio_kernel writes; the others are saved and their correction QP is set up (:1172-1185). G lanes
// per member (batch_nlp_ratio_kernel): lanes past the last member, and those of a member that sits out, skip the loops and stay in
// the shuffles. The last block to finish reports the number of members that go on through the mapped word
template <int G>
__global__ void __launch_bounds__(256) batch_soc_test_kernel(SocArgs a) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    const bool in = q < a.w.nq, act = in && a.t.what[q] != 0;
    MemberShape sh{0, 0, 0, 0};
    int n = 0, offN = 0;
    double s = 0.0, mx = 0.0;
    if (act) {
        sh = shape_of(a.desc, a.uniV, a.uniC, q);
        n = sh.nV - 2 * sh.nC; offN = sh.offV - 2 * sh.offC;
        s = infea_share<G>(a.t.c_trial + sh.offC, a.c_l + sh.offC, a.c_u + sh.offC, sh.nC, lane);
        for (int i = lane; i < n; i += G) mx = fmax(mx, fabs(a.x[sh.offV + i]));    // getInfNorm of p: exact in any order
    }
    s = group_sum<G>(s);
    mx = group_max<G>(mx);
    int todo = 0;
    double delta = 0.0;
    if (in && lane == 0) {
        if (act) {
            const rsqp_nlp_step_options &o = a.o;
            const double f_t = a.t.f_trial[q];
            const RatioTest r = ratio_test_of(o, a.t.rho[q], a.t.f_k[q], a.t.infea_k[q], f_t, s, a.obj[q]);
            delta = a.t.delta[q];
            if (r.acc || (a.t.what[q] & RSQP_SOC_CORRECT) == 0) {
                write_verdict<TEST_SOC_FIRST>(a.t, o, q, r, f_t, s, delta, mx, a.obj[q]);
                if (r.acc) todo = ACT_ACCEPT;
            } else {
                a.w.wd(SD_OBJ0, q) = a.obj[q];
                a.w.wd(SD_ACTUAL, q) = r.actual; a.w.wd(SD_PRED, q) = r.pred; a.w.wd(SD_INFEA, q) = s;
                todo = ACT_CORRECT;
            }
        }
        a.w.wi(SI_TAKE, q) = (todo & ACT_CORRECT) ? 1 : 0;
        a.w.wi(SI_PEND, q) = 0;
    }
    todo = __shfl(todo, 0, G);
    delta = __shfl(delta, 0, G);
    if (todo & ACT_ACCEPT) accept_step<G>(a.t, a.x, sh, lane);      // (only lanes of an active member hold it)
    if (todo & ACT_CORRECT) {
        for (int i = lane; i < sh.nV; i += G) a.w.x0[sh.offV + i] = a.x[sh.offV + i];
        const int *const jc = a.Hjc + a.desc[q].offHjc, *const ir = a.Hir + a.desc[q].offHnz;
        const double *const val = a.Hval + a.desc[q].offHnz, *const p = a.x + sh.offV;
        for (int i = lane; i < n; i += G) {
            const double hp = hess_row_times(jc, ir, val, p, n, i);
            a.g[sh.offV + i] = hp + a.t.grad[offN + i];                                  // update_grad(H_k p + grad_f) (:1181-1183)
            const double xt = a.t.x_k[offN + i] + p[i];                                   // x_trial_ = x_k + p
            a.lb[sh.offV + i] = hu_lb(a.x_l[offN + i], xt, delta);                        // update_bounds (:1184)
            a.ub[sh.offV + i] = hu_ub(a.x_u[offN + i], xt, delta);
        }
        for (int i = lane; i < sh.nC; i += G) {
            a.lbA[sh.offC + i] = hu_lbA(a.c_l[sh.offC + i], a.t.c_trial[sh.offC + i]);
            if (a.o.refresh_ubA) a.ubA[sh.offC + i] = hu_ubA(a.c_u[sh.offC + i], a.t.c_trial[sh.offC + i]);
        }
    }
    report_live((in && lane == 0 && (todo & ACT_CORRECT)) ? 1 : 0, a.w.cnt, a.w.live);
}

// soc_step, behind the correction solve: an unsolved member leaves with its status; the others get p + s in the x pool, their second
// trial point and the composite qp_obj_ (:1190-1199)
template <int G>
__global__ void __launch_bounds__(256) batch_soc_step_kernel(SocArgs a) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    const bool act = q < a.w.nq && a.w.wi(SI_TAKE, q) != 0;
    const bool solved = act && a.status[q] == QPS_SOLVED;
    MemberShape sh{0, 0, 0, 0};
    int n = 0, offN = 0;
    double sm = 0.0;
    if (solved) {
        sh = shape_of(a.desc, a.uniV, a.uniC, q);
        n = sh.nV - 2 * sh.nC; offN = sh.offV - 2 * sh.offC;
        if (!a.t.infea_model)
            for (int i = n + lane; i < sh.nV; i += G) sm += fabs(a.w.x0[sh.offV + i]);     // get_infea_measure_model of the first solve
    }
    sm = group_sum<G>(sm);
    if (act && lane == 0) {
        if (a.t.nwsr_soc) a.t.nwsr_soc[q] = a.used[q];
        if (!solved) {
            if (a.t.exitflag) a.t.exitflag[q] = dev_exitflag(a.status[q]);
            a.t.soc[q] = 0;
        } else {
            const double model = a.t.infea_model ? a.t.infea_model[q] : sm;
            const double qp_obj = a.obj[q] + (a.w.wd(SD_OBJ0, q) - a.t.rho[q] * model);    // :1198
            a.w.wd(SD_QPOBJ, q) = qp_obj;
            if (a.t.qp_obj) a.t.qp_obj[q] = qp_obj;
            if (a.t.actual_reduction) a.t.actual_reduction[q] = a.w.wd(SD_ACTUAL, q);
            if (a.t.pred_reduction) a.t.pred_reduction[q] = a.w.wd(SD_PRED, q);
            if (a.t.infea_trial) a.t.infea_trial[q] = a.w.wd(SD_INFEA, q);
            if (a.t.accept) a.t.accept[q] = 0;
            a.t.soc[q] = 1;
            a.w.wi(SI_PEND, q) = 1;
        }
    }
    if (solved)
        for (int i = lane; i < n; i += G) {
            const double v = a.w.x0[sh.offV + i] + a.x[sh.offV + i];                        // p_k_->add_vector(s_k) (:1199)
            a.x[sh.offV + i] = v;
            a.t.x_trial[offN + i] = a.t.x_k[offN + i] + v;
        }
}

// soc_end: the second ratio test of the members soc_begin set going, the restore of a rejected one, update_radius (:1200-1208, :92)
template <int G>
__global__ void __launch_bounds__(256) batch_soc_end_kernel(SocArgs a) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    const bool act = q < a.w.nq && a.t.soc[q] != 0 && a.w.wi(SI_PEND, q) != 0;
    MemberShape sh{0, 0, 0, 0};
    double s = 0.0, mx = 0.0, mx0 = 0.0;
    if (act) {
        sh = shape_of(a.desc, a.uniV, a.uniC, q);
        const int n = sh.nV - 2 * sh.nC;
        s = infea_share<G>(a.t.c_trial + sh.offC, a.c_l + sh.offC, a.c_u + sh.offC, sh.nC, lane);
        for (int i = lane; i < n; i += G) {
            mx = fmax(mx, fabs(a.x[sh.offV + i]));       // getInfNorm of p + s ...
            mx0 = fmax(mx0, fabs(a.w.x0[sh.offV + i]));    // ... and of the p a rejected member gets back
        }
    }
    s = group_sum<G>(s);
    mx = group_max<G>(mx);
    mx0 = group_max<G>(mx0);
    int todo = 0;
    if (act && lane == 0) {
        const rsqp_nlp_step_options &o = a.o;
        const double f_t = a.t.f_trial[q];
        // get_obj_QP() is the correction QP's own objective (:729); composite_pred: the qp_obj_ of :1198
        const double qp_obj = a.so.composite_pred ? a.w.wd(SD_QPOBJ, q) : a.obj[q];
        const RatioTest r = ratio_test_of(o, a.t.rho[q], a.t.f_k[q], a.t.infea_k[q], f_t, s, qp_obj);
        if (r.acc) {
            todo = ACT_ACCEPT;
        } else {
            a.obj[q] = a.w.wd(SD_OBJ0, q);
            if (a.t.qp_obj) a.t.qp_obj[q] = a.w.wd(SD_OBJ0, q);
            todo = ACT_RESTORE;
        }
        write_verdict<TEST_SOC_SECOND>(a.t, o, q, r, f_t, s, a.t.delta[q], r.acc ? mx : mx0);
        a.w.wi(SI_PEND, q) = 0;
    }
    todo = __shfl(todo, 0, G);
    if (todo & ACT_ACCEPT) accept_step<G>(a.t, a.x, sh, lane);
    if (todo & ACT_RESTORE)
        for (int i = lane; i < sh.nV; i += G) a.x[sh.offV + i] = a.w.x0[sh.offV + i];
}

__global__ void __launch_bounds__(256)
batch_set_objective_kernel(int nq, const int *__restrict__ named, const double *__restrict__ src, double *__restrict__ obj) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq && named[q] != 0) obj[q] = src[q];
}

// what both calls check before any device call; null: fine
const char *refused(const rsqp_batch *b, const rsqp_soc_trial *t, const rsqp_nlp_step_options *o, const rsqp_soc_options *so, bool begin) {
    if (!b || !t || !o || !so) return "the batch, the trial, the step options and the SOC options are required";
    if (!t->rho || !t->f_trial || !t->x_k || !t->f_k || !t->infea_k || !t->delta || !t->soc || (b->sumC > 0 && (!t->c_trial || !t->c_k)))
        return "rho, f_trial, x_k, f_k, infea_k, delta, soc (and c_trial, c_k) are required";
    if (begin && (!t->what || !t->x_trial)) return "what and x_trial are required";
    if (!b->have_problem) return "rsqp_batch_handler_set_problem has not been called";
    if (!b->haveH) return "the batch has no H";
    if (!b->keep_state) return "the batch keeps no state (rsqp_batch_set_keep_state(b, 0))";
    return nullptr;
}

void fill(const rsqp_batch *b, SocArgs &a) {
    a.w = b->soc.view(b->nq); a.uniV = uni_shape(b); a.uniC = a.uniV > 0 ? b->uniC : 0; a.desc = b->d_desc.p;
    a.x_l = b->h_xl.p; a.x_u = b->h_xu.p; a.c_l = b->h_cl.p; a.c_u = b->h_cu.p;
    a.x = b->x.p; a.obj = b->obj.p; a.g = b->g.p; a.lb = b->lb.p; a.ub = b->ub.p; a.lbA = b->lbA.p; a.ubA = b->ubA.p;
    a.status = b->status.p; a.used = b->used.dev;
    a.Hjc = b->Hjc.p; a.Hir = b->Hir.p; a.Hval = b->Hval.p;
}
}  // namespace

extern "C" int rsqp_soc_default_options(rsqp_soc_options *o) {
    if (!o) return fail(RSQP_ERR_ARG, "rsqp_soc_default_options: null pointer");
    o->composite_pred = 0;
    return RSQP_OK;
}

extern "C" int rsqp_batch_handler_soc_begin(rsqp_batch *b, const rsqp_soc_trial *t, const rsqp_nlp_step_options *o,
                                            const rsqp_soc_options *so, int on_device) {
    if (const char *why = refused(b, t, o, so, true)) return fail(RSQP_ERR_ARG, std::string("rsqp_batch_handler_soc_begin: ") + why);
    bool correct = on_device != 0;      // (device words cannot be read here: grad is required with them)
    if (!on_device)
        for (int q = 0; q < b->nq; q++) correct = correct || (t->what[q] & RSQP_SOC_CORRECT) != 0;
    if (correct && !t->grad) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_soc_begin: a word has CORRECT and grad is NULL");
    HIPCHK(hipSetDevice(b->device));
    const size_t nq = (size_t)b->nq;
    int rc;
    if ((rc = b->soc.ensure(SOC_INTS * nq, SOC_DOUBLES * nq, (size_t)b->sumV)) != RSQP_OK) return rc;
    if (!b->used.p) HIPCHK(b->used.alloc(nq, true));
    MaskLoan loan(b);      // the inner optimize call reads the mask the test kernel writes; put back however the call ends
    SocArgs a;
    std::memset(&a, 0, sizeof(a));
    a.t = *t; a.o = *o; a.so = *so;
    Staging st(b, on_device);
    if (st.active) stage_trial(st, a.t, stage_sizes(b));
    if ((rc = st.up()) != RSQP_OK) return rc;
    fill(b, a);
    int live = 0;
    if ((rc = launch_decision(b, b->soc, &live, [](auto g) { return batch_soc_test_kernel<decltype(g)::value>; }, a)) != RSQP_OK) return rc;
    b->soc_begun = true;
    if (live > 0) {
        MaskLoan::lend(b, b->soc.i.p + (size_t)SI_TAKE * nq, live);
        if ((rc = rsqp_batch_optimize_qp(b, nullptr)) != RSQP_OK) return rc;
        if ((rc = launch_groups(b, [](auto g) { return batch_soc_step_kernel<decltype(g)::value>; }, a)) != RSQP_OK) return rc;
        b->results_foreign = true;      // the x pool holds p + s, which is no solve's own x (rsqp_batch_set_results)
    }
    return st.down();
}

extern "C" int rsqp_batch_handler_soc_end(rsqp_batch *b, const rsqp_soc_trial *t, const rsqp_nlp_step_options *o,
                                          const rsqp_soc_options *so, int on_device) {
    if (const char *why = refused(b, t, o, so, false)) return fail(RSQP_ERR_ARG, std::string("rsqp_batch_handler_soc_end: ") + why);
    if (!b->soc_begun) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_soc_end: no rsqp_batch_handler_soc_begin has run on this batch");
    HIPCHK(hipSetDevice(b->device));
    SocArgs a;
    std::memset(&a, 0, sizeof(a));
    a.t = *t; a.o = *o; a.so = *so;
    Staging st(b, on_device);
    if (st.active) stage_trial(st, a.t, stage_sizes(b));
    int rc;
    if ((rc = st.up()) != RSQP_OK) return rc;
    fill(b, a);
    rc = launch_groups(b, [](auto g) { return batch_soc_end_kernel<decltype(g)::value>; }, a);
    return rc != RSQP_OK ? rc : st.down();
}

extern "C" int rsqp_batch_set_objective(rsqp_batch *b, const int *members, const double *obj) {
    if (!b || !obj) return fail(RSQP_ERR_ARG, "rsqp_batch_set_objective: the batch and obj are required");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (!members) { HIPCHK(b->obj.upload(obj, (size_t)b->nq)); return RSQP_OK; }
    const size_t nq = (size_t)b->nq;
    std::vector<int> m(nq);
    for (size_t q = 0; q < nq; q++) m[q] = members[q] != 0 ? 1 : 0;
    if (!b->named.p) HIPCHK(b->named.alloc(nq));
    HIPCHK(b->named.upload(m.data(), nq));
    int rc;
    if ((rc = ensure_scratch(b, nq)) != RSQP_OK) return rc;
    HIPCHK(hipMemcpy(b->scratch.p, obj, sizeof(double) * nq, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(batch_set_objective_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, b->stream, b->nq, b->named.p,
                       b->scratch.p, b->obj.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));   // (rsqp_batch::scratch: free again behind this)
    return RSQP_OK;
}
