// rsqp_batch_nlp.hip -- the decisions of a lock-step SQP loop for every member of a batch (rsqp_batch_handler_infeasibility /
// _ratio_test / _check_optimality of include/rsqp_hip_nlp_step.h): cal_infea, ratio_test + update_radius and check_optimality of
// src/Algorithm.cpp, read from the result pools of the last solve and from the canonical A pool, with their kernels.
#include "rsqp_batch_decide.h"

// Every scalar formula here must give the bits the same C expression gives on the host without contraction: hipcc would contract
// a + b*c into an FMA by default, so contraction is OFF for this whole unit (rsqp_batch_decide.h says so as well; the build flags of
// the other units stay as they are).
#pragma clang fp contract(off)

namespace {
constexpr double NLP_INF = 1.0e18;   // INF of the reference (Utils.hpp:35)

// the member's shape, the tree sums and cal_infea's share of a lane: rsqp_batch_decide.h
// G lanes per member, as batch_handler_step_kernel: lanes past the last member, and those of a member that sits out, skip the loops
// and stay in the shuffles
template <int G>
__global__ void __launch_bounds__(256)
batch_nlp_infea_kernel(int nq, int uniV, int uniC, const QPDesc *__restrict__ desc, const double *__restrict__ c,
                       const double *__restrict__ c_l, const double *__restrict__ c_u, double *__restrict__ infea) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    double s = 0.0;
    if (q < nq) {
        const MemberShape sh = shape_of(desc, uniV, uniC, q);
        s = infea_share<G>(c + sh.offC, c_l + sh.offC, c_u + sh.offC, sh.nC, lane);
    }
    s = group_sum<G>(s);
    if (q < nq && lane == 0) infea[q] = s;
}

// ratio_test + update_radius (src/Algorithm.cpp:722-801, 820-849). The sub-group's lane 0 computes the member's scalars behind the
// reduction; the verdict goes to the other lanes by a shuffle, and the copies of an accepted step walk the member's entries G at a time
struct NlpRatio {
    int nq, uniV, uniC;
    const QPDesc *desc;
    rsqp_nlp_trial t;
    rsqp_nlp_step_options o;
    const double *c_l, *c_u;        // rsqp_batch_handler_set_problem
    const double *x, *obj;          // the result pools of the last solve
};
template <int G>
__global__ void __launch_bounds__(256) batch_nlp_ratio_kernel(NlpRatio a) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    const bool act = q < a.nq && a.t.what[q] != 0;
    MemberShape sh{0, 0, 0, 0};
    double s = 0.0, mx = 0.0;
    if (act) {
        sh = shape_of(a.desc, a.uniV, a.uniC, q);
        const int n = sh.nV - 2 * sh.nC;
        s = infea_share<G>(a.t.c_trial + sh.offC, a.c_l + sh.offC, a.c_u + sh.offC, sh.nC, lane);
        for (int i = lane; i < n; i += G) mx = fmax(mx, fabs(a.x[sh.offV + i]));    // getInfNorm of p: exact in any order
    }
    s = group_sum<G>(s);
    mx = group_max<G>(mx);
    int acc = 0;
    if (act && lane == 0) {
        const double f_t = a.t.f_trial[q];
        const RatioTest r = ratio_test_of(a.o, a.t.rho[q], a.t.f_k[q], a.t.infea_k[q], f_t, s, a.obj[q]);
        acc = r.acc;
        write_verdict<TEST_PLAIN>(a.t, a.o, q, r, f_t, s, a.t.delta[q], mx);
    }
    acc = __shfl(acc, 0, G);
    if (acc) accept_step<G>(a.t, a.x, sh, lane);      // (only lanes of an active member hold 1)
}

// classify_single_constraint (src/Utils.cpp:29-45), exactly as written
enum { T_EQUAL, T_BOUNDED, T_BOUNDED_BELOW, T_BOUNDED_ABOVE, T_UNBOUNDED };
__device__ inline int classify(double lower_bound, double upper_bound) {
    if (lower_bound > -NLP_INF && upper_bound < NLP_INF) return (upper_bound - lower_bound) < 1.0e-8 ? T_EQUAL : T_BOUNDED;
    else if (lower_bound > -NLP_INF && upper_bound > NLP_INF) return T_BOUNDED_BELOW;
    else if (upper_bound < NLP_INF && lower_bound < -NLP_INF) return T_BOUNDED_ABOVE;
    return T_UNBOUNDED;
}
// one bound pair's terms of the dual and the complementarity sums (src/Algorithm.cpp:251-306); max / min as std::max / std::min
__device__ inline void kkt_terms(double l, double u, double v, double lam, double &dual, double &compl_) {
    switch (classify(l, u)) {
    case T_BOUNDED_ABOVE: dual += (lam < 0.0) ? 0.0 : lam; compl_ += fabs(lam * (u - v)); break;
    case T_BOUNDED_BELOW: dual += -((0.0 < lam) ? 0.0 : lam); compl_ += fabs(lam * (v - l)); break;
    case T_UNBOUNDED: compl_ += fabs(lam); break;
    default: break;
    }
}

// check_optimality (src/Algorithm.cpp:170-364). A lane owns the variables lane, lane + G, ... and with each its column of J: it
// walks the column's entries of the canonical CSC pool in index order (no atomics), adds lam_x, subtracts grad and contributes the
// absolute value. A one-shape, one-pattern batch (uni_pat) reads member 0's pattern arrays, as the solve kernels do
struct NlpKkt {
    int nq, uniV, uniC, uni_pat, uni_annz;
    const QPDesc *desc;
    rsqp_nlp_point pt;
    rsqp_nlp_step_options o;
    const double *x_l, *x_u, *c_l, *c_u;
    const double *y;                          // the multiplier pool of the last solve
    const int *Ajc, *Air; const double *Aval; // the canonical CSC pool of A
    rsqp_optimality_status *out;
    int *verdict;
};
template <int G>
__global__ void __launch_bounds__(256) batch_nlp_kkt_kernel(NlpKkt a) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    const bool act = q < a.nq && a.pt.what[q] != 0;
    double dual_v = 0.0, dual_c = 0.0, compl_v = 0.0, compl_c = 0.0, stat = 0.0;
    if (act) {
        const MemberShape sh = shape_of(a.desc, a.uniV, a.uniC, q);
        const int n = sh.nV - 2 * sh.nC, m = sh.nC, offN = sh.offV - 2 * sh.offC;
        const double *const lam_x = a.y + sh.offV + sh.offC, *const lam_c = lam_x + sh.nV;
        const int *const jc = a.Ajc + (a.uni_pat ? 0 : a.desc[q].offAjc), *const ir = a.Air + (a.uni_pat ? 0 : a.desc[q].offAnz);
        const double *const val = a.Aval + (a.uni_pat ? (long long)q * a.uni_annz : (long long)a.desc[q].offAnz);
        for (int i = lane; i < n; i += G) {
            const double lam = lam_x[i];
            kkt_terms(a.x_l[offN + i], a.x_u[offN + i], a.pt.x_k[offN + i], lam, dual_v, compl_v);
            double d = 0.0;
            for (int k = jc[i]; k < jc[i + 1]; k++) d += val[k] * lam_c[ir[k]];
            d = d + lam;
            d = d - a.pt.grad[offN + i];
            stat += fabs(d);
        }
        for (int i = lane; i < m; i += G)
            kkt_terms(a.c_l[sh.offC + i], a.c_u[sh.offC + i], a.pt.c_k[sh.offC + i], lam_c[i], dual_c, compl_c);
    }
    // variables then constraints in the dual sum, constraints then variables in the complementarity sum (:251-269, 277-306)
    const double dual = group_sum<G>(dual_v + dual_c), compl_ = group_sum<G>(compl_c + compl_v);
    stat = group_sum<G>(stat);
    if (act && lane == 0) {
        const double primal = a.pt.infea[q];
        if (a.out) {
            rsqp_optimality_status s;
            s.primal_violation = primal; s.dual_violation = dual; s.compl_violation = compl_; s.stationarity_violation = stat;
            s.KKT_error = dual + primal + compl_ + stat;
            a.out[q] = s;
        }
        if (a.verdict) {
            int v = (primal < a.o.opt_prim_fea_tol ? RSQP_KKT_PRIMAL : 0) | (dual < a.o.opt_dual_fea_tol ? RSQP_KKT_DUAL : 0) |
                    (compl_ < a.o.opt_compl_tol ? RSQP_KKT_COMPL : 0) | (stat < a.o.opt_stat_tol ? RSQP_KKT_STAT : 0);
            if (v == (RSQP_KKT_PRIMAL | RSQP_KKT_DUAL | RSQP_KKT_COMPL | RSQP_KKT_STAT)) v |= RSQP_KKT_FIRST_ORDER_OPT;
            a.verdict[q] = v;
        }
    }
}

}  // namespace

extern "C" int rsqp_nlp_step_default_options(rsqp_nlp_step_options *o) {
    if (!o) return fail(RSQP_ERR_ARG, "rsqp_nlp_step_default_options: null pointer");
    o->active_set_tol = 1.0e-5;
    o->opt_prim_fea_tol = 1.0e-4; o->opt_dual_fea_tol = 1.0e-4; o->opt_compl_tol = 1.0e-4; o->opt_stat_tol = 1.0e-4;
    o->eta_s = 1.0e-8; o->eta_c = 0.25; o->eta_e = 0.75;
    o->gamma_c = 0.5; o->gamma_e = 2;
    o->delta_min = 1.0e-16; o->delta_max = 1.0e8;
    o->tol = 1.0e-8;
    o->refresh_ubA = 0;
    return RSQP_OK;
}

extern "C" int rsqp_batch_handler_infeasibility(rsqp_batch *b, const double *c, double *infea, int on_device) {
    if (!b || !infea || (b->sumC > 0 && !c)) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_infeasibility: the batch, infea (and c) are required");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_infeasibility: rsqp_batch_handler_set_problem has not been called");
    HIPCHK(hipSetDevice(b->device));
    Staging st(b, on_device);
    if (st.active) stage_infeasibility(st, c, infea, stage_sizes(b));
    int rc;
    if ((rc = st.up()) != RSQP_OK) return rc;
    const int nq = b->nq, uniV = uni_shape(b), uniC = uniV > 0 ? b->uniC : 0;
    rc = launch_groups(b, [](auto g) { return batch_nlp_infea_kernel<decltype(g)::value>; }, nq, uniV, uniC, b->d_desc.p, c, b->h_cl.p,
                       b->h_cu.p, infea);
    return rc != RSQP_OK ? rc : st.down();
}

extern "C" int rsqp_batch_handler_ratio_test(rsqp_batch *b, const rsqp_nlp_trial *t, const rsqp_nlp_step_options *o, int on_device) {
    if (!b || !t || !o || !t->what || !t->rho || !t->f_trial || !t->x_k || !t->f_k || !t->infea_k || !t->delta ||
        (b->sumC > 0 && (!t->c_trial || !t->c_k)))
        return fail(RSQP_ERR_ARG, "rsqp_batch_handler_ratio_test: what, rho, f_trial, x_k, f_k, infea_k, delta (and c_trial, c_k) and the options are required");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_ratio_test: rsqp_batch_handler_set_problem has not been called");
    HIPCHK(hipSetDevice(b->device));
    NlpRatio a;
    std::memset(&a, 0, sizeof(a));
    a.t = *t; a.o = *o;
    Staging st(b, on_device);
    if (st.active) stage_trial(st, a.t, stage_sizes(b));
    int rc;
    if ((rc = st.up()) != RSQP_OK) return rc;
    a.nq = b->nq; a.uniV = uni_shape(b); a.uniC = a.uniV > 0 ? b->uniC : 0; a.desc = b->d_desc.p;
    a.c_l = b->h_cl.p; a.c_u = b->h_cu.p; a.x = b->x.p; a.obj = b->obj.p;
    rc = launch_groups(b, [](auto g) { return batch_nlp_ratio_kernel<decltype(g)::value>; }, a);
    return rc != RSQP_OK ? rc : st.down();
}

extern "C" int rsqp_batch_handler_check_optimality(rsqp_batch *b, const rsqp_nlp_point *pt, const rsqp_nlp_step_options *o,
                                                   rsqp_optimality_status *out, int *verdict, int on_device) {
    if (!b || !pt || !o || !pt->what || !pt->x_k || !pt->grad || !pt->infea || (b->sumC > 0 && !pt->c_k))
        return fail(RSQP_ERR_ARG, "rsqp_batch_handler_check_optimality: what, x_k, grad, infea (and c_k) and the options are required");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_check_optimality: rsqp_batch_handler_set_problem has not been called");
    HIPCHK(hipSetDevice(b->device));
    NlpKkt a;
    std::memset(&a, 0, sizeof(a));
    a.pt = *pt; a.o = *o; a.out = out; a.verdict = verdict;
    static_assert(sizeof(rsqp_optimality_status) == 5 * sizeof(double), "the records are packed as five doubles");
    Staging st(b, on_device);
    if (st.active) stage_point(st, a.pt, a.out, a.verdict, stage_sizes(b));
    int rc;
    if ((rc = st.up()) != RSQP_OK) return rc;
    a.nq = b->nq; a.uniV = uni_shape(b); a.uniC = a.uniV > 0 ? b->uniC : 0; a.desc = b->d_desc.p;
    a.uni_pat = b->uni_pat ? 1 : 0; a.uni_annz = b->uni_annz;
    a.x_l = b->h_xl.p; a.x_u = b->h_xu.p; a.c_l = b->h_cl.p; a.c_u = b->h_cu.p;
    a.y = b->y.p; a.Ajc = b->Ajc.p; a.Air = b->Air.p; a.Aval = b->Aval.p;
    rc = launch_groups(b, [](auto g) { return batch_nlp_kkt_kernel<decltype(g)::value>; }, a);
    return rc != RSQP_OK ? rc : st.down(out || verdict);      // (neither: nothing comes down)
}
