// rsqp_batch_decide.h -- what the decision units of a batch share (rsqp_batch_nlp.hip, rsqp_batch_penalty.hip, rsqp_batch_soc.hip):
// cal_infea, the arithmetic of ratio_test and update_radius (src/Algorithm.cpp:722-801, 820-849), what a ratio test writes for a
// member, the accepted step and the exit flag of an unsolved QP. What carries no floating-point formula (the member's shape, the
// G-lane groups, the launches, the staging block) is in rsqp_batch.h. Private to those units; device code does not cross a unit, so
// everything here is inline.
#pragma once
#include "rsqp_batch.h"

// Every scalar formula here must give the bits the same C expression gives on the host without contraction: hipcc would contract
// a + b*c into an FMA by default, so contraction is OFF from here to the end of every unit that includes this header.
#pragma clang fp contract(off)

namespace rsqp_batch_units {
// lane `lane`'s share of cal_infea(c, c_l, c_u) (src/Algorithm.cpp:584-589) over m constraints: entries lane, lane + G, ...
template <int G>
__device__ inline double infea_share(const double *__restrict__ c, const double *__restrict__ c_l, const double *__restrict__ c_u,
                                     int m, int lane) {
    double s = 0.0;
    for (int i = lane; i < m; i += G) {
        const double v = c[i];
        if (v < c_l[i]) s += (c_l[i] - v);
        else if (v > c_u[i]) s += (v - c_u[i]);
    }
    return s;
}

// ratio_test (src/Algorithm.cpp:725-729, the `#if 1` branch :768-769) on a member's scalars
struct RatioTest { double actual, pred; int acc; };
__device__ inline RatioTest ratio_test_of(const rsqp_nlp_step_options &o, double rho, double f_k, double infea_k, double f_t,
                                          double infea_t, double qp_obj) {
    const double P1_x = f_k + rho * infea_k;
    const double P1_x_trial = f_t + rho * infea_t;
    RatioTest r;
    r.actual = P1_x - P1_x_trial;
    r.pred = rho * infea_k - qp_obj;
    r.acc = (r.actual >= (o.eta_s * r.pred) && r.actual >= -o.tol) ? 1 : 0;
    return r;
}
// update_radius (:820-833): delta as it leaves; true when a branch was taken
__device__ inline bool radius_update(const rsqp_nlp_step_options &o, double actual, double pred, double norm_p, double &delta) {
    if (actual < o.eta_c * pred) {
        delta = o.gamma_c * delta;
        return true;
    } else if (actual > o.eta_e * pred && (o.tol > fabs(delta - norm_p))) {
        const double grown = o.gamma_e * delta;
        delta = (o.delta_max < grown) ? o.delta_max : grown;      // std::min(gamma_e * delta_, delta_max)
        return true;
    }
    return false;
}
// the words of an accepted step (:792-795) and the exit flag behind update_radius (:838-847)
__device__ inline int accepted_hu_word(const rsqp_nlp_step_options &o) {
    return RSQP_HU_BOUNDS | RSQP_HU_GRAD | (o.refresh_ubA ? RSQP_HU_UBA : 0);
}
__device__ inline int radius_exitflag(const rsqp_nlp_step_options &o, double delta) {
    return delta < o.delta_min ? RSQP_EXIT_TRUST_REGION_TOO_SMALL : RSQP_EXIT_UNKNOWN;
}

// exitflag_of (rsqp_host.h) on the device: qpOASESInterface::get_status (src/qpOASESInterface.cpp:332-357)
__device__ inline int dev_exitflag(int sw) {
    if (sw >= 200) return RSQP_QPERROR_UNBOUNDED;
    if (sw >= 100) return RSQP_QPERROR_INFEASIBLE;
    if (sw == QPS_SOLVED) return RSQP_QP_OPTIMAL;
    if (sw >= QPS_NOTINITIALISED && sw <= QPS_HOMOTOPYQPSOLVED) return RSQP_QPERROR_NOTINITIALISED + sw;
    return RSQP_QPERROR_UNKNOWN;
}

// What a ratio test writes for member q (lane 0 of its group), update_radius included: r from ratio_test_of on f_t and infea_t,
// delta as the member brought it, norm_p the norm the radius is judged by. Trial: rsqp_nlp_trial, or rsqp_soc_trial, which has its
// fields. TEST_PLAIN: rsqp_batch_handler_ratio_test. TEST_SOC_FIRST: soc_begin's, for a member that ends there -- it also clears
// soc and nwsr_soc and reports qp_obj. TEST_SOC_SECOND: soc_end's -- the words of an accepted step either way (rejected:
// update_grad + update_bounds at x_k, :1206-1207); norm_p is that of p + s, or of the restored p
enum { TEST_PLAIN, TEST_SOC_FIRST, TEST_SOC_SECOND };
template <int TEST, class Trial>
__device__ inline void write_verdict(const Trial &t, const rsqp_nlp_step_options &o, int q, const RatioTest &r, double f_t,
                                     double infea_t, double delta, double norm_p, double qp_obj = 0.0) {
    const bool radius = radius_update(o, r.actual, r.pred, norm_p, delta);
    if (radius) t.delta[q] = delta;
    if (r.acc) { t.f_k[q] = f_t; t.infea_k[q] = infea_t; }
    if (t.actual_reduction) t.actual_reduction[q] = r.actual;
    if (t.pred_reduction) t.pred_reduction[q] = r.pred;
    if (t.infea_trial) t.infea_trial[q] = infea_t;
    if (t.accept) t.accept[q] = r.acc;
    if (t.hu_word) t.hu_word[q] = (r.acc || TEST == TEST_SOC_SECOND) ? accepted_hu_word(o) : (radius ? RSQP_HU_DELTA : 0);
    if (t.hm_word) t.hm_word[q] = r.acc ? (RSQP_HM_JAC | RSQP_HM_HESS) : 0;
    if (t.exitflag) t.exitflag[q] = radius_exitflag(o, delta);
    if constexpr (TEST == TEST_SOC_FIRST) {
        t.soc[q] = 0;
        if (t.nwsr_soc) t.nwsr_soc[q] = 0;
        if (t.qp_obj) t.qp_obj[q] = qp_obj;
    }
}
// the accepted step (:792-795) by the G lanes of the member's group: x_k += p, the leading entries of the member's x; c_k = c_trial
template <int G, class Trial>
__device__ inline void accept_step(const Trial &t, const double *x, const MemberShape &sh, int lane) {
    const int n = sh.nV - 2 * sh.nC, offN = sh.offV - 2 * sh.offC;
    for (int i = lane; i < n; i += G) t.x_k[offN + i] = t.x_k[offN + i] + x[sh.offV + i];
    for (int i = lane; i < sh.nC; i += G) t.c_k[sh.offC + i] = t.c_trial[sh.offC + i];
}
}  // namespace rsqp_batch_units
