// rsqp_batch_decide.h -- what the decision units of a batch share (rsqp_batch_nlp.hip, rsqp_batch_penalty.hip, rsqp_batch_soc.hip):
// the member's shape, the G-lane groups and their tree sums, cal_infea, the arithmetic of ratio_test and update_radius
// (src/Algorithm.cpp:722-801, 820-849), the exit flag of an unsolved QP, the launch shape, the report of how many members go on and
// the loan of the members' mask to an inner optimize call. Private to those units; device code does not cross a unit, so everything
// here is inline.
#pragma once
#include "rsqp_batch.h"

// Every scalar formula here must give the bits the same C expression gives on the host without contraction: hipcc would contract
// a + b*c into an FMA by default, so contraction is OFF from here to the end of every unit that includes this header.
#pragma clang fp contract(off)

namespace rsqp_batch_units {
// the shape of member q: a one-shape batch (uniV > 0) multiplies, else the descriptor says
struct MemberShape { int nV, nC, offV, offC; };
__device__ inline MemberShape shape_of(const QPDesc *__restrict__ desc, int uniV, int uniC, int q) {
    if (uniV > 0) return MemberShape{uniV, uniC, q * uniV, q * uniC};
    return MemberShape{desc[q].nV, desc[q].nC, desc[q].offV, desc[q].offC};
}

// the sum of v over the G lanes of a sub-group, the same bits in every lane: partners G/2, G/4, ..., 1 lanes apart
template <int G>
__device__ inline double group_sum(double v) {
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    return v;
}
// the maximum over the sub-group (exact in any order)
template <int G>
__device__ inline double group_max(double v) {
    for (int o = G / 2; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, G));
    return v;
}

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

// hs071-scale members: 8 lanes each, eight members per wavefront; else a wavefront per member (rsqp_batch_handler_get_step)
inline int lanes_per_member(const rsqp_batch *b) { return (b->nVmax + b->nCmax <= 16) ? 8 : 64; }
inline dim3 grid_of(const rsqp_batch *b, int G) { return dim3((unsigned)(((long long)b->nq * G + 255) / 256)); }
inline int uni_shape(const rsqp_batch *b) { return (b->uniV > 0 && b->uniC >= 0) ? b->uniV : 0; }
// `ints` ints in doubles of the staging block
inline size_t int_words(size_t ints) { return (ints + 1) / 2; }

// how many members go on behind a decision kernel: added per member into cnt[0], reported through the host-mapped word by the block
// that finishes last (cnt[1] counts the blocks), which clears both for the next launch. Every thread of the block calls it
__device__ inline void report_live(int goes_on, int *cnt, int *live) {
    if (goes_on) atomicAdd(&cnt[0], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&cnt[1], 1) == (int)gridDim.x - 1) {
            __threadfence();
            *live = atomicExch(&cnt[0], 0);
            atomicExch(&cnt[1], 0);
        }
    }
}

// while a call runs an inner optimize call, that call reads the mask a decision kernel wrote where it reads the mask of
// rsqp_batch_set_members, which is put back when the loan ends, however the call ends
struct MaskLoan {
    rsqp_batch *b;
    int *take; size_t take_n; bool sitters;
    explicit MaskLoan(rsqp_batch *batch) : b(batch), take(batch->take.p), take_n(batch->take.n), sitters(batch->sitters) {}
    MaskLoan(const MaskLoan &) = delete;
    MaskLoan &operator=(const MaskLoan &) = delete;
    static void lend(rsqp_batch *b, int *mask, int live) { b->take.p = mask; b->take.n = (size_t)b->nq; b->sitters = live < b->nq; }
    ~MaskLoan() { b->take.p = take; b->take.n = take_n; b->sitters = sitters; }
};
}  // namespace rsqp_batch_units
