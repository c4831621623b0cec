// rsqp_batch_optimize.hip -- optimizeQP / optimizeLP for every member of a batch (rsqp_batch.h): the host side of
// rsqp_batch_optimize_qp / _lp and the one-thread- or one-wavefront-per-member kernels that take their decisions between the solve
// launches.
//
// Host logic restated from the reference adapter src/qpOASESInterface.cpp as rsqp_api.hip restates it for one handle: the
// FIXED/VARIED warm-start dispatch (:137-224, :227-284, :817-833), handle_error (:686-758).
#include "rsqp_batch.h"

// ---------------------------------------------------------------------------------
// optimizeQP for every member of a batch (qpOASESInterface.cpp:137-224 + handle_error :718-757): what rsqp_optimize_qp does on one
// handle, with the per-member decisions taken by one-thread-per-member kernels between the solve launches -- no host round trip
// inside a call. plan -> solve -> rescue plan -> rescue solve (members that need none leave at once) -> count -> one wait.
// ---------------------------------------------------------------------------------
namespace {
// a member that sits out a call (rsqp_batch_set_members; take == null: nobody does). The plan, rescue-plan and count kernels of a QP
// call and the plan, rescue-plan, prox-plan and finish kernels of an LP call ask this first, before any look at the member's status or
// counts: a stale "infeasible" of a member that sits out is not rescued (the solve launches skip it by its mode word, -1)
__device__ inline bool sits_out(const int *__restrict__ take, int q) { return take && take[q] == 0; }
// what the first kernel of a call leaves for such a member: no launch of the call runs it (every mode word -1, which is also what
// rsqp_batch_get_dispatch reports); what the call takes from the host for EVERYBODY is put down in its own words -- the batch-wide
// update mark, which the host clears behind the call, and the batch-wide family of the stored states, when the call is about to move
// the others to another one (fam_all1 = 1 + family, 0 nobody has a state, -1 the words hold already). Its nWSR_used = 0 comes from
// the kernel that writes everybody's (strided 4-byte stores of a second kernel into the host-mapped array cost 60 us at 65 536 members)
__device__ inline void plan_sitter(int nq, int q, int *__restrict__ opt, int updated, int fam_all1) {
    opt_word(opt, nq, OPT_MODE, q) = -1; opt_word(opt, nq, OPT_LMODE, q) = -1;
    opt_word(opt, nq, OPT_RMODE, q) = -1; opt_word(opt, nq, OPT_PMODE, q) = -1;
    opt_word(opt, nq, OPT_RESCUE, q) = 0;
    if (updated && opt_word(opt, nq, OPT_FIRST, q) != 0) opt_word(opt, nq, OPT_UPD, q) = 1;   // (:407, :427: firstQPsolved_ &&)
    if (fam_all1 >= 0) opt_word(opt, nq, OPT_FAM, q) = fam_all1;
}

// what both plan kernels decide first for a member that takes part: the call shape rsqp_dispatch_mode gives (its status words
// advanced), with updated = Update_A / Update_H of everybody (rsqp_batch_set_matrix_values) or the member's own mark; and hot_ok:
// the member's stored state is of the kernel family of this call's launches -- on another family's a hot start runs cold, as on a
// single handle. fam1 = 1 + that family, fam_all1 as in plan_sitter
struct MemberPlan { int old_status, new_status, mode; bool hot_ok; };
__device__ inline MemberPlan plan_member(int nq, int q, const int *opt, int updated, int fam_all1, int fam1) {
    MemberPlan m;
    m.old_status = opt_word(opt, nq, OPT_OLD, q); m.new_status = opt_word(opt, nq, OPT_NEW, q);
    const bool upd = updated != 0 || opt_word(opt, nq, OPT_UPD, q) != 0;
    m.mode = rsqp_dispatch_mode(opt_word(opt, nq, OPT_FIRST, q) != 0, upd, m.old_status, m.new_status);
    m.hot_ok = (fam_all1 >= 0 ? fam_all1 : opt_word(opt, nq, OPT_FAM, q)) == fam1;
    return m;
}
// ... and write back: the status words, the mode the call starts the member with, its own mark consumed (reset_flags, :488-496),
// the family its state is of from here on
__device__ inline void plan_member_done(int nq, int q, int *opt, const MemberPlan &m, int fam1) {
    opt_word(opt, nq, OPT_OLD, q) = m.old_status; opt_word(opt, nq, OPT_NEW, q) = m.new_status;
    opt_word(opt, nq, OPT_MODE, q) = m.mode;
    opt_word(opt, nq, OPT_UPD, q) = 0; opt_word(opt, nq, OPT_FAM, q) = fam1;
}

// before the first solve: the call shape of every member (plan_member); a FIXED <-> VARIED flip re-initialises from the
// member's own previous x, y and bound working set (:201-208), copied into the warm-start pools
__global__ void batch_plan_kernel(int nq, const QPDesc *__restrict__ desc, int *__restrict__ opt, const int *__restrict__ take,
                                  int updated, int fam_all1, int fam1, const double *__restrict__ x, const double *__restrict__ y,
                                  const int *__restrict__ ws_b, double *__restrict__ x0, double *__restrict__ y0, int *__restrict__ gb) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (sits_out(take, q)) { plan_sitter(nq, q, opt, updated, fam_all1); return; }
    MemberPlan m = plan_member(nq, q, opt, updated, fam_all1, fam1);
    if (!m.hot_ok && (m.mode == RSQP_MODE_HOT_VECTORS || m.mode == RSQP_MODE_HOT_MATRICES)) m.mode = RSQP_MODE_COLD;
    plan_member_done(nq, q, opt, m, fam1);
    if (m.mode == RSQP_MODE_WARM_REINIT) {
        const QPDesc d = desc[q];
        for (int v = 0; v < d.nV; v++) { x0[d.offV + v] = x[d.offV + v]; gb[d.offV + v] = ws_b[d.offV + v]; }
        for (int i = 0; i < d.nV + d.nC; i++) y0[d.offV + d.offC + i] = y[d.offV + d.offC + i];
    }
}

// behind the first solve: firstQPsolved_ (:156-158), handle_error's QP branch per member (:718-757) -- none / re-init from scratch /
// re-init from the slack point x_0 (written to the x0 pool) --, old = new = UNDEFINED for the rescued, the count so far
__global__ void batch_rescue_plan_kernel(int nq, const QPDesc *__restrict__ desc, int *__restrict__ opt, const int *__restrict__ status,
                                         const int *__restrict__ take, const int *__restrict__ nwsr, const double *__restrict__ lbA,
                                         const double *__restrict__ ubA, double *__restrict__ x0, int *__restrict__ used) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (sits_out(take, q)) { used[q] = 0; return; }   // (the plan kernel has written its words)
    const int sw = status[q], n1 = nwsr[q];
    const bool solved = sw == QPS_SOLVED, infeasible = sw >= 100 && sw < 200;
    opt_word(opt, nq, OPT_N1, q) = n1;
    if (solved) {
        opt_word(opt, nq, OPT_FIRST, q) = 1;
        opt_word(opt, nq, OPT_RMODE, q) = -1; opt_word(opt, nq, OPT_RESCUE, q) = 0; used[q] = n1;
        return;
    }
    const QPDesc d = desc[q];
    opt_word(opt, nq, OPT_OLD, q) = 0; opt_word(opt, nq, OPT_NEW, q) = 0;
    if (infeasible && d.nV >= 2 * d.nC) {
        for (int v = 0; v < d.nV; v++) x0[d.offV + v] = 0.0;
        for (int i = 0; i < d.nC; i++) {
            x0[d.offV + i + d.nV - 2 * d.nC] = fmax(0.0, lbA[d.offC + i]);
            x0[d.offV + i + d.nV - d.nC] = -fmin(0.0, ubA[d.offC + i]);
        }
        opt_word(opt, nq, OPT_RMODE, q) = RSQP_MODE_WARM_REINIT; opt_word(opt, nq, OPT_RESCUE, q) = 2;
    } else {
        opt_word(opt, nq, OPT_RMODE, q) = RSQP_MODE_COLD; opt_word(opt, nq, OPT_RESCUE, q) = 1;
    }
}

// behind the rescue solve: nWSR_used of the rescued members. A member whose FIRST init failed reports the rescue's count alone when
// the rescue fails too (the reference throws inside handle_error, :754-756, before :211-212 add the first count)
__global__ void batch_count_kernel(int nq, const int *__restrict__ opt, const int *__restrict__ take, const int *__restrict__ status,
                                   const int *__restrict__ nwsr, int *__restrict__ used) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq || sits_out(take, q) || opt_word(opt, nq, OPT_RESCUE, q) == 0) return;
    const int n1 = opt_word(opt, nq, OPT_N1, q), n2 = nwsr[q];
    const bool first_init_failed = opt_word(opt, nq, OPT_FIRST, q) == 0;
    used[q] = (first_init_failed && status[q] != QPS_SOLVED) ? n2 : n1 + n2;
}

// what both optimize entry points do before their first launch: the checks, the pools, the first event. kind: 1
// rsqp_batch_optimize_qp, 2 rsqp_batch_optimize_lp. The first call of the other kind starts every member over -- firstQPsolved_
// false, both status words UNDEFINED, hence a cold start that reads no stored factors -- as a single handle does (rsqp_optimize_qp /
// rsqp_optimize_lp; the reference keeps separate LP and QP objects, Algorithm.cpp:561-562)
int begin_optimize(rsqp_batch *b, int kind) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!b->keep_state)
        return fail(RSQP_ERR_ARG, std::string(kind == 1 ? "rsqp_batch_optimize_qp" : "rsqp_batch_optimize_lp") +
                                      ": the batch keeps no state (rsqp_batch_set_keep_state(b, 0))");
    HIPCHK(hipSetDevice(b->device));
    const int nq = b->nq;
    int rc = ensure_opt(b);
    if (rc != RSQP_OK) return rc;
    if (!b->used.p) HIPCHK(b->used.alloc(nq, true));
    if ((rc = ensure_warm_pools(b)) != RSQP_OK) return rc;
    b->have_x0 = b->have_y0 = b->have_gb = false;   // the pools are this call's from here on
    if (kind == 2 && !b->d_desc_lp.p) {
        std::vector<QPDesc> lp = b->desc;
        for (QPDesc &d : lp) { d.haveH = 0; d.hnnz = 0; d.hreg = 0.0; }
        HIPCHK(b->d_desc_lp.from(lp));
        HIPCHK(b->g_lp.alloc(b->sumV));
    }
    if (b->last_kind != 0 && b->last_kind != kind) {
        HIPCHK(hipMemsetAsync(b->opt.p, 0, sizeof(int) * (size_t)OPT_WORDS * nq, b->stream));
        b->opt_started = false;
    }
    b->last_kind = kind;
    if ((rc = begin_handover(b)) != RSQP_OK) return rc;   // (an LP call hands nobody over: its launches stay off the tableau kernels)
    if (!b->timing) HIPCHK(hipEventRecord(b->ev0, b->stream));
    return RSQP_OK;
}

// the solve launch behind a plan kernel: every member starts as word `word` of its opt block says (QPPools::member_mode)
int launch_members(rsqp_batch *b, QPPools &p, int word, int mode, int max_nWSR, bool first, bool lp, int warm = 0) {
    p.member_mode = b->opt.p + (size_t)word * b->nq;
    return launch_batch(b, p, mode, max_nWSR, first, lp, warm);
}

// what both optimize entry points do behind their last launch: the second event, the call's one wait, the members' counts
int finish_optimize(rsqp_batch *b, int *nWSR_used) {
    if (!b->timing) HIPCHK(hipEventRecord(b->ev1, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (nWSR_used) std::memcpy(nWSR_used, b->used.p, sizeof(int) * b->nq);
    return RSQP_OK;
}

// ---------------------------------------------------------------------------------
// optimizeLP for every member of a batch (qpOASESInterface.cpp:227-284 + handle_error's LP branch :688-717): what rsqp_optimize_lp
// does on one handle. plan -> solve -> rescue plan -> rescue solve -> proximal plan -> proximal step -> finish -> one wait. The plan
// kernels run one wavefront per member: the gradient norm, g - regVal x and g'x are reductions over up to RSQP_BATCH_MAX_V entries.
// ---------------------------------------------------------------------------------
__device__ inline double lp_wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// regVal of an init: (|g|_2 > 0 ? |g|_2 : 1) * 1e3 * EPS (the same value in every lane)
__device__ inline double lp_reg_val(const QPDesc &d, const double *__restrict__ g) {
    double s = 0.0;
    for (int v = (int)threadIdx.x; v < d.nV; v += 64) s += g[d.offV + v] * g[d.offV + v];
    const double ng = sqrt(lp_wave_sum(s));
    return (ng > 0.0 ? ng : 1.0) * 1.0e3 * RSQP_EPS;
}

// before the first solve: the call shape of every member (rsqp_dispatch_mode). A FIXED <-> VARIED flip is a plain init here
// (:266-270): OPT_MODE keeps what the dispatch said (3), OPT_LMODE what is launched (0). Every init fixes the member's regVal from
// the gradient of this call; a hot start keeps the one its factors were built with
__global__ void __launch_bounds__(64)
batch_lp_plan_kernel(int nq, QPDesc *__restrict__ desc, int *__restrict__ opt, const int *__restrict__ take, int updated, int fam_all1,
                     int fam1, const double *__restrict__ g) {
    const int q = (int)blockIdx.x;
    if (q >= nq) return;
    if (sits_out(take, q)) {   // (its descriptor keeps the regVal of its own last init)
        if (threadIdx.x == 0) plan_sitter(nq, q, opt, updated, fam_all1);
        return;
    }
    const QPDesc d = desc[q];
    MemberPlan m = plan_member(nq, q, opt, updated, fam_all1, fam1);
    const bool init = m.mode == RSQP_MODE_COLD || m.mode == RSQP_MODE_WARM_REINIT;
    const double reg = init ? lp_reg_val(d, g) : d.hreg;
    // (a stored state of another kernel family: the hot start runs cold on the regVal it has, as rsqp_solve does on a handle)
    if (!m.hot_ok && !init) m.mode = RSQP_MODE_COLD;
    __syncthreads();   // every lane has read the member's words
    if (threadIdx.x == 0) {
        plan_member_done(nq, q, opt, m, fam1);
        opt_word(opt, nq, OPT_LMODE, q) = init ? RSQP_MODE_COLD : m.mode;
        desc[q].hreg = reg;
    }
}

// behind the first solve: firstQPsolved_ (:248-250), handle_error's LP branch per member (:688-717) -- none / re-init from scratch /
// re-init from x_0 := the x of the failed solve with its slack entries overwritten (:693-699; written to the x0 pool) --, a fresh
// regVal for the re-init, old = new = UNDEFINED for the rescued
__global__ void __launch_bounds__(64)
batch_lp_rescue_plan_kernel(int nq, QPDesc *__restrict__ desc, int *__restrict__ opt, const int *__restrict__ take,
                            const int *__restrict__ status, const int *__restrict__ nwsr, const double *__restrict__ g,
                            const double *__restrict__ x, const double *__restrict__ lbA, const double *__restrict__ ubA,
                            double *__restrict__ x0) {
    const int q = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (q >= nq || sits_out(take, q)) return;
    const int sw = status[q];
    const bool solved = sw == QPS_SOLVED, infeasible = sw >= 100 && sw < 200;
    if (solved) {
        if (lane == 0) {
            opt_word(opt, nq, OPT_N1, q) = nwsr[q];
            opt_word(opt, nq, OPT_FIRST, q) = 1;
            opt_word(opt, nq, OPT_RMODE, q) = -1; opt_word(opt, nq, OPT_RESCUE, q) = 0;
        }
        return;
    }
    const QPDesc d = desc[q];
    const double reg = lp_reg_val(d, g);
    const bool slack = infeasible && d.nV >= 2 * d.nC;
    if (slack) {
        for (int v = lane; v < d.nV; v += 64) x0[d.offV + v] = x[d.offV + v];
        __syncthreads();
        for (int i = lane; i < d.nC; i += 64) {
            x0[d.offV + i + d.nV - 2 * d.nC] = fmax(0.0, lbA[d.offC + i]);
            x0[d.offV + i + d.nV - d.nC] = -fmin(0.0, ubA[d.offC + i]);
        }
    }
    if (lane == 0) {
        opt_word(opt, nq, OPT_N1, q) = nwsr[q];
        opt_word(opt, nq, OPT_OLD, q) = 0; opt_word(opt, nq, OPT_NEW, q) = 0;
        opt_word(opt, nq, OPT_RMODE, q) = slack ? RSQP_MODE_WARM_REINIT : RSQP_MODE_COLD;
        opt_word(opt, nq, OPT_RESCUE, q) = slack ? 2 : 1;
        desc[q].hreg = reg;
    }
}

// behind the rescue solve: the count so far (a member whose rescue failed too reports the rescue's count alone, on both branches:
// the reference throws inside handle_error, :714-716, before :278-279 add the other), and the proximal step of every member that is
// solved now (:280-283): a hot start on the gradient g - regVal x, written to the scratch pool -- the batch's g keeps the caller's
__global__ void __launch_bounds__(64)
batch_lp_prox_plan_kernel(int nq, const QPDesc *__restrict__ desc, int *__restrict__ opt, const int *__restrict__ take,
                          const int *__restrict__ status, const int *__restrict__ nwsr, const double *__restrict__ g,
                          const double *__restrict__ x, double *__restrict__ g_lp) {
    const int q = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (q >= nq || sits_out(take, q)) return;   // (OPT_PMODE is -1 since the plan kernel)
    const bool solved = status[q] == QPS_SOLVED, rescued = opt_word(opt, nq, OPT_RESCUE, q) != 0;
    const int n1 = opt_word(opt, nq, OPT_N1, q), n2 = nwsr[q];
    __syncthreads();
    if (lane == 0) {
        opt_word(opt, nq, OPT_N1, q) = rescued ? (solved ? n1 + n2 : n2) : n1;
        opt_word(opt, nq, OPT_PMODE, q) = solved ? RSQP_MODE_HOT_VECTORS : -1;
    }
    if (!solved) return;
    const QPDesc d = desc[q];
    for (int v = lane; v < d.nV; v += 64) g_lp[d.offV + v] = g[d.offV + v] - d.hreg * x[d.offV + v];
}

// behind the proximal step: nWSR_used, and the objective g'x with the caller's gradient (:283) for the members that took the step
__global__ void __launch_bounds__(64)
batch_lp_finish_kernel(int nq, const QPDesc *__restrict__ desc, const int *__restrict__ opt, const int *__restrict__ take,
                       const int *__restrict__ nwsr, const double *__restrict__ g, const double *__restrict__ x, double *__restrict__ obj,
                       int *__restrict__ used) {
    const int q = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (q >= nq) return;
    if (sits_out(take, q)) { if (lane == 0) used[q] = 0; return; }
    const int total = opt_word(opt, nq, OPT_N1, q);
    if (opt_word(opt, nq, OPT_PMODE, q) < 0) { if (lane == 0) used[q] = total; return; }
    const QPDesc d = desc[q];
    double s = 0.0;
    for (int v = lane; v < d.nV; v += 64) s += g[d.offV + v] * x[d.offV + v];
    s = lp_wave_sum(s);
    if (lane == 0) { obj[q] = s; used[q] = total + nwsr[q]; }
}
}  // namespace

extern "C" int rsqp_batch_optimize_qp(rsqp_batch *b, int *nWSR_used) {
    int rc = begin_optimize(b, 1);
    if (rc != RSQP_OK) return rc;
    const int nq = b->nq;
    const dim3 grid((unsigned)((nq + 255) / 256)), block(256);
    QPPools p = pools_of(b, false);
    const int *const take = b->sitters ? b->take.p : nullptr;   // (null: everybody takes part)
    if (!b->opt_started && !take) {
        // no member has a solved first QP: init for everybody -- the uniform cold launch (lane-per-problem and mid-size tableau
        // kernels included), no per-member modes, no warm-start pointers; the members' mode words are 0 = cold already
        rc = launch_batch(b, p, RSQP_MODE_COLD, b->qp_maxiter, true, false);
    } else {
        // (a first call that somebody sits out comes here as well: a member without a solved first QP comes out cold)
        hipLaunchKernelGGL(batch_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc.p, b->opt.p, take, b->mats_updated ? 1 : 0,
                           b->state_engine + 1, batch_family(b, p, false) + 1, b->x.p, b->y.p, b->ws_b.p, b->wx0.p, b->wy0.p, b->wgb.p);
        HIPCHK(hipGetLastError());
        p.x0 = b->wx0.p; p.y0 = b->wy0.p; p.guess_b = b->wgb.p;     // the flip: all three (:204-206)
        // with the batch-wide update mark rsqp_dispatch_mode gives every member 0, 2 or 3, never 1 (updated = true), which the host
        // knows without a look at the device: the launch may go to the lane-per-problem kernel's WARM build
        // (rsqp_batch_set_lane_warm). With rsqp_batch_set_lane_hot on as well the build carries the word 1 too, and the marks no longer
        // matter: batch-wide, per member or absent. The rescue launch and the LP calls stay where they were
        rc = launch_members(b, p, OPT_MODE, RSQP_MODE_COLD, b->qp_maxiter, true, false,
                            (lane_warm_ok(b) && (b->mats_updated || b->lane_hot)) ? lane_warm_level(b) : 0);
    }
    if (rc != RSQP_OK) return rc;
    // (also behind a call nobody took part in: its plan kernel has written -1 into the mode words, which the uniform cold launch
    //  relies on being 0; the next call goes through the plan kernel, where members without a solved first QP come out cold)
    b->opt_started = true;
    b->cert_lp = false;
    b->mats_updated = false;   // reset_flags (:488-496); a member that sat out has the mark in its own word now
    hipLaunchKernelGGL(batch_rescue_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc.p, b->opt.p, b->status.p, take, b->nwsr.p,
                       b->lbA.p, b->ubA.p, b->wx0.p, b->used.dev);
    HIPCHK(hipGetLastError());
    // the rescue launch is unconditional: a member that needs none leaves at its first instruction, and asking the device whether
    // anybody needs one would put a host round trip into every call
    p = pools_of(b, false);
    p.x0 = b->wx0.p;                                                 // handle_error: x_0 alone (:741-743)
    rc = launch_members(b, p, OPT_RMODE, RSQP_MODE_COLD, b->qp_maxiter, false, false);
    if (rc != RSQP_OK) return rc;
    hipLaunchKernelGGL(batch_count_kernel, grid, block, 0, b->stream, nq, b->opt.p, take, b->status.p, b->nwsr.p, b->used.dev);
    HIPCHK(hipGetLastError());
    return finish_optimize(b, nWSR_used);
}

extern "C" int rsqp_batch_set_lp_options(rsqp_batch *b, int lp_maxiter) {
    if (!b || lp_maxiter < 0) return fail(RSQP_ERR_ARG, "rsqp_batch_set_lp_options");
    b->lp_maxiter = lp_maxiter;
    return RSQP_OK;
}

extern "C" int rsqp_batch_optimize_lp(rsqp_batch *b, int *nWSR_used) {
    int rc = begin_optimize(b, 2);
    if (rc != RSQP_OK) return rc;
    const int nq = b->nq;
    const dim3 grid((unsigned)nq), block(64);
    int *const opt = b->opt.p;
    const int *const take = b->sitters ? b->take.p : nullptr;   // (null: everybody takes part)
    // every launch carries per-member modes and reads the LP descriptors: H absent, hreg = the member's regVal
    QPPools p = pools_of(b, true);
    hipLaunchKernelGGL(batch_lp_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->mats_updated ? 1 : 0,
                       b->state_engine + 1, batch_family(b, p, true) + 1, b->g.p);
    HIPCHK(hipGetLastError());
    if ((rc = launch_members(b, p, OPT_LMODE, RSQP_MODE_COLD, b->lp_maxiter, true, true)) != RSQP_OK) return rc;
    b->opt_started = true;
    b->cert_lp = true;
    b->mats_updated = false;   // reset_flags (:488-496); a member that sat out has the mark in its own word now
    hipLaunchKernelGGL(batch_lp_rescue_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->status.p, b->nwsr.p,
                       b->g.p, b->x.p, b->lbA.p, b->ubA.p, b->wx0.p);
    HIPCHK(hipGetLastError());
    // (unconditional, as in rsqp_batch_optimize_qp: a member that needs no rescue leaves at its first instruction)
    p.x0 = b->wx0.p;                                                 // handle_error: x_0 alone (:700-702)
    if ((rc = launch_members(b, p, OPT_RMODE, RSQP_MODE_COLD, b->lp_maxiter, false, true)) != RSQP_OK) return rc;
    hipLaunchKernelGGL(batch_lp_prox_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->status.p, b->nwsr.p,
                       b->g.p, b->x.p, b->g_lp.p);
    HIPCHK(hipGetLastError());
    p.x0 = nullptr;
    p.g = b->g_lp.p;
    if ((rc = launch_members(b, p, OPT_PMODE, RSQP_MODE_HOT_VECTORS, b->lp_maxiter, false, true)) != RSQP_OK) return rc;
    hipLaunchKernelGGL(batch_lp_finish_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->nwsr.p, b->g.p, b->x.p,
                       b->obj.p, b->used.dev);
    HIPCHK(hipGetLastError());
    return finish_optimize(b, nWSR_used);
}

extern "C" int rsqp_batch_get_dispatch(const rsqp_batch *b, int *mode, int *rescue) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!b->opt.p) return fail(RSQP_ERR_ARG, "rsqp_batch_get_dispatch: no rsqp_batch_optimize_qp / rsqp_batch_optimize_lp has run");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    const size_t nq = b->nq;
    if (mode) HIPCHK(hipMemcpy(mode, b->opt.p + OPT_MODE * nq, sizeof(int) * nq, hipMemcpyDeviceToHost));
    if (rescue) HIPCHK(hipMemcpy(rescue, b->opt.p + OPT_RESCUE * nq, sizeof(int) * nq, hipMemcpyDeviceToHost));
    return RSQP_OK;
}
