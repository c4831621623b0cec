// rsqp_batch.hip -- the batch of independent QPs of include/rsqp_hip.h (rsqp_batch_*) itself: create / destroy, the setters of the
// whole batch, warm start, options, the solve launch, results, certificate, records, timers. optimizeQP / optimizeLP per member are
// rsqp_batch_optimize.hip, everything that writes the pools member by member rsqp_batch_handler.hip; what they share is rsqp_batch.h.
//
// The status mapping is restated from the reference adapter src/qpOASESInterface.cpp (:332-357) as rsqp_api.hip restates it.
#include "rsqp_batch.h"
#include "rsqp_small_plan.h"
#include "rsqp_sparse.h"

// =====================================================================================
// batch of independent QPs
// =====================================================================================
static_assert(RSQP_BATCH_MAX_V == RSQP_HBM_MAX_V && RSQP_BATCH_MAX_C == RSQP_HBM_MAX_C, "batch size limits of rsqp_hip.h and rsqp_internal.h");

namespace {
// the knobs of a launch: LP launches stay off the register-resident tableau kernels, which answer RET_SETUP_FAILED on a pivot in
// their rounding band and have no hand-over inside a batch (a single handle re-solves on the Givens kernel, rsqp_solve)
SmallKnobs knobs_of(const rsqp_batch *b, bool lp) {
    SmallKnobs k = b->kn;
    if (lp) k.no_tiny = 2;   // (nor the mid-size tableau kernel, which would hand every LP member back: no H, hreg != 0)
    return k;
}
}  // namespace

namespace rsqp_batch_units {
// lp: a launch of rsqp_batch_optimize_lp -- the LP descriptors (no H, per-member hreg), read by every kernel it runs on
QPPools pools_of(rsqp_batch *b, bool lp) {
    QPPools p;
    std::memset(&p, 0, sizeof(p));
    p.desc = lp ? b->d_desc_lp.p : b->d_desc.p;
    p.Ajc = b->Ajc.p; p.Air = b->Air.p; p.Aval = b->Aval.p;
    p.Arp = b->Arp.p; p.Aci = b->Aci.p; p.Arv = b->Arv.p;
    p.Hjc = b->Hjc.p; p.Hir = b->Hir.p; p.Hval = b->Hval.p;
    p.g = b->g.p; p.lb = b->lb.p; p.ub = b->ub.p; p.lbA = b->lbA.p; p.ubA = b->ubA.p;
    p.x = b->x.p; p.y = b->y.p; p.ws_b = b->ws_b.p; p.ws_c = b->ws_c.p;
    p.status = b->status.p; p.ret = b->ret.p; p.nwsr = b->nwsr.p; p.nflips = b->nflips.p;
    p.obj = b->obj.p; p.state = b->state.p;
    p.uniV = b->uniV; p.uniC = b->uniC;
    p.keep_state = b->keep_state ? 1 : 0;
    p.done_flag = nullptr; p.done_val = 0;
    p.tiny_ok = (b->h_sym || !b->haveH || lp) ? 1 : 0;   // (as pools_of(rsqp_solver *): an unsymmetric H does not move the LPs)
    // the batch-wide uni_hreg / uni_haveH cannot say what an LP member needs: LP launches read the descriptors
    p.uni_pat = (b->uni_pat && !lp) ? 1 : 0;
    p.uni_annz = b->uni_annz; p.uni_hnnz = lp ? 0 : b->uni_hnnz; p.uni_haveH = (b->haveH && !lp) ? 1 : 0; p.uni_state = b->uni_state;
    p.lane_hblock = (p.uni_pat && b->kn.lane_hblock != 0) ? b->lane_hblock : 8;   // (uni_hreg stays 0 in a batch)
    return p;
}

int ensure_opt(rsqp_batch *b) {
    if (!b->opt.p) HIPCHK(b->opt.alloc((size_t)OPT_WORDS * b->nq));
    return RSQP_OK;
}
// (grows by replacing the block: it is free, see rsqp_batch::scratch)
int ensure_scratch(rsqp_batch *b, size_t words) {
    if (!b->scratch.p || b->scratch.n < words) HIPCHK(b->scratch.alloc(words, false));
    return RSQP_OK;
}

void judge_h_sym(rsqp_batch *b, const int *members, const double *Hval) {
    if (b->h_Hjc.empty()) return;
    b->h_sym = true;
    for (int q = 0; q < b->nq; q++) {
        const QPDesc &d = b->desc[q];
        if (Hval && (!members || members[q] != 0))
            b->h_symq[q] = small_csc_symmetric(d.nV, b->h_Hjc.data() + d.offHjc, b->h_Hir.data() + b->h_Huoff[q], Hval + b->h_Huoff[q]);
        b->h_sym = b->h_sym && b->h_symq[q];
    }
    if (Hval) b->symq_stale = true;
}

int settle_A(rsqp_batch *b) {
    if (!b->Afold.canon) HIPCHK(b->Afold.sum(b->Aval, (int)b->sumAnz, b->stream));
    if (rsqp_launch_gather((int)b->sumAnz, b->perm.p, b->Aval.p, b->Arv.p, b->stream) != hipSuccess)
        return fail(RSQP_ERR_DEVICE, "gather launch failed");
    return RSQP_OK;
}
int settle_H(rsqp_batch *b) {
    if (!b->Hfold.canon) HIPCHK(b->Hfold.sum(b->Hval, (int)b->sumHnz, b->stream));
    return RSQP_OK;
}
}  // namespace rsqp_batch_units

extern "C" int rsqp_batch_create(int nq, const int *nV, const int *nC, const int *Ajc_in, const int *Air_in,
                                 const double *Aval_in, const int *Hjc_in, const int *Hir_in, const double *Hval_in,
                                 int device, rsqp_batch **out) {
    if (!out || nq <= 0 || !nV || !nC || !Ajc_in) return fail(RSQP_ERR_ARG, "rsqp_batch_create");
    if (rsqp_device_count() <= 0) return fail(RSQP_ERR_DEVICE, "rsqp_batch_create: no HIP device visible");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    for (int q = 0; q < nq; q++)
        if (nV[q] <= 0 || nC[q] < 0) return fail(RSQP_ERR_ARG, "rsqp_batch_create: bad sizes");
    // from here on Ajc ... Hval are the canonical pools: the caller's arrays where they are canonical (PooledCsc)
    PooledCsc PA, PH;
    static const char *const why[] = {"", " column pointers must start at 0", " column pointers not monotone", " row index", " values missing"};
    if (const int f = pool_csc(nq, nC, nV, Ajc_in, Air_in, Aval_in, PA)) return fail(RSQP_ERR_ARG, std::string("rsqp_batch_create: A") + why[f]);
    if (Hjc_in)
        if (const int f = pool_csc(nq, nV, nV, Hjc_in, Hir_in, Hval_in, PH)) return fail(RSQP_ERR_ARG, std::string("rsqp_batch_create: H") + why[f]);
    const int *Ajc = PA.jc, *Air = PA.ir, *Hjc = Hjc_in ? PH.jc : nullptr, *Hir = Hjc_in ? PH.ir : nullptr;
    const double *Aval = PA.val, *Hval = Hjc_in ? PH.val : nullptr;
    rsqp_batch *b = new rsqp_batch();
    struct Guard { rsqp_batch *b; ~Guard() { delete b; } } guard{b};
    b->nq = nq;
    HIPCHK(hipGetDevice(&b->device));
    b->haveH = Hjc != nullptr;
    b->desc.resize(nq);
    std::vector<int> h_Arp, h_Aci, h_perm;
    long long offV = 0, offC = 0, offAjc = 0, offAnz = 0, offArp = 0, offHjc = 0, offHnz = 0, offState = 0;
    for (int q = 0; q < nq; q++) {
        QPDesc &d = b->desc[q];
        d.nV = nV[q]; d.nC = nC[q];
        d.offV = (int)offV; d.offC = (int)offC; d.offAjc = (int)offAjc; d.offAnz = (int)offAnz;
        d.offArp = (int)offArp; d.offHjc = (int)offHjc; d.offHnz = (int)offHnz; d.haveH = b->haveH;
        d.offState = offState;
        const int *jc = Ajc + offAjc;
        const int annz = jc[d.nV];
        d.annz = annz; d.hnnz = b->haveH ? Hjc[offHjc + d.nV] : 0;
        // (the J block of a member of the QPhandler shape, in the caller's layout: rsqp_batch_handler_set_matrices)
        b->h_jn.push_back(d.nV > 2 * d.nC ? Ajc_in[offAjc + d.nV - 2 * d.nC] : 0);
        b->sumJ += b->h_jn.back();
        CsrCopy r;
        csr_from_csc(d.nC, d.nV, jc, Air + offAnz, r);
        h_Arp.insert(h_Arp.end(), r.rp.begin(), r.rp.end());
        h_Aci.insert(h_Aci.end(), r.ci.begin(), r.ci.end());
        for (int v : r.perm) h_perm.push_back((int)offAnz + v);
        b->nVmax = std::max(b->nVmax, d.nV); b->nCmax = std::max(b->nCmax, d.nC);
        if (q == 0) { b->uniV = d.nV; b->uniC = d.nC; }
        else { if (b->uniV != d.nV) b->uniV = -1; if (b->uniC != d.nC) b->uniC = -1; }
        offV += d.nV; offC += d.nC; offAjc += d.nV + 1; offAnz += annz; offArp += d.nC + 1;
        b->mat_bytes_max = std::max(b->mat_bytes_max, rsqp_mat_lds_bytes(d.nV, d.nC, annz, b->haveH ? Hjc[offHjc + d.nV] : 0));
        if (b->haveH) {
            const int hnnz = Hjc[offHjc + d.nV];
            offHjc += d.nV + 1; offHnz += hnnz;
        }
        offState += rsqp_state_bytes(d.nV, d.nC) / 8;
    }
    if (!rsqp_small_qp_fits(b->nVmax, b->nCmax)) {
        // the whole batch runs the HBM-resident kernel: its state slices are the images used in place (plus the dense
        // matrices), with no extension for the KKT-tableau kernel
        if (!rsqp_hbm_qp_fits(b->nVmax, b->nCmax))
            return fail(RSQP_ERR_TOO_LARGE, "rsqp_batch_create: a problem exceeds the batch limit of " + std::to_string(RSQP_HBM_MAX_V) +
                                                " variables and " + std::to_string(RSQP_HBM_MAX_C) + " constraints");
        b->hbm = true;
        offState = 0;
        for (int q = 0; q < nq; q++) {
            b->desc[q].offState = offState;
            offState += rsqp_hbm_state_bytes(b->desc[q].nV, b->desc[q].nC) / 8;
        }
    }
    if (b->haveH && b->nVmax <= 8) {
        // (rsqp_batch_set_matrix_values gets the caller's layout: its pattern is kept)
        b->h_Hjc.assign(Hjc_in, Hjc_in + offHjc); b->h_Hir.assign(Hir_in, Hir_in + PH.unnz); b->h_Huoff = PH.uoff;
        b->h_symq.assign(nq, 1);
        judge_h_sym(b, nullptr, Hval_in);   // (on the caller's arrays: repeated positions are summed in the caller's order on both)
    } else if (b->haveH) b->h_sym = false;
    b->sumV = offV; b->sumC = offC; b->sumAnz = offAnz; b->sumHnz = offHnz;
    b->h_Ajc.assign(Ajc, Ajc + offAjc); b->h_Air.assign(Air, Air + offAnz);   // (rsqp_batch_handler_pair_lp compares them)
    // uniform batch: every member has the sizes and the patterns of member 0 (QPPools::uni_pat)
    b->uni_pat = b->uniV > 0 && b->uniC >= 0;
    if (b->uni_pat) {
        const QPDesc &d0 = b->desc[0];
        b->uni_annz = d0.annz; b->uni_hnnz = d0.hnnz;
        b->uni_state = (b->hbm ? rsqp_hbm_state_bytes(d0.nV, d0.nC) : rsqp_state_bytes(d0.nV, d0.nC)) / 8;
        for (int q = 1; q < nq && b->uni_pat; q++) {
            const QPDesc &d = b->desc[q];
            b->uni_pat = d.annz == d0.annz && d.hnnz == d0.hnnz &&
                         std::memcmp(Ajc + d.offAjc, Ajc, sizeof(int) * (d0.nV + 1)) == 0 &&
                         std::memcmp(Air + d.offAnz, Air, sizeof(int) * d0.annz) == 0 &&
                         (!b->haveH || (std::memcmp(Hjc + d.offHjc, Hjc, sizeof(int) * (d0.nV + 1)) == 0 &&
                                        std::memcmp(Hir + d.offHnz, Hir, sizeof(int) * d0.hnnz) == 0));
        }
    }
    // (the lane-per-problem kernel keeps H as its leading 4 x 4 block when the one pattern has nothing outside it: the slacks of
    //  the QPhandler formulation have no curvature)
    if (b->uni_pat) {
        bool inside = true;
        for (int c = 0; b->haveH && c < b->uniV; c++)
            for (int e = Hjc[c]; e < Hjc[c + 1]; e++) inside = inside && c < 4 && Hir[e] < 4;
        b->lane_hblock = inside ? 4 : 8;
    }
    b->uni_jn = b->uni_pat && PA.canon;   // (one canonical pattern: one J count; a folded layout may repeat positions per member)
    HIPCHK(hipStreamCreate(&b->stream));
    HIPCHK(hipEventCreate(&b->ev0)); HIPCHK(hipEventCreate(&b->ev1));
    HIPCHK(hipEventCreate(&b->ev2)); HIPCHK(hipEventCreate(&b->ev3));
    HIPCHK(b->d_desc.from(b->desc));
    HIPCHK(b->Ajc.alloc(offAjc)); HIPCHK(b->Ajc.upload(Ajc, offAjc));
    HIPCHK(b->Air.alloc(offAnz)); HIPCHK(b->Air.upload(Air, offAnz));
    HIPCHK(b->Aval.alloc(offAnz)); HIPCHK(b->Aval.upload(Aval, offAnz));
    HIPCHK(b->Arp.alloc(offArp)); HIPCHK(b->Arp.upload(h_Arp.data(), h_Arp.size()));
    HIPCHK(b->Aci.alloc(offAnz)); HIPCHK(b->Aci.upload(h_Aci.data(), h_Aci.size()));
    HIPCHK(b->perm.alloc(offAnz)); HIPCHK(b->perm.upload(h_perm.data(), h_perm.size()));
    HIPCHK(b->Arv.alloc(offAnz));
    // (the pool holds the sums the host took: only the CSR copy is due, whatever the layout)
    if (rsqp_launch_gather((int)offAnz, b->perm.p, b->Aval.p, b->Arv.p, b->stream) != hipSuccess)
        return fail(RSQP_ERR_DEVICE, "gather launch failed");
    HIPCHK(b->Hjc.alloc(b->haveH ? offHjc : 2)); HIPCHK(b->Hir.alloc(offHnz)); HIPCHK(b->Hval.alloc(offHnz));
    if (b->haveH) {
        HIPCHK(b->Hjc.upload(Hjc, offHjc)); HIPCHK(b->Hir.upload(Hir, offHnz)); HIPCHK(b->Hval.upload(Hval, offHnz));
    }
    // non-canonical layouts: the caller's values and the fold maps, for rsqp_batch_set_matrix_values
    // (with the caller's first values: rsqp_batch_set_matrix_values_of rewrites the named members' alone)
    HIPCHK(PA.fold_into(b->Afold));
    if (!b->Afold.canon) { HIPCHK(b->Afold.uval.upload(Aval_in, b->Afold.unnz)); HIPCHK(b->Auoff.from(PA.uoff)); }
    if (b->haveH) {
        HIPCHK(PH.fold_into(b->Hfold));
        if (!b->Hfold.canon) { HIPCHK(b->Hfold.uval.upload(Hval_in, b->Hfold.unnz)); HIPCHK(b->Huoff.from(PH.uoff)); }
    }
    HIPCHK(b->g.alloc(offV)); HIPCHK(b->lb.alloc(offV)); HIPCHK(b->ub.alloc(offV));
    HIPCHK(b->lbA.alloc(offC)); HIPCHK(b->ubA.alloc(offC));
    HIPCHK(b->x.alloc(offV)); HIPCHK(b->y.alloc(offV + offC)); HIPCHK(b->obj.alloc(nq));
    HIPCHK(b->ws_b.alloc(offV)); HIPCHK(b->ws_c.alloc(offC));
    HIPCHK(b->status.alloc(nq)); HIPCHK(b->ret.alloc(nq)); HIPCHK(b->nwsr.alloc(nq)); HIPCHK(b->nflips.alloc(nq));
    if (b->hbm) {
        const hipError_t e = b->state.alloc((size_t)offState);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(RSQP_ERR_TOO_LARGE, "rsqp_batch_create: the state block of the batch (" + std::to_string(8 * offState) +
                                                " bytes) cannot be allocated: " + hipGetErrorString(e));
        }
    } else {
        HIPCHK(b->state.alloc((size_t)offState));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    guard.b = nullptr;
    *out = b;
    return RSQP_OK;
}

extern "C" void rsqp_batch_destroy(rsqp_batch *b) { delete b; }

extern "C" int rsqp_batch_set_vectors(rsqp_batch *b, const double *g, const double *lb, const double *ub,
                                      const double *lbA, const double *ubA) {
    if (!b || !g || !lb || !ub || (b->sumC > 0 && (!lbA || !ubA))) return fail(RSQP_ERR_ARG, "rsqp_batch_set_vectors");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(b->g.upload(g, b->sumV)); HIPCHK(b->lb.upload(lb, b->sumV)); HIPCHK(b->ub.upload(ub, b->sumV));
    HIPCHK(b->lbA.upload(lbA, b->sumC)); HIPCHK(b->ubA.upload(ubA, b->sumC));
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_matrix_values(rsqp_batch *b, const double *Aval, const double *Hval) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    // (the caller's layout of rsqp_batch_create; a non-canonical one is folded into the canonical pools by one launch)
    int rc;
    if (Aval) {
        HIPCHK((b->Afold.canon ? b->Aval : b->Afold.uval).upload(Aval, (size_t)b->Afold.unnz));
        if ((rc = settle_A(b)) != RSQP_OK) return rc;
    }
    if (Hval && b->haveH) {
        HIPCHK((b->Hfold.canon ? b->Hval : b->Hfold.uval).upload(Hval, (size_t)b->Hfold.unnz));
        if ((rc = settle_H(b)) != RSQP_OK) return rc;
        judge_h_sym(b, nullptr, Hval);
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    // (qpOASESInterface.cpp:407-409, 427-429: counts for the members whose first QP is solved -- the plan kernel looks at that)
    if (Aval || (Hval && b->haveH)) b->mats_updated = true;
    return RSQP_OK;
}

namespace rsqp_batch_units {
int ensure_warm_pools(rsqp_batch *b) {
    if (b->wx0.p) return RSQP_OK;
    HIPCHK(b->wx0.alloc(b->sumV)); HIPCHK(b->wy0.alloc(b->sumV + b->sumC)); HIPCHK(b->wgb.alloc(b->sumV));
    return RSQP_OK;
}

// the plan of a launch on this batch (rsqp_small_plan.h): the batch remembers by itself when a launch keeps no state.
// handover: the plan of the same launch without the hs071-scale tableau kernels, as rsqp_solve plans its retry on a handle
static SmallPlan plan_of(const rsqp_batch *b, const QPPools &p, int mode, bool lp, bool handover = false, int warm = 0) {
    SmallFacts f = rsqp_small_facts(p, b->hbm, b->state_engine);
    f.skip_mark = 1;
    f.lane_warm = (warm >= 1 && !lp && !handover) ? 1 : 0;
    f.lane_hot = (warm >= 2 && !lp && !handover) ? 1 : 0;
    SmallKnobs k = knobs_of(b, lp);
    if (handover && k.no_tiny == 0) k.no_tiny = 1;
    return rsqp_plan_small_launch(k, f, b->nq, b->nVmax, b->nCmax, b->mat_bytes_max, mode);
}

// layout a launch on this batch leaves in the state blocks: 3 HBM-resident, 1 hs071-scale tableau (+ lane-per-problem), 0 LDS-resident
int batch_family(const rsqp_batch *b, const QPPools &p, bool lp) { return plan_of(b, p, RSQP_MODE_COLD, lp).state_family; }

// a handed member leaves a state block the result pools do not describe, and pools rsqp_batch_set_results has written are not the
// batch's own answer: either way a hot start with new matrices must read the stored state, which the 8-lane kernel does
bool lane_warm_ok(const rsqp_batch *b) { return b->lane_warm && !b->handover && !b->results_foreign; }
// the `warm` word of launch_batch for a call the WARM builds may take: 2 with rsqp_batch_set_lane_hot on as well, else 1
int lane_warm_level(const rsqp_batch *b) { return b->lane_hot ? 2 : 1; }

// one solve launch of the whole batch (p.member_mode: of the members it names). first: the launch rsqp_batch_get_last_kernel reports;
// lp: a launch of rsqp_batch_optimize_lp (pools_of, knobs_of)
int launch_batch(rsqp_batch *b, QPPools &p, int mode, int max_nWSR, bool first, bool lp, int warm) {
    const SmallPlan pl = plan_of(b, p, mode, lp, false, warm);
    if (pl.lane_warm) {
        // the guess of the WARM builds (QPPools::guess_*). A warm re-initialisation: what the caller gave; a hot start with new
        // matrices or on new vectors and per-member modes: the result pools -- the plan kernel of rsqp_batch_optimize_qp has copied a mode-3
        // member's x, y and bound statuses from there into the warm-start pools, so they hold the same values
        const bool reinit = !p.member_mode && pl.mode == RSQP_MODE_WARM_REINIT;
        p.guess_x = reinit ? p.x0 : b->x.p; p.guess_y = reinit ? p.y0 : b->y.p; p.guess_sb = reinit ? p.guess_b : b->ws_b.p;
        p.guess_sc = reinit ? nullptr : b->ws_c.p;
        p.guess_mode = pl.mode;
    }
    // the first launch of a call writes the pools of every member that takes part: with nobody sitting out they are the batch's own
    // answer again (a hand-over launch behind it says otherwise, below)
    if (first && !(p.member_mode && b->sitters)) b->results_foreign = false;
    // every member of the launch has a state of this family now; one that sits out keeps what it had. A launch that keeps no state
    // leaves no mark either: the record here says so
    const int fam = pl.state_family;
    b->state_engine = pl.skip_mark ? -1 : ((p.member_mode && b->sitters && b->state_engine != fam) ? -2 : fam);
    if (first) { b->last_kernel = pl.family; b->last_hblock = pl.hb; b->last_lane_shape = pl.lane_shape; rsqp_plan_words(pl, b->last_plan); }
    hipError_t e = rsqp_launch_small_qp(knobs_of(b, lp), pl, p, b->nq, max_nWSR, b->stream);
    if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, std::string("QP kernel launch: ") + hipGetErrorString(e));
    // rsqp_batch_set_handover: the members a hs071-scale tableau kernel gave up on go to the null-space kernel right behind it, with
    // the budget of the launch afresh (nWSR_in of rsqp_solve's retry). The records above stay what the tableau launch left: the
    // next call goes to the tableau kernel first again, and a member taken over has left its state block to it
    if (b->handover && (pl.family == 1 || pl.family == 2)) {
        e = rsqp_launch_small_handover(knobs_of(b, lp), plan_of(b, p, mode, lp, true), pl, p, b->nq, max_nWSR, b->handed.p, b->stream);
        if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, std::string("hand-over launch: ") + hipGetErrorString(e));
        b->results_foreign = true;   // (a member taken over: results of the null-space kernel, a state block that says "not initialised")
    }
    return RSQP_OK;
}

int begin_handover(rsqp_batch *b) {
    b->handed_valid = b->handover;
    if (!b->handover) return RSQP_OK;
    if (!b->handed.p) HIPCHK(b->handed.alloc((size_t)b->nq + 1));
    HIPCHK(hipMemsetAsync(b->handed.p, 0, sizeof(int) * ((size_t)b->nq + 1), b->stream));
    return RSQP_OK;
}
}  // namespace rsqp_batch_units

extern "C" int rsqp_batch_set_warm_start(rsqp_batch *b, const double *x0, const double *y0, const int *guess_b) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    if (guess_b)
        for (long long k = 0; k < b->sumV; k++)
            if (guess_b[k] < -1 || guess_b[k] > 1) return fail(RSQP_ERR_ARG, "rsqp_batch_set_warm_start: guess_b entries are -1, 0 or +1");
    int rc = ensure_warm_pools(b);
    if (rc != RSQP_OK) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    if (x0) HIPCHK(b->wx0.upload(x0, b->sumV));
    if (y0) HIPCHK(b->wy0.upload(y0, b->sumV + b->sumC));
    if (guess_b) HIPCHK(b->wgb.upload(guess_b, b->sumV));
    b->have_x0 = x0 != nullptr; b->have_y0 = y0 != nullptr; b->have_gb = guess_b != nullptr;
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_options(rsqp_batch *b, int qp_maxiter) {
    if (!b || qp_maxiter < 0) return fail(RSQP_ERR_ARG, "rsqp_batch_set_options");
    b->qp_maxiter = qp_maxiter;
    return RSQP_OK;
}

extern "C" int rsqp_batch_solve(rsqp_batch *b, int mode, int max_nWSR) {
    if (!b || mode < 0 || mode > 3 || max_nWSR < 0) return fail(RSQP_ERR_ARG, "rsqp_batch_solve");
    HIPCHK(hipSetDevice(b->device));
    QPPools p = pools_of(b, false);
    if (mode == RSQP_MODE_WARM_REINIT) {   // what rsqp_batch_set_warm_start gave; nothing given: init(.., nWSR, 0, 0, 0, 0)
        if (b->have_x0) p.x0 = b->wx0.p;
        if (b->have_y0) p.y0 = b->wy0.p;
        if (b->have_gb) p.guess_b = b->wgb.p;
    }
    int rc = begin_handover(b);
    if (rc != RSQP_OK) return rc;
    if (!b->timing) HIPCHK(hipEventRecord(b->ev0, b->stream));
    // (a warm re-initialisation reads the warm-start pools, whoever wrote the result pools)
    // (a hot start on new vectors goes there with rsqp_batch_set_lane_hot on as well: the plan reads the level)
    const bool warm = mode == RSQP_MODE_WARM_REINIT ? (b->lane_warm && !b->handover) : lane_warm_ok(b);
    if ((rc = launch_batch(b, p, mode, max_nWSR, true, false, warm ? lane_warm_level(b) : 0)) != RSQP_OK) return rc;
    b->cert_lp = false;
    if (!b->timing) HIPCHK(hipEventRecord(b->ev1, b->stream));
    return RSQP_OK;
}

extern "C" int rsqp_batch_get_last_kernel(const rsqp_batch *b) { return b ? b->last_kernel : -1; }
extern "C" int rsqp_batch_get_lane_hblock(const rsqp_batch *b) { return b ? b->last_hblock : 0; }
extern "C" int rsqp_batch_get_lane_shape(const rsqp_batch *b) { return b ? b->last_lane_shape : 0; }
extern "C" int rsqp_batch_get_last_plan(const rsqp_batch *b, int *out, int nout) {
    if (!b || !out || nout != RSQP_PLAN_OUT_WORDS) return fail(RSQP_ERR_ARG, "rsqp_batch_get_last_plan");
    if (b->last_kernel < 0) return fail(RSQP_ERR_ARG, "rsqp_batch_get_last_plan: the batch has not launched yet");
    std::copy(b->last_plan, b->last_plan + RSQP_PLAN_OUT_WORDS, out);
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_keep_state(rsqp_batch *b, int keep) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    b->keep_state = keep != 0;
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_lane_warm(rsqp_batch *b, int on) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    b->lane_warm = on != 0;
    return RSQP_OK;
}
extern "C" int rsqp_batch_get_lane_warm(const rsqp_batch *b) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    return b->lane_warm ? 1 : 0;
}

extern "C" int rsqp_batch_set_lane_hot(rsqp_batch *b, int on) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    b->lane_hot = on != 0;
    return RSQP_OK;
}
extern "C" int rsqp_batch_get_lane_hot(const rsqp_batch *b) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    return b->lane_hot ? 1 : 0;
}

extern "C" int rsqp_batch_set_handover(rsqp_batch *b, int on) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    b->handover = on != 0;
    return RSQP_OK;
}

extern "C" int rsqp_batch_get_handover(rsqp_batch *b, int *handed, int *count) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (!b->handed_valid) {      // the last call ran with the switch off (or nothing has run): nobody was handed over
        if (handed) std::fill(handed, handed + b->nq, 0);
        if (count) *count = 0;
        return RSQP_OK;
    }
    if (handed) HIPCHK(b->handed.download(handed, b->nq));
    if (count) HIPCHK(hipMemcpy(count, b->handed.p + b->nq, sizeof(int), hipMemcpyDeviceToHost));
    return RSQP_OK;
}

extern "C" int rsqp_batch_sync(rsqp_batch *b) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipStreamSynchronize(b->stream));
    return RSQP_OK;
}

extern "C" float rsqp_batch_last_solve_ms(rsqp_batch *b) {
    if (!b) return -1.f;
    if (hipEventSynchronize(b->ev1) != hipSuccess) return -1.f;
    float ms = -1.f;
    if (hipEventElapsedTime(&ms, b->ev0, b->ev1) != hipSuccess) return -1.f;
    b->last_ms = ms;
    return ms;
}

extern "C" int rsqp_batch_timer_start(rsqp_batch *b) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipEventRecord(b->ev2, b->stream));
    b->timing = true;
    return RSQP_OK;
}
extern "C" float rsqp_batch_timer_stop_ms(rsqp_batch *b) {
    if (!b) return -1.f;
    float ms = -1.f;
    b->timing = false;
    if (hipEventRecord(b->ev3, b->stream) != hipSuccess) return -1.f;
    if (hipEventSynchronize(b->ev3) != hipSuccess) return -1.f;
    if (hipEventElapsedTime(&ms, b->ev2, b->ev3) != hipSuccess) return -1.f;
    return ms;
}

extern "C" int rsqp_batch_get_results(rsqp_batch *b, double *x, double *y, int *ws_b, int *ws_c, int *status,
                                      int *nWSR, double *obj) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (x) HIPCHK(b->x.download(x, b->sumV));
    if (y) HIPCHK(b->y.download(y, b->sumV + b->sumC));
    if (ws_b) HIPCHK(b->ws_b.download(ws_b, b->sumV));
    if (ws_c) HIPCHK(b->ws_c.download(ws_c, b->sumC));
    if (status) {
        std::vector<int> sw(b->nq), rt(b->nq);
        HIPCHK(b->status.download(sw.data(), b->nq)); HIPCHK(b->ret.download(rt.data(), b->nq));
        for (int q = 0; q < b->nq; q++) status[q] = exitflag_of(sw[q], rt[q]);
    }
    if (nWSR) HIPCHK(b->nwsr.download(nWSR, b->nq));
    if (obj) HIPCHK(b->obj.download(obj, b->nq));
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_results(rsqp_batch *b, const double *x, const double *y, const int *ws_b, const int *ws_c) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (x) HIPCHK(b->x.upload(x, b->sumV));
    if (y) HIPCHK(b->y.upload(y, b->sumV + b->sumC));
    if (ws_b) HIPCHK(b->ws_b.upload(ws_b, b->sumV));
    if (ws_c) HIPCHK(b->ws_c.upload(ws_c, b->sumC));
    if (x || y || ws_b || ws_c) b->results_foreign = true;
    return RSQP_OK;
}

extern "C" int rsqp_batch_test_optimality(rsqp_batch *b, rsqp_optimality_status *out, int *ok) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    if (!b->Ax.p) {
        HIPCHK(b->Ax.alloc(b->sumC)); HIPCHK(b->ATy.alloc(b->sumV)); HIPCHK(b->Hx.alloc(b->sumV));
        HIPCHK(b->kkt.alloc(6 * (size_t)b->nq)); HIPCHK(b->Wb.alloc(b->sumV)); HIPCHK(b->Wc.alloc(b->sumC));
        std::vector<int> kv(b->nq), kc(b->nq);
        std::vector<long long> ov(b->nq), oc(b->nq);
        for (int q = 0; q < b->nq; q++) {
            kv[q] = b->desc[q].nV; kc[q] = b->desc[q].nC; ov[q] = b->desc[q].offV; oc[q] = b->desc[q].offC;
        }
        HIPCHK(b->kV.from(kv)); HIPCHK(b->kC.from(kc)); HIPCHK(b->koV.from(ov)); HIPCHK(b->koC.from(oc));
    }
    QPPools p = pools_of(b, b->cert_lp);   // behind an LP call: H absent (and no regVal term: the certificate reads no hreg)
    RsqpKktArgs a;
    std::memset(&a, 0, sizeof(a));
    a.nV = b->kV.p; a.nC = b->kC.p; a.offV = b->koV.p; a.offC = b->koC.p;
    a.x = b->x.p; a.y = b->y.p; a.g = b->g.p; a.lb = b->lb.p; a.ub = b->ub.p; a.lbA = b->lbA.p; a.ubA = b->ubA.p;
    a.Ax = b->Ax.p; a.ATy = b->ATy.p; a.Hx = b->Hx.p; a.ws_b = b->ws_b.p; a.ws_c = b->ws_c.p;
    a.W_b = b->Wb.p; a.W_c = b->Wc.p; a.out = b->kkt.p;
    if (rsqp_launch_small_certificate(p, a, b->nq, b->Ax.p, b->ATy.p, b->Hx.p, b->stream) != hipSuccess)
        return fail(RSQP_ERR_DEVICE, "certificate launch failed");
    HIPCHK(hipStreamSynchronize(b->stream));
    std::vector<double> o(6 * (size_t)b->nq);
    HIPCHK(b->kkt.download(o.data(), o.size()));
    for (int q = 0; q < b->nq; q++) {
        if (out) {
            out[q].primal_violation = o[6 * q]; out[q].dual_violation = o[6 * q + 1];
            out[q].compl_violation = o[6 * q + 2]; out[q].stationarity_violation = o[6 * q + 3];
            out[q].KKT_error = o[6 * q + 4];
        }
        if (ok) ok[q] = o[6 * q + 5] != 0.0 ? RSQP_ERR_WORKING_SET : (o[6 * q + 4] > 1.0e-6 ? 0 : 1);
    }
    return RSQP_OK;
}

extern "C" int rsqp_batch_get_working_set(rsqp_batch *b, int *W_b, int *W_c) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!b->Wb.p) return fail(RSQP_ERR_ARG, "rsqp_batch_get_working_set: rsqp_batch_test_optimality has not run yet");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (W_b) HIPCHK(b->Wb.download(W_b, b->sumV));
    if (W_c) HIPCHK(b->Wc.download(W_c, b->sumC));
    return RSQP_OK;
}

// ---------------------------------------------------------------------------------
// fixed-stride result records on the device: what a rank contributes to the gather of a sharded batch
// (SURVEY 8(e)). Layout = restartsqp_amd/parallel.py pack_records:
//   {exitflag, nWSR, objective, KKT_error, x[nVmax], y_bounds[nVmax], y_constr[nCmax], ws_b[nVmax], ws_c[nCmax]}
// One thread per record entry; unused tail entries of a smaller problem are zero.
// ---------------------------------------------------------------------------------
namespace {
__global__ void pack_records_kernel(int nq, int nVmax, int nCmax, const QPDesc *__restrict__ desc,
                                    const double *__restrict__ x, const double *__restrict__ y,
                                    const int *__restrict__ ws_b, const int *__restrict__ ws_c,
                                    const int *__restrict__ status, const int *__restrict__ nwsr,
                                    const double *__restrict__ obj, const double *__restrict__ kkt,
                                    double *__restrict__ rec) {
    const int stride = 4 + 3 * nVmax + 2 * nCmax;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nq * stride) return;
    const int q = (int)(t / stride), e = (int)(t % stride);
    const QPDesc d = desc[q];
    double v = 0.0;
    if (e < 4) {
        if (e == 0) {   // exitflag_of() of rsqp_host.h: qpOASESInterface::get_status (src/qpOASESInterface.cpp:332-357)
            const int sw = status[q];
            v = sw >= 200 ? RSQP_QPERROR_UNBOUNDED : (sw >= 100 ? RSQP_QPERROR_INFEASIBLE : (sw == QPS_SOLVED ? RSQP_QP_OPTIMAL : RSQP_QPERROR_NOTINITIALISED + sw));
        } else if (e == 1) v = nwsr[q];
        else if (e == 2) v = obj[q];
        else v = kkt ? kkt[6 * q + 4] : 0.0;
    } else {
        int o = e - 4;
        if (o < nVmax) { if (o < d.nV) v = x[d.offV + o]; }
        else if ((o -= nVmax) < nVmax) { if (o < d.nV) v = y[d.offV + d.offC + o]; }
        else if ((o -= nVmax) < nCmax) { if (o < d.nC) v = y[d.offV + d.offC + d.nV + o]; }
        else if ((o -= nCmax) < nVmax) { if (o < d.nV) v = ws_b[d.offV + o]; }
        else { o -= nVmax; if (o < d.nC) v = ws_c[d.offC + o]; }
    }
    rec[t] = v;
}
}  // namespace

extern "C" int rsqp_batch_record_stride(const rsqp_batch *b) {
    return b ? 4 + 3 * b->nVmax + 2 * b->nCmax : -1;
}

extern "C" int rsqp_batch_pack_records_dev(rsqp_batch *b, double *rec_dev) {
    if (!b || !rec_dev) return fail(RSQP_ERR_ARG, "rsqp_batch_pack_records_dev");
    HIPCHK(hipSetDevice(b->device));
    const long long tot = (long long)b->nq * rsqp_batch_record_stride(b);
    hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, b->stream, b->nq, b->nVmax,
                       b->nCmax, b->d_desc.p, b->x.p, b->y.p, b->ws_b.p, b->ws_c.p, b->status.p, b->nwsr.p, b->obj.p,
                       b->kkt.p /* null until the certificate has run */, rec_dev);
    HIPCHK(hipGetLastError());
    return RSQP_OK;
}

extern "C" int rsqp_batch_pack_records_host(rsqp_batch *b, double *rec_host) {
    if (!b || !rec_host) return fail(RSQP_ERR_ARG, "rsqp_batch_pack_records_host");
    HIPCHK(hipSetDevice(b->device));
    const size_t tot = (size_t)b->nq * rsqp_batch_record_stride(b);
    int rc;
    if ((rc = ensure_scratch(b, tot)) != RSQP_OK || (rc = rsqp_batch_pack_records_dev(b, b->scratch.p)) != RSQP_OK) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));   // (rsqp_batch::scratch: free again behind this)
    HIPCHK(b->scratch.download(rec_host, tot));
    return RSQP_OK;
}

// (rsqp_host.h: the native RCCL call sites of rsqp_rccl.cpp reach the batch through these)
hipStream_t rsqp_batch_stream_internal(rsqp_batch *b) { return b->stream; }
int rsqp_batch_device_internal(const rsqp_batch *b) { return b->device; }
int rsqp_batch_nq_internal(const rsqp_batch *b) { return b ? b->nq : 0; }
