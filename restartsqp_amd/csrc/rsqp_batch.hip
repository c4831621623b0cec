// rsqp_batch.hip -- the batch of independent QPs of include/rsqp_hip.h (rsqp_batch_*), host side and the one-thread- or
// one-wavefront-per-member kernels that take optimizeQP's / optimizeLP's decisions between the solve launches.
//
// Host logic restated from the reference adapter src/qpOASESInterface.cpp as rsqp_api.hip restates it for one handle: the
// FIXED/VARIED warm-start dispatch (:137-224, :227-284, :817-833), handle_error (:686-758), status mapping (:332-357).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rsqp_host.h"
#include "rsqp_matrix.h"
#include "rsqp_sparse.h"

// =====================================================================================
// batch of independent QPs
// =====================================================================================
static_assert(RSQP_BATCH_MAX_V == RSQP_HBM_MAX_V && RSQP_BATCH_MAX_C == RSQP_HBM_MAX_C, "batch size limits of rsqp_hip.h and rsqp_internal.h");
struct rsqp_batch {
    int nq = 0, device = 0, nVmax = 0, nCmax = 0, uniV = -1, uniC = -1;
    bool uni_pat = false; int uni_annz = 0, uni_hnnz = 0; long long uni_state = 0;     // (QPPools::uni_pat)
    long long sumV = 0, sumC = 0, sumAnz = 0, sumHnz = 0, mat_bytes_max = 0;
    bool haveH = false;
    SmallKnobs kn = rsqp_small_knobs_from_env();
    // kernel family that wrote the members' hot-start states (see rsqp_solver::state_engine): >= 0 every member's, -1 nobody has one,
    // -2 the members differ -- word OPT_FAM of each says (a call some members sat out ran on another family)
    int state_engine = -1;
    int last_kernel = -1;                 // rsqp_batch_get_last_kernel
    bool hbm = false;                     // images beyond the LDS of a CU: every member on the HBM-resident kernel (qp_small_hbm.hip)
    bool h_sym = true;                    // every H symmetric value by value (the tableau kernel of qp_tiny.hip may take the batch)
    std::vector<int> h_Hjc, h_Hir;        // host copy of the H patterns (re-examined when the values change), small batches only
    std::vector<long long> h_Huoff;       //   (the caller's layout: member q's entries start at h_Huoff[q])
    std::vector<char> h_symq;             //   member q's H is symmetric; h_sym = all of them (rsqp_batch_set_matrix_values_of)
    ValueFold Afold, Hfold;               // members given in a non-canonical layout (PooledCsc): the pools hold the canonical form
    std::vector<QPDesc> desc;
    std::vector<int> h_csr_perm;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    DevBuf<QPDesc> d_desc;
    DevBuf<int> Ajc, Air, Arp, Aci, perm, Hjc, Hir;
    DevBuf<double> Aval, Arv, Hval;
    DevBuf<double> g, lb, ub, lbA, ubA, x, y, obj, state;
    DevBuf<int> ws_b, ws_c, status, ret, nwsr, nflips;
    DevBuf<double> Ax, ATy, Hx, kkt;
    DevBuf<int> Wb, Wc, kV, kC;
    DevBuf<double> recbuf;   // rsqp_batch_pack_records_host
    DevBuf<long long> koV, koC;
    // warm re-initialisation inputs (RSQP_MODE_WARM_REINIT), pooled like the vectors; allocated at first use. have_*: what
    // rsqp_batch_set_warm_start gave (rsqp_batch_solve); rsqp_batch_optimize_qp fills the same pools on the device
    DevBuf<double> wx0, wy0;
    DevBuf<int> wgb;
    bool have_x0 = false, have_y0 = false, have_gb = false;
    // optimizeQP per member (rsqp_batch_optimize_qp): nq ints each, in one block -- firstQPsolved_, old / new matrix status, mode of
    // the call's first solve, mode of its rescue solve (-1: none), kind of rescue, count of the first solve
    // rsqp_batch_optimize_lp adds: mode the first solve is LAUNCHED with (a flip is a plain init there), mode of the proximal step
    // (-1: the member is unsolved and takes none)
    // per member across calls as well: OPT_UPD the update mark (Update_A / Update_H of rsqp_batch_set_matrix_values_of and rsqp_batch_handler_set_matrices, and of
    // rsqp_batch_set_matrix_values for a member that sat out the call that took the batch-wide mats_updated), OPT_FAM 1 + the kernel
    // family that wrote the member's stored state (0 none; read while state_engine == -2)
    enum { OPT_FIRST = 0, OPT_OLD, OPT_NEW, OPT_MODE, OPT_RMODE, OPT_RESCUE, OPT_N1, OPT_LMODE, OPT_PMODE, OPT_UPD, OPT_FAM, OPT_WORDS };
    DevBuf<int> opt;
    // rsqp_batch_set_members: who takes part in the optimize calls. The kernels get the mask only while somebody sits out; with the
    // default and with an all-ones mask the calls issue what they issued before there was a mask
    DevBuf<int> take;
    bool sitters = false;                 // somebody sits out
    // rsqp_batch_set_vectors_of / rsqp_batch_set_matrix_values_of: the caller's arrays and mask on the device, allocated at first use,
    // and where member q's entries start in a non-canonical caller layout (Afold / Hfold)
    DevBuf<double> stage;
    DevBuf<int> named;
    DevBuf<long long> Auoff, Huoff;
    // the QPhandler layer (rsqp_batch_handler_*): the NLP bounds of the members (x_l, x_u in the NLP layout, c_l, c_u in the
    // constraint layout), and the staging of host-pointer calls, allocated at first use -- the caller's arrays are packed into one
    // pinned block and cross in one copy each way (the stage of the named setters is too small for nq-sized words)
    DevBuf<double> h_xl, h_xu, h_cl, h_cu, h_in, h_out;
    double *h_pin = nullptr;              // pinned, max(words of an update, words of a step, words of a matrix call)
    size_t h_pin_words = 0;
    long long sumN = 0;                   // NLP variables of the batch: sumV - 2 sumC
    bool have_problem = false;            // rsqp_batch_handler_set_problem has run
    // rsqp_batch_handler_set_matrices: h_jn[q] = entries of columns [0, n_q) of member q's A in the caller's layout (from
    // rsqp_batch_create; sumJ of them in all). At the first call: where member q's entries start in jac (hm_joff, nq + 1), the
    // inverse of perm (hm_inv: CSC slot -> CSR slot) and the staging of host-pointer calls (hm_in: jac | hess | what)
    std::vector<int> h_jn;
    long long sumJ = 0;
    bool uni_jn = false;                  // a one-pattern batch in a canonical layout: every member has h_jn[0] entries in jac
    bool hm_ready = false;
    DevBuf<long long> hm_joff;
    DevBuf<int> hm_inv;
    DevBuf<double> hm_in;
    // the symmetry of every member's H on the device (batches of at most 8 variables): the device's copy of h_symq, stale after a
    // host setter has re-examined members, and the host-mapped word a verdict that differs from the copy is flagged through
    DevBuf<char> d_symq;
    bool symq_stale = true;
    int *sym_host = nullptr, *sym_dev = nullptr;
    // optimizeLP per member (rsqp_batch_optimize_lp): the members' descriptors with H absent and hreg = regVal of the member's last
    // init (written on the device, kept across hot starts), and the pool of the proximal step's gradients g - regVal x
    DevBuf<QPDesc> d_desc_lp;
    DevBuf<double> g_lp;
    int lp_maxiter = 100;                 // rsqp_batch_set_lp_options
    int last_kind = 0;                    // 0 no optimize call yet, 1 the last one was rsqp_batch_optimize_qp, 2 rsqp_batch_optimize_lp
    bool cert_lp = false;                 // the results in the pools are an LP call's: rsqp_batch_test_optimality certifies the LP
    // nWSR_used of the members, written by the kernels straight into host-mapped memory: ready behind the call's one wait, no copy
    // (and no second wait) behind it
    int *used_host = nullptr, *used_dev = nullptr;
    int qp_maxiter = 1000;                // rsqp_batch_set_options
    bool mats_updated = false;            // rsqp_batch_set_matrix_values since the last optimize call (Update_A / Update_H of everybody)
    bool opt_started = false;             // an rsqp_batch_optimize_qp has run: members are in different states from here on
    float last_ms = 0.f;
    bool keep_state = true;
    bool timing = false;   // between timer_start and timer_stop: no per-launch events (they cost ~10 us of stream time each)
    ~rsqp_batch() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
        if (stream) (void)hipStreamDestroy(stream);
        if (used_host) (void)hipHostFree(used_host);
        if (h_pin) (void)hipHostFree(h_pin);
        if (sym_host) (void)hipHostFree(sym_host);
    }
};

namespace {
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
    return p;
}
// the knobs of a launch: LP launches stay off the register-resident tableau kernels, which answer RET_SETUP_FAILED on a pivot in
// their rounding band and have no hand-over inside a batch (a single handle re-solves on the Givens kernel, rsqp_solve)
SmallKnobs knobs_of(const rsqp_batch *b, bool lp) {
    SmallKnobs k = b->kn;
    if (lp) k.no_tiny = 2;   // (nor the mid-size tableau kernel, which would hand every LP member back: no H, hreg != 0)
    return k;
}
}  // namespace

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
        for (int q = 0; q < nq; q++) {
            const QPDesc &d = b->desc[q];
            b->h_symq[q] = small_csc_symmetric(d.nV, Hjc + d.offHjc, Hir + d.offHnz, Hval + d.offHnz);
            b->h_sym = b->h_sym && b->h_symq[q];
        }
    } else if (b->haveH) b->h_sym = false;
    b->sumV = offV; b->sumC = offC; b->sumAnz = offAnz; b->sumHnz = offHnz;
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
    if (Aval) {
        HIPCHK(b->Afold.refresh(Aval, b->Aval, (int)b->sumAnz, b->stream));
        if (rsqp_launch_gather((int)b->sumAnz, b->perm.p, b->Aval.p, b->Arv.p, b->stream) != hipSuccess)
            return fail(RSQP_ERR_DEVICE, "gather launch failed");
    }
    if (Hval && b->haveH) {
        HIPCHK(b->Hfold.refresh(Hval, b->Hval, (int)b->sumHnz, b->stream));
        if (!b->h_Hjc.empty()) {
            b->h_sym = true; b->symq_stale = true;
            for (int q = 0; q < b->nq; q++) {
                const QPDesc &d = b->desc[q];
                b->h_symq[q] = small_csc_symmetric(d.nV, b->h_Hjc.data() + d.offHjc, b->h_Hir.data() + b->h_Huoff[q], Hval + b->h_Huoff[q]);
                b->h_sym = b->h_sym && b->h_symq[q];
            }
        }
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    // (qpOASESInterface.cpp:407-409, 427-429: counts for the members whose first QP is solved -- the plan kernel looks at that)
    if (Aval || (Hval && b->haveH)) b->mats_updated = true;
    return RSQP_OK;
}

// ---------------------------------------------------------------------------------
// members of a batch on their own: who takes part in the optimize calls, and setters that write the named members only
// ---------------------------------------------------------------------------------
namespace {
int ensure_opt(rsqp_batch *b) {
    if (!b->opt.p) HIPCHK(b->opt.alloc((size_t)rsqp_batch::OPT_WORDS * b->nq));
    return RSQP_OK;
}

// up to five pooled arrays in one launch: entry e of the concatenation belongs to array s (end[s-1] <= e < end[s]) and there to the
// member its position says; it is copied iff that member is named. uni[s] > 0: every member has uni[s] entries in array s; else the
// member is searched in the offsets `kind[s]` names -- of the descriptors (0 offV, 1 offC, 2 offAnz, 3 offHnz), or uoff[s] (4: a
// caller's layout that is not the canonical one). mark != null: the update mark of every named member whose first QP is solved
// (qpOASESInterface.cpp:407-409, 427-429). Consecutive lanes read and write consecutive entries.
struct MaskedCopy {
    int nseg, nq;
    long long end[5];
    int uni[5], kind[5];
    const double *src[5];
    double *dst[5];
    const long long *uoff[5];
    const QPDesc *desc;
    const int *named;
    int *mark;            // the OPT_UPD words of the opt block
    const int *first;     // the OPT_FIRST words
};
__device__ inline long long member_start(const MaskedCopy &a, int s, int q) {
    switch (a.kind[s]) {
    case 0: return a.desc[q].offV;
    case 1: return a.desc[q].offC;
    case 2: return a.desc[q].offAnz;
    case 3: return a.desc[q].offHnz;
    default: return a.uoff[s][q];
    }
}
__global__ void __launch_bounds__(256) batch_masked_copy_kernel(MaskedCopy a) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.mark && e < a.nq && a.named[e] != 0 && a.first[e] != 0) a.mark[e] = 1;
    if (a.nseg <= 0 || e >= a.end[a.nseg - 1]) return;
    int s = 0;
    while (e >= a.end[s]) s++;                        // (s < nseg: e is below the last end)
    const long long k = e - (s > 0 ? a.end[s - 1] : 0);
    int q;
    if (a.uni[s] > 0) q = (int)(k / a.uni[s]);
    else {                                            // the last member that starts at or before k (members without entries own none)
        int lo = 0, hi = a.nq - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (member_start(a, s, mid) <= k) lo = mid; else hi = mid - 1;
        }
        q = lo;
    }
    if (a.named[q] != 0) a.dst[s][k] = a.src[s][k];
}

// the mask on the device; *count = members named
int upload_mask(rsqp_batch *b, DevBuf<int> &dst, const int *mask, int *count) {
    std::vector<int> m(b->nq);
    int n = 0;
    for (int q = 0; q < b->nq; q++) n += (m[q] = mask[q] != 0 ? 1 : 0);
    *count = n;
    if (!dst.p) HIPCHK(dst.alloc(b->nq));
    HIPCHK(dst.upload(m.data(), b->nq));
    return RSQP_OK;
}
int ensure_stage(rsqp_batch *b) {
    const size_t need = (size_t)std::max<long long>(3 * b->sumV + 2 * b->sumC, b->Afold.unnz + (b->haveH ? b->Hfold.unnz : 0));
    if (!b->stage.p) HIPCHK(b->stage.alloc(need, false));
    return RSQP_OK;
}
void add_segment(MaskedCopy &a, long long n, int uni, int kind, const double *src, double *dst, const long long *uoff) {
    const int s = a.nseg++;
    a.end[s] = (s > 0 ? a.end[s - 1] : 0) + n;
    a.uni[s] = uni; a.kind[s] = kind; a.src[s] = src; a.dst[s] = dst; a.uoff[s] = uoff;
}
int launch_masked_copy(rsqp_batch *b, MaskedCopy &a) {
    a.nq = b->nq; a.desc = b->d_desc.p; a.named = b->named.p;
    const long long n = std::max<long long>(a.nseg > 0 ? a.end[a.nseg - 1] : 0, a.mark ? b->nq : 0);
    if (n <= 0) return RSQP_OK;
    hipLaunchKernelGGL(batch_masked_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, a);
    HIPCHK(hipGetLastError());
    return RSQP_OK;
}
}  // namespace

extern "C" int rsqp_batch_set_members(rsqp_batch *b, const int *take_part) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    int n = b->nq;
    if (take_part) {   // (everybody named: the calls run as they do without a mask)
        HIPCHK(hipSetDevice(b->device));
        const int rc = upload_mask(b, b->take, take_part, &n);
        if (rc != RSQP_OK) return rc;
    }
    b->sitters = n < b->nq;
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_vectors_of(rsqp_batch *b, const int *members, const double *g, const double *lb, const double *ub,
                                         const double *lbA, const double *ubA) {
    if (!b || !g || !lb || !ub || (b->sumC > 0 && (!lbA || !ubA))) return fail(RSQP_ERR_ARG, "rsqp_batch_set_vectors_of");
    if (!members) return rsqp_batch_set_vectors(b, g, lb, ub, lbA, ubA);
    HIPCHK(hipSetDevice(b->device));
    int rc, n = 0;
    if ((rc = upload_mask(b, b->named, members, &n)) != RSQP_OK || n == 0) return rc;
    if ((rc = ensure_stage(b)) != RSQP_OK) return rc;
    const long long sV = b->sumV, sC = b->sumC;
    double *const st = b->stage.p;
    HIPCHK(hipMemcpy(st, g, sizeof(double) * sV, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(st + sV, lb, sizeof(double) * sV, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(st + 2 * sV, ub, sizeof(double) * sV, hipMemcpyHostToDevice));
    if (sC > 0) {
        HIPCHK(hipMemcpy(st + 3 * sV, lbA, sizeof(double) * sC, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(st + 3 * sV + sC, ubA, sizeof(double) * sC, hipMemcpyHostToDevice));
    }
    MaskedCopy a;
    std::memset(&a, 0, sizeof(a));
    const int uV = b->uniV > 0 ? b->uniV : 0, uC = b->uniC > 0 ? b->uniC : 0;
    add_segment(a, sV, uV, 0, st, b->g.p, nullptr);
    add_segment(a, sV, uV, 0, st + sV, b->lb.p, nullptr);
    add_segment(a, sV, uV, 0, st + 2 * sV, b->ub.p, nullptr);
    add_segment(a, sC, uC, 1, st + 3 * sV, b->lbA.p, nullptr);
    add_segment(a, sC, uC, 1, st + 3 * sV + sC, b->ubA.p, nullptr);
    if ((rc = launch_masked_copy(b, a)) != RSQP_OK) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));   // (the staging pool is free again)
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_matrix_values_of(rsqp_batch *b, const int *members, const double *Aval, const double *Hval) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!members) return rsqp_batch_set_matrix_values(b, Aval, Hval);
    if (!b->haveH) Hval = nullptr;
    HIPCHK(hipSetDevice(b->device));
    int rc, n = 0;
    if ((rc = upload_mask(b, b->named, members, &n)) != RSQP_OK || n == 0 || (!Aval && !Hval)) return rc;
    if ((rc = ensure_stage(b)) != RSQP_OK || (rc = ensure_opt(b)) != RSQP_OK) return rc;
    const long long uA = b->Afold.unnz, uH = b->Hfold.unnz;
    double *const st = b->stage.p;
    MaskedCopy a;
    std::memset(&a, 0, sizeof(a));
    // (a canonical layout: straight into the pools; else into the caller's values, which are folded behind the copy)
    if (Aval) {
        HIPCHK(hipMemcpy(st, Aval, sizeof(double) * uA, hipMemcpyHostToDevice));
        if (b->Afold.canon) add_segment(a, uA, b->uni_pat ? b->uni_annz : 0, 2, st, b->Aval.p, nullptr);
        else add_segment(a, uA, 0, 4, st, b->Afold.uval.p, b->Auoff.p);
    }
    if (Hval) {
        HIPCHK(hipMemcpy(st + uA, Hval, sizeof(double) * uH, hipMemcpyHostToDevice));
        if (b->Hfold.canon) add_segment(a, uH, b->uni_pat ? b->uni_hnnz : 0, 3, st + uA, b->Hval.p, nullptr);
        else add_segment(a, uH, 0, 4, st + uA, b->Hfold.uval.p, b->Huoff.p);
    }
    a.mark = b->opt.p + (size_t)rsqp_batch::OPT_UPD * b->nq; a.first = b->opt.p + (size_t)rsqp_batch::OPT_FIRST * b->nq;
    if ((rc = launch_masked_copy(b, a)) != RSQP_OK) return rc;
    if (Aval) {
        if (!b->Afold.canon) HIPCHK(b->Afold.sum(b->Aval, (int)b->sumAnz, b->stream));
        if (rsqp_launch_gather((int)b->sumAnz, b->perm.p, b->Aval.p, b->Arv.p, b->stream) != hipSuccess)
            return fail(RSQP_ERR_DEVICE, "gather launch failed");
    }
    if (Hval) {
        if (!b->Hfold.canon) HIPCHK(b->Hfold.sum(b->Hval, (int)b->sumHnz, b->stream));
        if (!b->h_Hjc.empty()) {   // the named members' symmetry anew, from the values given
            b->h_sym = true; b->symq_stale = true;
            for (int q = 0; q < b->nq; q++) {
                const QPDesc &d = b->desc[q];
                if (members[q] != 0)
                    b->h_symq[q] = small_csc_symmetric(d.nV, b->h_Hjc.data() + d.offHjc, b->h_Hir.data() + b->h_Huoff[q], Hval + b->h_Huoff[q]);
                b->h_sym = b->h_sym && b->h_symq[q];
            }
        }
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return RSQP_OK;
}

// ---------------------------------------------------------------------------------
// the QPhandler of every member on the device (src/QPhandler.cpp; rsqp_batch_handler_* of rsqp_hip.h): the five QP vectors from an
// NLP iterate, and what Algorithm reads back from a solved QP. Member q: m = nC constraints, n = nV - 2 nC NLP variables, QP
// variables (p, u, v) (:39-51); its NLP entries start at offV - 2 offC
// ---------------------------------------------------------------------------------
namespace {
constexpr double HANDLER_INF = 1.0e18;   // INF of the reference (Utils.hpp:35)

// one thread per entry of the concatenation g | lb | ub | lbA | ubA; the member of an entry as in batch_masked_copy_kernel: a
// division in a one-shape batch (uniV > 0), else the last member whose offset is at or before the entry. Every formula is one
// subtraction and one fmax / fmin, as the host states them (QPhandler.cpp:167-201, 272-297, 342-368, 430-463, 533-567)
struct HandlerUpdate {
    int nq, uniV, uniC;   // uniV > 0: every member is uniV x uniC
    int sumV, sumC;
    const QPDesc *desc;
    const int *what;
    const double *delta, *rho, *x_k, *grad, *c_k;   // the iterate (rsqp_handler_iterate)
    const double *x_l, *x_u, *c_l, *c_u;            // rsqp_batch_handler_set_problem
    double *g, *lb, *ub, *lbA, *ubA;
};
__global__ void __launch_bounds__(256) batch_handler_update_kernel(HandlerUpdate a) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 3LL * a.sumV + 2LL * a.sumC) return;
    const bool isV = e < 3LL * a.sumV;
    int s, k;
    if (isV) { s = (e >= a.sumV) + (e >= 2LL * a.sumV); k = (int)(e - (long long)s * a.sumV); }
    else { k = (int)(e - 3LL * a.sumV); s = 3 + (k >= a.sumC); if (s == 4) k -= a.sumC; }
    int q, nV, nC, offV, offC;
    if (a.uniV > 0) {
        nV = a.uniV; nC = a.uniC;
        q = isV ? k / nV : k / nC;       // (a constraint entry exists: nC > 0)
        offV = q * nV; offC = q * nC;
    } else {
        int lo = 0, hi = a.nq - 1;       // (members without constraints own no entry of lbA / ubA)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((isV ? a.desc[mid].offV : a.desc[mid].offC) <= k) lo = mid; else hi = mid - 1;
        }
        q = lo;
        nV = a.desc[q].nV; nC = a.desc[q].nC; offV = a.desc[q].offV; offC = a.desc[q].offC;
    }
    const int W = a.what[q];
    if (W == 0) return;
    const bool set = (W & RSQP_HU_SET) != 0;
    if (!isV) {
        if (s == 3) { if (set || (W & RSQP_HU_BOUNDS)) a.lbA[k] = a.c_l[k] - a.c_k[k]; }
        else if (set || ((W & RSQP_HU_BOUNDS) && (W & RSQP_HU_UBA))) a.ubA[k] = a.c_u[k] - a.c_k[k];
        return;
    }
    const int i = k - offV, n = nV - 2 * nC, j = offV - 2 * offC + i;   // j: the entry in the NLP layout (i < n)
    if (i >= n) {            // a slack variable
        if (s == 0) { if (set || (W & RSQP_HU_PENALTY)) a.g[k] = a.rho[q]; }
        else if (set) { if (s == 1) a.lb[k] = 0.0; else a.ub[k] = HANDLER_INF; }
        return;
    }
    if (s == 0) {
        if (set) a.g[k] = a.grad ? a.grad[j] : 0.0;
        else if ((W & RSQP_HU_GRAD) && a.grad) a.g[k] = a.grad[j];
    } else if (set || (W & (RSQP_HU_BOUNDS | RSQP_HU_DELTA))) {
        if (s == 1) a.lb[k] = fmax(a.x_l[j] - a.x_k[j], -a.delta[q]);
        else a.ub[k] = fmin(a.x_u[j] - a.x_k[j], a.delta[q]);
    }
}

// G lanes per member (8 for hs071-scale batches, else a wavefront): the copies walk the member's entries G at a time, norm_p is a
// maximum over the sub-group (exact in any order), infea_model a sum over it. Lanes past the last member skip the loops and stay
// in the shuffles. Any output may be null
template <int G>
__global__ void __launch_bounds__(256)
batch_handler_step_kernel(int nq, const QPDesc *__restrict__ desc, const double *__restrict__ x, const double *__restrict__ y,
                          double *__restrict__ p, double *__restrict__ lam_c, double *__restrict__ lam_x,
                          double *__restrict__ infea, double *__restrict__ norm_p) {
    const int q = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) / G), lane = (int)threadIdx.x % G;
    double mx = 0.0, sm = 0.0;
    if (q < nq) {
        const int nV = desc[q].nV, nC = desc[q].nC, offV = desc[q].offV, offC = desc[q].offC;
        const int n = nV - 2 * nC, offN = offV - 2 * offC, offY = offV + offC;
        for (int i = lane; i < n; i += G) {
            const double v = x[offV + i];
            if (p) p[offN + i] = v;
            if (lam_x) lam_x[offN + i] = y[offY + i];
            mx = fmax(mx, fabs(v));
        }
        if (lam_c)
            for (int i = lane; i < nC; i += G) lam_c[offC + i] = y[offY + nV + i];
        for (int i = n + lane; i < nV; i += G) sm += fabs(x[offV + i]);
    }
    for (int o = G / 2; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, o, G));
        sm += __shfl_xor(sm, o, G);
    }
    if (q < nq && lane == 0) {
        if (norm_p) norm_p[q] = mx;
        if (infea) infea[q] = sm;
    }
}

// words (doubles) of the packed block of a host-pointer update: delta | rho | x_k | grad | c_k | what (ints); a step's is smaller
long long handler_in_words(const rsqp_batch *b) { return 2LL * b->nq + 2 * b->sumN + b->sumC + (b->nq + 1) / 2; }
// the pinned block holds `words` doubles (it is free: every call that uses it waits for its copy)
int ensure_pinned(rsqp_batch *b, size_t words) {
    if (b->h_pin_words >= words) return RSQP_OK;
    if (b->h_pin) HIPCHK(hipHostFree(b->h_pin));
    b->h_pin = nullptr; b->h_pin_words = 0;
    HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&b->h_pin), sizeof(double) * std::max<size_t>(words, 1), hipHostMallocDefault));
    b->h_pin_words = words;
    return RSQP_OK;
}
int ensure_handler_stage(rsqp_batch *b) {
    const size_t w = (size_t)handler_in_words(b);
    if (!b->h_in.p) { HIPCHK(b->h_in.alloc(w, false)); HIPCHK(b->h_out.alloc(w, false)); }
    return ensure_pinned(b, w);
}
}  // namespace

extern "C" int rsqp_batch_handler_set_problem(rsqp_batch *b, const double *x_l, const double *x_u, const double *c_l, const double *c_u) {
    if (!b || !x_l || !x_u || (b->sumC > 0 && (!c_l || !c_u))) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_set_problem");
    for (int q = 0; q < b->nq; q++)
        if (b->desc[q].nV < 2 * b->desc[q].nC + 1)
            return fail(RSQP_ERR_ARG, "rsqp_batch_handler_set_problem: member " + std::to_string(q) + " has nV < 2 nC + 1: not the (p, u, v) shape of QPhandler");
    HIPCHK(hipSetDevice(b->device));
    b->sumN = b->sumV - 2 * b->sumC;
    HIPCHK(b->h_xl.alloc(b->sumN, false)); HIPCHK(b->h_xu.alloc(b->sumN, false));
    HIPCHK(b->h_cl.alloc(b->sumC, false)); HIPCHK(b->h_cu.alloc(b->sumC, false));
    HIPCHK(b->h_xl.upload(x_l, b->sumN)); HIPCHK(b->h_xu.upload(x_u, b->sumN));
    HIPCHK(b->h_cl.upload(c_l, b->sumC)); HIPCHK(b->h_cu.upload(c_u, b->sumC));
    b->have_problem = true;
    return RSQP_OK;
}

extern "C" int rsqp_batch_handler_update(rsqp_batch *b, const rsqp_handler_iterate *it, int on_device) {
    if (!b || !it || !it->what || !it->delta || !it->rho || !it->x_k || (b->sumC > 0 && !it->c_k))
        return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update: what, delta, rho, x_k (and c_k) are required");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_update: rsqp_batch_handler_set_problem has not been called");
    HIPCHK(hipSetDevice(b->device));
    HandlerUpdate a;
    std::memset(&a, 0, sizeof(a));
    if (on_device) {
        a.what = it->what; a.delta = it->delta; a.rho = it->rho; a.x_k = it->x_k; a.grad = it->grad; a.c_k = it->c_k;
    } else {
        const int rc = ensure_handler_stage(b);
        if (rc != RSQP_OK) return rc;
        const size_t nq = (size_t)b->nq, sN = (size_t)b->sumN, sC = (size_t)b->sumC;
        const size_t o_rho = nq, o_x = 2 * nq, o_g = o_x + sN, o_c = o_g + sN, o_w = o_c + sC;
        // (the pinned block is free: every call that uses it waits for its copy)
        std::memcpy(b->h_pin, it->delta, sizeof(double) * nq); std::memcpy(b->h_pin + o_rho, it->rho, sizeof(double) * nq);
        std::memcpy(b->h_pin + o_x, it->x_k, sizeof(double) * sN);
        if (it->grad) std::memcpy(b->h_pin + o_g, it->grad, sizeof(double) * sN);
        if (sC > 0) std::memcpy(b->h_pin + o_c, it->c_k, sizeof(double) * sC);
        std::memcpy(b->h_pin + o_w, it->what, sizeof(int) * nq);
        HIPCHK(hipMemcpyAsync(b->h_in.p, b->h_pin, sizeof(double) * (size_t)handler_in_words(b), hipMemcpyHostToDevice, b->stream));
        double *const d = b->h_in.p;
        a.delta = d; a.rho = d + o_rho; a.x_k = d + o_x; a.grad = it->grad ? d + o_g : nullptr; a.c_k = d + o_c;
        a.what = reinterpret_cast<const int *>(d + o_w);
    }
    a.nq = b->nq; a.sumV = (int)b->sumV; a.sumC = (int)b->sumC; a.desc = b->d_desc.p;
    a.uniV = (b->uniV > 0 && b->uniC >= 0) ? b->uniV : 0; a.uniC = a.uniV > 0 ? b->uniC : 0;
    a.x_l = b->h_xl.p; a.x_u = b->h_xu.p; a.c_l = b->h_cl.p; a.c_u = b->h_cu.p;
    a.g = b->g.p; a.lb = b->lb.p; a.ub = b->ub.p; a.lbA = b->lbA.p; a.ubA = b->ubA.p;
    const long long n = 3 * b->sumV + 2 * b->sumC;
    hipLaunchKernelGGL(batch_handler_update_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->stream));
    return RSQP_OK;
}

extern "C" int rsqp_batch_handler_get_step(rsqp_batch *b, double *p, double *lam_c, double *lam_x, double *infea_model,
                                           double *norm_p, int on_device) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_get_step: rsqp_batch_handler_set_problem has not been called");
    HIPCHK(hipSetDevice(b->device));
    const size_t nq = (size_t)b->nq, sN = (size_t)b->sumN, sC = (size_t)b->sumC;
    const size_t o_lx = sN, o_lc = 2 * sN, o_in = o_lc + sC, o_np = o_in + nq, words = o_np + nq;
    double *dp = p, *dlc = lam_c, *dlx = lam_x, *din = infea_model, *dnp = norm_p;
    if (!on_device) {
        const int rc = ensure_handler_stage(b);
        if (rc != RSQP_OK) return rc;
        double *const d = b->h_out.p;
        dp = p ? d : nullptr; dlx = lam_x ? d + o_lx : nullptr; dlc = lam_c ? d + o_lc : nullptr;
        din = infea_model ? d + o_in : nullptr; dnp = norm_p ? d + o_np : nullptr;
    }
    // hs071-scale members: 8 lanes each, eight members per wavefront
    const int G = (b->nVmax + b->nCmax <= 16) ? 8 : 64;
    const dim3 grid((unsigned)(((long long)b->nq * G + 255) / 256)), block(256);
    if (G == 8)
        hipLaunchKernelGGL(batch_handler_step_kernel<8>, grid, block, 0, b->stream, b->nq, b->d_desc.p, b->x.p, b->y.p, dp, dlc, dlx, din, dnp);
    else
        hipLaunchKernelGGL(batch_handler_step_kernel<64>, grid, block, 0, b->stream, b->nq, b->d_desc.p, b->x.p, b->y.p, dp, dlc, dlx, din, dnp);
    HIPCHK(hipGetLastError());
    if (!on_device) HIPCHK(hipMemcpyAsync(b->h_pin, b->h_out.p, sizeof(double) * words, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (!on_device) {
        if (p) std::memcpy(p, b->h_pin, sizeof(double) * sN);
        if (lam_x) std::memcpy(lam_x, b->h_pin + o_lx, sizeof(double) * sN);
        if (lam_c) std::memcpy(lam_c, b->h_pin + o_lc, sizeof(double) * sC);
        if (infea_model) std::memcpy(infea_model, b->h_pin + o_in, sizeof(double) * nq);
        if (norm_p) std::memcpy(norm_p, b->h_pin + o_np, sizeof(double) * nq);
    }
    return RSQP_OK;
}

extern "C" int rsqp_batch_get_vectors(rsqp_batch *b, double *g, double *lb, double *ub, double *lbA, double *ubA) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (g) HIPCHK(b->g.download(g, b->sumV));
    if (lb) HIPCHK(b->lb.download(lb, b->sumV));
    if (ub) HIPCHK(b->ub.download(ub, b->sumV));
    if (lbA) HIPCHK(b->lbA.download(lbA, b->sumC));
    if (ubA) HIPCHK(b->ubA.download(ubA, b->sumC));
    return RSQP_OK;
}

// ---------------------------------------------------------------------------------
// the matrices of the QPhandler on the device (rsqp_batch_handler_set_matrices): set_A / set_H, update_A / update_H of
// src/QPhandler.cpp:310-334, 508-530 for every member, J without the identity entries of [J I -I]
// ---------------------------------------------------------------------------------
namespace {
// one thread per entry of the concatenation jac | hess; the member of an entry as in batch_masked_copy_kernel: a division where every
// member has as many entries (uniJ / uniH > 0), else the last member whose start is at or before the entry -- joff for jac, the
// descriptors' offHnz or the caller-layout starts Huoff for hess. A J value of a canonical batch is written twice, into its slot of
// the CSC pool and, through the inverse of perm, into its slot of the CSR copy (as scatter_values_csc_csr of sparse.hip writes both
// forms on a single handle); of a folded batch into the caller-layout copy, which is folded behind this launch. The first nq
// threads raise the update marks (qpOASESInterface.cpp:407-409, 427-429). bits: the RSQP_HM_* bits that count in this launch.
struct HandlerMatrices {
    int nq, bits;
    long long nJ, nH;                 // entries of jac and of hess (0: not given)
    int uniJ, uniA, uniH;             // uniA: entries of A per member where uniJ > 0
    const QPDesc *desc;
    const int *what;
    const double *jac, *hess;
    const long long *joff, *Auoff, *Huoff;   // Auoff / Huoff: null for a canonical layout
    const int *inv;                   // CSC slot -> CSR slot
    double *Aval, *Arv, *Auval, *Hdst;
    int *mark;
    const int *first;
};
__global__ void __launch_bounds__(256) batch_handler_matrices_kernel(HandlerMatrices a) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < a.nq && (a.what[e] & a.bits) != 0 && a.first[e] != 0) a.mark[e] = 1;
    if (e >= a.nJ + a.nH) return;
    const bool isJ = e < a.nJ;
    const long long k = isJ ? e : e - a.nJ;
    const int uni = isJ ? a.uniJ : a.uniH;
    int q;
    if (uni > 0) q = (int)(k / uni);
    else {                                            // (members without entries own none)
        int lo = 0, hi = a.nq - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            const long long start = isJ ? a.joff[mid] : (a.Huoff ? a.Huoff[mid] : (long long)a.desc[mid].offHnz);
            if (start <= k) lo = mid; else hi = mid - 1;
        }
        q = lo;
    }
    const int W = a.what[q] & a.bits;
    if (!isJ) {
        if (W & RSQP_HM_HESS) a.Hdst[k] = a.hess[k];
        return;
    }
    if (!(W & RSQP_HM_JAC)) return;
    const double v = a.jac[k];
    const long long i = k - (uni > 0 ? (long long)q * uni : a.joff[q]);     // the entry within the member's J block
    if (a.Auoff) { a.Auval[a.Auoff[q] + i] = v; return; }
    const long long slot = (uni > 0 ? (long long)q * a.uniA : (long long)a.desc[q].offAnz) + i;
    a.Aval[slot] = v;
    a.Arv[a.inv[slot]] = v;
}

__global__ void __launch_bounds__(256) invert_perm_kernel(int n, const int *__restrict__ perm, int *__restrict__ inv) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) inv[perm[p]] = p;
}

// one thread per member that carries HESS: small_csc_symmetric (rsqp_matrix.hip) on the canonical pools, where no position repeats
// (a folded layout has been summed in the caller's order, as small_csc_symmetric sums it). The dense comparison of that function,
// d[r][c] != d[c][r] for every pair with absent entries 0, is: every off-diagonal entry equals its transposed entry, or 0 where
// that is absent -- NaN differs from everything in both. A verdict that is not the one on record is flagged for the host
__global__ void __launch_bounds__(256)
batch_hess_symmetry_kernel(int nq, const QPDesc *__restrict__ desc, const int *__restrict__ what, const int *__restrict__ Hjc,
                           const int *__restrict__ Hir, const double *__restrict__ Hval, char *__restrict__ symq, int *__restrict__ changed) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq || (what[q] & RSQP_HM_HESS) == 0) return;
    const int nV = desc[q].nV;
    const int *const jc = Hjc + desc[q].offHjc, *const ir = Hir + desc[q].offHnz;
    const double *const val = Hval + desc[q].offHnz;
    bool sym = true;
    for (int c = 0; c < nV; c++)
        for (int k = jc[c]; k < jc[c + 1]; k++) {
            const int r = ir[k];
            if (r == c) continue;
            double other = 0.0;
            for (int t = jc[r]; t < jc[r + 1]; t++)
                if (ir[t] == c) other = val[t];
            if (val[k] != other) sym = false;
        }
    const char s = sym ? 1 : 0;
    if (symq[q] != s) { symq[q] = s; *changed = 1; }
}

// what the first call builds: where the members' entries start in jac, and the inverse of perm
int ensure_handler_matrices(rsqp_batch *b) {
    if (b->hm_ready) return RSQP_OK;
    std::vector<long long> joff((size_t)b->nq + 1, 0);
    for (int q = 0; q < b->nq; q++) joff[q + 1] = joff[q] + b->h_jn[q];
    HIPCHK(b->hm_joff.from(joff));
    HIPCHK(b->hm_inv.alloc((size_t)b->sumAnz, false));
    if (b->sumAnz > 0) {
        hipLaunchKernelGGL(invert_perm_kernel, dim3((unsigned)((b->sumAnz + 255) / 256)), dim3(256), 0, b->stream, (int)b->sumAnz,
                           b->perm.p, b->hm_inv.p);
        HIPCHK(hipGetLastError());
    }
    b->hm_ready = true;
    return RSQP_OK;
}
}  // namespace

extern "C" int rsqp_batch_handler_set_matrices(rsqp_batch *b, const int *what, const double *jac, const double *hess, int on_device) {
    if (!b || !what) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_set_matrices: the batch and what are required");
    if (!b->have_problem) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_set_matrices: rsqp_batch_handler_set_problem has not been called");
    if (!b->haveH) hess = nullptr;
    if (!on_device) {
        int seen = 0;
        for (int q = 0; q < b->nq; q++) seen |= what[q];
        if (!b->haveH) seen &= ~RSQP_HM_HESS;
        if ((seen & RSQP_HM_JAC) && !jac) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_set_matrices: a word has JAC and jac is NULL");
        if ((seen & RSQP_HM_HESS) && !hess) return fail(RSQP_ERR_ARG, "rsqp_batch_handler_set_matrices: a word has HESS and hess is NULL");
        if (!(seen & RSQP_HM_JAC)) jac = nullptr;
        if (!(seen & RSQP_HM_HESS)) hess = nullptr;
    }
    if (!jac && !hess) return RSQP_OK;   // nobody is named
    HIPCHK(hipSetDevice(b->device));
    int rc;
    if ((rc = ensure_opt(b)) != RSQP_OK || (rc = ensure_handler_matrices(b)) != RSQP_OK) return rc;
    const size_t nq = (size_t)b->nq;
    const long long nJ = jac ? b->sumJ : 0, nH = hess ? b->Hfold.unnz : 0;
    const bool judge = hess && !b->h_Hjc.empty();   // batches of at most 8 variables: the symmetry of the members that carry HESS
    if (judge) {
        if (!b->sym_host) {
            HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&b->sym_host), sizeof(int), hipHostMallocMapped));
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->sym_dev), b->sym_host, 0));
            HIPCHK(b->d_symq.alloc(nq, false));
        }
        if (b->symq_stale) {
            HIPCHK(hipMemcpyAsync(b->d_symq.p, b->h_symq.data(), nq, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));   // (pageable memory: the copy has read it)
            b->symq_stale = false;
        }
        *b->sym_host = 0;
    }
    HandlerMatrices a;
    std::memset(&a, 0, sizeof(a));
    if (on_device) {
        a.what = what; a.jac = jac; a.hess = hess;
    } else {
        // what | jac | hess, the arrays that are given alone: one copy up
        const size_t o_j = (nq + 1) / 2, o_h = o_j + (size_t)nJ, words = o_h + (size_t)nH;
        if ((rc = ensure_pinned(b, words)) != RSQP_OK) return rc;
        if (b->hm_in.n < words) HIPCHK(b->hm_in.alloc(words, false));
        std::memcpy(b->h_pin, what, sizeof(int) * nq);
        if (jac) std::memcpy(b->h_pin + o_j, jac, sizeof(double) * (size_t)nJ);
        if (hess) std::memcpy(b->h_pin + o_h, hess, sizeof(double) * (size_t)nH);
        HIPCHK(hipMemcpyAsync(b->hm_in.p, b->h_pin, sizeof(double) * words, hipMemcpyHostToDevice, b->stream));
        a.what = reinterpret_cast<const int *>(b->hm_in.p); a.jac = b->hm_in.p + o_j; a.hess = b->hm_in.p + o_h;
    }
    a.nq = b->nq; a.bits = (jac ? RSQP_HM_JAC : 0) | (hess ? RSQP_HM_HESS : 0);
    a.nJ = nJ; a.nH = nH;
    a.uniJ = b->uni_jn ? b->h_jn[0] : 0; a.uniA = b->uni_annz;
    a.uniH = (b->uni_pat && b->Hfold.canon) ? b->uni_hnnz : 0;
    a.desc = b->d_desc.p; a.joff = b->hm_joff.p; a.inv = b->hm_inv.p;
    a.Aval = b->Aval.p; a.Arv = b->Arv.p;
    if (!b->Afold.canon) { a.Auoff = b->Auoff.p; a.Auval = b->Afold.uval.p; }
    a.Hdst = b->Hval.p;
    if (hess && !b->Hfold.canon) { a.Huoff = b->Huoff.p; a.Hdst = b->Hfold.uval.p; }
    a.mark = b->opt.p + (size_t)rsqp_batch::OPT_UPD * nq; a.first = b->opt.p + (size_t)rsqp_batch::OPT_FIRST * nq;
    const long long n = std::max<long long>(nJ + nH, b->nq);
    hipLaunchKernelGGL(batch_handler_matrices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, a);
    HIPCHK(hipGetLastError());
    if (jac && !b->Afold.canon) {   // the folded layout: sum the caller's values, then the CSR copy from the sums
        HIPCHK(b->Afold.sum(b->Aval, (int)b->sumAnz, b->stream));
        if (rsqp_launch_gather((int)b->sumAnz, b->perm.p, b->Aval.p, b->Arv.p, b->stream) != hipSuccess)
            return fail(RSQP_ERR_DEVICE, "gather launch failed");
    }
    if (hess && !b->Hfold.canon) HIPCHK(b->Hfold.sum(b->Hval, (int)b->sumHnz, b->stream));
    if (judge) {
        hipLaunchKernelGGL(batch_hess_symmetry_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, b->stream, b->nq, b->d_desc.p,
                           a.what, b->Hjc.p, b->Hir.p, b->Hval.p, b->d_symq.p, b->sym_dev);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    if (judge && *b->sym_host != 0) {   // a verdict changed: the host's record follows (nq bytes)
        HIPCHK(hipMemcpy(b->h_symq.data(), b->d_symq.p, nq, hipMemcpyDeviceToHost));
        b->h_sym = true;
        for (int q = 0; q < b->nq; q++) b->h_sym = b->h_sym && b->h_symq[q];
    }
    return RSQP_OK;
}

extern "C" int rsqp_batch_get_matrix_values(rsqp_batch *b, double *Aval, double *Hval) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (Aval) HIPCHK((b->Afold.canon ? b->Aval : b->Afold.uval).download(Aval, (size_t)b->Afold.unnz));
    if (Hval && b->haveH) HIPCHK((b->Hfold.canon ? b->Hval : b->Hfold.uval).download(Hval, (size_t)b->Hfold.unnz));
    return RSQP_OK;
}

namespace {
int ensure_warm_pools(rsqp_batch *b) {
    if (b->wx0.p) return RSQP_OK;
    HIPCHK(b->wx0.alloc(b->sumV)); HIPCHK(b->wy0.alloc(b->sumV + b->sumC)); HIPCHK(b->wgb.alloc(b->sumV));
    return RSQP_OK;
}

// kernel family a launch on this batch runs: 3 HBM-resident, 1 hs071-scale tableau (+ lane-per-problem), 0 LDS-resident
int batch_family(const rsqp_batch *b, const QPPools &p, bool lp) {
    return b->hbm ? 3 : rsqp_small_launch_is_tiny(knobs_of(b, lp), p, b->nVmax, b->nCmax);
}

// one solve launch of the whole batch (p.member_mode: of the members it names). first: the launch rsqp_batch_get_last_kernel reports;
// lp: a launch of rsqp_batch_optimize_lp (pools_of, knobs_of)
int launch_batch(rsqp_batch *b, QPPools &p, int mode, int max_nWSR, bool first, bool lp) {
    const SmallKnobs kn = knobs_of(b, lp);
    const int fam = batch_family(b, p, lp);
    // the kernel families keep different layouts in the same state block: a hot start on another family's state starts cold
    // (per-member modes: the plan kernel was told, and `mode` is not read)
    if (!p.member_mode && (mode == RSQP_MODE_HOT_VECTORS || mode == RSQP_MODE_HOT_MATRICES) && b->state_engine != fam) mode = RSQP_MODE_COLD;
    // every member of the launch has a state of this family now; one that sits out keeps what it had
    b->state_engine = (p.member_mode && b->sitters && b->state_engine != fam) ? -2 : fam;
    hipError_t e;
    if (b->hbm) {
        if (first) b->last_kernel = 3;
        e = rsqp_launch_small_qp_hbm(kn, p, b->nq, b->nVmax, b->nCmax, mode, max_nWSR, b->stream);
    } else {
        // a cold-start-only batch on the tableau kernel keeps no state and leaves no mark: the handle remembers it instead
        if (fam == 1 && !b->keep_state) { p.skip_mark = 1; b->state_engine = -1; }
        if (first) b->last_kernel = fam == 1 ? (rsqp_lane_fits(kn, p, b->nq, b->nVmax, b->nCmax, mode) ? 2 : 1) : 0;
        e = rsqp_launch_small_qp(kn, p, b->nq, b->nVmax, b->nCmax, b->mat_bytes_max, mode, max_nWSR, b->stream);
    }
    if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, std::string("QP kernel launch: ") + hipGetErrorString(e));
    return RSQP_OK;
}
}  // namespace

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
    if (!b->timing) HIPCHK(hipEventRecord(b->ev0, b->stream));
    const int rc = launch_batch(b, p, mode, max_nWSR, true, false);
    if (rc != RSQP_OK) return rc;
    b->cert_lp = false;
    if (!b->timing) HIPCHK(hipEventRecord(b->ev1, b->stream));
    return RSQP_OK;
}

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
    opt[rsqp_batch::OPT_MODE * nq + q] = -1; opt[rsqp_batch::OPT_LMODE * nq + q] = -1;
    opt[rsqp_batch::OPT_RMODE * nq + q] = -1; opt[rsqp_batch::OPT_PMODE * nq + q] = -1;
    opt[rsqp_batch::OPT_RESCUE * nq + q] = 0;
    if (updated && opt[rsqp_batch::OPT_FIRST * nq + q] != 0) opt[rsqp_batch::OPT_UPD * nq + q] = 1;   // (:407, :427: firstQPsolved_ &&)
    if (fam_all1 >= 0) opt[rsqp_batch::OPT_FAM * nq + q] = fam_all1;
}

// before the first solve: the call shape of every member (rsqp_dispatch_mode); a FIXED <-> VARIED flip re-initialises from the
// member's own previous x, y and bound working set (:201-208), copied into the warm-start pools. updated: Update_A / Update_H of
// everybody (rsqp_batch_set_matrix_values), beside the member's own mark, which this call consumes (reset_flags, :488-496).
// fam1 = 1 + the kernel family of this call's launches, fam_all1 as in plan_sitter
__global__ void batch_plan_kernel(int nq, const QPDesc *__restrict__ desc, int *__restrict__ opt, const int *__restrict__ take,
                                  int updated, int fam_all1, int fam1, const double *__restrict__ x, const double *__restrict__ y,
                                  const int *__restrict__ ws_b, double *__restrict__ x0, double *__restrict__ y0, int *__restrict__ gb) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (sits_out(take, q)) { plan_sitter(nq, q, opt, updated, fam_all1); return; }
    int old_status = opt[rsqp_batch::OPT_OLD * nq + q], new_status = opt[rsqp_batch::OPT_NEW * nq + q];
    const bool upd = updated != 0 || opt[rsqp_batch::OPT_UPD * nq + q] != 0;
    int mode = rsqp_dispatch_mode(opt[rsqp_batch::OPT_FIRST * nq + q] != 0, upd, old_status, new_status);
    // the member's stored state is another kernel family's: a hot start runs cold, as on a single handle
    const bool hot_ok = (fam_all1 >= 0 ? fam_all1 : opt[rsqp_batch::OPT_FAM * nq + q]) == fam1;
    if (!hot_ok && (mode == RSQP_MODE_HOT_VECTORS || mode == RSQP_MODE_HOT_MATRICES)) mode = RSQP_MODE_COLD;
    opt[rsqp_batch::OPT_OLD * nq + q] = old_status; opt[rsqp_batch::OPT_NEW * nq + q] = new_status;
    opt[rsqp_batch::OPT_MODE * nq + q] = mode;
    opt[rsqp_batch::OPT_UPD * nq + q] = 0; opt[rsqp_batch::OPT_FAM * nq + q] = fam1;
    if (mode == RSQP_MODE_WARM_REINIT) {
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
    opt[rsqp_batch::OPT_N1 * nq + q] = n1;
    if (solved) {
        opt[rsqp_batch::OPT_FIRST * nq + q] = 1;
        opt[rsqp_batch::OPT_RMODE * nq + q] = -1; opt[rsqp_batch::OPT_RESCUE * nq + q] = 0; used[q] = n1;
        return;
    }
    const QPDesc d = desc[q];
    opt[rsqp_batch::OPT_OLD * nq + q] = 0; opt[rsqp_batch::OPT_NEW * nq + q] = 0;
    if (infeasible && d.nV >= 2 * d.nC) {
        for (int v = 0; v < d.nV; v++) x0[d.offV + v] = 0.0;
        for (int i = 0; i < d.nC; i++) {
            x0[d.offV + i + d.nV - 2 * d.nC] = fmax(0.0, lbA[d.offC + i]);
            x0[d.offV + i + d.nV - d.nC] = -fmin(0.0, ubA[d.offC + i]);
        }
        opt[rsqp_batch::OPT_RMODE * nq + q] = RSQP_MODE_WARM_REINIT; opt[rsqp_batch::OPT_RESCUE * nq + q] = 2;
    } else {
        opt[rsqp_batch::OPT_RMODE * nq + q] = RSQP_MODE_COLD; opt[rsqp_batch::OPT_RESCUE * nq + q] = 1;
    }
}

// behind the rescue solve: nWSR_used of the rescued members. A member whose FIRST init failed reports the rescue's count alone when
// the rescue fails too (the reference throws inside handle_error, :754-756, before :211-212 add the first count)
__global__ void batch_count_kernel(int nq, const int *__restrict__ opt, const int *__restrict__ take, const int *__restrict__ status,
                                   const int *__restrict__ nwsr, int *__restrict__ used) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq || sits_out(take, q) || opt[rsqp_batch::OPT_RESCUE * nq + q] == 0) return;
    const int n1 = opt[rsqp_batch::OPT_N1 * nq + q], n2 = nwsr[q];
    const bool first_init_failed = opt[rsqp_batch::OPT_FIRST * nq + q] == 0;
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
    if (!b->used_host) {
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&b->used_host), sizeof(int) * nq, hipHostMallocMapped));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->used_dev), b->used_host, 0));
    }
    if ((rc = ensure_warm_pools(b)) != RSQP_OK) return rc;
    b->have_x0 = b->have_y0 = b->have_gb = false;   // the pools are this call's from here on
    if (kind == 2 && !b->d_desc_lp.p) {
        std::vector<QPDesc> lp = b->desc;
        for (QPDesc &d : lp) { d.haveH = 0; d.hnnz = 0; d.hreg = 0.0; }
        HIPCHK(b->d_desc_lp.from(lp));
        HIPCHK(b->g_lp.alloc(b->sumV));
    }
    if (b->last_kind != 0 && b->last_kind != kind) {
        HIPCHK(hipMemsetAsync(b->opt.p, 0, sizeof(int) * (size_t)rsqp_batch::OPT_WORDS * nq, b->stream));
        b->opt_started = false;
    }
    b->last_kind = kind;
    if (!b->timing) HIPCHK(hipEventRecord(b->ev0, b->stream));
    return RSQP_OK;
}

// the solve launch behind a plan kernel: every member starts as word `word` of its opt block says (QPPools::member_mode)
int launch_members(rsqp_batch *b, QPPools &p, int word, int mode, int max_nWSR, bool first, bool lp) {
    p.member_mode = b->opt.p + (size_t)word * b->nq;
    return launch_batch(b, p, mode, max_nWSR, first, lp);
}

// what both optimize entry points do behind their last launch: the second event, the call's one wait, the members' counts
int finish_optimize(rsqp_batch *b, int *nWSR_used) {
    if (!b->timing) HIPCHK(hipEventRecord(b->ev1, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (nWSR_used) std::memcpy(nWSR_used, b->used_host, sizeof(int) * b->nq);
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
    int old_status = opt[rsqp_batch::OPT_OLD * nq + q], new_status = opt[rsqp_batch::OPT_NEW * nq + q];
    const bool upd = updated != 0 || opt[rsqp_batch::OPT_UPD * nq + q] != 0;
    int mode = rsqp_dispatch_mode(opt[rsqp_batch::OPT_FIRST * nq + q] != 0, upd, old_status, new_status);
    const bool init = mode == RSQP_MODE_COLD || mode == RSQP_MODE_WARM_REINIT;
    const double reg = init ? lp_reg_val(d, g) : d.hreg;
    // (a stored state of another kernel family: the hot start runs cold on the regVal it has, as rsqp_solve does on a handle)
    const bool hot_ok = (fam_all1 >= 0 ? fam_all1 : opt[rsqp_batch::OPT_FAM * nq + q]) == fam1;
    if (!hot_ok && !init) mode = RSQP_MODE_COLD;
    __syncthreads();   // every lane has read the member's words
    if (threadIdx.x == 0) {
        opt[rsqp_batch::OPT_OLD * nq + q] = old_status; opt[rsqp_batch::OPT_NEW * nq + q] = new_status;
        opt[rsqp_batch::OPT_MODE * nq + q] = mode;
        opt[rsqp_batch::OPT_UPD * nq + q] = 0; opt[rsqp_batch::OPT_FAM * nq + q] = fam1;
        opt[rsqp_batch::OPT_LMODE * nq + q] = init ? RSQP_MODE_COLD : mode;
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
            opt[rsqp_batch::OPT_N1 * nq + q] = nwsr[q];
            opt[rsqp_batch::OPT_FIRST * nq + q] = 1;
            opt[rsqp_batch::OPT_RMODE * nq + q] = -1; opt[rsqp_batch::OPT_RESCUE * nq + q] = 0;
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
        opt[rsqp_batch::OPT_N1 * nq + q] = nwsr[q];
        opt[rsqp_batch::OPT_OLD * nq + q] = 0; opt[rsqp_batch::OPT_NEW * nq + q] = 0;
        opt[rsqp_batch::OPT_RMODE * nq + q] = slack ? RSQP_MODE_WARM_REINIT : RSQP_MODE_COLD;
        opt[rsqp_batch::OPT_RESCUE * nq + q] = slack ? 2 : 1;
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
    const bool solved = status[q] == QPS_SOLVED, rescued = opt[rsqp_batch::OPT_RESCUE * nq + q] != 0;
    const int n1 = opt[rsqp_batch::OPT_N1 * nq + q], n2 = nwsr[q];
    __syncthreads();
    if (lane == 0) {
        opt[rsqp_batch::OPT_N1 * nq + q] = rescued ? (solved ? n1 + n2 : n2) : n1;
        opt[rsqp_batch::OPT_PMODE * nq + q] = solved ? RSQP_MODE_HOT_VECTORS : -1;
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
    const int total = opt[rsqp_batch::OPT_N1 * nq + q];
    if (opt[rsqp_batch::OPT_PMODE * nq + q] < 0) { if (lane == 0) used[q] = total; return; }
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
        rc = launch_members(b, p, rsqp_batch::OPT_MODE, RSQP_MODE_COLD, b->qp_maxiter, true, false);
    }
    if (rc != RSQP_OK) return rc;
    // (also behind a call nobody took part in: its plan kernel has written -1 into the mode words, which the uniform cold launch
    //  relies on being 0; the next call goes through the plan kernel, where members without a solved first QP come out cold)
    b->opt_started = true;
    b->cert_lp = false;
    b->mats_updated = false;   // reset_flags (:488-496); a member that sat out has the mark in its own word now
    hipLaunchKernelGGL(batch_rescue_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc.p, b->opt.p, b->status.p, take, b->nwsr.p,
                       b->lbA.p, b->ubA.p, b->wx0.p, b->used_dev);
    HIPCHK(hipGetLastError());
    // the rescue launch is unconditional: a member that needs none leaves at its first instruction, and asking the device whether
    // anybody needs one would put a host round trip into every call
    p = pools_of(b, false);
    p.x0 = b->wx0.p;                                                 // handle_error: x_0 alone (:741-743)
    rc = launch_members(b, p, rsqp_batch::OPT_RMODE, RSQP_MODE_COLD, b->qp_maxiter, false, false);
    if (rc != RSQP_OK) return rc;
    hipLaunchKernelGGL(batch_count_kernel, grid, block, 0, b->stream, nq, b->opt.p, take, b->status.p, b->nwsr.p, b->used_dev);
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
    if ((rc = launch_members(b, p, rsqp_batch::OPT_LMODE, RSQP_MODE_COLD, b->lp_maxiter, true, true)) != RSQP_OK) return rc;
    b->opt_started = true;
    b->cert_lp = true;
    b->mats_updated = false;   // reset_flags (:488-496); a member that sat out has the mark in its own word now
    hipLaunchKernelGGL(batch_lp_rescue_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->status.p, b->nwsr.p,
                       b->g.p, b->x.p, b->lbA.p, b->ubA.p, b->wx0.p);
    HIPCHK(hipGetLastError());
    // (unconditional, as in rsqp_batch_optimize_qp: a member that needs no rescue leaves at its first instruction)
    p.x0 = b->wx0.p;                                                 // handle_error: x_0 alone (:700-702)
    if ((rc = launch_members(b, p, rsqp_batch::OPT_RMODE, RSQP_MODE_COLD, b->lp_maxiter, false, true)) != RSQP_OK) return rc;
    hipLaunchKernelGGL(batch_lp_prox_plan_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->status.p, b->nwsr.p,
                       b->g.p, b->x.p, b->g_lp.p);
    HIPCHK(hipGetLastError());
    p.x0 = nullptr;
    p.g = b->g_lp.p;
    if ((rc = launch_members(b, p, rsqp_batch::OPT_PMODE, RSQP_MODE_HOT_VECTORS, b->lp_maxiter, false, true)) != RSQP_OK) return rc;
    hipLaunchKernelGGL(batch_lp_finish_kernel, grid, block, 0, b->stream, nq, b->d_desc_lp.p, opt, take, b->nwsr.p, b->g.p, b->x.p,
                       b->obj.p, b->used_dev);
    HIPCHK(hipGetLastError());
    return finish_optimize(b, nWSR_used);
}

extern "C" int rsqp_batch_get_dispatch(const rsqp_batch *b, int *mode, int *rescue) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!b->opt.p) return fail(RSQP_ERR_ARG, "rsqp_batch_get_dispatch: no rsqp_batch_optimize_qp / rsqp_batch_optimize_lp has run");
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipStreamSynchronize(b->stream));
    const size_t nq = b->nq;
    if (mode) HIPCHK(hipMemcpy(mode, b->opt.p + rsqp_batch::OPT_MODE * nq, sizeof(int) * nq, hipMemcpyDeviceToHost));
    if (rescue) HIPCHK(hipMemcpy(rescue, b->opt.p + rsqp_batch::OPT_RESCUE * nq, sizeof(int) * nq, hipMemcpyDeviceToHost));
    return RSQP_OK;
}

extern "C" int rsqp_batch_get_last_kernel(const rsqp_batch *b) { return b ? b->last_kernel : -1; }

extern "C" int rsqp_batch_set_keep_state(rsqp_batch *b, int keep) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    b->keep_state = keep != 0;
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
    if (b->recbuf.n < tot) HIPCHK(b->recbuf.alloc(tot, false));
    int rc = rsqp_batch_pack_records_dev(b, b->recbuf.p);
    if (rc != RSQP_OK) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    HIPCHK(b->recbuf.download(rec_host, tot));
    return RSQP_OK;
}

// (rsqp_host.h: the native RCCL call sites of rsqp_rccl.cpp reach the batch through these)
hipStream_t rsqp_batch_stream_internal(rsqp_batch *b) { return b->stream; }
int rsqp_batch_device_internal(const rsqp_batch *b) { return b->device; }
int rsqp_batch_nq_internal(const rsqp_batch *b) { return b ? b->nq : 0; }
