// rsqp_batch_handler.hip -- everything that writes the pools of a batch (rsqp_batch.h) member by member: who takes part in the
// optimize calls, the setters of the named members, and the QPhandler of every member on the device (rsqp_batch_handler_* of
// include/rsqp_hip.h), with their kernels.
#include "rsqp_batch.h"

namespace {
// the member of entry k of a pooled array: a division where every member has `uni` entries (uni > 0), else the LAST member whose
// start is at or before k -- a member without entries starts where the next one does and owns none. start(q): member q's start
template <class K, class Start>
__device__ inline int member_of(K k, int uni, int nq, Start start) {
    if (uni > 0) return (int)(k / uni);
    int lo = 0, hi = nq - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start(mid) <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}
}  // namespace

// ---------------------------------------------------------------------------------
// members of a batch on their own: who takes part in the optimize calls, and setters that write the named members only
// ---------------------------------------------------------------------------------
namespace {
// up to five pooled arrays in one launch: entry e of the concatenation belongs to array s (end[s-1] <= e < end[s]) and there to the
// member its position says (member_of); it is copied iff that member is named. uni[s] > 0: every member has uni[s] entries in array
// s; else the member is searched in the offsets `kind[s]` names -- of the descriptors (0 offV, 1 offC, 2 offAnz, 3 offHnz), or
// uoff[s] (4: a caller's layout that is not the canonical one). mark != null: the update mark of every named member whose first
// QP is solved (qpOASESInterface.cpp:407-409, 427-429). Consecutive lanes read and write consecutive entries.
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
    const int q = member_of(k, a.uni[s], a.nq, [&](int m) { return member_start(a, s, m); });
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
    const long long sV = b->sumV, sC = b->sumC;
    if ((rc = ensure_scratch(b, (size_t)(3 * sV + 2 * sC))) != RSQP_OK) return rc;
    double *const st = b->scratch.p;
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
    HIPCHK(hipStreamSynchronize(b->stream));   // (rsqp_batch::scratch: free again behind this)
    return RSQP_OK;
}

extern "C" int rsqp_batch_set_matrix_values_of(rsqp_batch *b, const int *members, const double *Aval, const double *Hval) {
    if (!b) return fail(RSQP_ERR_ARG, "null batch");
    if (!members) return rsqp_batch_set_matrix_values(b, Aval, Hval);
    if (!b->haveH) Hval = nullptr;
    HIPCHK(hipSetDevice(b->device));
    int rc, n = 0;
    if ((rc = upload_mask(b, b->named, members, &n)) != RSQP_OK || n == 0 || (!Aval && !Hval)) return rc;
    const long long uA = b->Afold.unnz, uH = b->Hfold.unnz;
    if ((rc = ensure_scratch(b, (size_t)(uA + uH))) != RSQP_OK || (rc = ensure_opt(b)) != RSQP_OK) return rc;
    double *const st = b->scratch.p;
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
    a.mark = b->opt.p + (size_t)OPT_UPD * b->nq; a.first = b->opt.p + (size_t)OPT_FIRST * b->nq;
    if ((rc = launch_masked_copy(b, a)) != RSQP_OK) return rc;
    if (Aval && (rc = settle_A(b)) != RSQP_OK) return rc;
    if (Hval) {
        if ((rc = settle_H(b)) != RSQP_OK) return rc;
        judge_h_sym(b, members, Hval);   // the named members' symmetry anew, from the values given
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

// one thread per entry of the concatenation g | lb | ub | lbA | ubA; the member of an entry by member_of, a one-shape batch
// (uniV > 0) dividing. Every formula is one subtraction and one fmax / fmin, as the host states them (QPhandler.cpp:167-201,
// 272-297, 342-368, 430-463, 533-567)
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
    // (a constraint entry exists: uniC > 0 where the batch has one shape)
    const int q = member_of(k, isV ? a.uniV : a.uniC, a.nq, [&](int m) { return isV ? a.desc[m].offV : a.desc[m].offC; });
    const MemberShape sh = shape_of(a.desc, a.uniV, a.uniC, q);
    const int nV = sh.nV, nC = sh.nC, offV = sh.offV, offC = sh.offC;
    const int W = a.what[q];
    if (W == 0) return;
    const bool set = (W & RSQP_HU_SET) != 0;
    if (!isV) {
        if (s == 3) { if (set || (W & RSQP_HU_BOUNDS)) a.lbA[k] = hu_lbA(a.c_l[k], a.c_k[k]); }
        else if (set || ((W & RSQP_HU_BOUNDS) && (W & RSQP_HU_UBA))) a.ubA[k] = hu_ubA(a.c_u[k], a.c_k[k]);
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
        if (s == 1) a.lb[k] = hu_lb(a.x_l[j], a.x_k[j], a.delta[q]);
        else a.ub[k] = hu_ub(a.x_u[j], a.x_k[j], a.delta[q]);
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
    mx = group_max<G>(mx);
    sm = group_sum<G>(sm);
    if (q < nq && lane == 0) {
        if (norm_p) norm_p[q] = mx;
        if (infea) infea[q] = sm;
    }
}
}  // namespace

// a host-pointer call packs its arrays into `words` doubles of the pinned block, which cross in one copy to or from the same
// words of the scratch block (rsqp_batch::scratch: both are free)
int rsqp_batch_units::ensure_staging(rsqp_batch *b, size_t words) {
    if (b->pin.n < words) HIPCHK(b->pin.alloc(words, false));
    return ensure_scratch(b, words);
}

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
    rsqp_handler_iterate d = *it;      // the arrays where the kernel reads them
    Staging st(b, on_device);
    if (st.active) stage_iterate(st, d, stage_sizes(b));
    const int rc = st.up();
    if (rc != RSQP_OK) return rc;
    a.what = d.what; a.delta = d.delta; a.rho = d.rho; a.x_k = d.x_k; a.grad = d.grad; a.c_k = d.c_k;
    a.nq = b->nq; a.sumV = (int)b->sumV; a.sumC = (int)b->sumC; a.desc = b->d_desc.p;
    a.uniV = uni_shape(b); a.uniC = a.uniV > 0 ? b->uniC : 0;
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
    Staging st(b, on_device);
    if (st.active) stage_step(st, p, lam_c, lam_x, infea_model, norm_p, stage_sizes(b));
    int rc;
    if ((rc = st.up()) != RSQP_OK) return rc;
    const int nq = b->nq;
    rc = launch_groups(b, [](auto g) { return batch_handler_step_kernel<decltype(g)::value>; }, nq, b->d_desc.p, b->x.p, b->y.p, p, lam_c,
                       lam_x, infea_model, norm_p);
    return rc != RSQP_OK ? rc : st.down();
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
// one thread per entry of the concatenation jac | hess; the member of an entry by member_of: a division where every member has as
// many entries (uniJ / uniH > 0), else searched in the starts -- joff for jac, the descriptors' offHnz or the caller-layout starts
// Huoff for hess. A J value of a canonical batch is written twice, into its slot of the CSC pool and, through the inverse of perm,
// into its slot of the CSR copy (as scatter_values_csc_csr of sparse.hip writes both forms on a single handle); of a folded batch
// into the caller-layout copy, which is folded behind this launch. The first nq threads raise the update marks
// (qpOASESInterface.cpp:407-409, 427-429). bits: the RSQP_HM_* bits that count in this launch.
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
    const int q = member_of(k, uni, a.nq, [&](int m) { return isJ ? a.joff[m] : (a.Huoff ? a.Huoff[m] : (long long)a.desc[m].offHnz); });
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

}  // namespace

// what the first call builds: where the members' entries start in jac, and the inverse of perm
int rsqp_batch_units::ensure_handler_matrices(rsqp_batch *b) {
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
        if (!b->sym.p) { HIPCHK(b->sym.alloc(1, true)); HIPCHK(b->d_symq.alloc(nq, false)); }
        if (b->symq_stale) {
            HIPCHK(hipMemcpyAsync(b->d_symq.p, b->h_symq.data(), nq, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));   // (pageable memory: the copy has read it)
            b->symq_stale = false;
        }
        *b->sym.p = 0;
    }
    HandlerMatrices a;
    std::memset(&a, 0, sizeof(a));
    a.what = what; a.jac = jac; a.hess = hess;
    Staging st(b, on_device);
    if (st.active) stage_matrices(st, a.what, a.jac, a.hess, nq, (size_t)nJ, (size_t)nH);
    if ((rc = st.up()) != RSQP_OK) return rc;
    a.nq = b->nq; a.bits = (jac ? RSQP_HM_JAC : 0) | (hess ? RSQP_HM_HESS : 0);
    a.nJ = nJ; a.nH = nH;
    a.uniJ = b->uni_jn ? b->h_jn[0] : 0; a.uniA = b->uni_annz;
    a.uniH = (b->uni_pat && b->Hfold.canon) ? b->uni_hnnz : 0;
    a.desc = b->d_desc.p; a.joff = b->hm_joff.p; a.inv = b->hm_inv.p;
    a.Aval = b->Aval.p; a.Arv = b->Arv.p;
    if (!b->Afold.canon) { a.Auoff = b->Auoff.p; a.Auval = b->Afold.uval.p; }
    a.Hdst = b->Hval.p;
    if (hess && !b->Hfold.canon) { a.Huoff = b->Huoff.p; a.Hdst = b->Hfold.uval.p; }
    a.mark = b->opt.p + (size_t)OPT_UPD * nq; a.first = b->opt.p + (size_t)OPT_FIRST * nq;
    const long long n = std::max<long long>(nJ + nH, b->nq);
    hipLaunchKernelGGL(batch_handler_matrices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b->stream, a);
    HIPCHK(hipGetLastError());
    // (a canonical layout: the kernel has written both forms of A)
    if (jac && !b->Afold.canon && (rc = settle_A(b)) != RSQP_OK) return rc;
    if (hess && (rc = settle_H(b)) != RSQP_OK) return rc;
    if (judge) {
        hipLaunchKernelGGL(batch_hess_symmetry_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, b->stream, b->nq, b->d_desc.p,
                           a.what, b->Hjc.p, b->Hir.p, b->Hval.p, b->d_symq.p, b->sym.dev);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    if (judge && *b->sym.p != 0) {   // a verdict changed: the host's record follows (nq bytes)
        HIPCHK(hipMemcpy(b->h_symq.data(), b->d_symq.p, nq, hipMemcpyDeviceToHost));
        judge_h_sym(b, nullptr, nullptr);
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
