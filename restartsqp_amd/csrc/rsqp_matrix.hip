// rsqp_matrix.hip -- matrix staging (rsqp_matrix.h): structure analysis of SpHbMat::setStructure (src/SpHbMat.cpp:196-355) once on the
// host, one upload of what it yields, and the value refresh of SpHbMat::setMatVal (:368-393). Host code only: the kernels it launches
// are those of sparse.hip.
#include "rsqp_matrix.h"

#include <numeric>

void csc_from_entries(int nrow, int ncol, const std::vector<int> &row1, const std::vector<int> &col1,
                      const std::vector<double> &v, Compressed &out) {
    const int n = (int)v.size();
    std::vector<int> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) {
        if (col1[a] != col1[b]) return col1[a] < col1[b];
        return row1[a] < row1[b];
    });
    out.nrow = nrow; out.ncol = ncol;
    out.jc.assign(ncol + 1, 0); out.ir.resize(n); out.val.resize(n); out.order.resize(n);
    for (int p = 0; p < n; p++) {
        int e = perm[p];
        out.ir[p] = row1[e] - 1;
        out.val[p] = v[e];
        out.order[e] = p;
        out.jc[col1[e]]++;  // 1-based col -> slot col (= 0-based col + 1)
    }
    for (int c = 0; c < ncol; c++) out.jc[c + 1] += out.jc[c];
}

void csr_from_csc(int nrow, int ncol, const int *jc, const int *ir, CsrCopy &out) {
    const int nnz = jc[ncol];
    out.rp.assign(nrow + 1, 0); out.ci.resize(nnz); out.perm.resize(nnz);
    for (int k = 0; k < nnz; k++) out.rp[ir[k] + 1]++;
    for (int r = 0; r < nrow; r++) out.rp[r + 1] += out.rp[r];
    std::vector<int> fill(nrow, 0);
    for (int c = 0; c < ncol; c++)
        for (int k = jc[c]; k < jc[c + 1]; k++) {
            int r = ir[k], p = out.rp[r] + fill[r]++;
            out.ci[p] = c;
            out.perm[p] = k;
        }
}

std::vector<int4> build_blocks(int nmajor, const int *ptr, int chunk) {
    std::vector<int4> blk;
    int start = 0;
    while (start < nmajor) {
        int end = start + 1;
        while (end < nmajor && ptr[end + 1] - ptr[start] <= chunk && end - start < 4096) end++;
        blk.push_back(make_int4(start, end, ptr[start], ptr[end]));
        start = end;
    }
    return blk;
}

int csc_fault(int nrow, int ncol, const int *jc, const int *ir) {
    if (jc[0] != 0) return CSC_START;
    for (int c = 0; c < ncol; c++) {
        if (jc[c] > jc[c + 1]) return CSC_MONOTONE;
        for (int k = jc[c]; k < jc[c + 1]; k++)
            if (ir[k] < 0 || ir[k] >= nrow) return CSC_ROW;
    }
    return CSC_OK;
}

bool csc_is_canonical(int ncol, const int *jc, const int *ir) {
    for (int c = 0; c < ncol; c++)
        for (int p = jc[c] + 1; p < jc[c + 1]; p++)
            if (ir[p] <= ir[p - 1]) return false;
    return true;
}

bool canonicalise(const Compressed &c, Compressed &k, std::vector<int> &cptr, std::vector<int> &cidx) {
    if (csc_is_canonical(c.ncol, c.jc.data(), c.ir.data())) return false;
    const int n = c.nnz();
    k.nrow = c.nrow; k.ncol = c.ncol; k.order = c.order; k.tmap = c.tmap;
    k.jc.assign(c.ncol + 1, 0); k.ir.clear(); k.val.clear(); k.ir.reserve(n); k.val.reserve(n); k.slot_of.assign(n, 0);
    cptr.assign(1, 0); cidx.resize(n);
    std::vector<int> idx(n);
    for (int col = 0; col < c.ncol; col++) {
        const int b = c.jc[col], e = c.jc[col + 1];
        std::iota(idx.begin() + b, idx.begin() + e, b);
        std::stable_sort(idx.begin() + b, idx.begin() + e, [&](int x, int y) { return c.ir[x] < c.ir[y]; });
        for (int p = b; p < e; p++) {
            const int u = idx[p];
            if (p == b || c.ir[u] != c.ir[idx[p - 1]]) { k.ir.push_back(c.ir[u]); k.val.push_back(c.val[u]); cptr.push_back(cptr.back()); }
            else k.val.back() += c.val[u];
            k.slot_of[u] = (int)k.ir.size() - 1;
            cidx[cptr.back()++] = u;
        }
        k.jc[col + 1] = (int)k.ir.size();
    }
    return true;
}

bool small_csc_symmetric(int n, const int *jc, const int *ir, const double *val) {
    if (n > 8) return false;
    double d[64] = {0.0};
    bool seen[64] = {false};
    for (int c = 0; c < n; c++)
        for (int k = jc[c]; k < jc[c + 1]; k++) {
            if (ir[k] < 0 || ir[k] >= n) return false;
            const int i = ir[k] * 8 + c;
            d[i] = seen[i] ? d[i] + val[k] : val[k];
            seen[i] = true;
        }
    for (int r = 0; r < n; r++)
        for (int c = 0; c < r; c++)
            if (d[r * 8 + c] != d[c * 8 + r]) return false;
    return true;
}

// =====================================================================================
// values in the caller's layout
// =====================================================================================
void ValueFold::set_canonical(long long nnz) {
    canon = true; unnz = nnz;
    uval.release(); cptr.release(); cidx.release();
    h_cptr.clear(); h_cidx.clear(); h_uval.clear();
}

hipError_t ValueFold::set_folded(std::vector<int> &&cptr_, std::vector<int> &&cidx_, long long unnz_, const double *val0, bool on_host) {
    canon = false; unnz = unnz_;
    if (on_host) {
        h_cptr = std::move(cptr_); h_cidx = std::move(cidx_);
        h_uval.assign(val0, val0 + unnz);
        uval.map(h_uval.data(), h_uval.data(), h_uval.size());
        return hipSuccess;
    }
    hipError_t e = uval.alloc(std::max<size_t>(unnz, 1), false);
    if (e == hipSuccess && val0) e = uval.upload(val0, unnz);
    if (e == hipSuccess) e = cptr.from(cptr_);
    if (e == hipSuccess) e = cidx.from(cidx_);
    return e;
}

hipError_t ValueFold::sum(DevBuf<double> &dst, int nnz, hipStream_t stream) {
    if (!uval.host) return rsqp_launch_fold(nnz, cptr.p, cidx.p, uval.p, dst.p, stream);
    for (int j = 0; j < nnz; j++) {
        int k = h_cptr[j];
        double t = h_uval[h_cidx[k]];
        for (k++; k < h_cptr[j + 1]; k++) t += h_uval[h_cidx[k]];
        dst.host[j] = t;
    }
    return hipSuccess;
}

int pool_csc(int nq, const int *nrow, const int *ncol, const int *jc, const int *ir, const double *val, PooledCsc &P) {
    long long ojc = 0, onz = 0;
    P.uoff.resize(nq);
    for (int q = 0; q < nq; q++) {
        const int *j = jc + ojc;
        if (const int f = csc_fault(nrow[q], ncol[q], j, ir + onz)) return f;
        if (!csc_is_canonical(ncol[q], j, ir + onz)) P.canon = false;
        P.uoff[q] = onz;
        ojc += ncol[q] + 1; onz += j[ncol[q]];
    }
    P.unnz = onz;
    P.jc = jc; P.ir = ir; P.val = val;
    if (P.canon) return 0;
    if (!val) return 4;
    // canonical slot j of the pool = sum of the caller's slots cidx[cptr[j] .. cptr[j+1])
    P.cptr.assign(1, 0);
    ojc = 0;
    for (int q = 0; q < nq; q++) {
        Compressed cu, ck;
        std::vector<int> cp, ci;
        const int *j = jc + ojc;
        const long long u0 = P.uoff[q];
        cu.nrow = nrow[q]; cu.ncol = ncol[q];
        cu.jc.assign(j, j + ncol[q] + 1); cu.ir.assign(ir + u0, ir + u0 + j[ncol[q]]); cu.val.assign(val + u0, val + u0 + j[ncol[q]]);
        const long long cbase = (long long)P.cidx.size();
        const bool folded = canonicalise(cu, ck, cp, ci);
        if (folded) {
            for (size_t t = 1; t < cp.size(); t++) P.cptr.push_back((int)(cbase + cp[t]));
            for (int u : ci) P.cidx.push_back((int)(u0 + u));
        } else {
            for (int t = 0; t < cu.nnz(); t++) { P.cidx.push_back((int)(u0 + t)); P.cptr.push_back((int)(cbase + t + 1)); }
        }
        const Compressed &c = folded ? ck : cu;
        P.kjc.insert(P.kjc.end(), c.jc.begin(), c.jc.end());
        P.kir.insert(P.kir.end(), c.ir.begin(), c.ir.end());
        P.kval.insert(P.kval.end(), c.val.begin(), c.val.end());
        ojc += ncol[q] + 1;
    }
    P.jc = P.kjc.data(); P.ir = P.kir.data(); P.val = P.kval.data();
    return 0;
}

hipError_t PooledCsc::fold_into(ValueFold &f) {
    if (canon) { f.set_canonical(unnz); return hipSuccess; }
    return f.set_folded(std::move(cptr), std::move(cidx), unnz, nullptr, false);
}

// =====================================================================================
// structure upload
// =====================================================================================
// every array the device needs for the canonical matrix `c`, computed once; where each is placed is DevMatrix::place's business
struct StructurePlan {
    const Compressed &c;   // jc, ir, order, tmap and the first values
    bool want_csr;
    std::vector<int4> blk_c, blk_r;
    CsrCopy r;
    std::vector<int> rorder;
};
static void plan_structure(StructurePlan &p) {
    const Compressed &c = p.c;
    p.blk_c = build_blocks(c.ncol, c.jc.data(), rsqp_spmv_chunk());
    if (!p.want_csr) return;
    csr_from_csc(c.nrow, c.ncol, c.jc.data(), c.ir.data(), p.r);
    // rorder = (CSC slot -> CSR slot) o order: where a refreshed triplet value lands in the CSR copy
    const int nnz = c.nnz();
    std::vector<int> inv(std::max(nnz, 1), 0);
    p.rorder.assign(std::max<size_t>(c.order.size(), 1), 0);
    for (int k = 0; k < nnz; k++) inv[p.r.perm[k]] = k;
    for (size_t i = 0; i < c.order.size(); i++) p.rorder[i] = inv[c.slot_of.empty() ? c.order[i] : c.slot_of[c.order[i]]];
    p.blk_r = build_blocks(c.nrow, p.r.rp.data(), rsqp_spmv_chunk());
}

hipError_t DevMatrix::reserve(int nrow_, int ncol_, bool mapped) {
    const size_t cap = (size_t)nrow_ * (size_t)ncol_ + 2 * (size_t)(nrow_ + ncol_) + 8;      // dense + an identity block or two
    arena_cap = 64 * cap + 64 * (size_t)(nrow_ + ncol_) + 4096;
    arena_mapped = mapped;
    hipError_t e;
    if (mapped) {
        e = hipHostMalloc(reinterpret_cast<void **>(&arena_stage), arena_cap, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&arena_dev), arena_stage, 0);
    } else {
        e = hipMalloc(reinterpret_cast<void **>(&arena_dev), arena_cap);
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&arena_stage), arena_cap, hipHostMallocDefault);
    }
    if (e == hipSuccess) {
        std::memset(arena_stage, 0, arena_cap);
        e = hipHostMalloc(&pin, 2 * (cap + 2) * sizeof(double), hipHostMallocMapped);
    }
    if (e != hipSuccess) { release_arena(); return e; }
    std::memset(pin, 0, 2 * (cap + 2) * sizeof(double));
    pin_cap = cap + 2;
    return hipSuccess;
}

void DevMatrix::drop_slices() {
    jc.release(); ir.release(); order.release(); tmap.release(); tv.release(); blk_c.release(); blk_r.release();
    rp.release(); ci.release(); perm.release(); rorder.release();
}

// the end of the arena and of the host-mapped values, at destruction, after a failed reserve() and when a matrix outgrows the arena
// (every array is then allocated on its own): the views into a block are dropped before the block is freed
void DevMatrix::release_arena() {
    if (arena_dev || arena_stage) drop_slices();
    if (pin) { val.release(); rval.release(); (void)hipHostFree(pin); }
    if (arena_dev && !arena_mapped) (void)hipFree(arena_dev);
    if (arena_stage) (void)hipHostFree(arena_stage);
    pin = nullptr; arena_dev = arena_stage = nullptr;
    pin_cap = arena_cap = arena_used = 0;
}

// one array: `padded` entries (the tail zero) in the next arena slice or in an allocation of its own, then the `count` entries of h.
// 1: the arena is too small
template <class T> int DevMatrix::put(DevBuf<T> &b, const T *h, size_t count, size_t padded, bool arena) {
    if (arena) {
        const size_t bytes = (std::max<size_t>(padded, 1) * sizeof(T) + 15) & ~(size_t)15;      // (slices are 16-byte aligned and zero-filled)
        if (arena_used + bytes > arena_cap) return 1;
        std::memset(arena_stage + arena_used, 0, bytes);
        b.carve(reinterpret_cast<T *>(arena_dev + arena_used), reinterpret_cast<T *>(arena_stage + arena_used), padded);
        arena_used += bytes;
    } else HIPCHK(b.alloc(padded, padded > count));
    HIPCHK(b.upload(h, count));
    return RSQP_OK;
}

hipError_t DevMatrix::csr_values(hipStream_t stream) {
    if (pin) { for (int k = 0; k < nnz; k++) rval.host[k] = val.host[h_perm[k]]; return hipSuccess; }
    return dense ? rsqp_launch_gather_dense(nrow, ncol, val.p, rval.p, stream) : rsqp_launch_gather(nnz, perm.p, val.p, rval.p, stream);
}

// the plan into the arena (no allocation; one asynchronous copy, none when the arena is host-mapped) or into allocations of its
// own. 1: the arena is too small for this matrix
int DevMatrix::place(const StructurePlan &p, bool arena, bool zero_copy, hipStream_t stream) {
    const Compressed &c = p.c;
    const size_t n = (size_t)nnz;
    if (arena) { arena_used = 0; drop_slices(); }      // (the values stay in the block reserve() made)
    else {
        if (pin) { val.release(); rval.release(); (void)hipHostFree(pin); pin = nullptr; pin_cap = 0; }
        if (zero_copy) { HIPCHK(hipHostMalloc(&pin, 2 * (n + 2) * sizeof(double), hipHostMallocMapped)); pin_cap = n + 2; }
    }
    if (pin) {
        void *dev = nullptr;
        HIPCHK(hipHostGetDevicePointer(&dev, pin, 0));
        val.map(static_cast<double *>(dev), static_cast<double *>(pin), pin_cap);
        rval.map(static_cast<double *>(dev) + pin_cap, static_cast<double *>(pin) + pin_cap, pin_cap);
        std::memset(pin, 0, 2 * pin_cap * sizeof(double));
    } else {
        HIPCHK(val.alloc(n + 2, true));
        if (p.want_csr) HIPCHK(rval.alloc(n + 2, true));
    }
    HIPCHK(val.upload(c.val.data(), c.val.size()));
    int rc;
    auto ok = [&rc](int r) { return (rc = r) == RSQP_OK; };
    if (!(ok(put(jc, c.jc.data(), c.jc.size(), c.jc.size(), arena)) && ok(put(ir, c.ir.data(), n, n + 2, arena)) &&
          ok(put(order, c.order.data(), c.order.size(), std::max<size_t>(c.order.size(), 1), arena)) &&
          ok(put(tv, (const double *)nullptr, 0, std::max(unnz(), 1), arena)) &&
          ok(put(blk_c, p.blk_c.data(), p.blk_c.size(), p.blk_c.size(), arena))))
        return rc;
    if (c.tmap.empty()) tmap.release();
    else if (!ok(put(tmap, c.tmap.data(), c.tmap.size(), c.tmap.size(), arena))) return rc;
    if (p.want_csr &&
        !(ok(put(rp, p.r.rp.data(), p.r.rp.size(), p.r.rp.size(), arena)) && ok(put(ci, p.r.ci.data(), n, n + 2, arena)) &&
          ok(put(perm, p.r.perm.data(), n, std::max<size_t>(n, 1), arena)) &&
          ok(put(rorder, p.rorder.data(), p.rorder.size(), p.rorder.size(), arena)) &&
          ok(put(blk_r, p.blk_r.data(), p.blk_r.size(), p.blk_r.size(), arena))))
        return rc;
    nblk_c = (int)p.blk_c.size(); nblk_r = (int)p.blk_r.size();
    have_csr = p.want_csr;
    if (arena && !arena_mapped) HIPCHK(hipMemcpyAsync(arena_dev, arena_stage, arena_used, hipMemcpyHostToDevice, stream));
    if (p.want_csr) {
        h_rorder = p.rorder; h_perm = p.r.perm;
        if (csr_values(nullptr) != hipSuccess) return rsqp_fail_msg(RSQP_ERR_DEVICE, "gather launch failed");
    }
    return RSQP_OK;
}

int DevMatrix::set_structure(const Compressed &cu, bool want_csr, bool zero_copy, hipStream_t stream) {
    Compressed ck;
    std::vector<int> cptr, cidx;
    const bool folded = canonicalise(cu, ck, cptr, cidx);
    StructurePlan p{folded ? ck : cu, want_csr};
    const Compressed &c = p.c;
    plan_structure(p);
    nrow = c.nrow; ncol = c.ncol; nnz = c.nnz();
    dense = (long long)nnz == (long long)nrow * ncol;   // (canonical: every position of every column, rows in order)
    h_jc = c.jc; h_ir = c.ir; h_order = c.order; h_tmap = c.tmap;
    fold.set_canonical(cu.nnz());
    if (folded) { h_ujc = cu.jc; h_uir = cu.ir; }
    else { h_ujc.clear(); h_uir.clear(); }
    int rc = 1;
    if (zero_copy && arena_dev && pin && (size_t)nnz + 2 <= pin_cap) {
        // (an earlier copy of the staging mirror may still be on its way -- or, mapped arena, a kernel may still be reading the old
        //  structure; nothing can be when the matrix is set for the first time)
        if (!(arena_mapped && !initialised)) (void)hipStreamSynchronize(stream);
        rc = place(p, true, true, stream);
        if (rc == 1) release_arena();
    }
    if (rc == 1) rc = place(p, false, zero_copy, stream);
    if (rc != RSQP_OK) return rc;
    initialised = true;
    // the caller's values: next to the host-mapped canonical ones, or on the device with the fold map
    if (folded) HIPCHK(fold.set_folded(std::move(cptr), std::move(cidx), cu.nnz(), cu.val.data(), pin != nullptr));
    return RSQP_OK;
}

// =====================================================================================
// value refresh
// =====================================================================================
int DevMatrix::refresh(const double *v, int n, RefreshKind kind, hipStream_t stream) {
    DevBuf<double> &u = fold.canon ? val : fold.uval;             // the values in the caller's layout
    const bool fused = kind == REFRESH_TRIPLET_A && fold.canon;   // every value goes to its CSC slot and to its slot of the CSR copy
    // SpHbMat::setMatVal(rhs, I_info): only the first nnz(J) entries of [J I -I] are rewritten, the identity entries keep their values
    // in both copies (SpHbMat.cpp:368-380); every entry of H is, a mirrored one from the triplet entry it mirrors
    const int cnt = kind == REFRESH_TRIPLET_H ? unnz() : n;
    hipError_t e = hipSuccess;
    if (kind == REFRESH_CSC) HIPCHK(u.upload(v, n));
    else if (pin) {
        // host-mapped values: the scatter through order_ is a host loop
        if (fused) for (int i = 0; i < n; i++) { u.host[h_order[i]] = v[i]; rval.host[h_rorder[i]] = v[i]; }
        else for (int j = 0; j < cnt; j++) u.host[h_order[j]] = v[h_tmap.empty() ? j : h_tmap[j]];
    } else {
        HIPCHK(tv.upload(v, n));
        e = fused ? rsqp_launch_scatter_csc_csr(n, order.p, rorder.p, tv.p, val.p, rval.p, stream)
                  : rsqp_launch_scatter(cnt, order.p, kind == REFRESH_TRIPLET_H ? tmap.p : nullptr, tv.p, u.p, stream);
    }
    // repeated positions or rows out of order: the canonical values are the sums of the caller's
    if (e == hipSuccess && !fold.canon) e = fold.sum(val, nnz, stream);
    if (e != hipSuccess) return rsqp_fail_msg(RSQP_ERR_DEVICE, "value refresh launch failed");
    if (have_csr && !fused && csr_values(stream) != hipSuccess) return rsqp_fail_msg(RSQP_ERR_DEVICE, "gather launch failed");
    return RSQP_OK;
}
