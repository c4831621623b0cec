// rsqp_spmv_plan.hip -- the batched SpMV plan of include/rsqp_hip.h (rsqp_spmv_plan_*): host side only, the kernels are sparse.hip.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "rsqp_host.h"
#include "rsqp_matrix.h"
#include "rsqp_sparse.h"

namespace {
// entry-parallel SpMV variant (sparse.hip csx_ldsvec_segscan): chunks of whole majors with at most 512 entries and 128 majors, one
// "starts a major" bit per entry (16 words per chunk), the non-empty majors in order, the empty ones
struct SegHost {
    std::vector<int4> chunks;
    std::vector<int> nz, empties;
    std::vector<unsigned> bits;
    bool ok = true;
};
SegHost build_seg(int nmajor, const int *ptr) {
    constexpr int CH = 512;
    SegHost h;
    for (int c = 0; c < nmajor; c++) {
        const int len = ptr[c + 1] - ptr[c];
        if (len == 0) h.empties.push_back(c);
        else { h.nz.push_back(c); if (len > CH) h.ok = false; }
    }
    if (!h.ok) return h;
    size_t i = 0;
    while (i < h.nz.size()) {
        const int e0 = ptr[h.nz[i]];
        size_t j = i;
        unsigned w[16] = {0};
        while (j < h.nz.size() && ptr[h.nz[j] + 1] - e0 <= CH && j - i < 128) {     // <= 128 majors: the kernel's LDS window
            const int b = ptr[h.nz[j]] - e0;
            w[b >> 5] |= 1u << (b & 31);
            j++;
        }
        const int nent = ptr[h.nz[j - 1] + 1] - e0;
        if (nent < CH) w[nent >> 5] |= 1u << (nent & 31);      // one bit behind the last entry: what a lane loads past the chunk
                                                               // becomes a dummy major that the kernel never stores
        h.chunks.push_back(make_int4(e0, (int)i, nent, (int)(j - i)));
        h.bits.insert(h.bits.end(), w, w + 16);
        i = j;
    }
    return h;
}
}  // namespace

// =====================================================================================
// batched SpMV plan (device resident)
// =====================================================================================
struct rsqp_spmv_plan {
    int nrow = 0, ncol = 0, nnz = 0, nbatch = 0, device = 0;
    int nblk_c = 0, nblk_r = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // every member owns a full copy of the index arrays: distinct HBM traffic per matrix
    DevBuf<int> jc, ir, rp, ci, perm;
    DevBuf<int4> blk_c, blk_r;
    DevBuf<int> slice_c, slice_r;   // one slice = all majors (1 workgroup per member)
    DevBuf<unsigned short> ir16, ci16;  // 16-bit index copies (vector length < 65536)
    // entry-parallel variant 40: per orientation (t: CSC majors = columns, n: CSR majors = rows)
    DevBuf<int4> seg_chunks[2];
    DevBuf<int> seg_nz[2], seg_empt[2];
    DevBuf<unsigned> seg_bits[2];       // one copy per member, like the index arrays
    int seg_nchunks[2] = {0, 0}, seg_nempty[2] = {0, 0};
    bool seg_ok[2] = {false, false};
    bool use16 = false;
    int variant_t = 0, variant_n = 0;  // 0: stream kernel; >0: LDS-resident-vector kernel
    int nslices = 1;
    DevBuf<double> val, rval, vin_r, vin_c, vout_r, vout_c;  // _r: length nrow, _c: length ncol
    ~rsqp_spmv_plan() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

extern "C" int rsqp_spmv_plan_create(int nrow, int ncol, const int *jc, const int *ir, int nbatch, int device,
                                     rsqp_spmv_plan **out) {
    if (!out || nrow <= 0 || ncol <= 0 || !jc || !ir || nbatch <= 0) return fail(RSQP_ERR_ARG, "rsqp_spmv_plan_create");
    if (rsqp_device_count() <= 0) return fail(RSQP_ERR_DEVICE, "rsqp_spmv_plan_create: no HIP device visible");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    rsqp_spmv_plan *p = new rsqp_spmv_plan();
    struct Guard { rsqp_spmv_plan *p; ~Guard() { delete p; } } guard{p};
    p->nrow = nrow; p->ncol = ncol; p->nnz = jc[ncol]; p->nbatch = nbatch;
    HIPCHK(hipGetDevice(&p->device));
    HIPCHK(hipStreamCreate(&p->stream));
    HIPCHK(hipEventCreate(&p->ev0)); HIPCHK(hipEventCreate(&p->ev1));
    CsrCopy r;
    csr_from_csc(nrow, ncol, jc, ir, r);
    std::vector<int4> bc = build_blocks(ncol, jc, rsqp_spmv_chunk()), br = build_blocks(nrow, r.rp.data(), rsqp_spmv_chunk());
    p->nblk_c = (int)bc.size(); p->nblk_r = (int)br.size();
    HIPCHK(p->blk_c.from(bc)); HIPCHK(p->blk_r.from(br));
    {
        const char *es = getenv("RSQP_SPMV_SLICES");
        p->nslices = es ? std::max(1, atoi(es)) : 1;
        auto cut = [&](int nmajor, const int *pt) {
            std::vector<int> sl(p->nslices + 1, nmajor);
            sl[0] = 0;
            for (int q = 1; q < p->nslices; q++) {   // equal share of entries per slice
                long long target = (long long)pt[nmajor] * q / p->nslices;
                sl[q] = (int)(std::lower_bound(pt, pt + nmajor + 1, (int)target) - pt);
            }
            return sl;
        };
        std::vector<int> sc = cut(ncol, jc), sr = cut(nrow, r.rp.data());
        HIPCHK(p->slice_c.from(sc)); HIPCHK(p->slice_r.from(sr));
        // default kernel choice: vector in LDS when it fits and the batch can fill the chip
        const char *ev = getenv("RSQP_SPMV_VARIANT");
        int forced = ev ? atoi(ev) : -1;
        bool fits_t = (size_t)nrow * 8 + 16 <= 160 * 1024, fits_n = (size_t)ncol * 8 + 16 <= 160 * 1024;
        // lanes per major by average segment length (measured on MI355X, tools/spmv_sweep.py):
        // >= 16 entries: 4 lanes x 2 entries x 3 steps; shorter: 2 lanes x 2 entries x 4 steps
        auto pick = [](double avg) { return avg >= 16.0 ? 35 : 38; };
        p->variant_t = forced >= 0 ? forced : (fits_t && nbatch >= 64 ? pick((double)p->nnz / ncol) : 0);
        p->variant_n = forced >= 0 ? forced : (fits_n && nbatch >= 64 ? pick((double)p->nnz / nrow) : 0);
        if (!fits_t) p->variant_t = 0;
        if (!fits_n) p->variant_n = 0;
    }
    const size_t B = nbatch, nnz = p->nnz;
    HIPCHK(p->jc.alloc(B * (ncol + 1), false)); HIPCHK(p->ir.alloc(B * nnz + 2, false));
    HIPCHK(p->rp.alloc(B * (nrow + 1), false)); HIPCHK(p->ci.alloc(B * nnz + 2, false));
    HIPCHK(p->perm.from(r.perm));
    for (size_t m = 0; m < B; m++) {
        HIPCHK(hipMemcpy(p->jc.p + m * (ncol + 1), jc, sizeof(int) * (ncol + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->ir.p + m * nnz, ir, sizeof(int) * nnz, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->rp.p + m * (nrow + 1), r.rp.data(), sizeof(int) * (nrow + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(p->ci.p + m * nnz, r.ci.data(), sizeof(int) * nnz, hipMemcpyHostToDevice));
    }
    HIPCHK(p->val.alloc(B * nnz + 528)); HIPCHK(p->rval.alloc(B * nnz + 528));   // variant 40 reads (and masks) up to 520 entries past a chunk
    {
        const char *e16 = getenv("RSQP_SPMV_IDX16");
        p->use16 = nrow < 65536 && ncol < 65536 && !(e16 && atoi(e16) == 0);
        if (p->use16) {
            std::vector<unsigned short> a16(ir, ir + nnz), c16(r.ci.begin(), r.ci.end());
            HIPCHK(p->ir16.alloc(B * nnz + 528, true)); HIPCHK(p->ci16.alloc(B * nnz + 528, true));
            for (size_t m = 0; m < B; m++) {
                HIPCHK(hipMemcpy(p->ir16.p + m * nnz, a16.data(), 2 * nnz, hipMemcpyHostToDevice));
                HIPCHK(hipMemcpy(p->ci16.p + m * nnz, c16.data(), 2 * nnz, hipMemcpyHostToDevice));
            }
        }
    }
    // entry-parallel kernel (variant 40): needs the 16-bit indices and majors of at most 512 entries; preferred over the
    // sub-wave-per-major kernels wherever those would be chosen (see the measurements below)
    if (p->use16) {
        const char *ev = getenv("RSQP_SPMV_VARIANT");
        const int forced = ev ? atoi(ev) : -1;
        for (int o = 0; o < 2; o++) {
            SegHost h = build_seg(o == 0 ? ncol : nrow, o == 0 ? jc : r.rp.data());
            if (!h.ok || h.chunks.empty()) continue;
            HIPCHK(p->seg_chunks[o].from(h.chunks)); HIPCHK(p->seg_nz[o].from(h.nz));
            HIPCHK(p->seg_empt[o].alloc(std::max<size_t>(h.empties.size(), 1))); HIPCHK(p->seg_empt[o].upload(h.empties.data(), h.empties.size()));
            HIPCHK(p->seg_bits[o].alloc(B * h.bits.size(), false));
            for (size_t m = 0; m < B; m++)
                HIPCHK(hipMemcpy(p->seg_bits[o].p + m * h.bits.size(), h.bits.data(), 4 * h.bits.size(), hipMemcpyHostToDevice));
            p->seg_nchunks[o] = (int)h.chunks.size(); p->seg_nempty[o] = (int)h.empties.size();
            p->seg_ok[o] = true;
            // measured on the 10k x 20k shape (tools/spmv_bound_check.py): majors of ~20 entries 0.120 ms vs 0.133 ms for the
            // sub-wave kernel <4,3>; majors of ~10 entries 0.128 vs 0.136 ms for <2,4>. Majors shorter than ~8 entries
            // (the [J I -I] columns) would leave the 128-major chunks mostly empty: those stay with <2,4>
            int &var = o == 0 ? p->variant_t : p->variant_n;
            const double avg = (double)p->nnz / std::max<size_t>(h.nz.size(), 1);
            if (forced < 0 ? (var == 35 || (var == 38 && avg >= 8.0)) : forced == 40) var = 40;
        }
    }
    if (p->variant_t == 40 && !p->seg_ok[0]) p->variant_t = 0;
    if (p->variant_n == 40 && !p->seg_ok[1]) p->variant_n = 0;
    HIPCHK(p->vin_r.alloc(B * nrow)); HIPCHK(p->vin_c.alloc(B * ncol));
    HIPCHK(p->vout_r.alloc(B * nrow)); HIPCHK(p->vout_c.alloc(B * ncol));
    guard.p = nullptr;
    *out = p;
    return RSQP_OK;
}

extern "C" void rsqp_spmv_plan_destroy(rsqp_spmv_plan *p) { delete p; }

extern "C" int rsqp_spmv_plan_upload(rsqp_spmv_plan *p, const double *vals, const double *xin, int transposed) {
    if (!p) return fail(RSQP_ERR_ARG, "null plan");
    HIPCHK(hipSetDevice(p->device));
    const size_t B = p->nbatch;
    if (vals) {
        HIPCHK(p->val.upload(vals, B * p->nnz));
        for (size_t m = 0; m < B; m++)
            if (rsqp_launch_gather(p->nnz, p->perm.p, p->val.p + m * p->nnz, p->rval.p + m * p->nnz, p->stream) != hipSuccess)
                return fail(RSQP_ERR_DEVICE, "gather launch failed");
        HIPCHK(hipStreamSynchronize(p->stream));
    }
    if (xin) {
        if (transposed) HIPCHK(p->vin_r.upload(xin, B * p->nrow));
        else HIPCHK(p->vin_c.upload(xin, B * p->ncol));
    }
    return RSQP_OK;
}

extern "C" int rsqp_spmv_plan_run(rsqp_spmv_plan *p, int transposed, int repeats, float *ms_per_launch) {
    if (!p || repeats <= 0) return fail(RSQP_ERR_ARG, "rsqp_spmv_plan_run");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipEventRecord(p->ev0, p->stream));
    for (int r = 0; r < repeats; r++) {
        hipError_t e;
        if (transposed && p->variant_t == 40)
            e = rsqp_launch_spmv_segscan(p->nrow, p->seg_chunks[0].p, p->seg_nchunks[0], p->seg_nz[0].p, p->seg_empt[0].p, p->seg_nempty[0],
                                         p->seg_bits[0].p, p->ir16.p, p->val.p, p->vin_r.p, p->vout_c.p, p->nbatch, p->nnz, p->nrow, p->ncol, p->stream);
        else if (!transposed && p->variant_n == 40)
            e = rsqp_launch_spmv_segscan(p->ncol, p->seg_chunks[1].p, p->seg_nchunks[1], p->seg_nz[1].p, p->seg_empt[1].p, p->seg_nempty[1],
                                         p->seg_bits[1].p, p->ci16.p, p->rval.p, p->vin_c.p, p->vout_r.p, p->nbatch, p->nnz, p->ncol, p->nrow, p->stream);
        else if (transposed && p->variant_t > 0)
            e = rsqp_launch_spmv_ldsvec(p->variant_t, p->nrow, p->nslices, p->slice_c.p, p->jc.p, p->ir.p, p->use16 ? p->ir16.p : nullptr, p->val.p, p->vin_r.p,
                                        p->vout_c.p, p->nbatch, p->ncol + 1, p->nnz, p->nrow, p->ncol, p->stream);
        else if (!transposed && p->variant_n > 0)
            e = rsqp_launch_spmv_ldsvec(p->variant_n, p->ncol, p->nslices, p->slice_r.p, p->rp.p, p->ci.p, p->use16 ? p->ci16.p : nullptr, p->rval.p, p->vin_c.p,
                                        p->vout_r.p, p->nbatch, p->nrow + 1, p->nnz, p->ncol, p->nrow, p->stream);
        else if (transposed)  // A'y on the CSC arrays (SpHbMat::transposed_times)
            e = rsqp_launch_spmv(p->blk_c.p, p->nblk_c, p->jc.p, p->ir.p, p->val.p, p->vin_r.p, p->vout_c.p, p->nbatch,
                                 p->ncol + 1, p->nnz, p->nrow, p->ncol, p->stream);
        else             // A x on the CSR copy (SpHbMat::times)
            e = rsqp_launch_spmv(p->blk_r.p, p->nblk_r, p->rp.p, p->ci.p, p->rval.p, p->vin_c.p, p->vout_r.p, p->nbatch,
                                 p->nrow + 1, p->nnz, p->ncol, p->nrow, p->stream);
        if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, "spmv launch failed");
    }
    HIPCHK(hipEventRecord(p->ev1, p->stream));
    HIPCHK(hipEventSynchronize(p->ev1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p->ev0, p->ev1));
    if (ms_per_launch) *ms_per_launch = ms / repeats;
    return RSQP_OK;
}

extern "C" int rsqp_spmv_plan_variant(const rsqp_spmv_plan *p, int transposed, int *idx16) {
    if (!p) return fail(RSQP_ERR_ARG, "null plan");
    if (idx16) *idx16 = p->use16 ? 1 : 0;
    return transposed ? p->variant_t : p->variant_n;
}

extern "C" int rsqp_spmv_plan_download(rsqp_spmv_plan *p, double *out, int transposed) {
    if (!p || !out) return fail(RSQP_ERR_ARG, "rsqp_spmv_plan_download");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (transposed) HIPCHK(p->vout_c.download(out, (size_t)p->nbatch * p->ncol));
    else HIPCHK(p->vout_r.download(out, (size_t)p->nbatch * p->nrow));
    return RSQP_OK;
}
