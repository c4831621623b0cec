// rsqp_matrix.h -- how a caller's matrix becomes device arrays (host side; rsqp_matrix.hip).
//
// The one decision of this module: the device holds the CANONICAL CSC of a matrix (rows strictly ascending within each column, one
// entry per position), a CSR copy of it where products by rows are wanted, and -- where the caller's layout is not canonical -- the
// caller's values with a fold map from each canonical slot to the caller's slots. SpHbMat::setStructure is DevMatrix::set_structure,
// SpHbMat::setMatVal is DevMatrix::refresh. The C ABI (rsqp_api.hip, rsqp_batch.hip) reads the device arrays; it does not know how they are filled.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "rsqp_host.h"
#include "rsqp_sparse.h"

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    T *host = nullptr;   // non-null: p is the device view of host-mapped pinned memory owned elsewhere
    T *stage = nullptr;  // non-null: p is a slice of a device arena owned elsewhere and `stage` the same slice of its pinned staging
                         // mirror -- uploads are written there, the owner copies the arena to the device in ONE piece (DevMatrix)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && !host && !stage) (void)hipFree(p);
        p = nullptr;
        host = nullptr;
        stage = nullptr;
        n = 0;
    }
    void map(T *dev, T *hst, size_t count) { release(); p = dev; host = hst; n = count; }
    void carve(T *dev, T *stg, size_t count) { release(); p = dev; stage = stg; n = count; }
    hipError_t alloc(size_t count, bool zero = true) {
        release();
        n = count;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) { p = nullptr; return e; }
        if (zero) e = hipMemset(p, 0, std::max<size_t>(count, 1) * sizeof(T));
        return e;
    }
    hipError_t upload(const T *h, size_t count) {
        if (count == 0) return hipSuccess;
        if (host) { std::memcpy(host, h, count * sizeof(T)); return hipSuccess; }
        if (stage) { std::memcpy(stage, h, count * sizeof(T)); return hipSuccess; }     // (reaches the device with the arena)
        return hipMemcpy(p, h, count * sizeof(T), hipMemcpyHostToDevice);
    }
    hipError_t from(const std::vector<T> &h) {
        hipError_t e = alloc(h.size(), false);
        if (e != hipSuccess) return e;
        return upload(h.data(), h.size());
    }
    hipError_t download(T *h, size_t count) const {
        if (count == 0) return hipSuccess;
        if (host) { std::memcpy(h, host, count * sizeof(T)); return hipSuccess; }   // caller has synchronised
        return hipMemcpy(h, p, count * sizeof(T), hipMemcpyDeviceToHost);
    }
};

// ---------------------------------------------------------------------------------
// structure analysis (host, one-off)
// ---------------------------------------------------------------------------------
struct Compressed {
    int nrow = 0, ncol = 0;
    std::vector<int> jc, ir, order, tmap;  // CSC; order[ext] = position; tmap[ext] = triplet index
    std::vector<int> slot_of;              // canonical form of a non-canonical layout (canonicalise): caller slot -> canonical slot
    std::vector<double> val;
    int nnz() const { return (int)ir.size(); }
};
struct CsrCopy {
    std::vector<int> rp, ci, perm;  // perm[p] = CSC position of CSR entry p
};

// SpHbMat::setStructure: sort the (extended) triplet list by (col,row); ties by position.
void csc_from_entries(int nrow, int ncol, const std::vector<int> &row1, const std::vector<int> &col1,
                      const std::vector<double> &v, Compressed &out);
void csr_from_csc(int nrow, int ncol, const int *jc, const int *ir, CsrCopy &out);
// blocks of consecutive majors with at most `chunk` entries; a longer major stands alone
std::vector<int4> build_blocks(int nmajor, const int *ptr, int chunk);

// what is wrong with a CSC array from outside: nothing, or the first of
enum { CSC_OK = 0, CSC_START = 1 /* jc[0] != 0 */, CSC_MONOTONE = 2 /* jc[c] > jc[c+1] */, CSC_ROW = 3 /* a row outside [0, nrow) */ };
int csc_fault(int nrow, int ncol, const int *jc, const int *ir);
// rows strictly ascending within each column (of a CSC array that csc_fault accepts)
bool csc_is_canonical(int ncol, const int *jc, const int *ir);

// The matrix a CSC array or a triplet list describes is the SUM of its entries (SpHbMat::times; contract of rsqp_hip.h). Every
// consumer -- products, certificate, CSR copy, dense copies, the engines' staging of A and H -- reads the canonical form. A caller's
// layout that is not canonical (rows out of order, repeated positions) is folded ONCE, at structure upload. Returns false when `c`
// is canonical already: nothing is built. Otherwise `k` is the canonical matrix (with the caller's order / tmap and slot_of) and
// its slot j the sum of the caller's slots cidx[cptr[j] .. cptr[j+1]), in the caller's order -- what ValueFold::sum adds up.
bool canonicalise(const Compressed &c, Compressed &k, std::vector<int> &cptr, std::vector<int> &cidx);

// is the matrix of a CSC array (n <= 8 columns) symmetric, value by value? (eligibility of the tableau kernel of qp_tiny.hip)
// (any layout: entries that repeat a position are summed in their order, as canonicalise sums them)
bool small_csc_symmetric(int n, const int *jc, const int *ir, const double *val);

// ---------------------------------------------------------------------------------
// values given in the caller's layout
// ---------------------------------------------------------------------------------
// A canonical layout needs nothing: the caller's values ARE the canonical ones. Otherwise the caller's values are kept beside the
// canonical ones with the fold map (canonicalise) -- on the device, or on the host where the canonical values are host-mapped.
struct ValueFold {
    bool canon = true;
    long long unnz = 0;               // entries of the caller's layout (= canonical entries when canon)
    DevBuf<double> uval;              // the caller's values (host: a view of h_uval that no kernel reads)
    DevBuf<int> cptr, cidx;           // device fold map
    std::vector<int> h_cptr, h_cidx;  // host fold map (host form only)
    std::vector<double> h_uval;
    void set_canonical(long long nnz);
    // (val0: the first values of the caller's layout, or null where every refresh rewrites all of them)
    hipError_t set_folded(std::vector<int> &&cptr_, std::vector<int> &&cidx_, long long unnz_, const double *val0, bool on_host);
    // dst[j] = sum of the caller's values of canonical slot j, in the caller's order (host loop and fold_values of sparse.hip add alike)
    hipError_t sum(DevBuf<double> &dst, int nnz, hipStream_t stream);
};

// the pooled CSC matrices of a batch (member q: nrow[q] x ncol[q]; its column pointers start at 0 and index its own slice). When some
// member's layout is not canonical, the canonical pools are built (canonicalise, member by member) and jc / ir / val point at them,
// else at the caller's arrays
struct PooledCsc {
    const int *jc = nullptr, *ir = nullptr;
    const double *val = nullptr;
    bool canon = true;
    long long unnz = 0;                  // entries of the caller's pool
    std::vector<long long> uoff;         // member q's entries in the caller's pool start at uoff[q]
    std::vector<int> kjc, kir, cptr, cidx;
    std::vector<double> kval;
    hipError_t fold_into(ValueFold &f);  // the fold state of the pool: every refresh brings all values (hands the fold map over)
};
// 0, or what csc_fault finds in the first member it refuses, or 4: a non-canonical pool without values
int pool_csc(int nq, const int *nrow, const int *ncol, const int *jc, const int *ir, const double *val, PooledCsc &P);

// ---------------------------------------------------------------------------------
// one matrix on the device (CSC + optional CSR copy + spmv blocks)
// ---------------------------------------------------------------------------------
enum RefreshKind {
    REFRESH_TRIPLET_A,   // n triplet values of J in [J I -I]: through order to the CSC and through rorder to the CSR copy
    REFRESH_TRIPLET_H,   // n triplet values of H: through order and tmap (a symmetric H mirrors each off-diagonal entry)
    REFRESH_CSC          // n values in the caller's CSC layout
};

struct StructurePlan;   // rsqp_matrix.hip: every array set_structure derives from the canonical matrix

struct DevMatrix {
    int nrow = 0, ncol = 0, nnz = 0;   // nnz: entries of the canonical form, the one every consumer reads (canonicalise)
    ValueFold fold;                    // the caller's layout where it is not canonical
    int unnz() const { return (int)fold.unnz; }   // entries of the caller's layout: rsqp_get_*_nnz, rsqp_get_*_csc, order_
    bool dense = false;                // the canonical pattern stores every entry: the CSR copy is a tiled transpose of the values
    bool initialised = false, symmetric = false, from_triplet = false;
    int n_ident_entries = 0, n_triplet = 0;
    double structure_seconds = 0.0;   // one-off structure analysis (setStructure: sort + CSC / CSR / SpMV plan + upload), rsqp_get_structure_seconds
    std::vector<int> h_jc, h_ir, h_order;  // host mirror of the (canonical) pattern; order[triplet entry] = slot of the caller's layout
    std::vector<int> h_ujc, h_uir;         // the pattern of a non-canonical caller layout
    const std::vector<int> &caller_jc() const { return fold.canon ? h_jc : h_ujc; }
    const std::vector<int> &caller_ir() const { return fold.canon ? h_ir : h_uir; }
    const DevBuf<double> &caller_val() const { return fold.canon ? val : fold.uval; }
    DevBuf<int> jc, ir, order, tmap;                 // CSC
    DevBuf<int4> blk_c, blk_r;
    DevBuf<double> val, tv;                          // tv: staging for triplet values
    DevBuf<int> rp, ci, perm, rorder;                // CSR copy (A only); rorder[i] = CSR position of triplet entry i (fused value refresh)
    DevBuf<double> rval;
    int nblk_c = 0, nblk_r = 0;
    bool have_csr = false;
    // LDS-scale single-QP handles: the VALUES (CSC and CSR copy) live in host-mapped pinned memory that the kernels read
    // directly -- a value refresh (SpHbMat::setMatVal through order_) is then a host loop over a few dozen entries, no copy
    // and no launch (a blocking hipMemcpy + a scatter launch cost ~15 us per matrix per SQP iteration of hs071)
    void *pin = nullptr;
    size_t pin_cap = 0;                    // entries each of the two value arrays in `pin` can hold
    std::vector<int> h_rorder, h_tmap, h_perm;
    // ... and everything else the structure analysis uploads (pattern, permutations, SpMV plan) is a slice of ONE device arena
    // with a pinned staging mirror, both allocated by rsqp_create -- where the reference allocates as well
    // (Algorithm::allocate_memory), outside the first SQP iteration: set_A / set_H of that iteration then cost one asynchronous
    // copy instead of 17 hipMalloc + 15 blocking hipMemcpy + 2 hipHostMalloc (365 -> ~90 us for the first iteration of hs071)
    char *arena_dev = nullptr, *arena_stage = nullptr;
    size_t arena_cap = 0, arena_used = 0;
    bool arena_mapped = false;             // the arena IS its staging mirror (host-mapped memory): no copy at all -- the kernels read the few
                                           // dozen pattern words of an hs071-scale matrix over the link, as they read its values already
    ~DevMatrix() { release_arena(); }

    // arena and host-mapped values for an nrow_ x ncol_ matrix. A failed reservation leaves "no arena": set_structure then allocates
    // per array, as it does for a matrix the arena turns out too small for
    hipError_t reserve(int nrow_, int ncol_, bool mapped = false);
    // SpHbMat::setStructure. `cu` is the caller's layout; the device receives its canonical form. zero_copy: host-mapped values
    // (and the arena, if reserved). With an arena: no allocation, one asynchronous copy on `stream` (none when the arena is mapped)
    int set_structure(const Compressed &cu, bool want_csr, bool zero_copy = false, hipStream_t stream = nullptr);
    // SpHbMat::setMatVal. The caller has waited for every kernel that may still read host-mapped values (`pin`): on that path this
    // is host loops only, no HIP call
    int refresh(const double *v, int n, RefreshKind kind, hipStream_t stream);

private:
    void release_arena();                                     // mapped views and slices first, then the blocks they view
    void drop_slices();
    template <class T> int put(DevBuf<T> &b, const T *h, size_t count, size_t padded, bool arena);
    int place(const StructurePlan &p, bool arena, bool zero_copy, hipStream_t stream);
    hipError_t csr_values(hipStream_t stream);               // the values of the CSR copy from the canonical CSC values
};
