// rsqp_api.hip -- the C ABI of include/rsqp_hip.h (host side of librsqp_hip.so): the library functions and the single handle
// (rsqp_solver). The batch is rsqp_batch.hip, the batched SpMV plan rsqp_spmv_plan.hip; what they share is rsqp_host.h.
//
// Host logic restated from the reference adapter src/qpOASESInterface.cpp: the
// FIXED/VARIED warm-start dispatch (:137-224, :817-833), dirty flags (:361-496),
// handle_error (:686-758), status mapping (:332-357). How a matrix becomes device arrays
// (SpHbMat::setStructure, setMatVal) is rsqp_matrix.h; every other per-iteration operation
// (products, certificate, QP solve) is a kernel.
#include <algorithm>
#include <cmath>
#include <chrono>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "rsqp_host.h"
#include "rsqp_large.h"
#include "rsqp_matrix.h"
#include "rsqp_small_plan.h"
#include "rsqp_sparse.h"

namespace { thread_local std::string g_err; }
int rsqp_fail_msg(int code, const char *msg) {
    g_err = msg ? msg : "";
    return code;
}

struct rsqp_solver {
    int nV = 0, nC = 0, device = 0;
    int qp_maxiter = 1000, lp_maxiter = 100;
    hipStream_t stream = nullptr;
    DevMatrix A, H;
    // host staging of the vectors (scalar setter storm of QPhandler::update_bounds)
    std::vector<double> h_vec[5];
    bool vec_dirty = true;
    DevBuf<double> d_vec[5];
    // engine pools (batch of one)
    DevBuf<QPDesc> d_desc;
    DevBuf<double> d_x, d_y, d_obj, d_state, d_x0, d_y0;
    DevBuf<int> d_wsb, d_wsc, d_status, d_ret, d_nwsr, d_nflips, d_guess;
    DevBuf<int> d_dummy_i; DevBuf<double> d_dummy_d;
    // certificate scratch
    DevBuf<double> d_Ax, d_ATy, d_Hx, d_kkt, d_in, d_out;
    DevBuf<int> d_Wb, d_Wc;
    // results mirrored on the host
    std::vector<double> h_x, h_y;
    std::vector<int> h_wsb, h_wsc;
    int status_word = QPS_NOTINITIALISED, last_ret = 0, last_nflips = 0;
    double obj = 0.0;
    // dispatch state (qpOASESInterface.hpp:225-250)
    bool firstQPsolved = false;
    bool upd_A = false, upd_H = false, upd_bounds = false, upd_g = false;
    int old_status = 0, new_status = 0;  // 0 UNDEFINED, 1 FIXED, 2 VARIED
    bool desc_ready = false;
    // small problems: vectors in and results out live in ONE host-mapped pinned block that the
    // kernels read / write directly (zero-copy): a solve costs one launch and one sync
    void *io_host = nullptr;
    int *d_done = nullptr, *h_done = nullptr;   // host-mapped completion word of single-QP solves (spun on by rsqp_solve)
    // the certificate of a single LDS-scale QP is launched right BEHIND its solve (QPhandler::solveQP always asks for it): by the time
    // rsqp_test_optimality is called it has run, and the call only waits for its completion value -- no launch on the critical path.
    // Dropped by every setter (the certificate then runs on demand, as before).
    bool spec_cert = false;
    int spec_cert_val = 0;
    bool cert_pending = false;   // a speculative certificate kernel may still be reading the (host-mapped) matrix values
    int done_seq = 0;
    bool lp_mode = false;   // optimizeLP: H ignored, H := hreg*I
    double hreg = 0.0;
    // engine: 1 = LDS-resident kernel, 2 = HBM-resident engine
    int engine = 1;
    bool fits_small = true;
    RsqpLargeEngine *large = nullptr;
    bool large_ready = false, profile_large = false;
    SmallKnobs kn = rsqp_small_knobs_from_env();   // the environment switches of the LDS-scale kernels as they were when this handle was created
    int state_engine = -1;        // which kernel family wrote the hot-start state of this handle: 1 the register-resident tableau kernel, 0 the
                                  // LDS-resident ones (different layouts in the same block), -1 none yet
    bool h_sym = true;            // H symmetric value by value (or absent): the tableau kernel of qp_tiny.hip may take the handle
    int last_mode = -1;           // RSQP_MODE_* of the last rsqp_solve (what the dispatch of optimizeQP / optimizeLP chose): rsqp_get_last_mode
    bool reinit_from_y0 = false;  // rsqp_set_reinit_guess: default = the reference rule (qpOASESInterface.cpp:199-207); 1 = opt-in shortcut
    DevBuf<double> denseA, denseAT, denseH;   // dense copies for the HBM-resident engine (dense matrices only)
    ~rsqp_solver() {
        delete large;
        if (io_host) {   // mapped views first, then the block
            for (int k = 0; k < 5; k++) d_vec[k].release();
            d_x.release(); d_y.release(); d_obj.release(); d_wsb.release(); d_wsc.release();
            d_kkt.release(); d_Wb.release(); d_Wc.release();
            d_status.release(); d_ret.release(); d_nwsr.release(); d_nflips.release();
            (void)hipHostFree(io_host);
        }
    }
};

namespace {

// the structure upload of a setter whose analysis began at t0 (rsqp_get_structure_seconds)
int stage_structure(rsqp_solver *s, DevMatrix &M, const Compressed &cs, bool want_csr, std::chrono::steady_clock::time_point t0) {
    s->desc_ready = false;
    const int rc = M.set_structure(cs, want_csr, s->fits_small, s->stream);
    if (rc != RSQP_OK) return rc;
    if (!M.arena_dev) (void)hipStreamSynchronize(s->stream);   // this handle's stream only (the uploads are blocking copies): other handles keep running
    M.structure_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return RSQP_OK;
}

// the value refresh of a setter. Host-mapped values are rewritten in place, and a speculative certificate may still be reading them (no
// other kernel of this handle is running: every solve and certificate of the single-QP boundary is waited for before its call returns)
int refresh_values(rsqp_solver *s, DevMatrix &M, const double *val, int n, RefreshKind kind) {
    if (M.pin && s->cert_pending) { HIPCHK(hipStreamSynchronize(s->stream)); s->cert_pending = false; }
    return M.refresh(val, n, kind, s->stream);
}

int flush_vectors(rsqp_solver *s) {
    if (!s->vec_dirty) return RSQP_OK;
    for (int k = 0; k < 5; k++) HIPCHK(s->d_vec[k].upload(s->h_vec[k].data(), s->h_vec[k].size()));
    s->vec_dirty = false;
    return RSQP_OK;
}

int ensure_desc(rsqp_solver *s) {
    if (s->desc_ready) return RSQP_OK;
    QPDesc d;
    std::memset(&d, 0, sizeof(d));
    d.nV = s->nV; d.nC = s->nC; d.haveH = (s->H.initialised && !s->lp_mode) ? 1 : 0;
    d.annz = d.hnnz = -1;
    d.hreg = s->hreg;
    if (s->d_desc.p) { HIPCHK(s->d_desc.upload(&d, 1)); }       // (host-mapped for LDS-scale handles: a store, no copy)
    else { std::vector<QPDesc> hd(1, d); HIPCHK(s->d_desc.from(hd)); }
    s->desc_ready = true;
    return RSQP_OK;
}

QPPools pools_of(rsqp_solver *s) {
    QPPools p;
    std::memset(&p, 0, sizeof(p));
    p.desc = s->d_desc.p;
    p.Ajc = s->A.initialised ? s->A.jc.p : s->d_dummy_i.p;
    p.Air = s->A.initialised ? s->A.ir.p : s->d_dummy_i.p;
    p.Aval = s->A.initialised ? s->A.val.p : s->d_dummy_d.p;
    p.Arp = s->A.initialised ? s->A.rp.p : s->d_dummy_i.p;
    p.Aci = s->A.initialised ? s->A.ci.p : s->d_dummy_i.p;
    p.Arv = s->A.initialised ? s->A.rval.p : s->d_dummy_d.p;
    p.Hjc = s->H.initialised ? s->H.jc.p : s->d_dummy_i.p;
    p.Hir = s->H.initialised ? s->H.ir.p : s->d_dummy_i.p;
    p.Hval = s->H.initialised ? s->H.val.p : s->d_dummy_d.p;
    p.g = s->d_vec[RSQP_VEC_G].p; p.lb = s->d_vec[RSQP_VEC_LB].p; p.ub = s->d_vec[RSQP_VEC_UB].p;
    p.lbA = s->d_vec[RSQP_VEC_LBA].p; p.ubA = s->d_vec[RSQP_VEC_UBA].p;
    p.x = s->d_x.p; p.y = s->d_y.p; p.ws_b = s->d_wsb.p; p.ws_c = s->d_wsc.p;
    p.status = s->d_status.p; p.ret = s->d_ret.p; p.nwsr = s->d_nwsr.p; p.nflips = s->d_nflips.p;
    p.obj = s->d_obj.p; p.state = s->d_state.p;
    p.uniV = s->nV; p.uniC = s->nC;
    p.keep_state = 1;
    p.done_flag = nullptr; p.done_val = 0;
    p.reinit_from_y0 = s->reinit_from_y0 ? 1 : 0;
    p.tiny_ok = (s->h_sym || !s->H.initialised || s->lp_mode) ? 1 : 0;
    // the batch of one: the hs071-scale kernel computes the (zero) offsets itself instead of loading the descriptor
    p.uni_pat = 1;
    p.uni_annz = s->A.initialised ? s->A.nnz : 0; p.uni_hnnz = s->H.initialised ? s->H.nnz : 0;
    p.uni_haveH = (s->H.initialised && !s->lp_mode) ? 1 : 0; p.uni_state = 0; p.uni_hreg = s->hreg;
    return p;
}

int fetch_results(rsqp_solver *s) {
    HIPCHK(s->d_x.download(s->h_x.data(), s->nV));
    HIPCHK(s->d_y.download(s->h_y.data(), s->nV + s->nC));
    HIPCHK(s->d_wsb.download(s->h_wsb.data(), s->nV));
    HIPCHK(s->d_wsc.download(s->h_wsc.data(), s->nC));
    HIPCHK(s->d_status.download(&s->status_word, 1));
    HIPCHK(s->d_ret.download(&s->last_ret, 1));
    HIPCHK(s->d_nflips.download(&s->last_nflips, 1));
    HIPCHK(s->d_obj.download(&s->obj, 1));
    return RSQP_OK;
}

// wait for a single-QP kernel that raises the host-mapped completion word to `val`: spin for up to 2 ms, then block
int wait_done(rsqp_solver *s, int val) {
    int *flag = s->h_done;
    const auto t0 = std::chrono::steady_clock::now();
    for (int it = 0;; it++) {
        // acquire: the results the kernel wrote to host-mapped memory BEFORE it raised the word are read after this load
        // (a plain volatile read orders nothing on non-x86 hosts and lets the compiler hoist the result reads)
        // (raising the word is the kernel's last action; a hipStreamQuery here measured +4 us per call, 8 us per solveQP --
        //  a fault is reported by the next HIP call of the handle, as for any asynchronous launch)
        // (>=: the word is a sequence number; the certificate launched behind a solve may have raised it further already)
        if ((int)(__atomic_load_n(flag, __ATOMIC_ACQUIRE) - val) >= 0) return RSQP_OK;
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
        if ((it & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    HIPCHK(hipStreamSynchronize(s->stream));
    return RSQP_OK;
}


bool solved(const rsqp_solver *s) { return s->status_word == QPS_SOLVED; }
bool infeasible(const rsqp_solver *s) { return s->status_word >= 100 && s->status_word < 200; }

}  // namespace

// =====================================================================================
// library
// =====================================================================================
extern "C" const char *rsqp_version(void) { return "restartsqp_amd 0.1 (gfx950)"; }
extern "C" const char *rsqp_last_error(void) { return g_err.c_str(); }
// a plan as the RSQP_PLAN_OUT_WORDS words of rsqp_hip.h (rsqp_describe_small_launch, rsqp_batch_get_last_plan)
void rsqp_plan_words(const SmallPlan &pl, int *out) {
    const int o[RSQP_PLAN_OUT_WORDS] = {pl.invalid, pl.empty, pl.family, pl.engine, pl.L, pl.mat_lds, pl.W, pl.shape, pl.mc, pl.keep, pl.uni, pl.hb,
                                        pl.first, (int)pl.grid, (int)pl.block, (int)pl.lds, pl.stride, pl.mode, pl.state_family, pl.skip_mark};
    std::copy(o, o + RSQP_PLAN_OUT_WORDS, out);
}
extern "C" int rsqp_describe_small_launch(const int *in, int n_in, int *out, int n_out) {
    if (!in || !out || n_in != RSQP_PLAN_IN_WORDS || n_out != RSQP_PLAN_OUT_WORDS) return fail(RSQP_ERR_ARG, "rsqp_describe_small_launch");
    SmallKnobs kn;
    kn.engine = in[0]; kn.lanes = in[1]; kn.waves = in[2]; kn.no_tiny = in[3]; kn.lane = in[4];
    const int *w = in + 12;
    const SmallFacts f{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], w[8], w[9], w[10], w[11], w[12], w[13], w[14], in[10], in[11]};
    rsqp_plan_words(rsqp_plan_small_launch(kn, f, in[5], in[6], in[7], in[8], in[9]), out);
    return RSQP_OK;
}

extern "C" int rsqp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// =====================================================================================
// one QP
// =====================================================================================
extern "C" int rsqp_create(int nV, int nC, int device, rsqp_solver **out) {
    if (!out || nV <= 0 || nC < 0) return fail(RSQP_ERR_ARG, "rsqp_create: bad sizes");
    if (rsqp_device_count() <= 0) return fail(RSQP_ERR_DEVICE, "rsqp_create: no HIP device visible");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    rsqp_solver *s = new rsqp_solver();
    struct Guard { rsqp_solver *s; ~Guard() { delete s; } } guard{s};
    s->nV = nV; s->nC = nC;
    s->fits_small = rsqp_small_qp_fits(nV, nC) != 0;
    s->engine = s->fits_small ? 1 : 2;
    HIPCHK(hipGetDevice(&s->device));
    for (int k = 0; k < 5; k++) s->h_vec[k].assign((k <= RSQP_VEC_UB) ? nV : nC, 0.0);
    if (s->fits_small) {
        const size_t nd = 3 * (size_t)nV + 2 * (size_t)nC + nV + (nV + nC) + 1 + 6;      // doubles
        const size_t ni = 2 * ((size_t)nV + nC) + 4 + 2;                                   // ints (+ the done flag)
        const size_t bytes_io = (nd * 8 + ni * 4 + 64 + 15) & ~(size_t)15;
        const size_t bytes = bytes_io + sizeof(QPDesc) + 16;          // (+ the problem descriptor: rewritten by a store, ensure_desc)
        HIPCHK(hipHostMalloc(&s->io_host, bytes, hipHostMallocMapped));
        std::memset(s->io_host, 0, bytes);
        void *dev = nullptr;
        HIPCHK(hipHostGetDevicePointer(&dev, s->io_host, 0));
        double *hd = static_cast<double *>(s->io_host), *dd = static_cast<double *>(dev);
        size_t o = 0;
        for (int k = 0; k < 5; k++) {
            const size_t n = (k <= RSQP_VEC_UB) ? nV : nC;
            s->d_vec[k].map(dd + o, hd + o, n);
            o += n;
        }
        s->d_x.map(dd + o, hd + o, nV); o += nV;
        s->d_y.map(dd + o, hd + o, nV + nC); o += nV + nC;
        s->d_obj.map(dd + o, hd + o, 1); o += 1;
        s->d_kkt.map(dd + o, hd + o, 6); o += 6;
        int *hi = reinterpret_cast<int *>(hd + o), *di = reinterpret_cast<int *>(dd + o);
        size_t q = 0;
        s->d_wsb.map(di + q, hi + q, nV); q += nV;
        s->d_wsc.map(di + q, hi + q, nC); q += nC;
        s->d_status.map(di + q, hi + q, 1); q++;
        s->d_ret.map(di + q, hi + q, 1); q++;
        s->d_nwsr.map(di + q, hi + q, 1); q++;
        s->d_nflips.map(di + q, hi + q, 1); q++;
        s->d_Wb.map(di + q, hi + q, nV); q += nV;
        s->d_Wc.map(di + q, hi + q, nC); q += nC;
        s->d_done = di + q; s->h_done = hi + q; q++;
        s->d_desc.map(reinterpret_cast<QPDesc *>(static_cast<char *>(dev) + bytes_io),
                      reinterpret_cast<QPDesc *>(static_cast<char *>(s->io_host) + bytes_io), 1);
        // (a failed reservation is "no arena": set_A / set_H then allocate per array as the HBM-scale handles do -- ADVICE r4)
        // (hs071-scale handles keep the arena in host-mapped memory: set_A / set_H then cost a store each instead of a stream wait and a
        //  copy -- 78 -> 37 us on the first QP of an SQP run, later QPs unchanged; RSQP_ARENA_MAPPED=0 / 1 forces either form)
        const bool am = s->kn.arena_mapped >= 0 ? s->kn.arena_mapped != 0 : rsqp_plan_tiny_fits(s->kn, nV, nC) != 0;
        if (nC > 0 && s->A.reserve(nC, nV, am) != hipSuccess) (void)hipGetLastError();
        if (s->H.reserve(nV, nV, am) != hipSuccess) (void)hipGetLastError();
    } else {
        for (int k = 0; k < 5; k++) HIPCHK(s->d_vec[k].alloc((k <= RSQP_VEC_UB) ? nV : nC));
        HIPCHK(s->d_x.alloc(nV)); HIPCHK(s->d_y.alloc(nV + nC)); HIPCHK(s->d_obj.alloc(1));
        HIPCHK(s->d_wsb.alloc(nV)); HIPCHK(s->d_wsc.alloc(nC));
        HIPCHK(s->d_status.alloc(1)); HIPCHK(s->d_ret.alloc(1)); HIPCHK(s->d_nwsr.alloc(1)); HIPCHK(s->d_nflips.alloc(1));
        HIPCHK(s->d_kkt.alloc(6)); HIPCHK(s->d_Wb.alloc(nV)); HIPCHK(s->d_Wc.alloc(nC));
    }
    HIPCHK(s->d_state.alloc(s->fits_small ? (size_t)rsqp_state_bytes(nV, nC) / 8 : 1));
    HIPCHK(s->d_x0.alloc(nV)); HIPCHK(s->d_y0.alloc(nV + nC)); HIPCHK(s->d_guess.alloc(nV));
    HIPCHK(s->d_dummy_i.alloc(std::max(nV, nC) + 2)); HIPCHK(s->d_dummy_d.alloc(4));
    HIPCHK(s->d_Ax.alloc(nC)); HIPCHK(s->d_ATy.alloc(nV)); HIPCHK(s->d_Hx.alloc(nV));
    HIPCHK(s->d_in.alloc(std::max(nV, nC))); HIPCHK(s->d_out.alloc(std::max(nV, nC)));
    s->h_x.assign(nV, 0.0); s->h_y.assign(nV + nC, 0.0); s->h_wsb.assign(nV, 0); s->h_wsc.assign(nC, 0);
    guard.s = nullptr;
    *out = s;
    return RSQP_OK;
}

extern "C" void rsqp_destroy(rsqp_solver *s) { delete s; }

extern "C" int rsqp_set_engine(rsqp_solver *s, int engine) {
    if (s) s->spec_cert = false;
    if (!s || engine < 0 || engine > 2) return fail(RSQP_ERR_ARG, "rsqp_set_engine");
    if (engine == 1 && !s->fits_small)
        return fail(RSQP_ERR_TOO_LARGE, "rsqp_set_engine: problem image exceeds the 160 KiB LDS-resident engine");
    s->engine = engine == 0 ? (s->fits_small ? 1 : 2) : engine;
    return RSQP_OK;
}
extern "C" int rsqp_get_engine(const rsqp_solver *s) { return s ? s->engine : -1; }
// measurement only: per-kernel-class device time of the HBM-resident engine (bench.py)
extern "C" int rsqp_set_engine_profiling(rsqp_solver *s, int on) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    s->profile_large = on != 0;
    if (s->large) s->large->profile_enable(s->profile_large);
    return RSQP_OK;
}
extern "C" int rsqp_get_engine_profile(const rsqp_solver *s, double *out4n, int n) {
    if (!s || !s->large) return 0;
    if (out4n && n >= RsqpLargeEngine::PROFILE_CLASSES) s->large->profile_get(out4n);
    return RsqpLargeEngine::PROFILE_CLASSES;
}
extern "C" int rsqp_engine_profile_names(const char **names, int n) {
    for (int k = 0; names && k < n && k < RsqpLargeEngine::PROFILE_CLASSES; k++) names[k] = RsqpLargeEngine::profile_name(k);
    return RsqpLargeEngine::PROFILE_CLASSES;
}
extern "C" int rsqp_get_setup_profile(const rsqp_solver *s, double *out8) {
    if (!s || !out8 || !s->large) return 0;
    return s->large->setup_profile(out8);
}
extern "C" double rsqp_get_structure_seconds(const rsqp_solver *s, int which) {
    if (!s) return -1.0;
    const DevMatrix &M = which == 0 ? s->A : s->H;
    return M.initialised ? M.structure_seconds : -1.0;
}
extern "C" int rsqp_get_last_mode(const rsqp_solver *s) { return s ? s->last_mode : -1; }
extern "C" int rsqp_get_large_path(const rsqp_solver *s) { return (s && s->large && s->large_ready) ? s->large->path() : -1; }
extern "C" int rsqp_get_nV(const rsqp_solver *s) { return s ? s->nV : -1; }
extern "C" int rsqp_get_nC(const rsqp_solver *s) { return s ? s->nC : -1; }

extern "C" int rsqp_set_reinit_guess(rsqp_solver *s, int from_y0) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    s->reinit_from_y0 = from_y0 != 0;
    return RSQP_OK;
}

extern "C" int rsqp_set_options(rsqp_solver *s, int qp_maxiter, int lp_maxiter) {
    if (!s || qp_maxiter < 0 || lp_maxiter < 0) return fail(RSQP_ERR_ARG, "rsqp_set_options");
    s->qp_maxiter = qp_maxiter; s->lp_maxiter = lp_maxiter;
    return RSQP_OK;
}

extern "C" int rsqp_set_A_triplet(rsqp_solver *s, int nnz, const int *irow, const int *jcol, const double *val,
                                  int n_ident, const int *id_irow, const int *id_jcol, const int *id_size,
                                  const double *id_value) {
    if (s) s->spec_cert = false;
    if (!s || nnz < 0 || (nnz > 0 && (!irow || !jcol || !val))) return fail(RSQP_ERR_ARG, "rsqp_set_A_triplet");
    if (s->firstQPsolved && !s->upd_A) s->upd_A = true;  // qpOASESInterface.cpp:427-429
    DevMatrix &M = s->A;
    if (!M.initialised) {
        std::vector<int> r(irow, irow + nnz), c(jcol, jcol + nnz);
        std::vector<double> v(val, val + nnz);
        int nid = 0;
        for (int b = 0; b < n_ident; b++)
            for (int j = 0; j < id_size[b]; j++) {
                r.push_back(id_irow[b] + j); c.push_back(id_jcol[b] + j); v.push_back(id_value[b]);
                nid++;
            }
        for (size_t k = 0; k < r.size(); k++)
            if (r[k] < 1 || r[k] > s->nC || c[k] < 1 || c[k] > s->nV)
                return fail(RSQP_ERR_ARG, "rsqp_set_A_triplet: index out of range (indices are 1-based)");
        const auto t0 = std::chrono::steady_clock::now();
        Compressed cs;
        csc_from_entries(s->nC, s->nV, r, c, v, cs);
        M.from_triplet = true; M.n_triplet = nnz; M.n_ident_entries = nid;
        return stage_structure(s, M, cs, true, t0);
    }
    if (!M.from_triplet || nnz != M.n_triplet) return fail(RSQP_ERR_ARG, "rsqp_set_A_triplet: pattern changed");
    return refresh_values(s, M, val, nnz, REFRESH_TRIPLET_A);
}

extern "C" int rsqp_set_H_triplet(rsqp_solver *s, int nnz, const int *irow, const int *jcol, const double *val,
                                  int is_symmetric) {
    if (s) s->spec_cert = false;
    if (!s || nnz < 0 || (nnz > 0 && (!irow || !jcol || !val))) return fail(RSQP_ERR_ARG, "rsqp_set_H_triplet");
    if (s->firstQPsolved && !s->upd_H) s->upd_H = true;  // :407-409
    DevMatrix &M = s->H;
    if (!M.initialised) {
        std::vector<int> r, c, tmap;
        std::vector<double> v;
        for (int i = 0; i < nnz; i++) {
            if (irow[i] < 1 || irow[i] > s->nV || jcol[i] < 1 || jcol[i] > s->nV)
                return fail(RSQP_ERR_ARG, "rsqp_set_H_triplet: index out of range (indices are 1-based)");
            r.push_back(irow[i]); c.push_back(jcol[i]); v.push_back(val[i]); tmap.push_back(i);
            if (is_symmetric && irow[i] != jcol[i]) {  // mirror right behind (SpHbMat.cpp:302-308)
                r.push_back(jcol[i]); c.push_back(irow[i]); v.push_back(val[i]); tmap.push_back(i);
            }
        }
        const auto t0 = std::chrono::steady_clock::now();
        Compressed cs;
        csc_from_entries(s->nV, s->nV, r, c, v, cs);
        cs.tmap = tmap;
        s->h_sym = is_symmetric != 0 || (s->nV <= 8 && small_csc_symmetric(s->nV, cs.jc.data(), cs.ir.data(), cs.val.data()));   // (sums repeats)
        M.from_triplet = true; M.n_triplet = nnz; M.symmetric = is_symmetric != 0;
        return stage_structure(s, M, cs, false, t0);
    }
    if (!M.from_triplet || nnz != M.n_triplet) return fail(RSQP_ERR_ARG, "rsqp_set_H_triplet: pattern changed");
    if (!M.symmetric) s->h_sym = false;       // (values of a general triplet matrix: re-examined below where they are at hand)
    const int rc = refresh_values(s, M, val, nnz, REFRESH_TRIPLET_H);
    if (rc == RSQP_OK && M.pin && !M.symmetric) s->h_sym = s->nV <= 8 && small_csc_symmetric(s->nV, M.h_jc.data(), M.h_ir.data(), M.val.host);
    return rc;
}

namespace {
int set_csc(rsqp_solver *s, DevMatrix &M, int nrow, int ncol, const int *jc, const int *ir, const double *val,
            bool want_csr, bool *flag) {
    if (!s || !jc || (jc[ncol] > 0 && (!ir || !val))) return fail(RSQP_ERR_ARG, "rsqp_set_*_csc");
    if (s->firstQPsolved && !*flag) *flag = true;
    const int nnz = jc[ncol];
    // same pattern as the caller's layout of the last call (compared entry by entry, not just by count): refresh values
    if (M.initialised && nnz == M.unnz() && !M.from_triplet && M.nrow == nrow && M.ncol == ncol &&
        std::equal(jc, jc + ncol + 1, M.caller_jc().begin()) && std::equal(ir, ir + nnz, M.caller_ir().begin()))
        return refresh_values(s, M, val, nnz, REFRESH_CSC);
    static const char *const why[] = {"", "rsqp_set_*_csc: column pointers must start at 0", "rsqp_set_*_csc: column pointers not monotone",
                                      "rsqp_set_*_csc: row index out of range"};
    if (const int f = csc_fault(nrow, ncol, jc, ir)) return fail(RSQP_ERR_ARG, why[f]);
    Compressed cs;
    cs.nrow = nrow; cs.ncol = ncol;
    cs.jc.assign(jc, jc + ncol + 1); cs.ir.assign(ir, ir + nnz); cs.val.assign(val, val + nnz);
    cs.order.resize(nnz);
    std::iota(cs.order.begin(), cs.order.end(), 0);
    // a new pattern on an initialised matrix: everything derived from the old one (CSR copy, SpMV
    // blocks, host mirror) is rebuilt; the dirty flag set above makes optimizeQP re-factorise
    M.from_triplet = false;
    const auto t0 = std::chrono::steady_clock::now();
    return stage_structure(s, M, cs, want_csr, t0);
}
int get_csc(const DevMatrix &M, hipStream_t stream, int *jc, int *ir, double *val, int *order) {
    if (!M.initialised) return fail(RSQP_ERR_ARG, "matrix not set");
    // (the caller's layout, as it was given: a non-canonical one is kept beside the canonical form)
    if (jc) std::copy(M.caller_jc().begin(), M.caller_jc().end(), jc);
    if (ir) std::copy(M.caller_ir().begin(), M.caller_ir().end(), ir);
    if (order) std::copy(M.h_order.begin(), M.h_order.end(), order);
    if (val) {
        HIPCHK(hipStreamSynchronize(stream));   // the value refresh kernels of this handle
        HIPCHK(M.caller_val().download(val, M.unnz()));
    }
    return RSQP_OK;
}
}  // namespace

extern "C" int rsqp_set_A_csc(rsqp_solver *s, const int *jc, const int *ir, const double *val) {
    if (s) s->spec_cert = false;
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    return set_csc(s, s->A, s->nC, s->nV, jc, ir, val, true, &s->upd_A);
}
extern "C" int rsqp_set_H_csc(rsqp_solver *s, const int *jc, const int *ir, const double *val) {
    if (s) s->spec_cert = false;
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    if (jc && (jc[s->nV] == 0 || (ir && val))) s->h_sym = s->nV <= 8 && small_csc_symmetric(s->nV, jc, ir, val);
    return set_csc(s, s->H, s->nV, s->nV, jc, ir, val, false, &s->upd_H);
}
extern "C" int rsqp_get_A_nnz(const rsqp_solver *s) { return s && s->A.initialised ? s->A.unnz() : -1; }
extern "C" int rsqp_get_H_nnz(const rsqp_solver *s) { return s && s->H.initialised ? s->H.unnz() : -1; }
extern "C" int rsqp_get_A_csc(const rsqp_solver *s, int *jc, int *ir, double *val, int *order) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    return get_csc(s->A, s->stream, jc, ir, val, order);
}
extern "C" int rsqp_get_H_csc(const rsqp_solver *s, int *jc, int *ir, double *val, int *order) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    return get_csc(s->H, s->stream, jc, ir, val, order);
}

extern "C" int rsqp_set_vector(rsqp_solver *s, int which, const double *v) {
    if (!s || which < 0 || which > 4 || !v) return fail(RSQP_ERR_ARG, "rsqp_set_vector");
    if (s->firstQPsolved) { if (which == RSQP_VEC_G) s->upd_g = true; else s->upd_bounds = true; }
    std::copy(v, v + s->h_vec[which].size(), s->h_vec[which].begin());
    s->vec_dirty = true;
    return RSQP_OK;
}
extern "C" int rsqp_set_entry(rsqp_solver *s, int which, int location, double value) {
    if (!s || which < 0 || which > 4 || location < 0 || location >= (int)s->h_vec[which].size())
        return fail(RSQP_ERR_ARG, "rsqp_set_entry");
    if (s->firstQPsolved) { if (which == RSQP_VEC_G) s->upd_g = true; else s->upd_bounds = true; }
    s->h_vec[which][location] = value;
    s->vec_dirty = true;
    return RSQP_OK;
}
extern "C" int rsqp_get_vector(const rsqp_solver *s, int which, double *v) {
    if (!s || which < 0 || which > 4 || !v) return fail(RSQP_ERR_ARG, "rsqp_get_vector");
    std::copy(s->h_vec[which].begin(), s->h_vec[which].end(), v);
    return RSQP_OK;
}
extern "C" int rsqp_reset_constraints(rsqp_solver *s) {
    if (s) s->spec_cert = false;
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    for (int k = RSQP_VEC_LB; k <= RSQP_VEC_UBA; k++) std::fill(s->h_vec[k].begin(), s->h_vec[k].end(), 0.0);
    s->vec_dirty = true;
    return RSQP_OK;
}

namespace {
// a dense copy for the HBM-resident engine: allocated at first use, rewritten from the CSC (or CSR: the CSC of the transpose) arrays
int densify(rsqp_solver *s, DevBuf<double> &dense, int nrow, int ncol, const int *jc, const int *ir, const double *val) {
    if (!dense.p) HIPCHK(dense.alloc((size_t)nrow * ncol, false));
    if (rsqp_launch_densify(nrow, ncol, jc, ir, val, dense.p, s->stream) != hipSuccess) return fail(RSQP_ERR_DEVICE, "densify launch failed");
    return RSQP_OK;
}

int solve_large(rsqp_solver *s, int mode, int *nWSR, const double *x0, const double *y0, const int *guess_b) {
    if (!s->large) { s->large = new RsqpLargeEngine(); if (s->profile_large) s->large->profile_enable(true); }
    if (!s->large_ready) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        if ((long long)free_b < RsqpLargeEngine::bytes_needed(s->nV, s->nC))
            return fail(RSQP_ERR_TOO_LARGE, "HBM-resident engine: not enough device memory");
        HIPCHK(s->large->init(s->nV, s->nC, s->stream));
        s->large_ready = true;
    }
    RsqpLargeMatrices m;
    if (s->A.initialised) {
        m.Ajc = s->A.jc.p; m.Air = s->A.ir.p; m.Aval = s->A.val.p; m.blk_c = s->A.blk_c.p; m.nblk_c = s->A.nblk_c;
        m.Arp = s->A.rp.p; m.Aci = s->A.ci.p; m.Arv = s->A.rval.p; m.blk_r = s->A.blk_r.p; m.nblk_r = s->A.nblk_r;
        m.sparse_rows = 8.0 * (double)s->A.nnz < (double)s->nC * s->nV;
        m.Annz = s->A.nnz;
    }
    m.hreg = s->hreg;
    if (s->H.initialised && !s->lp_mode) {
        m.Hjc = s->H.jc.p; m.Hir = s->H.ir.p; m.Hval = s->H.val.p; m.blk_h = s->H.blk_c.p; m.nblk_h = s->H.nblk_c;
        m.haveH = 1;
        if ((int)s->H.h_jc.size() == s->nV + 1 && (int)s->H.h_ir.size() == s->H.nnz) { m.h_Hjc = s->H.h_jc.data(); m.h_Hir = s->H.h_ir.data(); m.Hnnz = s->H.nnz; }
        // a diagonal Hessian (one entry per column, on the diagonal): the engine's range-space path
        bool diag = s->H.nnz == s->nV && (int)s->H.h_jc.size() == s->nV + 1;
        for (int c = 0; c < s->nV && diag; c++) diag = s->H.h_jc[c] == c && s->H.h_ir[c] == c;
        m.diagH = diag ? 1 : 0;
    }
    // dense copies when more than a quarter of the entries are stored (refreshed every solve
    // that follows a matrix update: cheap next to the solve)
    int rc;
    if (s->A.initialised && (double)s->A.nnz > 0.25 * (double)s->nC * s->nV) {
        if ((rc = densify(s, s->denseA, s->nC, s->nV, s->A.jc.p, s->A.ir.p, s->A.val.p)) != RSQP_OK) return rc;
        m.denseA = s->denseA.p;
        // the row-major copy (the CSR arrays are the CSC arrays of A')
        if ((rc = densify(s, s->denseAT, s->nV, s->nC, s->A.rp.p, s->A.ci.p, s->A.rval.p)) != RSQP_OK) return rc;
        m.denseAT = s->denseAT.p;
    }
    if (s->H.initialised && !s->lp_mode && (double)s->H.nnz > 0.25 * (double)s->nV * s->nV) {
        if ((rc = densify(s, s->denseH, s->nV, s->nV, s->H.jc.p, s->H.ir.p, s->H.val.p)) != RSQP_OK) return rc;
        m.denseH = s->denseH.p;
    }
    s->large->set_matrices(m);
    s->large->set_reinit_from_y0(s->reinit_from_y0);
    rc = s->large->solve(mode, s->d_vec[RSQP_VEC_G].p, s->d_vec[RSQP_VEC_LB].p, s->d_vec[RSQP_VEC_UB].p,
                         s->d_vec[RSQP_VEC_LBA].p, s->d_vec[RSQP_VEC_UBA].p, nWSR, x0, y0, guess_b);
    if (s->large->last_error() != hipSuccess)
        return fail(RSQP_ERR_DEVICE, std::string("HBM-resident engine: ") + hipGetErrorString(s->large->last_error()));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(s->d_x.p, s->large->d_x(), sizeof(double) * s->nV, hipMemcpyDefault));
    HIPCHK(hipMemcpy(s->d_y.p, s->large->d_y(), sizeof(double) * (s->nV + s->nC), hipMemcpyDefault));
    HIPCHK(hipMemcpy(s->d_wsb.p, s->large->d_Sb(), sizeof(int) * s->nV, hipMemcpyDefault));
    if (s->nC > 0) HIPCHK(hipMemcpy(s->d_wsc.p, s->large->d_Sc(), sizeof(int) * s->nC, hipMemcpyDefault));
    HIPCHK(s->d_x.download(s->h_x.data(), s->nV));
    HIPCHK(s->d_y.download(s->h_y.data(), s->nV + s->nC));
    HIPCHK(s->d_wsb.download(s->h_wsb.data(), s->nV));
    HIPCHK(s->d_wsc.download(s->h_wsc.data(), s->nC));
    s->status_word = s->large->status_word();
    s->last_ret = rc;
    s->last_nflips = s->large->nflips();
    s->obj = s->large->objective();
    return RSQP_OK;
}
}  // namespace

namespace { void launch_speculative_certificate(rsqp_solver *s, const QPPools &p); }

extern "C" int rsqp_solve(rsqp_solver *s, int mode, int *nWSR, const double *x0, const double *y0,
                          const int *guess_b) {
    if (!s || !nWSR || mode < 0 || mode > 3) return fail(RSQP_ERR_ARG, "rsqp_solve");
    s->spec_cert = false;
    s->last_mode = mode;
    if (!s->A.initialised && s->nC > 0) return fail(RSQP_ERR_ARG, "rsqp_solve: A not set");
    HIPCHK(hipSetDevice(s->device));
    int rc = flush_vectors(s);
    if (rc != RSQP_OK) return rc;
    rc = ensure_desc(s);
    if (rc != RSQP_OK) return rc;
    if (s->engine == 2) return solve_large(s, mode, nWSR, x0, y0, guess_b);
    const int nWSR_in = *nWSR;
    QPPools p = pools_of(s);
    // an LP (H = regVal*I with regVal ~ 1e-13) stays off the register-resident tableau kernel: the tableau carries H^-1, and its x
    // came out up to 9e-4 (relative) off the CPU reference's on the LPs of tests/lp_batch_ref.py -- flag, count and working set were
    // right. The Givens / TQ kernel is within 6e-12 on the same members; rsqp_batch_optimize_lp keeps its members off it as well
    SmallKnobs kn = s->kn;
    if (s->lp_mode) kn.no_tiny = 1;
    if (mode == RSQP_MODE_WARM_REINIT) {
        if (x0) { HIPCHK(s->d_x0.upload(x0, s->nV)); p.x0 = s->d_x0.p; }
        if (y0) { HIPCHK(s->d_y0.upload(y0, s->nV + s->nC)); p.y0 = s->d_y0.p; }
        if (guess_b) { HIPCHK(s->d_guess.upload(guess_b, s->nV)); p.guess_b = s->d_guess.p; }
    }
    if (s->d_done && !s->kn.no_spin) { p.done_flag = s->d_done; p.done_val = ++s->done_seq; }
    const long long mat_bytes = rsqp_mat_lds_bytes(s->nV, s->nC, s->A.initialised ? s->A.nnz : 0, s->H.initialised ? s->H.nnz : 0);
    // the plan of the solve (rsqp_small_plan.h). The tableau kernel and the LDS-resident kernels keep different layouts in the same
    // state block: a solve that changes the family (H lost or regained its symmetry between two solves) starts cold instead of
    // restoring the other's bytes -- the plan's mode says so
    auto plan = [&](const SmallKnobs &k, int m) {
        const SmallPlan pl = rsqp_plan_small_launch(k, rsqp_small_facts(p, false, s->state_engine), 1, s->nV, s->nC, mat_bytes, m);
        s->state_engine = pl.state_family;
        s->last_mode = pl.mode;
        return pl;
    };
    // the hs071-scale tableau kernel forms the certificate QPhandler::solveQP asks for at the end of the SAME launch
    // (asked for before the plan is made: a launch with a doorbell never takes the lane-per-problem kernel, with or without it)
    if (p.done_flag && !s->lp_mode && s->A.initialised == (s->nC > 0)) { p.cert_out = s->d_kkt.p; p.cert_Wb = s->d_Wb.p; p.cert_Wc = s->d_Wc.p; }
    const SmallPlan pl = plan(kn, mode);
    const bool fused_cert = p.cert_out && pl.family == 1;
    if (!fused_cert) { p.cert_out = nullptr; p.cert_Wb = nullptr; p.cert_Wc = nullptr; }
    // one solve of the handle: launch (with the certificate behind it, where the call has one), wait, fetch.
    // The results live in host-mapped memory and the kernel raises a host-mapped flag behind them: spinning on it saves
    // the ~10 us a blocking hipStreamSynchronize takes to wake up (a single hs071-scale solve is ~30 us end to end)
    auto run = [&](const SmallKnobs &k, const SmallPlan &pl, int maxWSR, bool certify) {
        const hipError_t e = rsqp_launch_small_qp(k, pl, p, 1, maxWSR, s->stream);
        if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, std::string("QP kernel launch: ") + hipGetErrorString(e));
        if (certify) {
            if (fused_cert) { s->spec_cert = true; s->spec_cert_val = p.done_val; s->cert_pending = false; }
            else launch_speculative_certificate(s, p);
        }
        if (p.done_flag) { if (const int rw = wait_done(s, p.done_val)) return rw; }
        else HIPCHK(hipStreamSynchronize(s->stream));
        return fetch_results(s);
    };
    if ((rc = run(kn, pl, *nWSR, true)) != RSQP_OK) return rc;
    if (s->state_engine == 1 && s->last_ret == RET_SETUP_FAILED) {
        // the register-resident tableau kernel gave up on a pivot in its rounding band (it has no hand-over of its own: the mid-size
        // tableau kernel bails to the null-space kernel inside the launcher): the LDS-resident Givens / TQ kernel takes the
        // same call over -- from scratch where the call wanted the tableau kernel's stored state
        SmallKnobs k2 = s->kn;
        k2.no_tiny = 1;
        p.cert_out = nullptr; p.cert_Wb = nullptr; p.cert_Wc = nullptr;
        if (p.done_flag) p.done_val = ++s->done_seq;
        s->spec_cert = false; s->cert_pending = false;
        if ((rc = run(k2, plan(k2, mode), nWSR_in, false)) != RSQP_OK) return rc;
    }
    HIPCHK(s->d_nwsr.download(nWSR, 1));
    return RSQP_OK;
}

namespace {
// qpOASESInterface::handle_error: the QP branch (src/qpOASESInterface.cpp:718-757) and the LP branch (:688-717), which differ in the
// budget and in what the slack point starts from -- zeros, or x_0 := x_qp with the slack entries overwritten (:693-699)
int handle_error(rsqp_solver *s, bool lp, int *total) {
    int nWSR = lp ? s->lp_maxiter : s->qp_maxiter, rc;
    if (infeasible(s) && s->nV >= 2 * s->nC) {
        std::vector<double> x0 = lp ? s->h_x : std::vector<double>(s->nV, 0.0);
        for (int i = 0; i < s->nC; i++) {
            x0[i + s->nV - 2 * s->nC] = std::max(0.0, s->h_vec[RSQP_VEC_LBA][i]);
            x0[i + s->nV - s->nC] = -std::min(0.0, s->h_vec[RSQP_VEC_UBA][i]);
        }
        rc = rsqp_solve(s, RSQP_MODE_WARM_REINIT, &nWSR, x0.data(), nullptr, nullptr);
    } else {
        rc = rsqp_solve(s, RSQP_MODE_COLD, &nWSR, nullptr, nullptr, nullptr);
    }
    s->old_status = s->new_status = 0;
    *total += nWSR;
    return rc;  // the adapter throws QP_NOT_OPTIMAL / LP_NOT_OPTIMAL when !rsqp_is_solved()
}
}  // namespace

extern "C" int rsqp_optimize_qp(rsqp_solver *s, int *nWSR_used) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    if (s->lp_mode) {
        // an LP was solved on this handle before (the reference keeps separate LP and QP objects,
        // Algorithm.cpp:561-562): the stored factors belong to H = regVal*I, so start over
        s->lp_mode = false; s->hreg = 0.0; s->desc_ready = false;
        s->firstQPsolved = false; s->old_status = s->new_status = 0;
    }
    int nWSR = s->qp_maxiter, total = 0, rc;
    if (!s->firstQPsolved) {
        rc = rsqp_solve(s, RSQP_MODE_COLD, &nWSR, nullptr, nullptr, nullptr);
        if (rc != RSQP_OK) return rc;
        if (solved(s)) s->firstQPsolved = true;
        else {
            // the reference leaves firstQPsolved_ false here even when the retry succeeds
            rc = handle_error(s, false, &total);
            if (rc != RSQP_OK) return rc;
            // still unsolved: the reference THROWS QP_NOT_OPTIMAL inside handle_error (:754-756) -- nothing behind the call runs: no
            // reset_flags, no second handle_error, and the first init's nWSR never reaches Stats::qp_iter (:211-212 are skipped), only
            // the retry's (:751-752). The adapter raises the exception from !rsqp_is_solved()
            if (!solved(s)) { if (nWSR_used) *nWSR_used = total; return RSQP_OK; }
        }
    } else {
        // get_Matrix_change_status (:817-833) and the call shape it selects: rsqp_dispatch_mode
        const int mode = rsqp_dispatch_mode(true, s->upd_A || s->upd_H, s->old_status, s->new_status);
        if (mode != RSQP_MODE_WARM_REINIT)
            rc = rsqp_solve(s, mode, &nWSR, nullptr, nullptr, nullptr);
        else {  // status flip: init(..., x_qp, y_qp, &bounds)  (:201-208)
            std::vector<double> x0 = s->h_x, y0 = s->h_y;
            std::vector<int> gb = s->h_wsb;
            rc = rsqp_solve(s, RSQP_MODE_WARM_REINIT, &nWSR, x0.data(), y0.data(), gb.data());
        }
        if (rc != RSQP_OK) return rc;
    }
    s->upd_A = s->upd_H = s->upd_bounds = s->upd_g = false;  // reset_flags (:488-496)
    total += nWSR;
    if (!solved(s)) {
        rc = handle_error(s, false, &total);
        if (rc != RSQP_OK) return rc;
    }
    if (nWSR_used) *nWSR_used = total;
    return RSQP_OK;
}

extern "C" int rsqp_optimize_lp(rsqp_solver *s, int *nWSR_used) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    if (!s->lp_mode) {   // a QP was solved on this handle before: its factors belong to another Hessian
        s->lp_mode = true; s->firstQPsolved = false; s->old_status = s->new_status = 0;
    }
    // qpOASES fixes regVal = getNorm(g) * epsRegularisation when the problem is initialised and keeps it
    // across hot starts (the factors stored in the engine were built with it); a later init -- the first
    // solve, a status flip, handle_error -- computes it afresh from the gradient of that call
    auto set_reg_for_init = [s]() {
        double ng = 0.0;
        for (double v : s->h_vec[RSQP_VEC_G]) ng += v * v;
        ng = std::sqrt(ng);
        s->hreg = (ng > 0.0 ? ng : 1.0) * 1.0e3 * RSQP_EPS;
        s->desc_ready = false;
    };
    int nWSR = s->lp_maxiter, total = 0, rc;
    if (!s->firstQPsolved) {
        set_reg_for_init();
        rc = rsqp_solve(s, RSQP_MODE_COLD, &nWSR, nullptr, nullptr, nullptr);
        if (rc != RSQP_OK) return rc;
        if (solved(s)) s->firstQPsolved = true;
        else {
            set_reg_for_init();
            if ((rc = handle_error(s, true, &total)) != RSQP_OK) return rc;
            // (LP_NOT_OPTIMAL thrown inside handle_error, :714-716: the count behind the call, :278-279, is never added)
            if (!solved(s)) { if (nWSR_used) *nWSR_used = total; return RSQP_OK; }
        }
    } else {
        const int mode = rsqp_dispatch_mode(true, s->upd_A || s->upd_H, s->old_status, s->new_status);
        if (mode != RSQP_MODE_WARM_REINIT)
            rc = rsqp_solve(s, mode, &nWSR, nullptr, nullptr, nullptr);
        else {   // :266-270: plain re-init on a status flip
            set_reg_for_init();
            rc = rsqp_solve(s, RSQP_MODE_COLD, &nWSR, nullptr, nullptr, nullptr);
        }
        if (rc != RSQP_OK) return rc;
        s->upd_A = s->upd_H = s->upd_bounds = s->upd_g = false;
        if (!solved(s)) {
            set_reg_for_init();
            if ((rc = handle_error(s, true, &total)) != RSQP_OK) return rc;
            if (!solved(s)) { if (nWSR_used) *nWSR_used = total; return RSQP_OK; }
        }
    }
    total += nWSR;
    if (solved(s)) {
        // one regularisation step: min (reg/2)|x - x_k|^2 + g'x  <=>  gradient g - reg*x_k
        const double reg = s->hreg;
        std::vector<double> gmod = s->h_vec[RSQP_VEC_G];
        for (int i = 0; i < s->nV; i++) gmod[i] -= reg * s->h_x[i];
        rc = flush_vectors(s);
        if (rc != RSQP_OK) return rc;
        HIPCHK(s->d_vec[RSQP_VEC_G].upload(gmod.data(), s->nV));
        int n2 = s->lp_maxiter;
        rc = rsqp_solve(s, RSQP_MODE_HOT_VECTORS, &n2, nullptr, nullptr, nullptr);
        s->vec_dirty = true;   // the true gradient goes back to the device with the next flush
        if (rc != RSQP_OK) return rc;
        total += n2;
        double o = 0.0;
        for (int i = 0; i < s->nV; i++) o += s->h_vec[RSQP_VEC_G][i] * s->h_x[i];
        s->obj = o;
    }
    if (nWSR_used) *nWSR_used = total;
    return RSQP_OK;
}

extern "C" int rsqp_get_primal(const rsqp_solver *s, double *x) {
    if (!s || !x) return fail(RSQP_ERR_ARG, "rsqp_get_primal");
    std::copy(s->h_x.begin(), s->h_x.end(), x);
    return RSQP_OK;
}
extern "C" int rsqp_get_dual(const rsqp_solver *s, double *y) {
    if (!s || !y) return fail(RSQP_ERR_ARG, "rsqp_get_dual");
    std::copy(s->h_y.begin(), s->h_y.end(), y);
    return RSQP_OK;
}
extern "C" double rsqp_get_objective(const rsqp_solver *s) { return s ? s->obj : 0.0; }
extern "C" int rsqp_get_status(const rsqp_solver *s) {
    return s ? exitflag_of(s->status_word, s->last_ret) : RSQP_QPERROR_UNKNOWN;
}
extern "C" int rsqp_is_solved(const rsqp_solver *s) { return s && solved(s); }
extern "C" int rsqp_get_working_set_raw(const rsqp_solver *s, int *ws_b, int *ws_c) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    if (ws_b) std::copy(s->h_wsb.begin(), s->h_wsb.end(), ws_b);
    if (ws_c) std::copy(s->h_wsc.begin(), s->h_wsc.end(), ws_c);
    return RSQP_OK;
}

namespace {
int spmv_csc(rsqp_solver *s, DevMatrix &M, const double *in, double *out) {  // out[col] = sum val*in[row]
    hipError_t e = rsqp_launch_spmv(M.blk_c.p, M.nblk_c, M.jc.p, M.ir.p, M.val.p, in, out, 1, 0, 0, 0, 0, s->stream);
    if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, "spmv launch failed");
    return RSQP_OK;
}
int spmv_csr(rsqp_solver *s, DevMatrix &M, const double *in, double *out) {  // out[row] = sum val*in[col]
    hipError_t e = rsqp_launch_spmv(M.blk_r.p, M.nblk_r, M.rp.p, M.ci.p, M.rval.p, in, out, 1, 0, 0, 0, 0, s->stream);
    if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, "spmv launch failed");
    return RSQP_OK;
}

int collect_certificate(rsqp_solver *s, rsqp_optimality_status *out, int *W_c, int *W_b, int *invalid) {
    double o[6];
    HIPCHK(s->d_kkt.download(o, 6));
    if (out) {
        out->primal_violation = o[0]; out->dual_violation = o[1]; out->compl_violation = o[2];
        out->stationarity_violation = o[3]; out->KKT_error = o[4];
    }
    *invalid = o[5] != 0.0;
    if (W_b) HIPCHK(s->d_Wb.download(W_b, s->nV));
    if (W_c) HIPCHK(s->d_Wc.download(W_c, s->nC));
    return RSQP_OK;
}
void fill_kkt_args(rsqp_solver *s, RsqpKktArgs &a) {
    std::memset(&a, 0, sizeof(a));
    a.nV1 = s->nV; a.nC1 = s->nC;
    a.x = s->d_x.p; a.y = s->d_y.p; a.g = s->d_vec[RSQP_VEC_G].p; a.lb = s->d_vec[RSQP_VEC_LB].p;
    a.ub = s->d_vec[RSQP_VEC_UB].p; a.lbA = s->d_vec[RSQP_VEC_LBA].p; a.ubA = s->d_vec[RSQP_VEC_UBA].p;
    a.Ax = s->d_Ax.p; a.ATy = s->d_ATy.p; a.Hx = s->d_Hx.p;
    a.ws_b = s->d_wsb.p; a.ws_c = s->d_wsc.p; a.W_b = s->d_Wb.p; a.W_c = s->d_Wc.p; a.out = s->d_kkt.p;
}

// an LDS-scale QP: the three products and the certificate are ONE launch (rsqp_launch_small_certificate)
bool fused_certificate(const rsqp_solver *s) { return s->fits_small && s->A.initialised == (s->nC > 0); }

// the fused products + certificate kernel of an LDS-scale QP right behind its solve kernel (same stream), see rsqp_solver::spec_cert
void launch_speculative_certificate(rsqp_solver *s, const QPPools &p) {
    s->spec_cert = false;
    if (s->lp_mode || !p.done_flag || !fused_certificate(s)) return;
    RsqpKktArgs a;
    fill_kkt_args(s, a);
    a.done_flag = s->d_done; a.done_val = ++s->done_seq;
    if (rsqp_launch_small_certificate(p, a, 1, s->d_Ax.p, s->d_ATy.p, s->d_Hx.p, s->stream) != hipSuccess) return;
    s->spec_cert = true; s->spec_cert_val = a.done_val; s->cert_pending = true;
}

int run_certificate(rsqp_solver *s, rsqp_optimality_status *out, int *W_c, int *W_b, int *invalid) {
    HIPCHK(hipSetDevice(s->device));
    if (s->spec_cert && !s->vec_dirty) {      // launched behind the solve, nothing changed since: only wait for it
        s->spec_cert = false;
        int rcw = wait_done(s, s->spec_cert_val);
        s->cert_pending = false;
        if (rcw != RSQP_OK) return rcw;
        return collect_certificate(s, out, W_c, W_b, invalid);
    }
    s->spec_cert = false;
    int rc = flush_vectors(s);
    if (rc != RSQP_OK) return rc;
    const bool fused = fused_certificate(s);
    if (fused) {
        // hs0xx-scale: the three products and the certificate in ONE launch (one workgroup), below
        if ((rc = ensure_desc(s)) != RSQP_OK) return rc;
    } else {
        if (s->nC > 0) {
            if ((rc = spmv_csr(s, s->A, s->d_x.p, s->d_Ax.p)) != RSQP_OK) return rc;             // A x
            if ((rc = spmv_csc(s, s->A, s->d_y.p + s->nV, s->d_ATy.p)) != RSQP_OK) return rc;    // A'y_c
        } else {
            HIPCHK(hipMemsetAsync(s->d_ATy.p, 0, sizeof(double) * s->nV, s->stream));
        }
        if (s->H.initialised && !s->lp_mode) {   // (behind an LP call the certificate is the LP's: no H, as the LDS-scale one and the batch's)
            if ((rc = spmv_csc(s, s->H, s->d_x.p, s->d_Hx.p)) != RSQP_OK) return rc;             // H x (symmetric)
        } else {
            HIPCHK(hipMemsetAsync(s->d_Hx.p, 0, sizeof(double) * s->nV, s->stream));
        }
    }
    RsqpKktArgs a;
    fill_kkt_args(s, a);
    if (s->d_done && !s->kn.no_spin) { a.done_flag = s->d_done; a.done_val = ++s->done_seq; }
    if (fused) {
        QPPools p = pools_of(s);
        if (rsqp_launch_small_certificate(p, a, 1, s->d_Ax.p, s->d_ATy.p, s->d_Hx.p, s->stream) != hipSuccess)
            return fail(RSQP_ERR_DEVICE, "certificate launch failed");
    } else if (rsqp_launch_kkt(a, 1, s->stream) != hipSuccess) return fail(RSQP_ERR_DEVICE, "kkt launch failed");
    if (a.done_flag) { if ((rc = wait_done(s, a.done_val)) != RSQP_OK) return rc; }
    else HIPCHK(hipStreamSynchronize(s->stream));
    return collect_certificate(s, out, W_c, W_b, invalid);
}
}  // namespace

extern "C" int rsqp_get_working_set(rsqp_solver *s, int *W_c, int *W_b) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    int invalid = 0;
    int rc = run_certificate(s, nullptr, W_c, W_b, &invalid);
    if (rc != RSQP_OK) return rc;
    return invalid ? fail(RSQP_ERR_WORKING_SET, "INVALID_WORKING_SET") : RSQP_OK;
}

extern "C" int rsqp_test_optimality(rsqp_solver *s, int *W_c, int *W_b, rsqp_optimality_status *out) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    rsqp_optimality_status st;
    int invalid = 0;
    int rc = run_certificate(s, &st, W_c, W_b, &invalid);
    if (rc != RSQP_OK) return rc;
    if (out) *out = st;
    if (invalid) return fail(RSQP_ERR_WORKING_SET, "INVALID_WORKING_SET");
    return st.KKT_error > 1.0e-6 ? 0 : 1;  // :673
}

namespace {
int product(rsqp_solver *s, DevMatrix &M, bool use_csr, int nin, int nout, const double *p, double *result) {
    if (!s || !p || !result) return fail(RSQP_ERR_ARG, "product: null argument");
    if (!M.initialised) return fail(RSQP_ERR_ARG, "product: matrix not set");
    HIPCHK(hipSetDevice(s->device));
    HIPCHK(s->d_in.upload(p, nin));
    int rc = use_csr ? spmv_csr(s, M, s->d_in.p, s->d_out.p) : spmv_csc(s, M, s->d_in.p, s->d_out.p);
    if (rc != RSQP_OK) return rc;
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(s->d_out.download(result, nout));
    return RSQP_OK;
}
}  // namespace

extern "C" int rsqp_A_times(rsqp_solver *s, const double *p, double *result) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    return product(s, s->A, true, s->nV, s->nC, p, result);
}
extern "C" int rsqp_A_transposed_times(rsqp_solver *s, const double *p, double *result) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    return product(s, s->A, false, s->nC, s->nV, p, result);
}
extern "C" int rsqp_H_times(rsqp_solver *s, const double *p, double *result) {
    if (!s) return fail(RSQP_ERR_ARG, "null solver");
    return product(s, s->H, false, s->nV, s->nV, p, result);
}

// setMatVal on the device (SpHbMat.cpp:368-393): time `repeats` launches of the scatter through `order`
// and of the CSR-copy gather on the values already staged by rsqp_set_A_triplet (no host transfer inside)
extern "C" int rsqp_time_value_refresh_fused(rsqp_solver *s, int repeats, float *ms) {
    if (!s || repeats <= 0 || !ms || !s->A.initialised || !s->A.from_triplet || !s->A.have_csr) return fail(RSQP_ERR_ARG, "rsqp_time_value_refresh_fused");
    if (s->A.pin) return fail(RSQP_ERR_ARG, "rsqp_time_value_refresh_fused: this handle refreshes its values on the host (no kernel to time)");
    if (!s->A.fold.canon) return fail(RSQP_ERR_ARG, "rsqp_time_value_refresh_fused: the matrix repeats positions (its refresh folds)");
    HIPCHK(hipSetDevice(s->device));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    DevMatrix &M = s->A;
    HIPCHK(hipEventRecord(e0, s->stream));
    for (int r = 0; r < repeats; r++)
        if (rsqp_launch_scatter_csc_csr(M.n_triplet, M.order.p, M.rorder.p, M.tv.p, M.val.p, M.rval.p, s->stream) != hipSuccess)
            return fail(RSQP_ERR_DEVICE, "value refresh launch failed");
    HIPCHK(hipEventRecord(e1, s->stream));
    HIPCHK(hipEventSynchronize(e1));
    HIPCHK(hipEventElapsedTime(ms, e0, e1));
    *ms /= repeats;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return RSQP_OK;
}

extern "C" int rsqp_time_value_refresh(rsqp_solver *s, int repeats, float *ms_scatter, float *ms_gather) {
    if (!s || repeats <= 0 || !s->A.initialised || !s->A.from_triplet) return fail(RSQP_ERR_ARG, "rsqp_time_value_refresh");
    if (s->A.pin) return fail(RSQP_ERR_ARG, "rsqp_time_value_refresh: this handle refreshes its values on the host (no kernel to time)");
    if (!s->A.fold.canon) return fail(RSQP_ERR_ARG, "rsqp_time_value_refresh: the matrix repeats positions (its refresh folds)");
    HIPCHK(hipSetDevice(s->device));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    DevMatrix &M = s->A;
    for (int pass = 0; pass < 2; pass++) {
        float *out = pass == 0 ? ms_scatter : ms_gather;
        HIPCHK(hipEventRecord(e0, s->stream));
        for (int r = 0; r < repeats; r++) {
            hipError_t e = pass == 0 ? rsqp_launch_scatter(M.n_triplet, M.order.p, nullptr, M.tv.p, M.val.p, s->stream)
                                     : rsqp_launch_gather(M.nnz, M.perm.p, M.val.p, M.rval.p, s->stream);
            if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, "value refresh launch failed");
        }
        HIPCHK(hipEventRecord(e1, s->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        if (out) *out = ms / repeats;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return RSQP_OK;
}

extern "C" int rsqp_time_large_kernel(int device, int n, int kind, int nrows, int ncols, int repeats, float *ms) {
    if (n <= 0 || !ms) return fail(RSQP_ERR_ARG, "rsqp_time_large_kernel");
    HIPCHK(hipSetDevice(device));
    RsqpLargeEngine eng;
    hipStream_t st = nullptr;
    HIPCHK(hipStreamCreate(&st));
    hipError_t e = eng.init(n, 0, st);
    int rc = e == hipSuccess ? eng.time_kernel(kind, nrows, ncols, repeats, ms) : -1;
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) return fail(RSQP_ERR_DEVICE, std::string("rsqp_time_large_kernel: ") + hipGetErrorString(e));
    return rc == 0 ? RSQP_OK : fail(RSQP_ERR_ARG, "rsqp_time_large_kernel: bad shape or launch failure");
}
