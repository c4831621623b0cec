// rsqp_batch.h -- struct rsqp_batch and what more than one of its translation units uses. Private to the units:
//   rsqp_batch.hip           the batch itself: create, whole-batch setters, solve, results, certificate, records
//   rsqp_batch_optimize.hip  optimizeQP / optimizeLP per member and their plan kernels
//   rsqp_batch_handler.hip   everything that writes the pools member by member
//   rsqp_batch_nlp.hip       the decisions of the SQP loop, which read the pools member by member
//   rsqp_batch_penalty.hip   update_penalty_parameter across a QP batch and its LP batch
//   rsqp_batch_soc.hip       second_order_correction
// and the two shared headers: rsqp_batch_staging.h (the staging block of a host-pointer call, plain C++; included here) and
// rsqp_batch_decide.h (the arithmetic of the decisions, with FP contraction off; the last three units include it).
// Device code does not cross a unit: the __device__ helpers here are inline. Everything but the struct itself (the opaque type
// of the C ABI) is in namespace rsqp_batch_units, which the units open.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rsqp_batch_staging.h"
#include "rsqp_host.h"
#include "rsqp_matrix.h"

namespace rsqp_batch_units {
// pinned host memory, with its device view where it is mapped; freed with its owner
template <class T>
struct HostBuf {
    T *p = nullptr, *dev = nullptr;
    size_t n = 0;
    HostBuf() = default;
    HostBuf(const HostBuf &) = delete;
    HostBuf &operator=(const HostBuf &) = delete;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t count, bool mapped) {
        if (p) (void)hipHostFree(p);
        p = dev = nullptr; n = 0;
        hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&p), sizeof(T) * std::max<size_t>(count, 1), mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (e == hipSuccess && mapped) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), p, 0);
        if (e == hipSuccess) n = count;
        return e;
    }
};

// optimizeQP per member (rsqp_batch_optimize_qp): nq ints each, in one block (rsqp_batch::opt) -- firstQPsolved_, old / new matrix
// status, mode of the call's first solve, mode of its rescue solve (-1: none), kind of rescue, count of the first solve
// rsqp_batch_optimize_lp adds: mode the first solve is LAUNCHED with (a flip is a plain init there), mode of the proximal step
// (-1: the member is unsolved and takes none)
// per member across calls as well: OPT_UPD the update mark (Update_A / Update_H of rsqp_batch_set_matrix_values_of and
// rsqp_batch_handler_set_matrices, and of rsqp_batch_set_matrix_values for a member that sat out the call that took the batch-wide
// mats_updated), OPT_FAM 1 + the kernel family that wrote the member's stored state (0 none; read while state_engine == -2)
enum { OPT_FIRST = 0, OPT_OLD, OPT_NEW, OPT_MODE, OPT_RMODE, OPT_RESCUE, OPT_N1, OPT_LMODE, OPT_PMODE, OPT_UPD, OPT_FAM, OPT_WORDS };
// word `word` of member q
__device__ inline int &opt_word(int *opt, int nq, int word, int q) { return opt[word * nq + q]; }
__device__ inline const int &opt_word(const int *opt, int nq, int word, int q) { return opt[word * nq + q]; }

// the bound formulas of QPhandler (src/QPhandler.cpp:167-201, 342-368, 533-567), one subtraction and one fmax / fmin each: what
// batch_handler_update_kernel writes for RSQP_HU_SET / _BOUNDS / _DELTA, and second_order_correction's update_bounds at x_k + p
__device__ inline double hu_lb(double x_l, double x_k, double delta) { return fmax(x_l - x_k, -delta); }
__device__ inline double hu_ub(double x_u, double x_k, double delta) { return fmin(x_u - x_k, delta); }
__device__ inline double hu_lbA(double c_l, double c_k) { return c_l - c_k; }
__device__ inline double hu_ubA(double c_u, double c_k) { return c_u - c_k; }
// the per-member work of a call whose decisions are taken on the device, allocated at its first use: `ints` ints and `doubles`
// doubles, nq of each per word (word w of member q at [w * nq + q]), the x of the first solve (sumV), the block counters of the
// decision kernels (report_live) and the host-mapped word they report through. DecisionView: what the kernels get of it
struct DecisionView {
    int nq;
    int *i; double *d;
    double *x0;                               // pooled like x
    int *cnt;                                 // [0] members that go on, [1] blocks that have finished
    int *live;                                // host-mapped: [0] of the finished launch
    __device__ int &wi(int w, int q) const { return i[(size_t)w * nq + q]; }
    __device__ double &wd(int w, int q) const { return d[(size_t)w * nq + q]; }
};
struct DecisionWork {
    DevBuf<int> i, cnt;
    DevBuf<double> d, x0;
    HostBuf<int> live;
    int ensure(size_t ints, size_t doubles, size_t sumV) {
        if (i.p) return RSQP_OK;
        HIPCHK(i.alloc(ints)); HIPCHK(d.alloc(doubles)); HIPCHK(x0.alloc(sumV)); HIPCHK(cnt.alloc(2)); HIPCHK(live.alloc(1, true));
        return RSQP_OK;
    }
    DecisionView view(int nq) const { return DecisionView{nq, i.p, d.p, x0.p, cnt.p, live.dev}; }
};
}  // namespace rsqp_batch_units
using namespace rsqp_batch_units;

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
    int last_plan[RSQP_PLAN_OUT_WORDS] = {};      // rsqp_batch_get_last_plan: the plan of that launch, as rsqp_plan_words writes it
    // the lane-per-problem kernel's build (qp_lane.hip): lane_hblock = 4 when the batch's one pattern keeps H inside its leading
    // 4 x 4 block (judged once, at create: values change later, patterns never), else 8; last_hblock = what the last launch took
    int lane_hblock = 8, last_hblock = 0; // rsqp_batch_get_lane_hblock
    int last_lane_shape = 0;              // rsqp_batch_get_lane_shape: SmallPlan::lane_shape of the last launch
    bool hbm = false;                     // images beyond the LDS of a CU: every member on the HBM-resident kernel (qp_small_hbm.hip)
    // the host's record of H's symmetry (judge_h_sym): h_sym = every H symmetric value by value (the tableau kernel of qp_tiny.hip
    // may take the batch); h_symq[q] = member q's is. Kept for batches of at most 8 variables, with the H patterns in the caller's
    // layout (member q's entries start at h_Huoff[q]), which are re-examined when the values change
    bool h_sym = true;
    std::vector<int> h_Hjc, h_Hir;
    std::vector<long long> h_Huoff;
    std::vector<char> h_symq;
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
    DevBuf<long long> koV, koC;
    // the one device scratch block (ensure_scratch; grows, never shrinks) and the pinned block host-pointer calls pack their arrays
    // into (ensure_staging of rsqp_batch_handler.hip). Every call that uses either waits for the stream before it returns, so both
    // are free at every entry and each user lays out its own offsets from 0: the named setters (the caller's arrays), the
    // host-pointer handler calls (one packed block up or down), rsqp_batch_pack_records_host (the records; it waits before its
    // download). rsqp_batch_solve and rsqp_batch_pack_records_dev return without waiting and use neither
    DevBuf<double> scratch;
    HostBuf<double> pin;
    // warm re-initialisation inputs (RSQP_MODE_WARM_REINIT), pooled like the vectors; allocated at first use. have_*: what
    // rsqp_batch_set_warm_start gave (rsqp_batch_solve); rsqp_batch_optimize_qp fills the same pools on the device
    DevBuf<double> wx0, wy0;
    DevBuf<int> wgb;
    bool have_x0 = false, have_y0 = false, have_gb = false;
    DevBuf<int> opt;                      // the OPT_* words, OPT_WORDS * nq (ensure_opt)
    // rsqp_batch_set_members: who takes part in the optimize calls. The kernels get the mask only while somebody sits out; with the
    // default and with an all-ones mask the calls issue what they issued before there was a mask
    DevBuf<int> take;
    bool sitters = false;                 // somebody sits out
    // rsqp_batch_set_vectors_of / rsqp_batch_set_matrix_values_of: the caller's mask on the device, allocated at first use, and where
    // member q's entries start in a non-canonical caller layout (Afold / Hfold)
    DevBuf<int> named;
    DevBuf<long long> Auoff, Huoff;
    // the QPhandler layer (rsqp_batch_handler_*): the NLP bounds of the members (x_l, x_u in the NLP layout, c_l, c_u in the
    // constraint layout)
    DevBuf<double> h_xl, h_xu, h_cl, h_cu;
    long long sumN = 0;                   // NLP variables of the batch: sumV - 2 sumC
    bool have_problem = false;            // rsqp_batch_handler_set_problem has run
    // rsqp_batch_handler_set_matrices: h_jn[q] = entries of columns [0, n_q) of member q's A in the caller's layout (from
    // rsqp_batch_create; sumJ of them in all). At the first call: where member q's entries start in jac (hm_joff, nq + 1) and the
    // inverse of perm (hm_inv: CSC slot -> CSR slot)
    std::vector<int> h_jn;
    long long sumJ = 0;
    bool uni_jn = false;                  // a one-pattern batch in a canonical layout: every member has h_jn[0] entries in jac
    bool hm_ready = false;
    DevBuf<long long> hm_joff;
    DevBuf<int> hm_inv;
    // the symmetry of every member's H on the device (batches of at most 8 variables): the device's copy of h_symq, stale after a
    // host setter has re-examined members, and the host-mapped word a verdict that differs from the copy is flagged through
    DevBuf<char> d_symq;
    bool symq_stale = true;
    HostBuf<int> sym;
    // optimizeLP per member (rsqp_batch_optimize_lp): the members' descriptors with H absent and hreg = regVal of the member's last
    // init (written on the device, kept across hot starts), and the pool of the proximal step's gradients g - regVal x
    DevBuf<QPDesc> d_desc_lp;
    DevBuf<double> g_lp;
    int lp_maxiter = 100;                 // rsqp_batch_set_lp_options
    int last_kind = 0;                    // 0 no optimize call yet, 1 the last one was rsqp_batch_optimize_qp, 2 rsqp_batch_optimize_lp
    bool cert_lp = false;                 // the results in the pools are an LP call's: rsqp_batch_test_optimality certifies the LP
    // nWSR_used of the members, written by the kernels straight into host-mapped memory: ready behind the call's one wait, no copy
    // (and no second wait) behind it
    HostBuf<int> used;
    // rsqp_batch_set_handover: every launch on the hs071-scale tableau kernels (families 1, 2) is followed by the hand-over launch
    // (launch_batch). handed: nq flags + their count, cleared where a solve / optimize call with the switch on begins, written by the
    // members that are taken over; handed_valid: the last call was such a call (else rsqp_batch_get_handover reports zeros)
    bool handover = false, handed_valid = false;
    DevBuf<int> handed;
    // rsqp_batch_set_lane_warm: hot starts with new matrices and warm re-initialisations of a batch the lane-per-problem kernel takes
    // go to its WARM builds (lane_warm_ok of rsqp_batch.hip says which launches). results_foreign: the result pools may not describe
    // the members' stored states, which such a hot start assumes -- rsqp_batch_set_results has overwritten them, or a hand-over launch
    // has run, since the last call whose first launch ran everybody without one (launch_batch)
    bool lane_warm = false, results_foreign = false;
    // rsqp_batch_set_lane_hot: where lane_warm_ok holds, hot starts on new vectors and optimize calls whose update marks are per
    // member go to the WARM builds of level 2 as well. Alone it changes nothing
    bool lane_hot = false;
    int qp_maxiter = 1000;                // rsqp_batch_set_options
    bool mats_updated = false;            // rsqp_batch_set_matrix_values since the last optimize call (Update_A / Update_H of everybody)
    bool opt_started = false;             // an rsqp_batch_optimize_qp has run: members are in different states from here on
    float last_ms = 0.f;
    bool keep_state = true;
    // rsqp_batch_handler_pair_lp / rsqp_batch_handler_update_penalty (rsqp_batch_penalty.hip): the host's copy of the canonical A
    // pattern (what the pairing compares), the LP batch paired with this one, and the call's work on the device
    std::vector<int> h_Ajc, h_Air;
    rsqp_batch *lp_pair = nullptr;
    DecisionWork pen;
    // rsqp_batch_handler_soc_begin / _soc_end (rsqp_batch_soc.hip): the calls' work on the device, which lives from soc_begin to
    // soc_end (so it is not the penalty call's). soc_begun: a soc_begin has run
    DecisionWork soc;
    bool soc_begun = false;
    bool timing = false;   // between timer_start and timer_stop: no per-launch events (they cost ~10 us of stream time each)
    ~rsqp_batch() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace rsqp_batch_units {
// rsqp_batch.hip
QPPools pools_of(rsqp_batch *b, bool lp);
int batch_family(const rsqp_batch *b, const QPPools &p, bool lp);
// warm: the launch may take a WARM build of the lane-per-problem kernel (lane_warm_ok, and what the caller knows of the call): 1, or
// 2 = one that carries hot starts on new vectors as well (lane_warm_level)
int launch_batch(rsqp_batch *b, QPPools &p, int mode, int max_nWSR, bool first, bool lp, int warm = 0);
// the batch's side of SmallFacts::lane_warm: the switch is on, nothing is handed over, the result pools are the batch's own
bool lane_warm_ok(const rsqp_batch *b);
int lane_warm_level(const rsqp_batch *b);
// where a solve / optimize call begins: the hand-over flags and their count cleared (on the stream) when the switch is on
int begin_handover(rsqp_batch *b);
int ensure_opt(rsqp_batch *b);
int ensure_warm_pools(rsqp_batch *b);
int ensure_scratch(rsqp_batch *b, size_t words);
// members == null: everybody's h_symq anew from Hval, else the named members' (values in the caller's layout); then h_sym, and the
// device's copy is stale. Hval == null: h_symq is on record already (read back from the device) and h_sym alone follows it
void judge_h_sym(rsqp_batch *b, const int *members, const double *Hval);
// after values have been written: the sums of a folded layout into the canonical pool, and (A) the CSR copy from that pool
int settle_A(rsqp_batch *b);
int settle_H(rsqp_batch *b);
// rsqp_batch_handler.hip: the pinned block and the scratch block of at least `words` doubles each (rsqp_batch::scratch)
int ensure_staging(rsqp_batch *b, size_t words);
// what rsqp_batch_handler_set_matrices builds at its first call: hm_joff, and hm_inv, the inverse of perm (CSC slot -> CSR slot)
int ensure_handler_matrices(rsqp_batch *b);

// ---- what the member-by-member kernels and their calls share; no floating-point formula (those: rsqp_batch_decide.h) ----
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

// hs071-scale members: 8 lanes each, eight members per wavefront; else a wavefront per member
inline int lanes_per_member(const rsqp_batch *b) { return (b->nVmax + b->nCmax <= 16) ? 8 : 64; }
inline dim3 grid_of(const rsqp_batch *b, int G) { return dim3((unsigned)(((long long)b->nq * G + 255) / 256)); }
inline int uni_shape(const rsqp_batch *b) { return (b->uniV > 0 && b->uniC >= 0) ? b->uniV : 0; }
inline StageSizes stage_sizes(const rsqp_batch *b) { return StageSizes{(size_t)b->nq, (size_t)b->sumN, (size_t)b->sumC}; }

// the one launch of a kernel with G lanes per member: kernel(g) is its instance for g = std::integral_constant<int, G>, e.g.
// [](auto g) { return batch_nlp_ratio_kernel<decltype(g)::value>; }. On the batch's stream, grid_of(b, G) x 256
template <class Kernel, class... Args>
int launch_groups(rsqp_batch *b, Kernel kernel, const Args &... args) {
    const int G = lanes_per_member(b);
    if (G == 8) hipLaunchKernelGGL(kernel(std::integral_constant<int, 8>()), grid_of(b, G), dim3(256), 0, b->stream, args...);
    else hipLaunchKernelGGL(kernel(std::integral_constant<int, 64>()), grid_of(b, G), dim3(256), 0, b->stream, args...);
    HIPCHK(hipGetLastError());
    return RSQP_OK;
}
// ... of a decision kernel (report_live): waits for it; *live = how many members go on
template <class Kernel, class... Args>
int launch_decision(rsqp_batch *b, const DecisionWork &w, int *live, Kernel kernel, const Args &... args) {
    const int rc = launch_groups(b, kernel, args...);
    if (rc != RSQP_OK) return rc;
    HIPCHK(hipStreamSynchronize(b->stream));
    *live = *w.live.p;
    return RSQP_OK;
}

// The HIP side of a call's staging block (StagingLayout): the fields are declared while `active` (a host-pointer call); with
// on_device the caller's pointers pass through and only down()'s wait remains. up(): the caller's arrays into the pinned block,
// what goes up in one copy to the same words of the scratch block, the declared fields to their device addresses. down(): the
// tail that comes down in one copy (`copy`: somebody takes it), the wait for the stream, the tail into the caller's arrays
struct Staging : StagingLayout {
    rsqp_batch *b;
    bool active;
    Staging(rsqp_batch *batch, int on_device) : b(batch), active(on_device == 0) {}
    int up() {
        if (!active) return RSQP_OK;
        if (!ok()) return fail(RSQP_ERR_ARG, "staging block: more fields than the table holds, or an up-only field behind the tail");
        const int rc = ensure_staging(b, words());
        if (rc != RSQP_OK) return rc;
        pack(b->pin.p);
        if (up_words() > 0) HIPCHK(hipMemcpyAsync(b->scratch.p, b->pin.p, sizeof(double) * up_words(), hipMemcpyHostToDevice, b->stream));
        address(b->scratch.p);
        return RSQP_OK;
    }
    int down(bool copy = true) {
        if (active && copy && words() > tail())
            HIPCHK(hipMemcpyAsync(b->pin.p + tail(), b->scratch.p + tail(), sizeof(double) * (words() - tail()), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (active) unpack(b->pin.p);
        return RSQP_OK;
    }
};

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
