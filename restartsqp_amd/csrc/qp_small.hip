// qp_small.hip -- batched online active-set QP engine for gfx950: the whole solver state of a
// problem (Q, T, R, iterate, working set) resident in LDS, L = 16 / 32 / 64 lanes of a wave per
// problem (64 / L problems share a one-wave workgroup).
//
// Replaces, for hs0xx-scale problems, the qpOASES 3.2.1 SQProblem::init / hotstart calls
// made at reference src/qpOASESInterface.cpp:155,180,184,191,197,204. Algorithm = dense
// null-space online active-set strategy (see DESIGN.md section "Algorithm"):
//   A_AC,FR * Q = [0 T]  (T reverse triangular),  R'R = Z'HZ,  Givens up/down-dates,
//   primal + dual ratio tests with lowest-candidate-id tie break, exchange on linear
//   dependence, bound flipping when Z'HZ would lose definiteness.
//
// MI355X mapping:
//   * workgroup = one wave = 64 / L problems, grid = ceil(nq * L / 64) -- a batch fills the 256
//     CUs with independent problems; no inter-workgroup communication and no s_barrier: the
//     problems of a wave follow their own control flow under exec masking, and a wave's LDS
//     instructions execute in program order, so a compiler fence is all the sync it needs.
//     hs0xx-scale problems (nV <= 16) use L = 16: their vectors never filled 64 lanes.
//   * LDS image per problem (rsqp_image_bytes): Q and R column-major with an ODD leading
//     dimension so that the lane<->row and lane<->column access patterns below are both
//     bank-conflict free for ds_read_b64; T row-major with the same stride.
//   * sparse H / A stay in global memory in CSC (+ a CSR copy of A): they are read-only
//     and L2-resident; lane-per-row / lane-per-column products, no atomics.
//   * reductions are butterflies over the L lanes of a problem (DPP permutations inside a row, identical result
//     in each of them) so control flow stays uniform per problem; argmin carries the candidate
//     id for the deterministic tie break. With nV <= L every lane owns at most one entry of a
//     vector, so the sums are bit-identical for every L (tools/small_pack_check.py).
//   * the image is written back to HBM at the end of a solve and reloaded by the next
//     hot start (qpOASES keeps the same data inside the SQProblem object).
#include <cstdlib>
#include <type_traits>

#include "rsqp_small_plan.h"

// diagnostic build only (-DRSQP_STAMPS, tools/stamp_small_kernel.py): cycles per phase of block 0
#ifdef RSQP_STAMPS
__device__ unsigned long long g_stamps[48];
#define STAMP(k)                                                                                    \
    do {                                                                                            \
        long long t_ = clock64();                                                                   \
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_stamps[k], (unsigned long long)(t_ - tlast)); \
        tlast = t_;                                                                                 \
    } while (0)
extern "C" void rsqp_debug_stamps(unsigned long long *out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 48);
    if (reset) {
        unsigned long long z[48] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z));
    }
}
#else
#define STAMP(k) do { } while (0)
#endif

namespace {

#include "qp_small_engine.h"

#include "qp_small_x.h"

// ------------------------------------------------------------------------------------
// bytes of LDS needed to stage the sparse matrices of one problem behind its image
__host__ __device__ inline long long mat_lds_bytes(int nV, int nC, int annz, int hnnz) {
    long long idx = 2LL * (nV + 1) + (nC + 1) + 2LL * annz + hnnz, dbl = 2LL * annz + hnnz;   // 16-bit indices
    return ((idx * 2 + 7) & ~7LL) + dbl * 8;
}

// L = lanes per problem (64 / L problems share one wave; each owns `stride` bytes of LDS),
// W = minimum waves per SIMD the register allocator has to leave room for
// SHAPE = NVC * 256 + NCC > 0: every problem of the batch has the shape NVC x NCC, known at COMPILE time
// (parameter scans / the hs071-scale batch: 8 x 2 through the QPhandler formulation). Sizes, loop bounds and
// the offsets of the LDS image are then constants: every vector of the engine sits at an immediate offset of
// ONE per-lane base address instead of in a register of its own, and every loop over a vector is straight-line.
// (Passing the uniform shape as kernel ARGUMENTS instead -- wave-uniform scalars -- measured 221 VGPRs instead
// of 256 but 214 vs 226 M solves/s on 65 536 hs071-scale QPs: not built.)
// HAND: the build of the hand-over launch of a batch (rsqp_launch_small_handover, small_qp_handover_kernel below): it runs the
// members a hs071-scale tableau kernel left with ret == RET_SETUP_FAILED as rsqp_solve's retry runs a handle, and leaves their state
// blocks to that kernel. The builds of every other launch carry nothing of it
template <class ENG, int L, bool MAT_LDS, int SHAPE, bool HAND>
__device__ __forceinline__ void small_qp_solve(const QPPools &P, int nq, int stride, int mode, int maxWSR, int *handed, int mark_at) {
    constexpr int NVC = SHAPE >> 8, NCC = SHAPE & 255;
    extern __shared__ __attribute__((aligned(16))) char smem_generic[];
    const int lane = L >= 64 ? (int)threadIdx.x : (int)threadIdx.x & (L - 1);
    const int grp = L >= 64 ? 0 : (int)threadIdx.x / L;  // L >= 64: everything below stays workgroup-uniform
    const int q = L >= 64 ? (int)blockIdx.x : blockIdx.x * (64 / L) + grp;
    if (q >= nq) return;  // no workgroup barrier anywhere below: idle groups may leave
    if constexpr (!HAND) {
        if (P.only_bailed && P.ret[q] != RET_BAIL) return;   // second pass behind the tableau kernel (qp_small_g.h)
    }
    if (P.member_mode) { mode = P.member_mode[q]; if (mode < 0) return; }   // per-member call shape; < 0: not in this launch
    if constexpr (HAND) {
        // second pass behind a hs071-scale tableau kernel: the members it gave up on. Asked AFTER the member's mode: the ret of a
        // member that is not in the launch is a stale one
        if (P.ret[q] != RET_SETUP_FAILED) return;
        // the stored state is the tableau kernel's: a hot start begins cold, as rsqp_solve's retry does on a handle (a warm
        // re-initialisation keeps its inputs). The member raises its flag, and the count the first time in a call
        if (mode == 1 || mode == 2) mode = 0;
        if (handed && lane == 0 && handed[q] == 0) { handed[q] = 1; atomicAdd(handed + nq, 1); }
    }
    lchar *smem = (lchar *)smem_generic + grp * stride;
    QPDesc d = P.desc[q];
    if constexpr (SHAPE > 0) { d.nV = NVC; d.nC = NCC; }
    if constexpr (L < 64) {
        // packed waves are only launched when every problem of the batch has nV, nC <= L: a loop over a
        // vector of the engine is then a single predicated trip (no back edge, no counter)
        __builtin_assume(d.nV <= L && d.nV >= 0);
        __builtin_assume(d.nC <= L && d.nC >= 0);
    }
    ENG E;
    E.lane = lane;
    if constexpr (L > 64) E.part = (ldouble *)(smem + stride) - L;   // the launcher reserves 8 L bytes at the end
#ifdef RSQP_STAMPS
    E.tlast = clock64();
    long long &tlast = E.tlast;
#endif
    E.carve(smem, d.nV, d.nC);
    const int nd = (int)ENG::image_doubles(d.nV, d.nC), ni = (int)ENG::image_ints(d.nV, d.nC);
    const int np = (int)ENG::persist_doubles(d.nV, d.nC);   // what goes to / comes from HBM: [np doubles][ni ints]
    const int img_bytes = (nd * 8 + ni * 2 + 7) & ~7;   // the staged matrices follow 8-byte aligned
    E.haveH = d.haveH;
    E.hreg = d.hreg;
    const int *gAjc = P.Ajc + d.offAjc, *gAir = P.Air + d.offAnz, *gArp = P.Arp + d.offArp, *gAci = P.Aci + d.offAnz;
    const int *gHjc = P.Hjc + d.offHjc, *gHir = P.Hir + d.offHnz;
    const double *gAval = P.Aval + d.offAnz, *gArv = P.Arv + d.offAnz, *gHval = P.Hval + d.offHnz;
    if constexpr (ENG::DENSE_MATS) {
        E.stage_dense(smem + img_bytes, gAjc, gAir, gAval, gHjc, gHir, gHval);
    } else if constexpr (MAT_LDS) {
        // stage CSC(A), CSR(A), CSC(H) behind the image
        const int annz = d.annz >= 0 ? d.annz : gAjc[d.nV], hnnz = !d.haveH ? 0 : (d.hnnz >= 0 ? d.hnnz : gHjc[d.nV]);
        LDS unsigned short *ip0 = (LDS unsigned short *)(smem + img_bytes), *ip = ip0;
        LDS unsigned short *lAjc = ip; ip += d.nV + 1;
        LDS unsigned short *lArp = ip; ip += d.nC + 1;
        LDS unsigned short *lHjc = ip; ip += d.nV + 1;
        LDS unsigned short *lAir = ip; ip += annz;
        LDS unsigned short *lAci = ip; ip += annz;
        LDS unsigned short *lHir = ip; ip += hnnz;
        ldouble *dp = (ldouble *)(smem + img_bytes + (((ip - ip0) * 2 + 7) & ~7));
        ldouble *lAval = dp; dp += annz;
        ldouble *lArv = dp; dp += annz;
        ldouble *lHval = dp;
        for (int k = lane; k <= d.nV; k += L) { lAjc[k] = gAjc[k]; lHjc[k] = d.haveH ? gHjc[k] : 0; }
        for (int k = lane; k <= d.nC; k += L) lArp[k] = gArp[k];
        for (int k = lane; k < annz; k += L) { lAir[k] = gAir[k]; lAci[k] = gAci[k]; lAval[k] = gAval[k]; lArv[k] = gArv[k]; }
        for (int k = lane; k < hnnz; k += L) { lHir[k] = gHir[k]; lHval[k] = gHval[k]; }
        E.Ajc = lAjc; E.Air = lAir; E.Aval = lAval; E.Arp = lArp; E.Aci = lAci; E.Arv = lArv;
        E.Hjc = lHjc; E.Hir = lHir; E.Hval = lHval;
    } else {
        E.Ajc = gAjc; E.Air = gAir; E.Aval = gAval; E.Arp = gArp; E.Aci = gAci; E.Arv = gArv;
        E.Hjc = gHjc; E.Hir = gHir; E.Hval = gHval;
    }
    E.nflips = 0; E.infeasible = E.unbounded = 0; E.status = QPS_NOTINITIALISED; E.nFR = E.nAC = 0;
    double *img = P.state + d.offState;
    int *iimg = reinterpret_cast<int *>(img + np);
    ldouble *simg = (ldouble *)smem;
    lint *siimg = (lint *)(simg + nd);

    int rcode = RET_OK, nWSR = 0;
    if (mode == 0) {
        // (the factor arrays at the head of the image are zeroed by setup_aux itself)
        for (int k = (int)ENG::factor_doubles(d.nV, d.nC) + lane; k < nd; k += L) simg[k] = 0.0;
        for (int k = lane; k < ni; k += L) siimg[k] = 0;
        SYNC();
    }
    if (mode != 0) {  // reload the image of the previous solve
        for (int k = lane; k < np; k += L) simg[k] = img[k];
        for (int k = np + lane; k < nd; k += L) simg[k] = 0.0;
        for (int k = lane; k < ni; k += L) siimg[k] = iimg[k];
        SYNC();
        E.restore(E.iscal[1], E.iscal[2], E.iscal[3]);
        SYNC();
        if (E.status == QPS_NOTINITIALISED) mode = 0;
    }
    STAMP(0);
    E.store_targets(P.g + d.offV, P.lb + d.offV, P.ub + d.offV, P.lbA + d.offC, P.ubA + d.offC);
    if (E.bounds_inconsistent()) {  // qpOASES areBoundsConsistent: infeasible before any change
        E.infeasible = 1; E.unbounded = 0;
        rcode = RET_INFEASIBLE;
    } else if (mode == 0) {
        rcode = E.setup_aux(false, false, false, false);
    } else if (mode == 2) {  // hot start with new matrices: keep x, y and the working set
        for (int v = lane; v < d.nV; v += L) { E.wv4[v] = E.x[v]; E.wq[v] = (double)E.Sb[v]; }
        for (int i = lane; i < d.nV + d.nC; i += L) E.dy[i] = E.y[i];
        for (int i = lane; i < d.nC; i += L) E.wc1[i] = (double)E.Sc[i];
        SYNC();
        rcode = E.setup_aux(true, true, true, true);
        if (rcode != RET_OK) rcode = E.setup_aux(false, false, false, false);
    } else if (mode == 3) {  // warm re-initialisation from (x0, y0, guessed bounds)
        if (P.x0) for (int v = lane; v < d.nV; v += L) E.wv4[v] = P.x0[d.offV + v];
        if (P.y0) for (int i = lane; i < d.nV + d.nC; i += L) E.dy[i] = P.y0[d.offV + d.offC + i];
        if (P.guess_b) for (int v = lane; v < d.nV; v += L) E.wq[v] = (double)P.guess_b[d.offV + v];
        SYNC();
        // no guessed constraints in this call shape (qpOASESInterface.cpp:204-206): their sides come from the signs of
        // A x0 as qpOASES does (the default) -- or, opt-in (P.reinit_from_y0), from the signs of y0
        rcode = E.setup_aux(P.x0 != nullptr, P.y0 != nullptr, P.guess_b != nullptr, false, P.reinit_from_y0 != 0);
        if (rcode != RET_OK) rcode = E.setup_aux(false, false, false, false);
    } else {
        E.infeasible = E.unbounded = 0;
        if constexpr (ENG::K_IMAGE) {
            // the state is one the KKT-tableau kernel wrote (and then bailed out of this hot start): its factors
            // are not this engine's -- rebuild them for the stored working set, keep the homotopy data
            if (E.iscal[4] != 0) {     // (1: round 3, M = K^-1; 2: the tableau of qp_small_g.h -- either way not this engine's factors)
                rcode = E.rebuild_factors();
                if (rcode != RET_OK) rcode = E.setup_aux(false, false, false, false);
            }
        }
    }
    STAMP(2);
    if (rcode == RET_OK) rcode = E.homotopy(maxWSR, nWSR);
    double obj = E.objective();
    STAMP(8);

    // results
    for (int v = lane; v < d.nV; v += L) { P.x[d.offV + v] = E.x[v]; P.ws_b[d.offV + v] = E.Sb[v]; }
    for (int i = lane; i < d.nV + d.nC; i += L) P.y[d.offV + d.offC + i] = E.y[i];
    for (int i = lane; i < d.nC; i += L) P.ws_c[d.offC + i] = E.Sc[i];
    if (lane == 0) {
        int st = E.status;
        P.status[q] = E.infeasible ? 100 + st : (E.unbounded ? 200 + st : st);
        P.ret[q] = rcode;
        P.nwsr[q] = nWSR;
        P.nflips[q] = E.nflips;
        P.obj[q] = obj;
        E.iscal[1] = E.nFR; E.iscal[2] = E.nAC; E.iscal[3] = E.status;
        if constexpr (ENG::K_IMAGE) E.iscal[4] = 0;      // this engine's factors
    }
    if (P.done_flag) __threadfence_system();      // the results above are in host-mapped memory: visible before the flag
    SYNC();
    if (P.done_flag && q == 0 && lane == 0) *reinterpret_cast<volatile int *>(P.done_flag) = P.done_val;
    if constexpr (HAND) {
        // the member's next call goes to the tableau kernel first again, which must read "not initialised" here: in ITS layout,
        // mark_at doubles into the block (< 0: that launch keeps no state and leaves no mark, neither does this one). Nothing of
        // this engine's image is stored: no call would ever read it
        if (lane == 0 && mark_at >= 0) {
            int *si = reinterpret_cast<int *>(img + mark_at);
            si[16] = QPS_NOTINITIALISED; si[18] = TINY_MAGIC;
        }
        STAMP(9);
        return;
    }
    if (P.keep_state) {
        for (int k = lane; k < np; k += L) img[k] = simg[k];
        for (int k = lane; k < ni; k += L) iimg[k] = siimg[k];
    } else if (lane == 0) {
        iimg[(int)(E.iscal - siimg) + 3] = QPS_NOTINITIALISED;
    }
    STAMP(9);
}

template <class ENG, int L, bool MAT_LDS, int W, int SHAPE>
__global__ void __launch_bounds__(L > 64 ? L : 64, W)
small_qp_kernel(QPPools P, int nq, int stride, int mode, int maxWSR) {
    small_qp_solve<ENG, L, MAT_LDS, SHAPE, false>(P, nq, stride, mode, maxWSR, nullptr, -1);
}
template <class ENG, int L, bool MAT_LDS, int W, int SHAPE>
__global__ void __launch_bounds__(L > 64 ? L : 64, W)
small_qp_handover_kernel(QPPools P, int nq, int stride, int mode, int maxWSR, int *handed, int mark_at) {
    small_qp_solve<ENG, L, MAT_LDS, SHAPE, true>(P, nq, stride, mode, maxWSR, handed, mark_at);
}

#include "qp_small_g.h"

static_assert(EngineG<3, 1, 9, 4>::MAXV == 72 && EngineG<3, 1, 9, 4>::MAXC == 32 && EngineG<2, 2, 8, 8>::MAXV == 64 && EngineG<2, 2, 8, 8>::MAXC == 64,
              "the sizes rsqp_plan_small_launch sends to the tableau kernels");

}  // namespace

int rsqp_small_qp_fits(int nVmax, int nCmax) {
    return rsqp_align16(rsqp_image_bytes(nVmax, nCmax)) <= kSmallMaxLds;
}

static int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

SmallKnobs rsqp_small_knobs_from_env() {
    SmallKnobs k;
    k.engine = env_int("RSQP_SMALL_ENGINE", -1); k.k_debug_bail = env_int("RSQP_K_DEBUG_BAIL", -1);
    k.lanes = env_int("RSQP_SMALL_LANES", -1); k.waves = env_int("RSQP_SMALL_WAVES", -1);
    k.lane = env_int("RSQP_LANE", -1); k.lane_hblock = env_int("RSQP_LANE_HBLOCK", -1); k.lane_shape = env_int("RSQP_LANE_SHAPE", -1); k.arena_mapped = env_int("RSQP_ARENA_MAPPED", -1);
    k.no_spin = getenv("RSQP_NO_SPIN") != nullptr;
    return k;
}

namespace {
// one instantiation of the null-space kernel: launches the plan it matches (the full LDS is allowed once per kernel and device)
// (the plan sizes the image by its own restatement of the engine's counts: compared once per build, over every size that fits)
template <int E, class ENG, int SHAPE>
bool plan_agrees() {
    for (int nV = 1; nV <= 128; nV++)
        for (int nC = 0; nC <= 128; nC++)
            if (ENG::image_doubles(nV, nC) != rsqp_plan_image_doubles(E, SHAPE != 0, nV, nC) ||
                ENG::image_ints(nV, nC) != rsqp_plan_image_ints(E, nV, nC)) return false;
    return true;
}
template <int E, class ENG, int L, bool ML, int W, int SHAPE>
hipError_t launch_build(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream) {
    static std::atomic<unsigned long long> set_{0};
    static const bool agrees = plan_agrees<E, ENG, SHAPE>();
    if (!agrees) return hipErrorInvalidValue;
    rsqp_allow_full_lds(reinterpret_cast<const void *>(&small_qp_kernel<ENG, L, ML, W, SHAPE>), set_, (int)kSmallMaxLds);
    hipLaunchKernelGGL((small_qp_kernel<ENG, L, ML, W, SHAPE>), dim3(pl.grid), dim3(pl.block), (size_t)pl.lds, stream, p, nq, pl.stride, pl.mode, maxWSR);
    return hipGetLastError();
}
// ... and its hand-over build (small_qp_handover_kernel)
template <int E, class ENG, int L, bool ML, int W, int SHAPE>
hipError_t launch_handover_build(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, int *handed, int mark_at, hipStream_t stream) {
    static std::atomic<unsigned long long> set_{0};
    static const bool agrees = plan_agrees<E, ENG, SHAPE>();
    if (!agrees) return hipErrorInvalidValue;
    rsqp_allow_full_lds(reinterpret_cast<const void *>(&small_qp_handover_kernel<ENG, L, ML, W, SHAPE>), set_, (int)kSmallMaxLds);
    hipLaunchKernelGGL((small_qp_handover_kernel<ENG, L, ML, W, SHAPE>), dim3(pl.grid), dim3(pl.block), (size_t)pl.lds, stream, p, nq, pl.stride,
                       pl.mode, maxWSR, handed, mark_at);
    return hipGetLastError();
}
// every instantiation of this unit, by the plan's (engine, L, mat_lds, W, shape). The two quick-turnaround builds for tuning
// (tools/small_experiment.sh) keep a part of the table: -DRSQP_SMALL_EXPERIMENT the 8-lane Givens / TQ kernels, with the builds for
// 3 and 4 waves per SIMD the product does not have; -DRSQP_SMALL_EXPERIMENT=2 the four-wave explicit-inverse kernel (mid-size
// problems, BASELINE configs[4]). A plan outside the table is an invalid launch.
// handover: the build of the hand-over launch, for the plans rsqp_plan_small_launch gives a launch of at most 8 x 8 without the tableau
// kernels (SmallKnobs::no_tiny = 1) -- the Givens / TQ engine with its matrices in LDS, whatever lanes and waves the knobs ask for
struct Build {
    int engine, L, mat_lds, W, shape;
    hipError_t (*launch)(const SmallPlan &, const QPPools &, int, int, hipStream_t);
    hipError_t (*handover)(const SmallPlan &, const QPPools &, int, int, int *, int, hipStream_t);
};
template <int E, class ENG, int L, bool ML, int W, int SHAPE = 0>
constexpr Build build() { return {E, L, ML, W, SHAPE, &launch_build<E, ENG, L, ML, W, SHAPE>, nullptr}; }
template <int E, class ENG, int L, bool ML, int W, int SHAPE = 0>
constexpr Build build_h() { return {E, L, ML, W, SHAPE, &launch_build<E, ENG, L, ML, W, SHAPE>, &launch_handover_build<E, ENG, L, ML, W, SHAPE>}; }
constexpr int S82 = 8 * 256 + 2;      // the compile-time shape 8 x 2, target vectors in registers
const Build kBuilds[] = {
#if defined(RSQP_SMALL_EXPERIMENT) && RSQP_SMALL_EXPERIMENT == 2
    build<1, EngineX<256, true>, 256, true, 1>(),
#elif defined(RSQP_SMALL_EXPERIMENT)
    build<0, Engine<8, true, true>, 8, true, 2, S82>(), build<0, Engine<8, true, true>, 8, true, 3, S82>(),
    build<0, Engine<8, true, true>, 8, true, 4, S82>(),
    build<0, Engine<8, true>, 8, true, 2>(), build<0, Engine<8, true>, 8, true, 3>(), build<0, Engine<8, true>, 8, true, 4>(),
#else
    build<1, EngineX<64, false>, 64, false, 3>(), build<1, EngineX<16, true>, 16, true, 2>(),
    build<1, EngineX<32, true>, 32, true, 2>(), build<1, EngineX<256, true>, 256, true, 1>(),
    build<1, EngineX<64, true>, 64, true, 4>(),
    build<0, Engine<64, false>, 64, false, 3>(),
    build_h<0, Engine<8, true, true>, 8, true, 2, S82>(), build_h<0, Engine<8, true>, 8, true, 2>(),
    build_h<0, Engine<16, true>, 16, true, 2>(), build_h<0, Engine<16, true>, 16, true, 3>(), build_h<0, Engine<16, true>, 16, true, 4>(),
    build_h<0, Engine<32, true>, 32, true, 2>(), build_h<0, Engine<32, true>, 32, true, 3>(), build_h<0, Engine<32, true>, 32, true, 4>(),
    build_h<0, Engine<64, true>, 64, true, 3>(), build_h<0, Engine<64, true>, 64, true, 4>(),      // (W = 6: wrong results, rsqp_small_plan.h)
#endif
};
const Build *find_build(const SmallPlan &pl, int W) {
    for (const Build &k : kBuilds)
        if (k.engine == pl.engine && k.L == pl.L && k.mat_lds == pl.mat_lds && k.W == W && k.shape == pl.shape) return &k;
    return nullptr;
}
}  // namespace

// launches what the plan says (rsqp_small_plan.h): no decision is taken here
hipError_t rsqp_launch_small_qp(const SmallKnobs &kn, const SmallPlan &pl, const QPPools &p_in, int nq, int maxWSR, hipStream_t stream) {
    if (pl.empty) return hipSuccess;
    if (pl.invalid) return hipErrorInvalidValue;
    QPPools p = p_in;
    p.only_bailed = 0;
    p.k_debug_bail = pl.family == 3 ? -1 : kn.k_debug_bail;
    p.skip_mark = pl.skip_mark;
    if (pl.family == 3) return rsqp_launch_small_qp_hbm(pl, p, nq, maxWSR, stream);
    if (pl.family == 2) return rsqp_launch_lane_qp(pl, p, nq, maxWSR, stream);
    if (pl.family == 1) return rsqp_launch_tiny_qp(pl, p, nq, maxWSR, stream);
    int W = pl.W;
#if defined(RSQP_SMALL_EXPERIMENT) && RSQP_SMALL_EXPERIMENT != 2
    if (pl.L == 8 && (pl.waves == 3 || pl.waves == 4)) W = pl.waves;
#endif
    const Build *b = find_build(pl, W);
    if (!b) return hipErrorInvalidValue;
    if (pl.first) {
        if (pl.first == 1) hipLaunchKernelGGL((small_qpg_kernel<3, 1, 9, 4>), dim3(nq), dim3(256), 0, stream, p, nq, pl.mode, maxWSR);
        else hipLaunchKernelGGL((small_qpg_kernel<2, 2, 8, 8>), dim3(nq), dim3(256), 0, stream, p, nq, pl.mode, maxWSR);
        p.only_bailed = 1;
    }
    return b->launch(pl, p, nq, maxWSR, stream);
}

hipError_t rsqp_launch_small_handover(const SmallKnobs &kn, const SmallPlan &pl, const SmallPlan &tableau, const QPPools &p_in, int nq,
                                      int maxWSR, int *handed, hipStream_t stream) {
    if (pl.empty) return hipSuccess;
    // (the plan of a launch the tableau kernels serve, without them: an LDS-resident null-space kernel by itself)
    if (pl.invalid || pl.family != 0 || pl.first || (tableau.family != 1 && tableau.family != 2)) return hipErrorInvalidValue;
    QPPools p = p_in;
    p.only_bailed = 0;        // (the build itself takes the members with ret == RET_SETUP_FAILED, and nobody else)
    p.k_debug_bail = kn.k_debug_bail;
    p.skip_mark = pl.skip_mark;
    // where the tableau kernel of that launch keeps its ints (-1: it keeps no state and leaves no mark)
    long long at = -1;
    if (p.keep_state || !tableau.skip_mark)
        at = tableau.mc == 2 ? tiny_state_doubles<2>() : (tableau.mc == 4 ? tiny_state_doubles<4>() : tiny_state_doubles<8>());
    const Build *b = find_build(pl, pl.W);
    if (!b || !b->handover) return hipErrorInvalidValue;
    return b->handover(pl, p, nq, maxWSR, handed, (int)at, stream);
}

long long rsqp_mat_lds_bytes(int nV, int nC, int annz, int hnnz) { return mat_lds_bytes(nV, nC, annz, hnnz); }
