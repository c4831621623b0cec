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

#include "rsqp_internal.h"

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
template <class ENG, int L, bool MAT_LDS, int W, int SHAPE>
__global__ void __launch_bounds__(L > 64 ? L : 64, W)
small_qp_kernel(QPPools P, int nq, int stride, int mode, int maxWSR) {
    constexpr int NVC = SHAPE >> 8, NCC = SHAPE & 255;
    extern __shared__ __attribute__((aligned(16))) char smem_generic[];
    const int lane = L >= 64 ? (int)threadIdx.x : (int)threadIdx.x & (L - 1);
    const int grp = L >= 64 ? 0 : (int)threadIdx.x / L;  // L >= 64: everything below stays workgroup-uniform
    const int q = L >= 64 ? (int)blockIdx.x : blockIdx.x * (64 / L) + grp;
    if (q >= nq) return;  // no workgroup barrier anywhere below: idle groups may leave
    if (P.only_bailed && P.ret[q] != RET_BAIL) return;   // second pass behind the tableau kernel (qp_small_g.h)
    if (P.member_mode) { mode = P.member_mode[q]; if (mode < 0) return; }   // per-member call shape; < 0: not in this launch
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
    if (P.keep_state) {
        for (int k = lane; k < np; k += L) img[k] = simg[k];
        for (int k = lane; k < ni; k += L) iimg[k] = siimg[k];
    } else if (lane == 0) {
        iimg[(int)(E.iscal - siimg) + 3] = QPS_NOTINITIALISED;
    }
    STAMP(9);
}

#include "qp_small_g.h"

}  // namespace

static const long long kMaxLds = 160 * 1024;

static long long align16(long long v) { return (v + 15) & ~15LL; }

int rsqp_small_qp_fits(int nVmax, int nCmax) {
    return align16(rsqp_image_bytes(nVmax, nCmax)) <= kMaxLds;
}

static int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
}

SmallKnobs rsqp_small_knobs_from_env() {
    SmallKnobs k;
    k.engine = env_int("RSQP_SMALL_ENGINE", -1); k.k_debug_bail = env_int("RSQP_K_DEBUG_BAIL", -1);
    k.lanes = env_int("RSQP_SMALL_LANES", -1); k.waves = env_int("RSQP_SMALL_WAVES", -1);
    k.lane = env_int("RSQP_LANE", -1); k.lane_hblock = env_int("RSQP_LANE_HBLOCK", -1); k.arena_mapped = env_int("RSQP_ARENA_MAPPED", -1);
    k.no_spin = getenv("RSQP_NO_SPIN") != nullptr;
    return k;
}
int rsqp_small_launch_is_tiny(const SmallKnobs &kn, const QPPools &p, int nVmax, int nCmax) {
    return (kn.engine < 0 && p.tiny_ok && rsqp_tiny_fits(kn, nVmax, nCmax)) ? 1 : 0;
}
hipError_t rsqp_launch_small_qp(const SmallKnobs &kn, const QPPools &p_in, int nq, int nVmax, int nCmax, long long mat_bytes_max, int mode,
                                int maxWSR, hipStream_t stream) {
    QPPools p = p_in;
    p.only_bailed = 0;
    p.k_debug_bail = kn.k_debug_bail;
    if (nq <= 0) return hipSuccess;
    if (align16(rsqp_image_bytes(nVmax, nCmax)) > kMaxLds) return hipErrorInvalidValue;
    // formulation: 0 = Givens / TQ (Engine), 1 = explicit inverses (EngineX, qp_small_x.h), which keeps
    // DENSE copies of A and H in LDS. Measured per shape on the 512-QP hs0xx batch (ms, TQ vs explicit):
    // 5x1 0.14 / 0.16, 8x2 0.045 / 0.051, 8x3 0.25 / 0.21, 12x4 0.49 / 0.42, 16x6 0.73 / 0.55,
    // 23x6 1.26 / 1.01, 37x14 2.57 / 1.51, 69x28 10.8 / 4.1 -- the chains of the TQ form grow with nZ.
    const int forcedE = kn.engine;
    // hs071-scale problems: the register-resident tableau kernel (qp_tiny.hip) serves every call shape
    if (rsqp_small_launch_is_tiny(kn, p, nVmax, nCmax) && rsqp_lane_fits(kn, p, nq, nVmax, nCmax, mode)) return rsqp_launch_lane_qp(p, nq, maxWSR, stream);
    if (rsqp_small_launch_is_tiny(kn, p, nVmax, nCmax)) return rsqp_launch_tiny_qp(kn, p, nq, nVmax, nCmax, mode, maxWSR, stream);
    const int eng = forcedE == 0 || forcedE == 1 ? forcedE : (nVmax > 8 ? 1 : 0);
    if (eng == 1 && mat_bytes_max >= 0) mat_bytes_max = 8LL * ((long long)nVmax * nVmax + (long long)nCmax * nVmax);
    // uniform hs071-scale batches (8 x 2 through the QPhandler formulation; parameter scans of one NLP iterate) run
    // the build with the shape as a compile-time constant and the target vectors in registers (see RegVec)
    const int forcedL0 = kn.lanes;
    const bool shape82 = eng == 0 && p.uniV == 8 && p.uniC == 2 && mat_bytes_max >= 0 &&
                         (forcedL0 < 0 || forcedL0 == 8);        // only the 8-lane build has the shape instantiation
    // LDS image of the chosen formulation (the persistent copy in HBM is sized for the larger one)
    const long long imgd = eng == 1 ? EngineX<64, true>::image_doubles(nVmax, nCmax)
                                    : (shape82 ? Engine<8, true, true>::image_doubles(nVmax, nCmax) : Engine<64, true>::image_doubles(nVmax, nCmax));
    const long long imgi = eng == 1 ? EngineX<64, true>::image_ints(nVmax, nCmax) : Engine<64, true>::image_ints(nVmax, nCmax);
    const long long img = (8 * imgd + 2 * imgi + 7) & ~7LL;
    const bool mat_lds = mat_bytes_max >= 0 && align16(img + mat_bytes_max) <= kMaxLds;
    // LDS of one problem: image, then its staged matrices, 16-byte granular.
    long long stride = align16(img + (mat_lds ? mat_bytes_max : 0));
    // (an odd number of 16-byte units would spread the problems of a wave over the banks, but the LDS is
    // allocated in 512-byte steps and the 8-lane build needs 8 x 2880 = 45 x 512 bytes for 7 workgroups per CU)
    // lanes per problem: the vectors of the engine have nV (+ nC) entries, a wave of 64 lanes is
    // mostly idle on hs0xx-scale problems, so 64 / L of them share a wave. Problems in one wave
    // follow their own control flow (exec masking); the LDS capacity bounds the problems in flight.
    const int forcedL = kn.lanes, forcedW = kn.waves;
    const int nmax = nVmax > nCmax ? nVmax : nCmax;
    int L = nmax <= 8 ? 8 : (nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64));
    if ((forcedL == 8 || forcedL == 16 || forcedL == 32 || forcedL == 64) && forcedL >= L) L = forcedL;   // never fewer lanes than entries
    if (eng == 1 && L < 16) L = 16;   // the explicit-inverse build has no 8-lane instantiation
    if (!mat_lds) L = 64;
    while (L < 64 && (64 / L) * stride > kMaxLds) L *= 2;
    if (L == 64 && stride > kMaxLds) stride = align16(mat_lds ? img + mat_bytes_max : img);
    const bool wide0 = eng == 1 && mat_lds && L == 64 && nVmax > 32;
    bool wide = false;
    // several waves per problem: four (256 lanes, one wave per SIMD). The kernel keeps ~430 values live per lane
    // (256 VGPRs + AGPRs), so an eight-wave build spills 233 of them (measured).
    // With one wave per SIMD every wave instruction costs its full 4+ cycles: the four-wave kernel is bound by the
    // instruction count per wave (~350 per 69 x 69 product stage), not by LDS bandwidth or barriers.
    constexpr int wideL = 256;
    if (wide0 && stride + 8 * wideL <= kMaxLds) { stride += 8 * wideL; wide = true; }   // one double per lane of the wide build
    // bank spread of packed waves: a 32-lane LDS access group holds 32 / L problems, each touching 2 L consecutive
    // banks of the 64 (ds_read_b64: bank = dword address mod 64; stores: 16-lane groups, mod 32). Their images must
    // therefore start 2 L dwords apart modulo 64, i.e. stride = 8 L (mod 256) bytes -- with stride = 0 (mod 256)
    // every vector access of an 8-lane build is a 4-way conflict (measured: 54 % of the LDS-array cycles, LDS busy
    // 73 % of the kernel). The stride is padded to the next such value when that does not cost a resident workgroup.
    if (L < 64) {
        long long s1 = stride;
        while ((s1 & 255) != ((8 * L) & 255)) s1 += 16;
        auto wgs = [&](long long st) { const long long a = (((64 / L) * st) + 511) / 512 * 512; return a > 0 ? kMaxLds / a : 0; };
        if (wgs(s1) == wgs(stride) && (64 / L) * s1 <= kMaxLds) stride = s1;
    }
    const int G = 64 / L, nblk = (nq + G - 1) / G;
    const size_t lds = (size_t)(G * stride);
    // minimum resident waves per SIMD = register budget. One problem per wave keeps the uniform
    // state in SGPRs and runs best with 6 (small images) or 4 waves; packed waves hold that state
    // in VGPRs and need ~230 of them, so they run 2 waves/SIMD without spills (measured on
    // 16 384 hs071-scale QPs: L=16 W=2 159 M solves/s, W=3 142 M, W=4 116 M; L=64 W=6 74 M; with the
    // single-trip loop hints L=16 187 M, and on 65 536 QPs L=8 219 M vs L=16 194 M).
    // Packed builds with W=6 (80 VGPRs, ~180 spilled) returned wrong results and are not built.
    int waves = L == 64 ? (nVmax <= 16 ? 6 : 4) : 2;
    if (forcedW >= 2 && forcedW <= (L == 64 ? 6 : 4)) waves = forcedW;
    // ---- batches of mid-size problems (cold starts and hot starts on new vectors): the tableau kernel first (qp_small_g.h: 3 phases
    // per working-set change instead of ~50); members it cannot carry (non-symmetric H, LP, undecidable tests) come back with
    // ret == RET_BAIL and are solved by the null-space kernel launched right behind it, which skips everybody else
    // 32 row blocks x 8 column blocks of lanes: up to 72 variables x 32 constraints -- the 69 x 28 class of the hs0xx batch.
    typedef EngineG<3, 1, 9, 4> EK;      // up to 72 variables x 32 constraints
    typedef EngineG<2, 2, 8, 8> EK2;     // up to 64 variables x 64 constraints
    // (only where the null-space kernel would give a problem four waves as well: batches of SMALL problems are throughput-bound
    //  and better served by 16 / 32 lanes per problem, several problems per wave)
    // (per-member modes: the kernel itself leaves the members whose mode it does not carry to the null-space kernel)
    // (kn.no_tiny == 2, the LP launches of a batch: every member would come back with RET_BAIL -- no H, hreg != 0)
    if (forcedE < 0 && kn.no_tiny < 2 && eng == 1 && (nVmax > 32 || nCmax > 32) && (p.member_mode || mode == 0 || mode == 1) && !p.done_flag) {
#define KK_LAUNCH(RV_, RC_, CV_, CC_)                                                                                            \
        do {                                                                                                                     \
            hipLaunchKernelGGL((small_qpg_kernel<RV_, RC_, CV_, CC_>), dim3(nq), dim3(256), 0, stream, p, nq, mode, maxWSR);     \
            p.only_bailed = 1;                                                                                                   \
        } while (0)
        if (nVmax <= EK::MAXV && nCmax <= EK::MAXC) KK_LAUNCH(3, 1, 9, 4);
        else if (nVmax <= EK2::MAXV && nCmax <= EK2::MAXC) KK_LAUNCH(2, 2, 8, 8);
#undef KK_LAUNCH
    }
#define SQ_LAUNCH_U(ENG, LL, ML, W, U)                                                                        \
    do {                                                                                                      \
        static std::atomic<unsigned long long> set_{0};                                                       \
        rsqp_allow_full_lds(reinterpret_cast<const void *>(&small_qp_kernel<ENG<LL, ML>, LL, ML, W, U>), set_, (int)kMaxLds); \
        hipLaunchKernelGGL((small_qp_kernel<ENG<LL, ML>, LL, ML, W, U>), dim3(nblk), dim3(LL > 64 ? LL : 64), lds, stream, p, nq, \
                           (int)stride, mode, maxWSR);                                                        \
    } while (0)
    // compile-time shape NV x NC, target vectors in registers
#define SQ_LAUNCH_SHAPE(LL, W, NV, NC)                                                                        \
    do {                                                                                                      \
        static std::atomic<unsigned long long> set_{0};                                                       \
        rsqp_allow_full_lds(reinterpret_cast<const void *>(&small_qp_kernel<Engine<LL, true, true>, LL, true, W, NV * 256 + NC>), set_, (int)kMaxLds); \
        hipLaunchKernelGGL((small_qp_kernel<Engine<LL, true, true>, LL, true, W, NV * 256 + NC>), dim3(nblk), dim3(64), lds, stream, p, nq, \
                           (int)stride, mode, maxWSR);                                                        \
    } while (0)
#define SQ_LAUNCH_E(ENG, LL, ML, W) SQ_LAUNCH_U(ENG, LL, ML, W, 0)
#define SQ_LAUNCH(LL, ML, W) SQ_LAUNCH_E(Engine, LL, ML, W)
#define SQ_WAVES(LL)                                                                                          \
    switch (waves) {                                                                                          \
    case 3: SQ_LAUNCH(LL, true, 3); break;                                                                    \
    case 4: SQ_LAUNCH(LL, true, 4); break;                                                                    \
    default: SQ_LAUNCH(LL, true, 2); break;                                                                   \
    }
#if defined(RSQP_SMALL_EXPERIMENT) && RSQP_SMALL_EXPERIMENT == 2
    // quick-turnaround build for tuning (tools/small_experiment.sh -DRSQP_SMALL_EXPERIMENT=2): only the four-wave
    // explicit-inverse kernel (mid-size problems, BASELINE configs[4])
    {
        if (!(eng == 1 && wide)) return hipErrorInvalidValue;
        SQ_LAUNCH_E(EngineX, 256, true, 1);
        return hipGetLastError();
    }
#elif defined(RSQP_SMALL_EXPERIMENT)
    // quick-turnaround build for tuning (tools/small_experiment.sh): only the 8-lane Givens / TQ kernel
    {
        const bool fixed = shape82;
        if (L != 8 || eng != 0 || !mat_lds) return hipErrorInvalidValue;
        if (fixed) { switch (waves) { case 3: SQ_LAUNCH_SHAPE(8, 3, 8, 2); break; case 4: SQ_LAUNCH_SHAPE(8, 4, 8, 2); break; default: SQ_LAUNCH_SHAPE(8, 2, 8, 2); } }
        else { switch (waves) { case 3: SQ_LAUNCH_U(Engine, 8, true, 3, 0); break; case 4: SQ_LAUNCH_U(Engine, 8, true, 4, 0); break; default: SQ_LAUNCH_U(Engine, 8, true, 2, 0); } }
        return hipGetLastError();
    }
#else
    if (eng == 1) {
        if (!mat_lds) SQ_LAUNCH_E(EngineX, 64, false, 3);
        else if (L == 16) SQ_LAUNCH_E(EngineX, 16, true, 2);
        else if (L == 32) SQ_LAUNCH_E(EngineX, 32, true, 2);
        else if (wide) SQ_LAUNCH_E(EngineX, 256, true, 1);   // four waves per problem: the O(n^2) phases split over 256 lanes
        else SQ_LAUNCH_E(EngineX, 64, true, 4);
    } else if (!mat_lds) {
        SQ_LAUNCH(64, false, 3);
    } else if (L == 8) {
        // shape build: 160 instead of 253 VGPRs, no per-vector address registers, straight-line vector loops; the
        // occupancy of both builds is capped at 2 waves per SIMD by the LDS a wave of 8 problems needs
        if (shape82) SQ_LAUNCH_SHAPE(8, 2, 8, 2);
        else SQ_LAUNCH(8, true, 2);
    } else if (shape82) {
        return hipErrorInvalidValue;    // the image was sized for the 8-lane shape build: never launch another one on it
    } else if (L == 16) {
        SQ_WAVES(16)
    } else if (L == 32) {
        SQ_WAVES(32)
    } else {
        switch (waves) {
        case 3: SQ_LAUNCH(64, true, 3); break;
        case 6: SQ_LAUNCH(64, true, 6); break;
        default: SQ_LAUNCH(64, true, 4); break;
        }
    }
#endif
#undef SQ_LAUNCH_SHAPE
#undef SQ_LAUNCH_E
#undef SQ_LAUNCH_U
#undef SQ_WAVES
#undef SQ_LAUNCH
    return hipGetLastError();
}

long long rsqp_mat_lds_bytes(int nV, int nC, int annz, int hnnz) { return mat_lds_bytes(nV, nC, annz, hnnz); }
