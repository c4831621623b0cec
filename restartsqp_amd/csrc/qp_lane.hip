// qp_lane.hip -- hs071-scale QPs of a ONE-SHAPE batch, cold start, ONE LANE PER PROBLEM (round 5); in the WARM builds also the hot
// start with new matrices and the warm re-initialisation (lane_qp_body, rsqp_batch_set_lane_warm), at level 2 also the hot start on new
// vectors (rsqp_batch_set_lane_hot).
//
// Replaces, for large batches of one shape (one sparsity pattern -- parameter scans, perturbations of one QP: bench.py's
// headline workload, 65 536 x the hs071 QP through the QPhandler formulation -- or patterns of their own), the qpOASES 3.2.1 SQProblem::init call made
// at reference src/qpOASESInterface.cpp:155,180. Same algorithm as qp_tiny.hip -- the symmetric tableau
//      G = - SWEEP_S(K),  K = [H A'; A 0],  S = free variables + active constraints,  N = 8 + MC fixed slots
// with one product per step direction, one principal pivot per working-set change (2 x 2 block for an exchange), exact
// products with the data after an exchange / every 8 changes and at the end, the same ratio tests, tie breaks and tolerances --
// but mapped the other way round: qp_tiny.hip gives a problem 8 lanes and keeps the tableau in their registers, so every
// pivot row, product input and argmin crosses lanes (ds_bpermute / DPP) and 3 of 4 constraint rows are idle at MC = 2; a wave
// (8 problems) takes ~45 k cycles, two waves per SIMD: 16 384 problems in flight, 4 rounds for 65 536.
// Here a LANE owns a problem:
//   * the tableau (upper triangle, N (N + 1) / 2 doubles) and the dense A of the data live in LDS (H's upper triangle, only ever
//     read at compile-time positions, in registers), entry e of
//     lane i at (e * 64 + i) * 8: a wave's access to one entry is 512 consecutive bytes -- conflict-free for static AND for
//     lane-varying entries (the pivot row of each lane's own problem), no index arithmetic for static ones (immediate offsets);
//   * every vector of the solver state (x, limits, targets, multipliers, gradients: 9 per variable, 6 per constraint) is a
//     register array indexed by compile-time slots; "slot idx of my problem" is a predicated pass over the slots;
//   * nothing crosses lanes: no permutes, no barriers, no reductions -- a wave is 64 independent scalar programs in lockstep
//     (identical paths for perturbations of one QP; diverging members cost the union of their paths, as in any SIMT code).
// One wave per workgroup, LDS 36.4 KB (MC = 2; 40.4 KB in the builds that stage in dependency order, see stage_matrices): four
// waves per CU, one per SIMD with the whole register file (512 per lane) -- 65 536 problems in flight on the 256 CUs.
#include <type_traits>

#include "rsqp_small_plan.h"

#define LDS __attribute__((address_space(3)))
typedef LDS double ldouble;

// diagnostic build only (-DRSQP_STAMPS, tools/stamp_lane_kernel.py): cycles per phase of wave 0
#ifdef RSQP_STAMPS
constexpr int kLaneStamps = 24;
__device__ unsigned long long g_lane_stamps[kLaneStamps];
// (fenced on both sides: the scheduler otherwise moves a phase's instructions across the clock read that should bound it -- the
//  step's 255 instructions once lay below the stamp behind them, and were booked on the working-set change)
#define LSTAMP(k)                                                                                        \
    do {                                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        long long t_ = clock64();                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_lane_stamps[k], (unsigned long long)(t_ - tlast)); \
        tlast = t_;                                                                                      \
    } while (0)
// stamps INSIDE a phase (the parts of a working-set change): the product build has no fence there
#define LSTAMP_IN(k) LSTAMP(k)
extern "C" void rsqp_debug_lane_stamps(unsigned long long *out, int reset) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lane_stamps), sizeof(unsigned long long) * kLaneStamps);
    if (reset) {
        unsigned long long z[kLaneStamps] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lane_stamps), z, sizeof(z));
    }
}
#else
// the phase boundaries stay fences for the instruction scheduler in the product build: without them it hoists the loads and
// row fetches of a phase far up into the one before, and the 234 registers of persistent state (of the 256 the vector ALU can
// name) leave no room for that -- 0.0566 ms per launch of the headline batch without, 0.0433 ms with them (the build with the
// time stamps had been the faster one). Finer fences (per slot, inside the pivots) measured no better (0.0442 ms)
#define LSTAMP(k) __builtin_amdgcn_sched_barrier(0)
#define LSTAMP_IN(k)
#endif

// the exchange's votes of the headline build (LaneT::VOTE >> 5, see change_exchange()): 1 the sums and li, 2 / 4 the partner's kind
// 2 / 1, 8 the ranges of the slots. Shipped: the sums and li alone -- with the partner's kind, the ranges or both the headline batch
// ran 1 to 2.5 % SLOWER than with bit 0 alone, in every round (5 to 7 KB more text). A tuning build screens them
// bit by bit (tools/lane_experiment.sh -DRSQP_LANE_XVOTE=<bits>)
#ifndef RSQP_LANE_XVOTE
#define RSQP_LANE_XVOTE 1
#endif
// the stores of a full wave's results and kept state (WaveRun): bit 0 x, y and the working sets, bit 1 the state's tableau, bit 2 the
// state's tail go out write-through; a bit that is off keeps the plain store (tuning builds screen them, -DRSQP_LANE_WT=<bits>)
#ifndef RSQP_LANE_WT
#define RSQP_LANE_WT 7
#endif
// timing-only builds that price those stores (never shipped: they leave the pools unwritten): bit 0 gives a full wave's result pools
// and its five per-lane words, bit 1 its state pool a buffer descriptor of ZERO records -- the range check drops every store through
// it, the instruction stream and the waits stay. The launch's time against the product's is what the bytes cost, dirty lines included
#ifndef RSQP_LANE_NOSTORE
#define RSQP_LANE_NOSTORE 0
#endif

namespace {

constexpr int MV = 8, WL = 64;
typedef double v2d __attribute__((ext_vector_type(2)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
// ---- a full wave's run of a pool (its 64 members' consecutive elements) as the target of its stores. WT: write-through (sc1) -- the
// line leaves the L2 as the store is issued. A plain store leaves it there dirty until the launch ends; the write-back then runs
// with every CU idle and the next launch of the stream waits for it (13.6 MB behind the headline launch, 111 MB, of which the L2s
// hold 32 MiB, with the state kept; DESIGN.md 4.3b, "The results' stores"). The kernel that reads the pools next finds them in HBM,
// not in this launch's L2. Operands, order and values are those of the plain store. The descriptor is the wave's own (base = its
// run, records = the run's bytes): offsets stay small whatever the batch, and a store beyond the run is dropped, not performed
template <bool WT, bool DROP = false> struct WaveRun {
    static constexpr bool BUF = WT || DROP;
    __amdgpu_buffer_rsrc_t r;
    char *base;
    __device__ __forceinline__ WaveRun(void *b, int bytes) {
        if constexpr (BUF) {
            // (wave-uniform by construction -- kernel arguments and blockIdx --; the descriptor wants that provable)
            const unsigned long long a = (unsigned long long)b;
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
            r = __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0,
                                                  DROP ? 0 : __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
        } else base = (char *)b;
    }
    static constexpr int AUX = WT ? 16 : 0;                 // (16: sc1)
    // element k of the run, counted in 16 / 8 / 4 bytes
    template <class V> __device__ __forceinline__ void put16(int k, V v) const {
        static_assert(sizeof(V) == 16, "16 bytes per lane");
        if constexpr (BUF) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), r, k * 16, 0, AUX);
        else reinterpret_cast<V *>(base)[k] = v;
    }
    template <class V> __device__ __forceinline__ void put8(int k, V v) const {
        static_assert(sizeof(V) == 8, "8 bytes per lane");
        if constexpr (BUF) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, k * 8, 0, AUX);
        else reinterpret_cast<V *>(base)[k] = v;
    }
#if RSQP_LANE_NOSTORE
    __device__ __forceinline__ void put4(int k, int v) const { __builtin_amdgcn_raw_buffer_store_b32(v, r, k * 4, 0, AUX); }
#endif
};
// loops over slots with COMPILE-TIME indices: the register arrays of the solver state are split into scalars before any other
// transformation sees them (a run-time loop, even one that is fully unrolled later, leaves selects between member addresses
// behind, and the whole state goes to scratch memory)
template <int I, int E, class F> __device__ __forceinline__ void sfor_(F &&f) {
    if constexpr (I < E) { f(std::integral_constant<int, I>{}); sfor_<I + 1, E>(f); }
}
#define SFOR(var, n, ...) sfor_<0, (n)>([&](auto var##_c) { constexpr int var = decltype(var##_c)::value; (void)var; __VA_ARGS__ })
#define SFOR1(var, n, ...) sfor_<1, (n) + 1>([&](auto var##_c) { constexpr int var = decltype(var##_c)::value; (void)var; __VA_ARGS__ })

// a status word the compiler must not look through: the slot passes of homotopy() each start from a fresh copy, so the lane masks
// derived from it (free / at lower / at upper) are re-formed per pass (one compare) instead of kept in scalar registers across the
// whole iteration, from where they were spilled to lanes of vector registers and read back (2-3 % of the kernel)
__device__ __forceinline__ int opq(int v) { asm volatile("" : "+v"(v)); return v; }
// a product that is not contracted into the sum that takes it
__device__ __forceinline__ double mul_alone(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__host__ __device__ constexpr int tri(int j, int k) { return j <= k ? k * (k + 1) / 2 + j : j * (j + 1) / 2 + k; }

#include "qp_leaf.h"

// HB: H has entries only in its leading HB x HB block (4, or 8 = anywhere) and no regularisation is added to it -- the host's
// word for the whole batch (QPPools::lane_hblock). In the QPhandler formulation [x u v] the slacks have no curvature, so the
// headline's H (11 entries on 4 variables) takes 10 register pairs instead of 36; everything beyond the block is the +0 the full
// build holds there, and the products with it are left out: fma(+0, x, h) is h for finite x (h starts at +0), bit for bit
// ROLES: the ratio test of homotopy() BRANCHES on the role of a variable slot (free / fixed) instead of computing both roles and
// selecting, and the re-relaxation in front of the homotopy, which a cold start cannot need, is left out (kernel's choice, see
// lane_qp_kernel: the headline build only)
// SHV / SHC: the batch's shape as compile-time words (the full-shape build, 8 x 2), or -1: the run-time words P.uniV / P.uniC. With
// the constants every `l < nV` / `i < nC` of the slot passes, the candidate ids and the parity arms of the staging and results
// helpers fold: one text, the shape decides what is left of it (lane_qp_body)
template <int S> struct ShapeWord {
    __device__ __forceinline__ ShapeWord &operator=(int) { return *this; }
    __device__ __forceinline__ constexpr operator int() const { return S; }
};
template <> struct ShapeWord<-1> {
    int v;
    __device__ __forceinline__ ShapeWord &operator=(int w) { v = w; return *this; }
    __device__ __forceinline__ operator int() const { return v; }
};
// VOTE: the wave's lanes vote (ballot over the lanes still in the loop) on what happens next, and a wave that agrees runs a text
// in which that is a constant. Bit 0: the homotopy step by `done` (step); bit K, K = 1 .. 4: change() with every lane's change of
// kind K; bits 5 .. 8: the votes inside a wave's kind-3 change (change_exchange: the sums and li, the partner's kind, the slots' ranges).
// A wave that disagrees runs the text of the builds without the flag; per lane every text performs the same operations
// on the same operands in the same order (kernel's choice, see lane_qp_body: the full-shape build without kept state)
// WARM: the build for hot starts with new matrices and warm re-initialisations (lane_qp_body): the set-up from a guess (setup_warm,
// warm_pivots), the guess's way in (take_guess) and results / state stores that leave out the members a launch does not run. A
// level: 0 no, 1 those two call shapes, 2 also the hot start on new vectors (take_limits, setup_warm's `hot`)
template <int MC, int HB, int CH1 = 2, int CH2 = 2, bool ROLES = false, int SHV = -1, int SHC = -1, int VOTE = 0, int WARM = 0>
struct LaneT {
    static_assert((SHV < 0) == (SHC < 0) && SHV <= MV && SHC <= MC, "both words of the shape, or neither");
    static_assert(HB == 4 || HB == MV, "leading block of H");
    static constexpr int N = MV + MC, NT = N * (N + 1) / 2, NH = HB * (HB + 1) / 2, NA = MC * MV, REFRESH = 8;
    ldouble *G, *K;                      // my problem's tableau / the dense A of the data: entry e at [e * WL]
    double Hr[NH];                       // the upper triangle of H's block: registers (compile-time positions only; staged through LDS)
    double xv[MV], lo[MV], up[MV], loN[MV], upN[MV], yv[MV], g[MV], gN[MV], gy[MV];
    double ax[MC], loA[MC], upA[MC], cloN[MC], cupN[MC], yc[MC];
    int sv[MV], sc[MC];
    ShapeWord<SHV> nV; ShapeWord<SHC> nC;
    int fmask, amask, status, infeasible, unbounded, nflips, since_refresh;
    double hscale, hreg;
    long long tlast;                     // (-DRSQP_STAMPS builds)

    __device__ __forceinline__ double Hs(int i, int k) const { return Hr[tri(i, k)]; }                     // static i, k < HB
    __device__ __forceinline__ double As(int i, int k) const { return K[(i * MV + k) * WL]; }             // i may vary by lane
    __device__ __forceinline__ int nFR() const { return __popc(fmask); }
    __device__ __forceinline__ int nAC() const { return __popc(amask); }
    // row q of G (q varies by lane): by symmetry from the stored triangle
    __device__ __forceinline__ void fetch_row(int q, double (&u)[N]) const {
        const int tq = (q * (q + 1)) >> 1;
        SFOR(k, N, const int e = k <= q ? tq + k : k * (k + 1) / 2 + q; u[k] = G[e * WL];);
    }
    __device__ __forceinline__ void store_row(int q, const double (&w)[N]) {
        const int tq = (q * (q + 1)) >> 1;
        SFOR(k, N, const int e = k <= q ? tq + k : k * (k + 1) / 2 + q; G[e * WL] = w[k];);
    }
    __device__ __forceinline__ double Gd(int p, int q) const {
        const int a = p < q ? p : q, b = p < q ? q : p;
        return G[(((b * (b + 1)) >> 1) + a) * WL];
    }

    // ------------------------------------------------------------------ products
    // gyx = A'y_C - H x, axx = A x, hxx = H x (sums in ascending column / row order, as qp_tiny.hip forms them)
    __device__ __forceinline__ void exact_products(double (&gyx)[MV], double (&axx)[MC], double (&hxx)[MV]) const {
        double h[MV], aty[MV], a[MC];
        SFOR(k, MV, h[k] = 0.0; aty[k] = 0.0;);
        SFOR(i, MC, a[i] = 0.0;);
        SFOR(k, HB, SFOR(j, (k) + 1, const double w = Hs(j, k);
                h[j] = fma(w, xv[k], h[j]);
                if (j != k) h[k] = fma(w, xv[j], h[k]);););
        // (h[k] above: the terms j < k arrive in its own pass, the diagonal last of that pass, the terms beyond in later passes)
        // (GROUPED: A's reads go out together, ahead of the sums -- see sweep_triangle)
        double ak[NA];
        if constexpr (GROUPED) {
            SFOR(k, MV, SFOR(i, MC, ak[i * MV + k] = As(i, k);););
            __builtin_amdgcn_sched_group_barrier(0x100, NA, 0);
        }
        SFOR(k, MV, SFOR(i, MC, double w; if constexpr (GROUPED) w = ak[i * MV + k]; else w = As(i, k);
                a[i] = fma(w, xv[k], a[i]);
                aty[k] = fma(w, yc[i], aty[k]);););
                SFOR(k, MV, gyx[k] = aty[k] - h[k]; hxx[k] = h[k];);
                SFOR(i, MC, axx[i] = a[i];);
    }
    // out = G in (in = [inV; inC]), every row's sum in ascending column order
    __device__ __forceinline__ void g_times(const double (&in)[N], double (&o)[N]) const {
        SFOR(k, N, o[k] = 0.0;);
        SFOR(k, N, SFOR(j, (k) + 1, const double w = G[tri(j, k) * WL];
                o[j] = fma(w, in[k], o[j]);
                if (j != k) o[k] = fma(w, in[j], o[k]);););
    }

    // ------------------------------------------------------------------ pivots
    // G_jk <- f(j, k, G_jk) for every stored pair, CH entries at a time: a chunk's reads go out together, then its arithmetic (VPE
    // vector instructions per entry), then its stores. The entries are independent, so the order between them is free; the groups
    // pin it, because the scheduler, with the register file full of persistent state, otherwise sends every pair of entries
    // through one register quad -- read, wait, two FMAs, store, 28 times --, and a lone wave on its SIMD waits out each of those
    // LDS round trips. CH = 2 is that text, pair by pair: the builds whose registers have no room for a chunk
    // (state kept, H in full) stay on it. CH1 / CH2: the chunks of pivot1 / pivot2 (kernel's choice, see lane_qp_kernel)
    static constexpr bool GROUPED = CH1 > 2;         // this build pins its LDS reads into groups elsewhere too (g_from_K, exact_products)
    static constexpr int col_of(int e) { int k = 0; while ((k + 1) * (k + 2) / 2 <= e) k++; return k; }
    template <int CH, int VPE, class F> __device__ __forceinline__ void sweep_triangle(F &&f) {
        SFOR(c, (NT + CH - 1) / CH,
             constexpr int n = (c + 1) * CH <= NT ? CH : NT - c * CH;
             double v[CH];
             SFOR(i, n, v[i] = G[(c * CH + i) * WL];);
             SFOR(i, n, constexpr int e = c * CH + i; constexpr int k = col_of(e); constexpr int j = e - k * (k + 1) / 2;
                  v[i] = f(std::integral_constant<int, j>{}, std::integral_constant<int, k>{}, v[i]););
             SFOR(i, n, G[(c * CH + i) * WL] = v[i];);
             // (the compiler moves two neighbouring entries per LDS instruction, ds_read2st64_b64 / ds_write2st64_b64)
             if constexpr (CH > 2) {
                 __builtin_amdgcn_sched_group_barrier(0x100, (n + 1) / 2, 0);
                 __builtin_amdgcn_sched_group_barrier(0x002, VPE * n, 0);
                 __builtin_amdgcn_sched_group_barrier(0x200, (n + 1) / 2, 0);
             });
    }
    // principal pivot on slot q: G <- G0 - (1 / pi) u~ u~', G0 = G with row and column q zeroed, u~ = u except u~_q = sgn.
    // Every stored pair gets the update; row q (whose old entries do not enter) is then written from scratch.
    __device__ __forceinline__ void pivot1(const double (&u)[N], int q, double sgn, double pi) {
        const double c = -recip(pi);
        double ut[N], t[N];
        SFOR(k, N, ut[k] = k == q ? sgn : u[k]; t[k] = c * ut[k];);
        sweep_triangle<CH1, 1>([&](auto jc, auto kc, double w_) {
            constexpr int j = decltype(jc)::value; constexpr int k = decltype(kc)::value;
            return fma(t[j], ut[k], w_); });
        double w[N];
        const double tq = c * sgn;
        SFOR(k, N, w[k] = tq * ut[k];);
        store_row(q, w);
    }
    // 2 x 2 block pivot on (p, q) with W = [G_pp G_pq; G_pq G_qq]^-1: G <- G00 - U~ W U~', U~ = [u_p u_q], rows p, q = diag(sp, sq)
    __device__ __forceinline__ void pivot2(const double (&up_)[N], const double (&uq)[N], int p, double sp, int q, double sq, double w11,
                                           double w12, double w22) {
        double a[N], b[N], cp[N], cq[N];
        SFOR(k, N, const bool hp = k == p, hq = k == q;
            a[k] = hp ? sp : (hq ? 0.0 : up_[k]);
            b[k] = hq ? sq : (hp ? 0.0 : uq[k]);
            cp[k] = fma(w11, a[k], w12 * b[k]);
            cq[k] = fma(w12, a[k], w22 * b[k]););
            // (one pass; as two passes of one rank-1 term each -- 20 instead of 40 doubles of vectors live -- 0.0449 against 0.0433 ms)
        sweep_triangle<CH2, 2>([&](auto jc, auto kc, double w_) {
            constexpr int j = decltype(jc)::value; constexpr int k = decltype(kc)::value;
            return fma(-a[j], cp[k], fma(-b[j], cq[k], w_)); });
        double w[N];
        SFOR(k, N, w[k] = -sp * cp[k];);
        store_row(p, w);
        SFOR(k, N, w[k] = -sq * cq[k];);
        store_row(q, w);
    }

    // ------------------------------------------------------------------ staging: the wave's 64 problems, HBM -> LDS -> registers
    // In HBM a problem's values are consecutive (member-major pools, the layout every kernel of the library shares), so the block
    // of the wave's 64 problems is one contiguous run per array: lane j loads elements j, j + 64, ... (512 consecutive bytes per
    // instruction) and drops each one into the LDS slot of the lane that owns its problem, [entry][owner]; a lane then finds its
    // own values at compile-time offsets. (One lane gathering its own problem touches 64 cache lines per instruction to use 8
    // bytes of each: 4 waves per CU staging that way spent 21 k cycles here, a fifth of the kernel.)
    // T: the wave's LDS block from lane 0's point of view (G = T + lane); nqw: problems of this wave (64, less in the last one)
    template <int CH> __device__ __forceinline__ void load_block(const double *src, int n, int t0, int cnt, int lane, double (&w)[CH]) const {
        // elements m = (t0 + t) * 64 + lane of the block, t < CH (beyond the block: its last element, dropped by drop_block)
        SFOR(t, CH, const int m = (t0 + t) * WL + lane; w[t] = src[m < cnt ? m : cnt - 1];);
    }
    template <int CH> __device__ __forceinline__ void drop_block(ldouble *T, int s0, int n, int t0, int cnt, int lane, const double (&w)[CH]) const {
        const float rn = 1.0f / (float)n;
        SFOR(t, CH, if (t0 + t < n) {
                 const int m = (t0 + t) * WL + lane;
                 const int qq = (int)(((float)m + 0.5f) * rn), e = m - qq * n;      // (m < 64 * 64: the quotient is exact)
                 if (m < cnt) T[(s0 + e) * WL + qq] = w[t];
             });
    }
    // ---- the same for a FULL wave (nqw == 64) whose pools are 16-byte aligned: the run of an array is exactly 64 n elements and
    // starts on a multiple of 512 n bytes, so lane j moves 16 bytes per instruction (two doubles / four ints: group c * 64 + p(j) of the
    // run) with no clamp and no bounds test per element -- a run of odd n ends in a half group of lanes, nothing is read or written
    // beyond it. Owner and entry of a lane's first element come from one quotient per array SIZE and advance from group to group by
    // add and carry (Walk). p(j) = 4 (j & 15) + (j >> 4): a 16-byte access of 64 lanes is one kilobyte whatever the order of the lanes
    // inside it, and the LDS serves an 8-byte store (or one half of a two-address access) in groups of 16 consecutive lanes, 32 banks
    // of 4 bytes: the bank of slot (e, owner) is 2 owner mod 32, so the 16 lanes of a group must hold 16 different owners mod 16.
    // In natural order 16 lanes hold 32 / n owners (4 at n = 8: 4-way conflicts); with p(j) lane j of a group holds element 8 (j & 15)
    // of the chunk, owner 8 (j & 15) / n -- distinct up to n = 8, two by two beyond (A, H, y: 2-way, which an 8-byte store hides
    // behind its data transfer). Measured on the headline batch: 1 780 conflict cycles per wave with the 8-byte path, 1 036 with
    // 16 bytes in natural order, 232 with p(j).
    static constexpr bool PERM = true;
    static __device__ __forceinline__ int pair_of(int lane) { return PERM ? ((lane & 15) << 2) | (lane >> 4) : lane; }
    struct Walk { int qq, e, dq, dr; };
    // element U * p of a run with n per problem; (dq, dr) = the step of U * 64 elements to the lane's next group
    template <int U> static __device__ __forceinline__ Walk walk(int n, int p) {
        const float rn = 1.0f / (float)n;
        Walk w;
        const int m = U * p;
        w.qq = (int)(((float)m + 0.5f) * rn); w.e = m - w.qq * n;                              // (m < 64 * 64: the quotients are exact)
        w.dq = (int)(((float)(U * WL) + 0.5f) * rn); w.dr = U * WL - w.dq * n;
        return w;
    }
    static __device__ __forceinline__ void next_group(Walk &w, int n) {
        w.qq += w.dq; w.e += w.dr;
        const bool carry = w.e >= n;
        w.e = carry ? w.e - n : w.e; w.qq = carry ? w.qq + 1 : w.qq;
    }
    // EVEN: n is even (wave-uniform, chosen by the caller) -- every group of lanes is full and a pair never straddles two owners
    template <int CH, bool EVEN> __device__ __forceinline__ void load_pairs(const double *src, int n, int p, double (&w)[CH]) const {
        static_assert((CH & 1) == 0, "pairs");
        const double2 *s2 = reinterpret_cast<const double2 *>(src) + p;
        SFOR(c, CH / 2, if (2 * c < n) {
                 if (EVEN || c * WL + p < 32 * n) { const double2 v = s2[c * WL]; w[2 * c] = v.x; w[2 * c + 1] = v.y; }
             });
    }
    // the same with EVERY group's load issued, whatever n: a lane beyond the run (odd n), or a group beyond it, reads the run's
    // first pair again, which drop_pairs never looks at. The number of loads in flight behind an array is then a compile-time
    // constant, and the wait for that array leaves the later ones outstanding (stage_matrices)
    template <int CH> __device__ __forceinline__ void load_pairs_all(const double *src, int n, int p, double (&w)[CH]) const {
        static_assert((CH & 1) == 0, "pairs");
        const double2 *s2 = reinterpret_cast<const double2 *>(src);
        SFOR(c, CH / 2, const int m = c * WL + p; const double2 v = s2[m < 32 * n ? m : 0]; w[2 * c] = v.x; w[2 * c + 1] = v.y;);
    }
    // pairs into slots s0 + entry of their owners
    template <int CH, bool EVEN> __device__ __forceinline__ void drop_pairs(ldouble *T, int s0, int n, int p, Walk wk, const double (&w)[CH]) const {
        SFOR(c, CH / 2, if (2 * c < n) {
                 if (EVEN || c * WL + p < 32 * n) {
                     ldouble *a = T + (s0 + wk.e) * WL + wk.qq;
                     a[0] = w[2 * c];
                     if constexpr (EVEN) a[WL] = w[2 * c + 1];
                     else (wk.e + 1 == n ? T + s0 * WL + wk.qq + 1 : a + WL)[0] = w[2 * c + 1];
                 }
                 next_group(wk, n);
             });
    }
    // pairs of a matrix: entry e goes to slot tab[e] (a full wave's table names a spare slot for the entries to skip)
    template <int CH, bool EVEN> __device__ __forceinline__ void drop_pair_entries(ldouble *T, const __attribute__((address_space(3))) int *tab, int n,
                                                                                   int p, Walk wk, const double (&w)[CH]) const {
        SFOR(c, CH / 2, if (2 * c < n) {
                 if (EVEN || c * WL + p < 32 * n) {
                     const bool over = !EVEN && wk.e + 1 == n;
                     const int e1 = over ? 0 : wk.e + 1, q1 = over ? wk.qq + 1 : wk.qq;
                     const int d0 = tab[wk.e], d1 = tab[e1];
                     T[d0 * WL + wk.qq] = w[2 * c];
                     T[d1 * WL + q1] = w[2 * c + 1];
                 }
                 next_group(wk, n);
             });
    }
    // the reverse for results: x / y as pairs in the order p(j); the working sets (the low halves of their slots) four ints at a time
    // in natural lane order (a 4-byte read is served in groups of 32 lanes, and four consecutive ints mostly share an owner)
    template <int CH, bool EVEN, bool WT> __device__ __forceinline__ void put_pairs(double *dst, int n, int p, const ldouble *T, int s0) const {
        static_assert((CH & 1) == 0, "pairs");
        Walk wk = walk<2>(n, p);
        const WaveRun<WT, (RSQP_LANE_NOSTORE & 1) != 0> d2(dst, n * WL * 8);
        SFOR(c, CH / 2, if (2 * c < n) {
                 if (EVEN || c * WL + p < 32 * n) {
                     const ldouble *a = T + (s0 + wk.e) * WL + wk.qq;
                     v2d v;
                     v.x = a[0];
                     if constexpr (EVEN) v.y = a[WL];
                     else v.y = (wk.e + 1 == n ? T + s0 * WL + wk.qq + 1 : a + WL)[0];
                     d2.put16(c * WL + p, v);
                 }
                 next_group(wk, n);
             });
    }
    template <int CH, bool WT> __device__ __forceinline__ void put_quads(int *dst, int n, int lane, const ldouble *T, int s0) const {
        typedef const __attribute__((address_space(3))) int clint;
        Walk wk = walk<4>(n, lane);
        const WaveRun<WT, (RSQP_LANE_NOSTORE & 1) != 0> d4(dst, n * WL * 4);
        SFOR(c, (CH + 3) / 4, if (4 * c < n) {
                 if (c * WL + lane < 16 * n) {
                     int v[4], qq = wk.qq, e = wk.e;
                     SFOR(u, 4, v[u] = ((clint *)(T + (s0 + e) * WL + qq))[0];
                          const bool wrap = e + 1 == n; e = wrap ? 0 : e + 1; qq = wrap ? qq + 1 : qq;);
                     v4i w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
                     d4.put16(c * WL + lane, w);
                 }
                 next_group(wk, n);
             });
    }
#define BYPARITY(n, ...) do { if ((n) & 1) { constexpr bool EV = false; __VA_ARGS__ } else { constexpr bool EV = true; __VA_ARGS__ } } while (0)
    // ---- the state blocks of the wave's problems (QPPools::keep_state: what the next hot start continues from), LDS -> HBM. A
    // problem's block is N N + 96 doubles + 20 ints, consecutive, blocks `stride` doubles apart (the layout of qp_tiny.hip, see
    // LANE_TINY_MAGIC). A lane storing its own block piece by piece touches 64 lines per instruction for 8 bytes of each -- 0.17 ms
    // instead of 0.04 for the headline launch with its state kept; instead lane j handles pairs j, j + 64, ... of the wave's run
    // of blocks (two doubles of one problem per instruction, consecutive lanes consecutive pairs): 0.075 ms.
    // The tableau part: both triangles in HBM (what the 8-lane kernel holds), from the upper one in the LDS slots
    // (live, WARM: bit qq = problem qq of the wave is in the launch; the others' blocks stay as they are)
    // (FULL: a full wave with every member in the launch -- no store of its is masked, and they go write-through by the run of the
    //  pool, WaveRun)
    template <bool FULL> __device__ __forceinline__ void state_put_tableau(double *sbase, long long stride, int nqw, int lane, const ldouble *T,
                                                                           unsigned long long live = ~0ull) const {
        static_assert((N & 1) == 0, "pairs of a row");
        constexpr int PAIRS = N * N / 2;
        const WaveRun<FULL && (RSQP_LANE_WT & 2), FULL && (RSQP_LANE_NOSTORE & 2)> run(sbase, (int)stride * WL * 8);
        // (a run-time loop: nothing here indexes a register array, and 50 unrolled trips were hoisted in front of each other until
        //  1 493 registers spilled)
#pragma unroll 5
        for (int t = 0; t < PAIRS; t++) {
            const int m = t * WL + lane;
            const int qq = m / PAIRS, e = (m - qq * PAIRS) * 2, r = e / N, k = e - r * N;            // entries (r, k), (r, k + 1)
            const int hi0 = r > k ? r : k, lo0 = r > k ? k : r, hi1 = r > k + 1 ? r : k + 1, lo1 = r > k + 1 ? k + 1 : r;
            v2d v;
            v.x = T[(((hi0 * (hi0 + 1)) >> 1) + lo0) * WL + qq]; v.y = T[(((hi1 * (hi1 + 1)) >> 1) + lo1) * WL + qq];
            if constexpr (FULL) run.put16((qq * (int)stride + e) >> 1, v);
            else {
                bool mine = qq < nqw;
                if constexpr (WARM != 0) mine = mine && ((live >> (qq & 63)) & 1) != 0;
                if (mine) *reinterpret_cast<v2d *>(sbase + (long long)qq * stride + e) = v;
            }
        }
    }
    // the slot state + status words behind it: TAILD doubles (the ints as pairs), staged in LDS slots 0 .. in two halves
    static constexpr int TAILD = 96 + 10, THALF = TAILD / 2;
    static_assert(THALF <= NT, "the halves of the slot state pass through the tableau's slots");
    template <bool FULL> __device__ __forceinline__ void state_put_tail_half(double *sbase, long long stride, int nqw, int lane, const ldouble *T, int half,
                                                                             unsigned long long live = ~0ull) const {
        const WaveRun<FULL && (RSQP_LANE_WT & 4), FULL && (RSQP_LANE_NOSTORE & 2)> run(sbase, (int)stride * WL * 8);
#pragma unroll 4
        for (int t = 0; t < THALF; t++) {
            const int m = t * WL + lane;
            const int qq = m / THALF, f = m - qq * THALF;
            if constexpr (FULL) run.put8(qq * (int)stride + N * N + half * THALF + f, (double)T[f * WL + qq]);
            else {
                bool mine = qq < nqw;
                if constexpr (WARM != 0) mine = mine && ((live >> (qq & 63)) & 1) != 0;
                if (mine) sbase[(long long)qq * stride + N * N + half * THALF + f] = T[f * WL + qq];
            }
        }
    }
    // my slot state as the TAILD doubles behind the tableau: f < 48 field f / 8 (x g lo up gy y) of variable slot f % 8; f < 80 field
    // (f - 48) / 8 (A x, loA, upA, y) of constraint slot (f - 48) % 8 (slots beyond MC: zero); f < 96 the tableau's diagonal (G_ll of the
    // 8 variable slots, then G_{8+l,8+l}: the 8-lane kernel tracks them apart); then the status words two by two: sv (8), sc (8), status, masks, magic, pivots since G was built from the data
    template <int W> __device__ __forceinline__ int state_word(int pivots) const {
        if constexpr (W < 8) return sv[W];
        else if constexpr (W < 16) { if constexpr (W - 8 < MC) return sc[W - 8]; else return 0; }
        else if constexpr (W == 16) return status;
        else if constexpr (W == 17) return (fmask & 0xff) | ((amask & 0xff) << 8);
        else if constexpr (W == 18) return 0x7a11e;
        else return pivots;
    }
    template <int F> __device__ __forceinline__ double tail_value(const double (&dg)[N], int pivots) const {
        if constexpr (F < 48) {
            constexpr int c = F / 8, l = F % 8;
            if constexpr (c == 0) return xv[l]; else if constexpr (c == 1) return g[l]; else if constexpr (c == 2) return lo[l];
            else if constexpr (c == 3) return up[l]; else if constexpr (c == 4) return gy[l]; else return yv[l];
        } else if constexpr (F < 80) {
            constexpr int c = (F - 48) / 8, l = (F - 48) % 8;
            if constexpr (l >= MC) return 0.0;
            else if constexpr (c == 0) return ax[l]; else if constexpr (c == 1) return loA[l]; else if constexpr (c == 2) return upA[l]; else return yc[l];
        } else if constexpr (F < 96) {
            constexpr int c = (F - 80) / 8, l = (F - 80) % 8;
            if constexpr (c == 0) return dg[l]; else if constexpr (l < MC) return dg[MV + l]; else return 0.0;
        } else {
            constexpr int w = (F - 96) * 2;
            return __hiloint2double(state_word<w + 1>(pivots), state_word<w>(pivots));
        }
    }
    template <int HALF> __device__ __forceinline__ void tail_put_half(ldouble *Gm, const double (&dg)[N], int pivots) const {
        SFOR(fl, THALF, Gm[fl * WL] = tail_value<HALF * THALF + fl>(dg, pivots););
    }
    // the reverse for results: every lane has put its n values into slots s0 .. s0 + n - 1 of its own column; lane j stores
    // elements j, j + 64, ... of the wave's contiguous block (64-bit values, or 32-bit ones kept in the low halves of the slots)
    template <int CH, class TV> __device__ __forceinline__ void put_block(TV *dst, int n, int cnt, int lane, const ldouble *T, int s0,
                                                                          unsigned long long live = ~0ull) const {
        const float rn = 1.0f / (float)n;
        SFOR(t, CH, if (t < n) {
                 const int m = t * WL + lane;
                 const int qq = (int)(((float)m + 0.5f) * rn), e = m - qq * n;
                 bool mine = m < cnt;
                 if constexpr (WARM != 0) mine = mine && ((live >> (qq & 63)) & 1) != 0;
                 if (mine) {
                     if constexpr (sizeof(TV) == 8) dst[m] = T[(s0 + e) * WL + qq];
                     else dst[m] = ((const __attribute__((address_space(3))) int *)(T + (s0 + e) * WL + qq))[0];
                 }
             });
    }
    __device__ __forceinline__ void wave_sync() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // drop_block for a matrix: entry e of a problem goes to the slot the wave's table names for it (tab[e]: a slot, or -1 = skip)
    template <int CH> __device__ __forceinline__ void drop_entries(ldouble *T, const __attribute__((address_space(3))) int *tab, int n, int cnt,
                                                                   int lane, const double (&w)[CH]) const {
        const float rn = 1.0f / (float)n;
        SFOR(t, CH, if (t < n) {
                 const int m = t * WL + lane;
                 const int qq = (int)(((float)m + 0.5f) * rn), e = m - qq * n;
                 const int d = tab[e < CH ? e : 0];
                 if (m < cnt && d >= 0) T[d * WL + qq] = w[t];
             });
    }
    // the entries of MY problem's A (into the dense copy) or H (upper triangle into slots 0 ..) from its own CSC arrays: column
    // pointers first, then the entries four at a time (index and value loads of a round in flight together), a column by counting
    // the pointers an entry has passed. Lanes differ in their counts: the loop runs to the longest of the wave
    template <bool ISH> __device__ __forceinline__ void own_entries(const int *jc, const int *ir_pool, const double *val_pool, int off) {
        int cp[MV + 1];
        SFOR(j, (MV) + 1, cp[j] = jc[j <= nV ? j : nV];);
        const int cnt = cp[MV] - cp[0];                       // (cp[j] = cp[nV] beyond nV)
        const int *ir = ir_pool + off; const double *val = val_pool + off;
        for (int e0 = 0; e0 < cnt; e0 += 4) {
            int r[4]; double w[4];
            SFOR(t, 4, const int e = e0 + t < cnt ? e0 + t : cnt - 1; r[t] = ir[e]; w[t] = val[e];);
            SFOR(t, 4, if (e0 + t < cnt) {
                     const int e = cp[0] + e0 + t;
                     int c = 0;
                     SFOR1(j, MV, c += (j <= nV && e >= cp[j]) ? 1 : 0;);
                     if constexpr (ISH) { if (r[t] <= c) G[(((c * (c + 1)) >> 1) + r[t]) * WL] = w[t]; }
                     else K[(r[t] * MV + c) * WL] = w[t];
                 });
        }
    }
    // UNI: the batch has ONE sparsity pattern (QPPools::uni_pat). Otherwise -- one SHAPE, patterns of their own -- the vectors still
    // come through the wave's block, but every lane walks the CSC arrays of its own problem (own_entries)
    template <bool UNI> __device__ __forceinline__ void stage(const QPPools &P, long long q0, int lane, int nqw, ldouble *T) {
        typedef __attribute__((address_space(3))) int lint;
        const int annz = UNI ? P.uni_annz : 0, hnnz = (UNI && P.uni_haveH) ? P.uni_hnnz : 0;       // (entries that travel through the block)
        constexpr int SV = 0, SC = 3 * MV, HC = 16;          // slots of the vectors' pass; H passes through the table when it has <= 16 entries
        static_assert(3 * MV + 2 * MC <= NT && NA <= HC, "staging slots");
        const int cV = nqw * nV, cC = nqw * nC, cA = nqw * annz, cH = nqw * hnnz;
        const bool hfast = hnnz > 0 && hnnz <= HC;
        // a full wave of 16-byte aligned pools moves 16 bytes per lane (load_pairs); with H as its block, the block's entries land in
        // spare slots behind the vectors in the SAME pass (SH ..), and the entries to skip in slot SPARE
        constexpr int SH = 3 * MV + 2 * MC, SPARE = NT - 1;
        static_assert(SH + 10 <= SPARE && MV * (MV + 1) / 2 <= SPARE, "spare slots of the full wave's pass");
        const bool full = nqw == WL && annz <= NA &&
                          (((size_t)P.g | (size_t)P.lb | (size_t)P.ub | (size_t)P.lbA | (size_t)P.ubA | (size_t)P.Aval | (size_t)P.Hval) & 15) == 0;
        const bool onepass = HB < MV && full;
        const int pp = pair_of(lane);
        // lanes beyond the batch (last wave) take the LAST problem's values: they run the same path beside it, store nothing, and
        // stay for the joint work of the wave (staging here, the stores of the results at the end)
        const ldouble *S = T + (lane < nqw ? lane : nqw - 1);
        lint *tab = (lint *)(T + (NT + NA) * WL);            // 2 x 16 destination slots (A, H), behind the tableau and A
        // ---- every load before anything waits: vectors, the entries of A, up to 16 entries of H, and the batch's one pattern
        // (member 0's arrays): lane e < 16 takes entry e of A, lane 16 + e entry e of H -- its row index, its column by counting
        // the column pointers it has passed (wave-uniform scalars)
        double wg[MV], wl[MV], wu[MV], wla[MC], wua[MC], wa[NA], wh[HC];
        if (full) {
            BYPARITY(nV, load_pairs<MV, EV>(P.g + q0 * nV, nV, pp, wg); load_pairs<MV, EV>(P.lb + q0 * nV, nV, pp, wl);
                     load_pairs<MV, EV>(P.ub + q0 * nV, nV, pp, wu););
            if (nC > 0) BYPARITY(nC, load_pairs<MC, EV>(P.lbA + q0 * nC, nC, pp, wla); load_pairs<MC, EV>(P.ubA + q0 * nC, nC, pp, wua););
            if (annz > 0) BYPARITY(annz, load_pairs<NA, EV>(P.Aval + q0 * annz, annz, pp, wa););
            if (hfast) BYPARITY(hnnz, load_pairs<HC, EV>(P.Hval + q0 * hnnz, hnnz, pp, wh););
        } else {
        load_block<MV>(P.g + q0 * nV, nV, 0, cV, lane, wg);
        load_block<MV>(P.lb + q0 * nV, nV, 0, cV, lane, wl);
        load_block<MV>(P.ub + q0 * nV, nV, 0, cV, lane, wu);
        if (nC > 0) { load_block<MC>(P.lbA + q0 * nC, nC, 0, cC, lane, wla); load_block<MC>(P.ubA + q0 * nC, nC, 0, cC, lane, wua); }
        if (annz > 0) load_block<NA>(P.Aval + q0 * annz, annz, 0, cA, lane, wa);
        if (hfast) load_block<HC>(P.Hval + q0 * hnnz, hnnz, 0, cH, lane, wh);
        }
        if constexpr (UNI) {
        const bool forH = lane >= HC;
        const int pe = forH ? lane - HC : lane, pn = forH ? (hfast ? hnnz : 0) : annz;
        int prow = 0;
        if (pe < pn) prow = forH ? P.Hir[pe] : P.Air[pe];
        int pcol = 0;
        SFOR1(j, MV, const int ja = P.Ajc[j <= nV ? j : nV], jh = hfast ? P.Hjc[j <= nV ? j : nV] : 0;
              const int jj = forH ? jh : ja; pcol += (j <= nV && pe >= jj) ? 1 : 0;);
        LSTAMP(10);
        // (an entry of H outside the block cannot come: the host checked the pattern; it would be skipped, not written out of place)
        const bool hin = prow <= pcol && (HB == MV || pcol < HB);
        const int hs0 = onepass ? SH : 0, skip = full ? SPARE : -1;
        if (lane < 2 * HC) tab[lane] = pe < pn ? (forH ? (hin ? hs0 + ((pcol * (pcol + 1)) >> 1) + prow : skip) : NT + prow * MV + pcol) : skip;
        }
        SFOR(e, NA, K[e * WL] = 0.0;);
        if constexpr (HB < MV) {
            if (full) { SFOR(e, NH, G[(SH + e) * WL] = 0.0;); }
        }
        wave_sync();
        if (full) {
            BYPARITY(nV, const Walk wk = walk<2>(nV, pp);
                     drop_pairs<MV, EV>(T, SV, nV, pp, wk, wg); drop_pairs<MV, EV>(T, SV + MV, nV, pp, wk, wl);
                     drop_pairs<MV, EV>(T, SV + 2 * MV, nV, pp, wk, wu););
            if (nC > 0) BYPARITY(nC, const Walk wk = walk<2>(nC, pp);
                                 drop_pairs<MC, EV>(T, SC, nC, pp, wk, wla); drop_pairs<MC, EV>(T, SC + MC, nC, pp, wk, wua););
            if (annz > 0) BYPARITY(annz, drop_pair_entries<NA, EV>(T, tab, annz, pp, walk<2>(annz, pp), wa););
            if constexpr (HB < MV) {
                if (hfast) BYPARITY(hnnz, drop_pair_entries<HC, EV>(T, tab + HC, hnnz, pp, walk<2>(hnnz, pp), wh););
            }
        } else {
        drop_block<MV>(T, SV, nV, 0, cV, lane, wg);
        drop_block<MV>(T, SV + MV, nV, 0, cV, lane, wl);
        drop_block<MV>(T, SV + 2 * MV, nV, 0, cV, lane, wu);
        if (nC > 0) { drop_block<MC>(T, SC, nC, 0, cC, lane, wla); drop_block<MC>(T, SC + MC, nC, 0, cC, lane, wua); }
        if (annz > 0) drop_entries<NA>(T, tab, annz, cA, lane, wa);          // (straight to their places in the dense copy)
        }
        wave_sync();
        LSTAMP(11);
        // ---- my vectors (slots beyond the sizes: neutral values)
        double lb_[MV], ub_[MV], la_[MC], ua_[MC];
        SFOR(l, MV, const bool v = l < nV;
             const double a0 = S[(SV + l) * WL], a1 = S[(SV + MV + l) * WL], a2 = S[(SV + 2 * MV + l) * WL];
             gN[l] = v ? a0 : 0.0; lb_[l] = v ? a1 : 0.0; ub_[l] = v ? a2 : 0.0;);
        SFOR(i, MC, const bool c = i < nC;
             const double a0 = S[(SC + i) * WL], a1 = S[(SC + MC + i) * WL];
             la_[i] = c ? a0 : -RSQP_INFTY; ua_[i] = c ? a1 : RSQP_INFTY;);
        if (UNI && lane >= nqw) {        // (a lane beyond the batch: its own column of A is the last problem's as well)
            SFOR(e, NA, K[e * WL] = S[(NT + e) * WL];);
        }
        const long long qown = q0 + (lane < nqw ? lane : nqw - 1);
        if constexpr (!UNI) own_entries<false>(P.Ajc + qown * (nV + 1), P.Air, P.Aval, P.desc[qown].offAnz);
        wave_sync();           // (every lane has read its slots: the space is the tableau's / H's from here on)
        LSTAMP(12);
        // ---- H: the upper triangle of its block is collected in slots 0 .. NH - 1 (H arrives with both triangles: the table skips the lower one).
        // Up to 16 entries per problem (the headline's H has 11) come through the table like A; a fuller H is gathered by its owner
        // (a round of 16 load instructions covers ALL entries of 1024 / hnnz problems, not 16 entries of each)
        if (!onepass) {
        SFOR(e, NH, G[e * WL] = 0.0;);
        wave_sync();
        }
        if (onepass) {
            // (the block came with the vectors: it waits in slots SH .., which nobody writes before the tableau is built)
        } else if (hfast) {
            if (full) BYPARITY(hnnz, drop_pair_entries<HC, EV>(T, tab + HC, hnnz, pp, walk<2>(hnnz, pp), wh););
            else drop_entries<HC>(T, tab + HC, hnnz, cH, lane, wh);
            wave_sync();
            if (lane >= nqw) {
                SFOR(e, NH, G[e * WL] = S[e * WL];);
            }
        } else if constexpr (HB < MV) {
            // (a block of 4 x 4 has at most 16 entries: they came through the table, or there are none)
        } else if (!UNI) {
            if (P.uni_haveH) own_entries<true>(P.Hjc + qown * (nV + 1), P.Hir, P.Hval, P.desc[qown].offHnz);
        } else if (hnnz > HC) {
            int hjc[MV + 1];
            SFOR(j, (MV) + 1, hjc[j] = P.Hjc[j <= nV ? j : nV]; if (j > nV) hjc[j] = 0x7fffffff;);
            const double *gH = P.Hval + (q0 + (lane < nqw ? lane : nqw - 1)) * hnnz;
            for (int e0 = 0; e0 < hnnz; e0 += 8) {
                double w[8];
                SFOR(t, 8, w[t] = gH[e0 + t < hnnz ? e0 + t : hnnz - 1];);
                SFOR(t, 8, if (e0 + t < hnnz) {
                         const int e = e0 + t, r = P.Hir[e];
                         int c = 0;
                         SFOR1(j, MV, c += e >= hjc[j] ? 1 : 0;);
                         if (r <= c) G[(((c * (c + 1)) >> 1) + r) * WL] = w[t];
                     });
            }
        }
        // (H + hreg I: the LP regularisation; hscale = the largest diagonal entry -- beyond the block the diagonal is 0 and moves nothing)
        hscale = 0.0;
        const ldouble *GH = G + (onepass ? SH * WL : 0);
        SFOR(k, HB, SFOR(j, k + 1, double w = GH[tri(j, k) * WL];
                         if (j == k) { w = (k < nV) ? w + hreg : w; hscale = fmax(hscale, k < nV ? fabs(w) : 0.0); }
                         Hr[tri(j, k)] = w;););
        LSTAMP(13);
        SFOR(l, MV, const bool v = l < nV;
             loN[l] = v ? clampinf(lb_[l]) : 0.0; upN[l] = v ? clampinf(ub_[l]) : 0.0;);
        SFOR(i, MC, const bool c = i < nC;
             cloN[i] = c ? clampinf(la_[i]) : -RSQP_INFTY; cupN[i] = c ? clampinf(ua_[i]) : RSQP_INFTY;);
    }
    // ---- the same staging in DEPENDENCY ORDER, for the waves stage() serves in one pass (H as its block, a full wave, aligned
    // pools: ordered_wave). The wave's 26 KB arrive at 8 bytes per cycle and CU, every wave of the chip asking at once, and
    // stage() waits for the last byte before anything is computed. The tableau of the empty working set, Hr and hscale need
    // A and H only; the set-up needs the bounds; g is first read in the homotopy. The counter of outstanding loads retires
    // them in issue order, so the loads go out as (pattern rows,) A, H, lb, ub, lbA, ubA, g -- all of them before anything
    // waits, as in stage() -- and are consumed in that order: the tableau is built while the vectors are still on their way.
    // The vectors can then no longer transpose through the tableau's slots: they pass, one array (the two of the constraints
    // together) at a time, through SPV spare slots behind A (drop, wave_sync, read, wave_sync); the pattern table, which
    // lies there, is dead once A and H are dropped. The LDS reads and writes of my own column need no barrier between them.
    static constexpr int SPV = MV;                       // spare slots of the ordered build, behind the tableau and A
    struct Inflight { double wg[MV], wl[MV], wu[MV], wla[MC], wua[MC]; int pp; };
    __device__ __forceinline__ bool ordered_wave(const QPPools &P, int nqw) const {         // (stage()'s `onepass`)
        return HB < MV && nqw == WL && P.uni_annz <= NA &&
               (((size_t)P.g | (size_t)P.lb | (size_t)P.ub | (size_t)P.lbA | (size_t)P.ubA | (size_t)P.Aval | (size_t)P.Hval) & 15) == 0;
    }
    // loads issued; A and H taken; Hr, hscale; G = -K
    __device__ __forceinline__ void stage_matrices(const QPPools &P, long long q0, int lane, ldouble *T, Inflight &F) {
        typedef __attribute__((address_space(3))) int lint;
        static_assert(HB < MV, "the block build");
        constexpr int HC = 16, SH = 3 * MV + 2 * MC, SPARE = NT - 1;
        const int annz = P.uni_annz, hnnz = P.uni_haveH ? P.uni_hnnz : 0;
        const bool hfast = hnnz > 0 && hnnz <= HC;
        const int pp = pair_of(lane);
        F.pp = pp;
        lint *tab = (lint *)(T + (NT + NA) * WL);
        // the pattern's row of my table entry FIRST (lane e < 16 entry e of A, lane 16 + e entry e of H, as in stage()): it is
        // the first thing needed, and behind the data it would be the last thing to arrive
        const bool forH = lane >= HC;
        const int pe = forH ? lane - HC : lane, pn = forH ? (hfast ? hnnz : 0) : annz;
        int prow = 0;
        if (pe < pn) prow = forH ? P.Hir[pe] : P.Air[pe];
        int ja[MV], jh[MV];
        SFOR(j, MV, ja[j] = P.Ajc[j + 1 <= nV ? j + 1 : nV]; jh[j] = hfast ? P.Hjc[j + 1 <= nV ? j + 1 : nV] : 0;);
        __builtin_amdgcn_sched_barrier(0);
        double wa[NA], wh[HC];
        if (annz > 0) load_pairs_all<NA>(P.Aval + q0 * annz, annz, pp, wa);
        if (hfast) load_pairs_all<HC>(P.Hval + q0 * hnnz, hnnz, pp, wh);
        load_pairs_all<MV>(P.lb + q0 * nV, nV, pp, F.wl);
        load_pairs_all<MV>(P.ub + q0 * nV, nV, pp, F.wu);
        if (nC > 0) { load_pairs_all<MC>(P.lbA + q0 * nC, nC, pp, F.wla); load_pairs_all<MC>(P.ubA + q0 * nC, nC, pp, F.wua); }
        load_pairs_all<MV>(P.g + q0 * nV, nV, pp, F.wg);
        __builtin_amdgcn_sched_barrier(0);
        int pcol = 0;
        SFOR1(j, MV, const int jj = forH ? jh[j - 1] : ja[j - 1]; pcol += (j <= nV && pe >= jj) ? 1 : 0;);
        LSTAMP(10);
        const bool hin = prow <= pcol && pcol < HB;
        if (lane < 2 * HC) tab[lane] = pe < pn ? (forH ? (hin ? SH + ((pcol * (pcol + 1)) >> 1) + prow : SPARE) : NT + prow * MV + pcol) : SPARE;
        SFOR(e, NA, K[e * WL] = 0.0;);
        SFOR(e, NH, G[(SH + e) * WL] = 0.0;);
        wave_sync();
        if (annz > 0) BYPARITY(annz, drop_pair_entries<NA, EV>(T, tab, annz, pp, walk<2>(annz, pp), wa););
        if (hfast) BYPARITY(hnnz, drop_pair_entries<HC, EV>(T, tab + HC, hnnz, pp, walk<2>(hnnz, pp), wh););
        wave_sync();
        LSTAMP(11);
        hscale = 0.0;
        const ldouble *GH = G + SH * WL;
        SFOR(k, HB, SFOR(j, k + 1, double w = GH[tri(j, k) * WL];
                         if (j == k) { w = (k < nV) ? w + hreg : w; hscale = fmax(hscale, k < nV ? fabs(w) : 0.0); }
                         Hr[tri(j, k)] = w;););
        g_from_K();
        LSTAMP(17);
    }
    // one array's pairs into spare slots s0 .. of their owners
    template <int CH> __device__ __forceinline__ void take_pass(ldouble *T, int n, int pp, const double (&w)[CH], int s0) {
        BYPARITY(n, drop_pairs<CH, EV>(T, NT + NA + s0, n, pp, walk<2>(n, pp), w););
    }
    __device__ __forceinline__ void take_bounds(ldouble *T, int lane, const Inflight &F) {
        const ldouble *S = T + lane + (NT + NA) * WL;
        double lb_[MV], ub_[MV], la_[MC], ua_[MC];
        take_pass<MV>(T, nV, F.pp, F.wl, 0);
        wave_sync();
        SFOR(l, MV, const double a1 = S[l * WL]; lb_[l] = l < nV ? a1 : 0.0;);
        wave_sync();
        take_pass<MV>(T, nV, F.pp, F.wu, 0);
        wave_sync();
        SFOR(l, MV, const double a2 = S[l * WL]; ub_[l] = l < nV ? a2 : 0.0;);
        wave_sync();
        if (nC > 0) { take_pass<MC>(T, nC, F.pp, F.wla, 0); take_pass<MC>(T, nC, F.pp, F.wua, MC); }
        wave_sync();
        SFOR(i, MC, const bool c = i < nC;
             const double a0 = S[i * WL], a1 = S[(MC + i) * WL];
             la_[i] = c ? a0 : -RSQP_INFTY; ua_[i] = c ? a1 : RSQP_INFTY;);
        wave_sync();
        SFOR(l, MV, const bool v = l < nV;
             loN[l] = v ? clampinf(lb_[l]) : 0.0; upN[l] = v ? clampinf(ub_[l]) : 0.0;);
        SFOR(i, MC, const bool c = i < nC;
             cloN[i] = c ? clampinf(la_[i]) : -RSQP_INFTY; cupN[i] = c ? clampinf(ua_[i]) : RSQP_INFTY;);
        LSTAMP(12);
    }
    __device__ __forceinline__ void take_g(ldouble *T, int lane, const Inflight &F) {
        const ldouble *S = T + lane + (NT + NA) * WL;
        take_pass<MV>(T, nV, F.pp, F.wg, 0);
        wave_sync();
        SFOR(l, MV, const double a0 = S[l * WL]; gN[l] = l < nV ? a0 : 0.0;);
        LSTAMP(18);
    }
    __device__ __forceinline__ void g_from_K() {     // S empty: G = -K
        SFOR(k, MV, SFOR(j, k + 1, if constexpr (k < HB) G[tri(j, k) * WL] = -Hs(j, k); else G[tri(j, k) * WL] = -0.0;););
        if constexpr (GROUPED) {
            // (the builds with chunked pivots: A's reads together in front of its stores, pinned like a chunk's -- one pair at a
            //  time through one register quad they are NA / 2 round trips)
            double a[NA];
            SFOR(e, NA, a[e] = K[e * WL];);
            SFOR(i, MC, SFOR(k, MV, G[tri(k, MV + i) * WL] = -a[i * MV + k];); SFOR(j, i + 1, G[tri(MV + j, MV + i) * WL] = 0.0;););
            __builtin_amdgcn_sched_group_barrier(0x100, NA / 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, NA, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, NA / 2, 0);
        } else {
            SFOR(i, MC, SFOR(k, MV, G[tri(k, MV + i) * WL] = -As(i, k);); SFOR(j, i + 1, G[tri(MV + j, MV + i) * WL] = 0.0;););
        }
    }
    __device__ __forceinline__ bool bounds_inconsistent() const {
        bool bad = false;
        SFOR(l, MV, bad = bad || (l < nV && loN[l] > upN[l] + RSQP_EPS););
        SFOR(i, MC, bad = bad || (i < nC && cloN[i] > cupN[i] + RSQP_EPS););
        return bad;
    }

    // ------------------------------------------------------------------ auxiliary QP of a cold start (setup_aux of the CPU restatement)
    // x = 0, y = 0, every variable on a finite bound (lower first); variables without one are free and enter S by principal pivots
    // (those with curvature, repeatedly: a pivot may give the next one its curvature). false: free variables are left over
    // (built: the tableau of the empty working set is in place already -- stage_matrices)
    __device__ __forceinline__ bool setup_cold(bool built = false) {
        status = QPS_PREPARINGAUXILIARYQP;
        infeasible = unbounded = 0;
        int pf = 0;
        SFOR(l, MV, xv[l] = 0.0; yv[l] = 0.0;
            int s = -1;
            if (loN[l] <= -RSQP_INFTY) s = upN[l] < RSQP_INFTY ? 1 : 0;
            sv[l] = l < nV ? s : -1;
            pf |= (l < nV && s == 0) ? 1 << l : 0;);
            SFOR(i, MC, yc[i] = 0.0; ax[i] = 0.0; sc[i] = 0;);
        if (!built) g_from_K();
        fmask = amask = 0;
        for (int round = 0; round < 2 * N && pf != 0; round++) {
            bool progress = false;
#pragma unroll 1
            for (int v = 0; v < MV; v++)
                if ((pf >> v) & 1) {
                    const double pi = Gd(v, v);
                    if (-pi > 1e-8 * hscale) {
                        double u[N];
                        fetch_row(v, u);
                        pivot1(u, v, 1.0, pi);
                        fmask |= 1 << v; pf &= ~(1 << v); progress = true;
                    }
                }
            if (!progress) break;
        }
        if (pf != 0) return false;
        SFOR(l, MV, gy[l] = 0.0; g[l] = 0.0;
            lo[l] = sv[l] == -1 ? xv[l] : fmin(loN[l], xv[l] - RSQP_BOUND_RELAXATION);
            up[l] = sv[l] == 1 ? xv[l] : fmax(upN[l], xv[l] + RSQP_BOUND_RELAXATION);
            if (l >= nV) { lo[l] = 0.0; up[l] = 0.0; });
            SFOR(i, MC, loA[i] = fmin(cloN[i], ax[i] - RSQP_BOUND_RELAXATION);
            upA[i] = fmax(cupN[i], ax[i] + RSQP_BOUND_RELAXATION););
        status = QPS_AUXILIARYQPSOLVED;
        return true;
    }

    // ------------------------------------------------------------------ the set-up from a guess (WARM builds)
    // The guess of the wave's problems (QPPools::guess_x / _y / _sb / _sc: x, y = [bounds; constraints] and the two working sets,
    // member-major like the results; any of them absent), HBM -> slots 0 .. of the tableau's space -> my registers xv / yv / yc / sv / sc.
    // The space is free here: setup_warm builds the tableau of the empty working set by itself. A full wave of 16-byte aligned
    // pools moves 16 bytes per lane (the reverse of put_pairs / put_quads), any other wave element by element. In a hot start
    // with new matrices the pools ARE the result pools: the wave reads its members' ranges here and writes them at the end
    template <int CH> __device__ __forceinline__ void get_quads(const int *src, int n, int lane, ldouble *T, int s0) const {
        typedef __attribute__((address_space(3))) int lint;
        Walk wk = walk<4>(n, lane);
        const int4 *s4 = reinterpret_cast<const int4 *>(src) + lane;
        SFOR(c, (CH + 3) / 4, if (4 * c < n) {
                 if (c * WL + lane < 16 * n) {
                     const int4 v4 = s4[c * WL];
                     const int v[4] = {v4.x, v4.y, v4.z, v4.w};
                     int qq = wk.qq, e = wk.e;
                     SFOR(u, 4, ((lint *)(T + (s0 + e) * WL + qq))[0] = v[u];
                          const bool wrap = e + 1 == n; e = wrap ? 0 : e + 1; qq = wrap ? qq + 1 : qq;);
                 }
                 next_group(wk, n);
             });
    }
    template <int CH, class TV> __device__ __forceinline__ void get_block(const TV *src, int n, int cnt, int lane, ldouble *T, int s0) const {
        typedef __attribute__((address_space(3))) int lint;
        const float rn = 1.0f / (float)n;
        TV w[CH];
        SFOR(t, CH, const int m = t * WL + lane; if (t < n) w[t] = src[m < cnt ? m : cnt - 1];);
        SFOR(t, CH, if (t < n) {
                 const int m = t * WL + lane;
                 const int qq = (int)(((float)m + 0.5f) * rn), e = m - qq * n;
                 if (m < cnt) {
                     if constexpr (sizeof(TV) == 8) T[(s0 + e) * WL + qq] = w[t];
                     else ((lint *)(T + (s0 + e) * WL + qq))[0] = w[t];
                 }
             });
    }
    __device__ __forceinline__ void take_guess(const QPPools &P, long long q0, int lane, int nqw, ldouble *T) {
        typedef const __attribute__((address_space(3))) int clint;
        constexpr int SX = 0, SY = MV, SB = 2 * MV + MC, SW = 3 * MV + MC;
        static_assert(SW + MC <= NT, "the guess passes through the tableau's slots");
        const int nY = nV + nC;
        const bool hx = P.guess_x != nullptr, hy = P.guess_y != nullptr, hb = P.guess_sb != nullptr, hc = P.guess_sc != nullptr && nC > 0;
        wave_sync();           // (every lane is through with what the staging left in these slots)
        if (nqw == WL && (((size_t)P.guess_x | (size_t)P.guess_y | (size_t)P.guess_sb | (size_t)P.guess_sc) & 15) == 0) {
            const int pp = pair_of(lane);
            double wx[MV], wy[MV + MC];
            if (hx) BYPARITY(nV, load_pairs<MV, EV>(P.guess_x + q0 * nV, nV, pp, wx););
            if (hy) BYPARITY(nY, load_pairs<MV + MC, EV>(P.guess_y + q0 * nY, nY, pp, wy););
            if (hb) get_quads<MV>(P.guess_sb + q0 * nV, nV, lane, T, SB);
            if (hc) get_quads<MC>(P.guess_sc + q0 * nC, nC, lane, T, SW);
            if (hx) BYPARITY(nV, drop_pairs<MV, EV>(T, SX, nV, pp, walk<2>(nV, pp), wx););
            if (hy) BYPARITY(nY, drop_pairs<MV + MC, EV>(T, SY, nY, pp, walk<2>(nY, pp), wy););
        } else {
            if (hx) get_block<MV>(P.guess_x + q0 * nV, nV, nqw * nV, lane, T, SX);
            if (hy) get_block<MV + MC>(P.guess_y + q0 * nY, nY, nqw * nY, lane, T, SY);
            if (hb) get_block<MV>(P.guess_sb + q0 * nV, nV, nqw * nV, lane, T, SB);
            if (hc) get_block<MC>(P.guess_sc + q0 * nC, nC, nqw * nC, lane, T, SW);
        }
        wave_sync();
        // (a lane beyond the batch takes the last problem's guess, as it took its data; slots beyond the sizes: neutral values)
        const ldouble *S = T + (lane < nqw ? lane : nqw - 1);
        SFOR(l, MV, const bool v = l < nV;
             const double a0 = S[(SX + l) * WL], a1 = S[(SY + l) * WL]; const int s0 = ((clint *)(S + (SB + l) * WL))[0];
             xv[l] = (hx && v) ? a0 : 0.0; yv[l] = (hy && v) ? a1 : 0.0; sv[l] = v ? (hb ? s0 : 0) : -1;);
        SFOR(i, MC, const bool c = i < nC;
             const double a1 = S[(SY + (c ? nV + i : 0)) * WL]; const int s0 = ((clint *)(S + (SW + i) * WL))[0];
             yc[i] = (hy && c) ? a1 : 0.0; sc[i] = (hc && c) ? s0 : 0;);
        wave_sync();           // (every lane has read its slots: the space is the tableau's again)
    }
    // WARM level 2, a hot start on new vectors: the limits the members' last homotopy ended on -- lo, up (fields 2, 3 of the variable
    // slots: 16 consecutive doubles of a state block's tail) and loA, upA (fields 1, 2 of the constraint slots, MC of each) --, HBM ->
    // slots of the tableau's space -> my registers lo / up / loA / upA. They are all a hot start needs of the block beyond the guess:
    // g, gy and A x are exact products of the homotopy's first iteration, the tableau is built by setup_warm, and the tableau half
    // of the block is not read. Four lanes share a member's 32-byte piece, and a member's 128-byte run is used up by four
    // instructions in a row (a lane walking its own block: 64 lines per instruction for 8 bytes of each); in LDS the 16 lanes
    // of a store group then hold 4 owners (4-way conflicts on 20 stores; a member's run per 16 lanes would be 16-way)
    __device__ __forceinline__ void take_limits(const double *sbase, long long stride, int lane, int nqw, ldouble *T) {
        constexpr int SL = 0, SA = 2 * MV, PV = 2 * MV, PC = 2 * MC;
        static_assert(SA + PC <= NT && WL % PC == 0 && PV % 4 == 0, "the limits pass through the tableau's slots");
        const double *tail = sbase + N * N;
        double wv[PV], wc[PC];
        SFOR(t, PV, const int qq = (lane >> 2) + (WL / 4) * (t >> 2), f = (lane & 3) + 4 * (t & 3);
             wv[t] = tail[(long long)(qq < nqw ? qq : nqw - 1) * stride + 2 * MV + f];);
        SFOR(t, PC, const int qq = lane / PC + (WL / PC) * t, f = lane % PC;
             wc[t] = tail[(long long)(qq < nqw ? qq : nqw - 1) * stride + 6 * MV + (1 + f / MC) * 8 + f % MC];);
        SFOR(t, PV, const int qq = (lane >> 2) + (WL / 4) * (t >> 2), f = (lane & 3) + 4 * (t & 3);
             T[(SL + f) * WL + qq] = wv[t];);
        SFOR(t, PC, const int qq = lane / PC + (WL / PC) * t, f = lane % PC;
             T[(SA + f) * WL + qq] = wc[t];);
        wave_sync();
        const ldouble *S = T + (lane < nqw ? lane : nqw - 1);
        SFOR(l, MV, lo[l] = S[(SL + l) * WL]; up[l] = S[(SL + MV + l) * WL];);
        SFOR(i, MC, loA[i] = S[(SA + i) * WL]; upA[i] = S[(SA + MC + i) * WL];);
        wave_sync();           // (every lane has read its slots: the space is the tableau's again)
    }
    // sum of u_v^2 over the free variables; sum of a_v^2 over them for row `arow` of A
    __device__ __forceinline__ void free_norms(const double (&u)[N], int arow, double &pn2, double &na2) const {
        double s1 = 0.0, s2 = 0.0;
        SFOR(k, MV, const bool fr = (fmask >> k) & 1; const double a = As(arow, k);
             const double p1 = fma(u[k], u[k], s1), n1 = fma(a, a, s2);
             s1 = fr ? p1 : s1; s2 = fr ? n1 : s2;);
        pn2 = s1; na2 = s2;
    }
    // G for a guessed working set, from G = -K: the pending free variables (mask pf) and guessed active constraints (mask pa) enter S
    // by principal pivots, in the order and with the thresholds of qp_tiny.hip's warm_pivots: single pivots of the right sign first
    // (a variable with curvature, a constraint independent of S; slot by slot, ONE text for both), then 2 x 2 blocks (variable,
    // constraint) with an indefinite block. Variables left over: no positive definite reduced Hessian (false). Constraints left
    // over: dependent on the others, they stay out (pa returns what was skipped). The slot counters are the wave's, the masks a lane's
    __device__ __forceinline__ bool warm_pivots(int pf, int &pa) {
        for (int round = 0; round < 2 * N && (pf | pa) != 0; round++) {
            bool progress = false;
#pragma unroll 1
            for (int q = 0; q < MV + MC; q++) {
                const bool isc = q >= MV;
                const int i = isc ? q - MV : 0;
                if (!(((isc ? pa >> i : pf >> q) & 1) != 0)) continue;
                // (the tests that need no row first: a slot that stays out costs one LDS round trip, or none)
                if (isc && !(nFR() - nAC() > 0)) continue;
                const double pi = Gd(q, q);
                if (!isc && !(-pi > 1e-8 * hscale)) continue;
                double u[N];
                fetch_row(q, u);
                bool take = true;
                if (isc) {
                    double pn2, na2;
                    free_norms(u, i, pn2, na2);
                    take = na2 > 0.0 && hscale * hscale * pn2 > 1e-18 * na2 && pi * hscale > 1e-10 * na2;
                }
                if (take) {
                    pivot1(u, q, 1.0, pi);
                    if (isc) { amask |= 1 << i; pa &= ~(1 << i); } else { fmask |= 1 << q; pf &= ~(1 << q); }
                    progress = true;
                }
            }
            if (!progress && pf != 0 && pa != 0) {
#pragma unroll 1
                for (int vi = 0; vi < MV * MC; vi++) {
                    const int v = vi / MC, i = vi - v * MC;
                    if (progress || !((pf >> v) & 1) || !((pa >> i) & 1)) continue;
                    const double pp = Gd(v, v), qq = Gd(MV + i, MV + i), pq = Gd(v, MV + i);
                    const double det = pp * qq - pq * pq;
                    if (det < 0.0 && -det > 1e-10 * fmax(fabs(pp * qq), pq * pq) && pq * pq > 1e-16 * hscale * hscale) {
                        double uv[N], ui[N];
                        fetch_row(v, uv); fetch_row(MV + i, ui);
                        const double rd = recip(det);
                        pivot2(uv, ui, v, 1.0, MV + i, 1.0, qq * rd, -pq * rd, pp * rd);
                        fmask |= 1 << v; amask |= 1 << i; pf &= ~(1 << v); pa &= ~(1 << i);
                        progress = true;
                    }
                }
            }
            if (!progress) break;
        }
        return pf == 0;
    }
    // EngineT::setup of qp_tiny.hip for a lane that holds all slots: the same decisions in the same order. The guess waits in
    // xv / yv / yc / sv / sc (take_guess); have_*: the parts of it this lane takes (none of them: the cold start, x = 0, y = 0,
    // every variable on a finite bound, lower first). false: the guess gives no positive definite reduced Hessian (the caller
    // falls back to the cold start)
    // hot (WARM level 2, a hot start on new vectors): the guess is the stored iterate, and lo / up / loA / upA hold the limits it was
    // reached under (take_limits). The working set was valid under THOSE limits, so the targets, which are new, take no side away,
    // no multiplier is clipped, and the limits stay: the homotopy runs from them to the targets, as qp_tiny.hip's mode 1 does
    __device__ __forceinline__ bool setup_warm(bool have_x0, bool have_y0, bool have_gb, bool have_gc, bool c_from_y0, bool hot = false) {
        status = QPS_PREPARINGAUXILIARYQP;
        infeasible = unbounded = 0;
        int pf = 0;
        SFOR(l, MV, const bool v = l < nV;
             xv[l] = (have_x0 && v) ? xv[l] : 0.0; yv[l] = (have_y0 && v) ? yv[l] : 0.0;
             const int sx = xv[l] <= loN[l] + RSQP_BOUND_TOLERANCE ? -1 : (xv[l] >= upN[l] - RSQP_BOUND_TOLERANCE ? 1 : 0);
             const int sy = yv[l] > RSQP_EPS ? -1 : (yv[l] < -RSQP_EPS ? 1 : 0);
             int s = have_gb ? sv[l] : (have_x0 ? sx : (have_y0 ? sy : -1));
             if (!hot && s == -1 && loN[l] <= -RSQP_INFTY) s = (upN[l] < RSQP_INFTY && !have_x0 && !have_gb) ? 1 : 0;
             if (!hot && s == 1 && upN[l] >= RSQP_INFTY) s = 0;
             sv[l] = v ? s : -1;
             pf |= (v && s == 0) ? 1 << l : 0;);
        SFOR(i, MC, yc[i] = (have_y0 && i < nC) ? yc[i] : 0.0;);
        g_from_K();
        fmask = amask = 0;
        // A x of the guess and the constraints' sides (qpOASES: from the guess, else from y0, else from A x0)
        double gyx[MV], axx[MC], hxx[MV];
        exact_products(gyx, axx, hxx);           // (x = 0, y = 0: every product is +0, what qp_tiny.hip sets without forming them)
        int pa = 0;
        SFOR(i, MC, const bool c = i < nC;
             ax[i] = c ? axx[i] : 0.0;
             const int sy = yc[i] > RSQP_EPS ? -1 : (yc[i] < -RSQP_EPS ? 1 : 0);
             const int sx = ax[i] <= cloN[i] + RSQP_BOUND_TOLERANCE ? -1 : (ax[i] >= cupN[i] - RSQP_BOUND_TOLERANCE ? 1 : 0);
             int sgc = 0;
             if (have_gc) sgc = sc[i];
             else if (have_y0 && (!have_x0 || c_from_y0)) sgc = sy;
             else if (have_x0) sgc = sx;
             if (!hot && sgc == -1 && cloN[i] <= -RSQP_INFTY) sgc = 0;
             if (!hot && sgc == 1 && cupN[i] >= RSQP_INFTY) sgc = 0;
             if (!c) sgc = 0;
             sc[i] = sgc;
             pa |= sgc != 0 ? 1 << i : 0;);
        if (!warm_pivots(pf, pa)) return false;
        SFOR(i, MC, sc[i] = ((pa >> i) & 1) ? 0 : sc[i];);          // (what is left in pa was dependent: it stays out)
        // multipliers: zero when inactive, clipped to the sign their side requires
        SFOR(l, MV, const bool z = sv[l] == 0 || (!hot && ((sv[l] == -1 && yv[l] < 0.0) || (sv[l] == 1 && yv[l] > 0.0))); yv[l] = z ? 0.0 : yv[l];);
        SFOR(i, MC, const bool z = sc[i] == 0 || (!hot && ((sc[i] == -1 && yc[i] < 0.0) || (sc[i] == 1 && yc[i] > 0.0))); yc[i] = z ? 0.0 : yc[i];);
        // gradient of the auxiliary QP from stationarity, its limits around the iterate
        exact_products(gyx, axx, hxx);
        if constexpr (WARM >= 2) {
        SFOR(l, MV, gy[l] = gyx[l]; g[l] = gyx[l] + yv[l];
             const double l1 = sv[l] == -1 ? xv[l] : fmin(loN[l], xv[l] - RSQP_BOUND_RELAXATION);
             const double u1 = sv[l] == 1 ? xv[l] : fmax(upN[l], xv[l] + RSQP_BOUND_RELAXATION);
             lo[l] = hot ? lo[l] : l1; up[l] = hot ? up[l] : u1;
             if (l >= nV) { lo[l] = 0.0; up[l] = 0.0; });
        SFOR(i, MC, const double l1 = sc[i] == -1 ? ax[i] : fmin(cloN[i], ax[i] - RSQP_BOUND_RELAXATION);
             const double u1 = sc[i] == 1 ? ax[i] : fmax(cupN[i], ax[i] + RSQP_BOUND_RELAXATION);
             loA[i] = (hot && i < nC) ? loA[i] : l1; upA[i] = (hot && i < nC) ? upA[i] : u1;);
        } else {
        SFOR(l, MV, gy[l] = gyx[l]; g[l] = gyx[l] + yv[l];
             lo[l] = sv[l] == -1 ? xv[l] : fmin(loN[l], xv[l] - RSQP_BOUND_RELAXATION);
             up[l] = sv[l] == 1 ? xv[l] : fmax(upN[l], xv[l] + RSQP_BOUND_RELAXATION);
             if (l >= nV) { lo[l] = 0.0; up[l] = 0.0; });
        SFOR(i, MC, loA[i] = sc[i] == -1 ? ax[i] : fmin(cloN[i], ax[i] - RSQP_BOUND_RELAXATION);
             upA[i] = sc[i] == 1 ? ax[i] : fmax(cupN[i], ax[i] + RSQP_BOUND_RELAXATION););
        }
        status = QPS_AUXILIARYQPSOLVED;
        return true;
    }

    // ------------------------------------------------------------------ one working-set change
    // kind 1 constraint idx leaves | 2 bound of idx leaves | 3 constraint idx enters at `side` | 4 variable idx gets fixed at `side`
    // (style of the slot passes here and in homotopy(): every arm of a choice is computed first, then selected -- plain selects
    //  between values; a ternary with arithmetic in its arms becomes a tree of divergent branches per slot. The one exception is
    //  measured: the variable slots of homotopy()'s ratio test in the headline build, ROLES)
    // The parts of a change that both of its texts below hold -- change<KIND>() and change_exchange() --, each stated once. They are
    // macros, expanded in place with the partner's kind by lane (`pk`) or as a literal: change<KIND>() must stay, token for token,
    // the text it was, because every build of the kernel holds it and the builds without the exchange's votes keep their device
    // code. (As lambdas or member templates, inlined in full either way, each of the parts changed the register allocation of every
    // build; so did a pair of braces around one of them.) They declare their locals in the scope that expands them.
    // CHANGE_SUMS: the sum of u_v^2 over the free variables and of a_v^2 over them for the incoming row (row idx of A, or e_idx), and
    // from them li: 1 the row is independent of the active ones (plain entry), 0 it depends on them (exchange); in the band between
    // the two thresholds the residual of the row's representation by the active rows decides (qp_small_g.h)
#define CHANGE_SUMS                                                                                                                  \
            double arow[MV];                                                                                                         \
            double pn2 = 0.0, na2 = 0.0;                                                                                             \
            const int ia = kind == 3 ? idx : 0;                                                                                      \
            SFOR(k, MV, const bool fr = (fmask >> k) & 1;                                                                            \
                 const double aA = As(ia, k), aE = k == idx ? 1.0 : 0.0;                                                             \
                 arow[k] = kind == 3 ? aA : aE;                                                                                      \
                 const double p1 = fma(u[k], u[k], pn2), n1 = fma(arow[k], arow[k], na2);                                            \
                 pn2 = fr ? p1 : pn2; na2 = fr ? n1 : na2;);                                                                         \
            int li;                                                                                                                  \
            if (nFR() - nAC() <= 0 || !(na2 > 0.0)) li = 0;                                                                          \
            else {                                                                                                                   \
                const double p2 = hscale * hscale * pn2;                                                                             \
                li = p2 > 1e-12 * na2 ? 1 : (p2 < 1e-24 * na2 ? 0 : -1);                                                             \
            }                                                                                                                        \
            if (li < 0) {                                                                                                            \
                double rn2 = 0.0;                                                                                                    \
                SFOR(l, MV, double r = l < nV ? arow[l] : 0.0;                                                                       \
                     SFOR(i, MC, const double r1 = fma(-As(i, l), sg * u[MV + i], r); r = ((amask >> i) & 1) ? r1 : r;);             \
                     rn2 += ((l < nV) & (sv[l] == 0)) ? r * r : 0.0;);                                                               \
                li = rn2 > 9e-16 * na2 ? 1 : 0;                 /* |r| / |a_FR| > 3e-8 */                                            \
            }                                                                                                                        \
            LSTAMP_IN(21);
    // CHANGE_PARTNER: the exchange's first half -- shift the multipliers along the dependency until one of them reaches zero; that
    // one leaves (pk, pidx). No partner: infeasible beyond this point of the homotopy -- unless that point IS its end to rounding
#define CHANGE_PARTNER                                                                                                               \
                const double sgn = side == 1 ? -1.0 : 1.0, ss = sgn * sg;                                                            \
                double xiv[MV], xic[MC];                                                                                             \
                double bt = RSQP_INFTY;                                                                                              \
                int bid = 0x7fffffff;                                                                                                \
                SFOR(i, MC, const bool on = (i < nC) & (sc[i] != 0), wl = sc[i] == -1;                                               \
                     const double xu = ss * u[MV + i];                                                                               \
                     xic[i] = on ? xu : 0.0;                                                                                         \
                     const double num = wl ? yc[i] : -yc[i], den = wl ? xic[i] : -xic[i];                                            \
                     if (on & (den > RSQP_EPS_DEN)) {                                                                                \
                         const double t = (num > 0.0 ? num : 0.0) / den;                                                             \
                         const bool better = (t < bt) | ((t == bt) & (i < bid));                                                     \
                         bt = better ? t : bt; bid = better ? i : bid;                                                               \
                     });                                                                                                             \
                SFOR(l, MV, const bool on = (l < nV) & (sv[l] != 0), wl = sv[l] == -1;                                               \
                     const double xu = ss * u[l];                                                                                    \
                     xiv[l] = on ? xu : 0.0;                                                                                         \
                     const double num = wl ? yv[l] : -yv[l], den = wl ? xiv[l] : -xiv[l];                                            \
                     if (on & (den > RSQP_EPS_DEN)) {                                                                                \
                         const double t = (num > 0.0 ? num : 0.0) / den;                                                             \
                         const bool better = (t < bt) | ((t == bt) & (nC + l < bid));                                                \
                         bt = better ? t : bt; bid = better ? nC + l : bid;                                                          \
                     });                                                                                                             \
                if (bid == 0x7fffffff) {                                                                                             \
                    if (tau >= 1.0 - 1e-9) { treat_done = true; return RET_OK; }                                                     \
                    return RET_INFEASIBLE;                                                                                           \
                }                                                                                                                    \
                if (bid < nC) { pk = 1; pidx = bid; } else { pk = 2; pidx = bid - nC; }                                              \
                SFOR(l, MV, yv[l] -= bt * xiv[l];);                                                                                  \
                SFOR(i, MC, yc[i] -= bt * xic[i];);                                                                                  \
                ynew = sgn * bt;                                                                                                     \
                LSTAMP_IN(22);
    // CHANGE_BLOCK_PIVOT(PK): the exchange's second half, the 2 x 2 block pivot on (partner, incoming). PK: `pk`, or the kind of the
    // partner as a literal (a wave whose lanes agree on it): p and the pivot's signs fold
#define CHANGE_BLOCK_PIVOT(PK)                                                                                                       \
                const int p = PK == 1 ? MV + pidx : pidx;                                                                            \
                double u2[N];                                                                                                        \
                fetch_row(p, u2);                                                                                                    \
                const double pp = Gd(p, p), qq = pi, pq = Gd(p, q);                                                                  \
                const double det = pp * qq - pq * pq;                                                                                \
                if (!(det < 0.0) || !(-det > 1e-10 * fmax(fabs(pp * qq), pq * pq))) return RET_SETUP_FAILED;                         \
                const double rd = recip(det);                                                                                        \
                LSTAMP_IN(23);                                                                                                       \
                pivot2(u2, u, p, PK == 1 ? -1.0 : 1.0, q, kind == 3 ? 1.0 : -1.0, qq * rd, -pq * rd, pp * rd);                       \
                LSTAMP_IN(16);                                                                                                       \
                since_refresh = REFRESH;
    // CHANGE_ENTRY_TEST: the set-up test of a plain entry
#define CHANGE_ENTRY_TEST                                                                                                            \
                if (kind == 3) { if (!(pi * hscale > 1e-10 * na2)) return RET_SETUP_FAILED; }                                        \
                else if (!(pi * hscale > 1e-10)) return RET_SETUP_FAILED;
    // CHANGE_FINISH(PK): the pivot on q alone where no partner leaves, and the working set. PK as above, or the literal 0: no lane
    // has a partner
#define CHANGE_FINISH(PK)                                                                                                            \
        LSTAMP_IN(14);                                                                                                               \
        if (PK == 0) pivot1(u, q, (kind == 2 || kind == 3) ? 1.0 : -1.0, pi);                                                        \
        LSTAMP_IN(16);                                                                                                               \
        const bool leaves = (kind == 1) | (kind == 2);                                                                               \
        const int snew = leaves ? 0 : side;                                                                                          \
        const double ynw = leaves ? 0.0 : ynew;                                                                                      \
        SFOR(l, MV, const bool my = !isc & (l == idx), pr = (PK == 2) & (l == pidx);                                                 \
             const int s1 = pr ? 0 : sv[l]; const double y1 = pr ? 0.0 : yv[l];                                                      \
             sv[l] = my ? snew : s1; yv[l] = my ? ynw : y1;);                                                                        \
        SFOR(i, MC, const bool my = isc & (i == idx), pr = (PK == 1) & (i == pidx);                                                  \
             const int s1 = pr ? 0 : sc[i]; const double y1 = pr ? 0.0 : yc[i];                                                      \
             sc[i] = my ? snew : s1; yc[i] = my ? ynw : y1;);                                                                        \
        if (kind == 1) amask &= ~(1 << idx); else if (kind == 2) fmask |= 1 << idx; else if (kind == 3) amask |= 1 << idx; else fmask &= ~(1 << idx); \
        if (PK == 1) amask &= ~(1 << pidx); else if (PK == 2) fmask |= 1 << pidx;                                                    \
        return RET_OK;

    // KIND: the kind as a constant (a wave whose lanes agree on it, VOTE), or 0: `kind_` by lane. With the constant, `isc`,
    // `leaves`, the pivot's sign and `sg` fold and the arms of the other kinds are not in the text; idx, side and q stay by lane,
    // and so do the arms a lane may take alone: the flip (kinds 1, 2) and the exchange (kinds 3, 4)
    template <int KIND> __device__ __forceinline__ int change(int kind_, int idx, int side, double tau, bool &treat_done) {
        const int kind = KIND != 0 ? KIND : kind_;
        const bool isc = (kind == 1) | (kind == 3);
        const int q = isc ? MV + idx : idx;
        double u[N];
        fetch_row(q, u);
        const double pi = Gd(q, q);
        bool flip = false;
        if (kind == 1) {
            double d2 = 0.0;
            SFOR(k, MV, const double d2n = fma(u[k], u[k], d2); d2 = ((fmask >> k) & 1) ? d2n : d2;);
            flip = !(d2 > 0.0 && -pi > 1e-8 * hscale * d2);
        } else if (kind == 2) flip = !(-pi > 1e-8 * hscale);
        if (flip) {
            // the released direction has no curvature: the constraint / bound goes to its OPPOSITE side, G is unchanged
            double opp = 0.0;
            SFOR(i, MC, const double o1 = sc[i] == -1 ? cupN[i] : cloN[i]; opp = (isc & (i == idx)) ? o1 : opp;);
            SFOR(l, MV, const double o1 = sv[l] == -1 ? upN[l] : loN[l]; opp = (!isc & (l == idx)) ? o1 : opp;);
            if (opp >= RSQP_INFTY || opp <= -RSQP_INFTY) return RET_UNBOUNDED;
            SFOR(i, MC, const bool my = isc & (i == idx); const bool wl = sc[i] == -1, wu = sc[i] == 1;
                 upA[i] = (my & wl) ? ax[i] : upA[i]; loA[i] = (my & wu) ? ax[i] : loA[i];
                 yc[i] = my ? 0.0 : yc[i]; sc[i] = my ? -sc[i] : sc[i];);
            SFOR(l, MV, const bool my = !isc & (l == idx); const bool wl = sv[l] == -1, wu = sv[l] == 1;
                 up[l] = (my & wl) ? xv[l] : up[l]; lo[l] = (my & wu) ? xv[l] : lo[l];
                 yv[l] = my ? 0.0 : yv[l]; sv[l] = my ? -sv[l] : sv[l];);
            nflips++;
            since_refresh = REFRESH;
            return RET_OK;
        }
        int pk = 0, pidx = -1;
        double ynew = 0.0;
        if (kind >= 3) {
            const double sg = kind == 3 ? -1.0 : 1.0;
            LSTAMP_IN(14);
            CHANGE_SUMS
            if (li == 0) {
                CHANGE_PARTNER
                CHANGE_BLOCK_PIVOT(pk)
            } else {
                CHANGE_ENTRY_TEST
            }
        }
        CHANGE_FINISH(pk)
    }
    // change<3>() with the exchange's votes, XV (VOTE, bits 5 .. 8): the lanes still in the function vote once more on what that text
    // leaves by lane, and a wave that agrees runs a text in which it is a constant.
    // Bit 0: whether any lane needs the sums at all -- nFR - nAC <= 0 in every lane: li is 0 whatever they say, and neither they
    // nor the band are on that path (both changes of every headline member) --, and, behind the sums, li: all 0 the exchange, all
    // 1 the plain entry with pivot1 unmasked, else the text by lane. Bit 1 / bit 2: the partner's kind behind the exchange's ratio
    // test, all bounds / all constraints: p, pivot2's signs, the `pr` selects of the working-set pass and the mask updates fold.
    // Bit 3: the ranges of idx and, with the partner's kind, of pidx are stated, so that the `k <= q` of the row helpers and
    // pivot2's slot compares fold where the range decides them (q = MV + idx >= every variable slot; a bound's p < every
    // constraint slot). Per lane every path performs the operations of change<3>() on the same operands in the same order
    template <int XV> __device__ __forceinline__ int change_exchange(int idx, int side, double tau, bool &treat_done) {
        static_assert((XV & 1) != 0, "the votes on the partner and the ranges ride on the vote on the sums");
        constexpr int kind = 3;
        constexpr bool isc = true;
        if constexpr ((XV & 8) != 0) { __builtin_assume(idx >= 0); __builtin_assume(idx < MC); }
        const int q = MV + idx;
        double u[N];
        fetch_row(q, u);
        const double pi = Gd(q, q);
        int pk = 0, pidx = -1;
        double ynew = 0.0;
        const double sg = -1.0;
        LSTAMP_IN(14);
        const unsigned long long here = __builtin_amdgcn_ballot_w64(true);
        if (__builtin_amdgcn_ballot_w64(nFR() - nAC() <= 0) != here) {
            CHANGE_SUMS
            const unsigned long long l0 = __builtin_amdgcn_ballot_w64(li == 0);
            if (l0 != here) {
                if (l0 == 0) {
                    CHANGE_ENTRY_TEST
                    CHANGE_FINISH(0)
                }
                if (li == 0) {
                    CHANGE_PARTNER
                    CHANGE_BLOCK_PIVOT(pk)
                } else {
                    CHANGE_ENTRY_TEST
                }
                CHANGE_FINISH(pk)
            }
        }
        // every lane exchanges
        CHANGE_PARTNER
        // (the lanes without a partner have returned)
        const unsigned long long left = __builtin_amdgcn_ballot_w64(true);
        if ((XV & 2) != 0 && __builtin_amdgcn_ballot_w64(pk == 2) == left) {
            if constexpr ((XV & 8) != 0) { __builtin_assume(pidx >= 0); __builtin_assume(pidx < MV); }
            CHANGE_BLOCK_PIVOT(2)
            CHANGE_FINISH(2)
        }
        if ((XV & 4) != 0 && __builtin_amdgcn_ballot_w64(pk == 1) == left) {
            if constexpr ((XV & 8) != 0) { __builtin_assume(pidx >= 0); __builtin_assume(pidx < MC); }
            CHANGE_BLOCK_PIVOT(1)
            CHANGE_FINISH(1)
        }
        CHANGE_BLOCK_PIVOT(pk)
        CHANGE_FINISH(pk)
    }
#undef CHANGE_SUMS
#undef CHANGE_PARTNER
#undef CHANGE_BLOCK_PIVOT
#undef CHANGE_ENTRY_TEST
#undef CHANGE_FINISH

    __device__ __forceinline__ int homotopy(int maxit, int &nWSR) {
        int iter = 0, rcode = RET_OK;
        status = QPS_PERFORMINGHOMOTOPY;
        since_refresh = REFRESH;
        // limits that are infinite where the targets are finite get relaxed ones (a hot start's concern, kept from qp_tiny.hip). This
        // kernel only runs cold starts, and after setup_cold() the pass changes nothing: lo is x (finite) for a variable at its lower
        // bound and fmin(loN, x - relaxation) otherwise, so lo <= -INFTY implies loN <= -INFTY, and c1 asks for the opposite; the same
        // holds for up / upN, loA / cloN, upA / cupN, and the slots beyond nV / nC hold 0 / the infinite targets. ROLES leaves it out
        if constexpr (!ROLES) {
        SFOR(l, MV, const double l1 = fmin(loN[l], xv[l] - RSQP_BOUND_RELAXATION), u1 = fmax(upN[l], xv[l] + RSQP_BOUND_RELAXATION);
             const bool c1 = (sv[l] != -1) & (lo[l] <= -RSQP_INFTY) & (loN[l] > -RSQP_INFTY);
             const bool c2 = (sv[l] != 1) & (up[l] >= RSQP_INFTY) & (upN[l] < RSQP_INFTY);
             lo[l] = c1 ? l1 : lo[l]; up[l] = c2 ? u1 : up[l];);
        SFOR(i, MC, const double l1 = fmin(cloN[i], ax[i] - RSQP_BOUND_RELAXATION), u1 = fmax(cupN[i], ax[i] + RSQP_BOUND_RELAXATION);
             const bool c1 = (sc[i] != -1) & (loA[i] <= -RSQP_INFTY) & (cloN[i] > -RSQP_INFTY);
             const bool c2 = (sc[i] != 1) & (upA[i] >= RSQP_INFTY) & (cupN[i] < RSQP_INFTY);
             loA[i] = c1 ? l1 : loA[i]; upA[i] = c2 ? u1 : upA[i];);
        }
        for (;;) {
            // ---- x exactly on its active bounds; (exact products); drift correction + input of the product
            SFOR(l, MV, const int s_ = opq(sv[l]); const double xb = s_ == -1 ? lo[l] : up[l]; xv[l] = s_ != 0 ? xb : xv[l];);
            if (since_refresh >= REFRESH) {
                double gyx[MV], axx[MC], hxx[MV];
                exact_products(gyx, axx, hxx);
                SFOR(l, MV, gy[l] = gyx[l];);
                SFOR(i, MC, ax[i] = i < nC ? axx[i] : 0.0;);
                since_refresh = 0;
            }
            double in[N], o[N];
            SFOR(l, MV, const int s_ = opq(sv[l]); const double gl = gy[l] + yv[l]; g[l] = gl;
                 const double a0 = -(gN[l] - gl), a1 = loN[l] - lo[l], a2 = upN[l] - up[l];
                 const double a12 = s_ == -1 ? a1 : a2;
                 in[l] = s_ == 0 ? a0 : a12;);              // (slots beyond nV: fixed at 0 = lo = loN)
            SFOR(i, MC, const int s_ = opq(sc[i]); const bool wl = s_ == -1, wu = s_ == 1;
                 loA[i] = wl ? ax[i] : loA[i]; upA[i] = wu ? ax[i] : upA[i];
                 const double a1 = cloN[i] - loA[i], a2 = cupN[i] - upA[i];
                 const double a12 = wl ? a1 : a2;
                 in[MV + i] = s_ == 0 ? 0.0 : a12;);
            LSTAMP(5);
            // ---- out = G in; dx / dy / A dx and the ratio test over my slots (ties go to the lowest id)
            g_times(in, o);
            LSTAMP(6);
            double dxv[MV], dyv[MV], hd[MV], dax[MC], dyc[MC];
            double bt = 1.0;
            int bid = 0x7fffffff;
            // (one branch per candidate, around its division: perturbations of one QP agree on which candidates are dead -- half
            //  of them on the headline batch --, and the wave skips those)
            auto cand = [&](double num, double den, int id, bool ok) {
                const bool live = ok & (den >= RSQP_EPS_DEN);
                if (live) {
                    const double t = (num > 0.0 ? num : 0.0) / den;
                    const bool better = (t < bt) | ((t == bt) & (id < bid));
                    bt = better ? t : bt; bid = better ? id : bid;
                }
            };
            SFOR(i, MC, const int s_ = opq(sc[i]); const double oc = o[MV + i], noc = -oc;
                 const bool act = s_ != 0, wl = s_ == -1;
                 dax[i] = act ? in[MV + i] : noc; dyc[i] = act ? noc : 0.0;
                 const double nA = wl ? yc[i] : -yc[i], nI = ax[i] - loA[i];
                 const double dA = wl ? -dyc[i] : dyc[i], dI = (cloN[i] - loA[i]) - dax[i];
                 const double num1 = act ? nA : nI, den1 = act ? dA : dI;
                 const int id1 = act ? i : nC + nV + i;
                 cand(num1, den1, id1, (i < nC) & (act | (cloN[i] > -RSQP_INFTY)));
                 cand(upA[i] - ax[i], dax[i] - (cupN[i] - upA[i]), 2 * nC + nV + i, (i < nC) & !act & (cupN[i] < RSQP_INFTY)););
            if constexpr (ROLES) {
            // one arm per role of a variable slot: a fixed slot (all eight of the headline's first pass, seven and six in the next
            // two) no longer pays for the free role's two bound candidates, their masks and the selects between the roles. Per
            // lane the operands, the candidate ids and their order are the ones below; lanes that disagree on a slot's role run
            // both arms, as the selects did. (The same arms for the constraint slots, for the drift / input pass and for the
            // exchange's ratio test measured slower or no different on the headline batch: DESIGN.md 4.3b)
            SFOR(l, MV, const int s_ = opq(sv[l]); const double ov = o[l], dg = gN[l] - g[l];
                 if (s_ == 0) {
                     dxv[l] = ov; dyv[l] = 0.0; hd[l] = -dg;
                     cand(xv[l] - lo[l], (loN[l] - lo[l]) - ov, 3 * nC + nV + l, (l < nV) & (loN[l] > -RSQP_INFTY));
                     cand(up[l] - xv[l], ov - (upN[l] - up[l]), 3 * nC + 2 * nV + l, (l < nV) & (upN[l] < RSQP_INFTY));
                 } else {
                     const bool wl = s_ == -1; const double dgo = dg - ov;
                     dxv[l] = in[l]; dyv[l] = dgo; hd[l] = -ov;
                     cand(wl ? yv[l] : -yv[l], wl ? -dgo : dgo, nC + l, l < nV);
                 });
            } else {
            SFOR(l, MV, const int s_ = opq(sv[l]); const double ov = o[l], dg = gN[l] - g[l], nov = -ov, dgo = dg - ov, ndg = -dg;
                 const bool fr = s_ == 0, wl = s_ == -1;
                 dxv[l] = fr ? ov : in[l]; dyv[l] = fr ? 0.0 : dgo; hd[l] = fr ? ndg : nov;
                 const double nA = wl ? yv[l] : -yv[l], nI = xv[l] - lo[l];
                 const double dA = wl ? -dyv[l] : dyv[l], dI = (loN[l] - lo[l]) - dxv[l];
                 const double num1 = fr ? nI : nA, den1 = fr ? dI : dA;
                 const int id1 = fr ? 3 * nC + nV + l : nC + l;
                 cand(num1, den1, id1, (l < nV) & (!fr | (loN[l] > -RSQP_INFTY)));
                 cand(up[l] - xv[l], dxv[l] - (upN[l] - up[l]), 3 * nC + 2 * nV + l, (l < nV) & fr & (upN[l] < RSQP_INFTY)););
            }
            if (!(bt < 1.0)) { bt = 1.0; bid = 0x7fffffff; }
            LSTAMP(7);
            int kind = 0, idx = -1, side = 0;
            if (bid != 0x7fffffff) {
                if (bid < nC) { kind = 1; idx = bid; }
                else if (bid < nC + nV) { kind = 2; idx = bid - nC; }
                else if (bid < 2 * nC + nV) { kind = 3; idx = bid - nC - nV; side = -1; }
                else if (bid < 3 * nC + nV) { kind = 3; idx = bid - 2 * nC - nV; side = 1; }
                else if (bid < 3 * nC + 2 * nV) { kind = 4; idx = bid - 3 * nC - nV; side = -1; }
                else { kind = 4; idx = bid - 3 * nC - 2 * nV; side = 1; }
            }
            const double tau = bt;
            const bool done = kind == 0;
            const bool cap = iter >= maxit;
            const bool go_lane = !done & !cap;
            // ---- homotopy step on my slots. DM: what the wave agreed on (VOTE) -- 1 no lane is done, 2 every lane is: `done` is that
            // constant, the selects on it fold, and of the values a done lane discards (the interpolated limits and gradient) nothing
            // is computed; 0: `done` by lane, the text of the builds without the flag
            const bool done_lane = done;
            auto step = [&](auto dm_c) {
                constexpr int DM = decltype(dm_c)::value;
                const bool done = DM == 0 ? done_lane : DM == 2;
                const bool go = DM == 0 ? go_lane : !done & !cap;
                SFOR(l, MV, const int s_ = opq(sv[l]); yv[l] += tau * dyv[l];
                     const double xn = xv[l] + tau * dxv[l];
                     const double l1 = lo[l] + tau * (loN[l] - lo[l]), u1 = up[l] + tau * (upN[l] - up[l]);
                     const double gn = g[l] + tau * (gN[l] - g[l]);
                     const bool hit = go & (kind == 4) & (l == idx);
                     const double xe1 = s_ == 1 ? upN[l] : xn, xe = s_ == -1 ? loN[l] : xe1;
                     xv[l] = done ? xe : xn;
                     g[l] = done ? gN[l] : gn;
                     gy[l] -= tau * hd[l];
                     const double l2 = (hit & (side == -1)) ? xn : l1, u2 = (hit & (side == 1)) ? xn : u1;
                     lo[l] = done ? loN[l] : l2; up[l] = done ? upN[l] : u2;);
                SFOR(i, MC, yc[i] += tau * dyc[i];
                     const double an = ax[i] + tau * dax[i];
                     const double l1 = loA[i] + tau * (cloN[i] - loA[i]), u1 = upA[i] + tau * (cupN[i] - upA[i]);
                     const bool hit = go & (kind == 3) & (i == idx);
                     ax[i] = done ? ax[i] : an;
                     const double l2 = (hit & (side == -1)) ? an : l1, u2 = (hit & (side == 1)) ? an : u1;
                     loA[i] = done ? cloN[i] : l2; upA[i] = done ? cupN[i] : u2;);
            };
            LSTAMP_IN(20);
            if constexpr ((VOTE & 1) != 0) {
                // (the lanes still in the loop vote; those that have left it are masked off and do not enter the ballot)
                const unsigned long long in_loop = __builtin_amdgcn_ballot_w64(true), dn = __builtin_amdgcn_ballot_w64(done_lane);
                if (dn == 0) step(std::integral_constant<int, 1>{});
                else if (dn == in_loop) step(std::integral_constant<int, 2>{});
                else step(std::integral_constant<int, 0>{});
            } else step(std::integral_constant<int, 0>{});
            LSTAMP(8);
            if (done || cap) {
                if (done) status = QPS_SOLVED; else rcode = RET_MAX_NWSR;
                break;
            }
            bool treat_done = false;
            if constexpr ((VOTE & ~1) != 0) {
                // every lane here is about to change its working set (done and capped lanes have left): one text per kind the wave
                // agrees on, the text by lane otherwise
                const unsigned long long in_loop = __builtin_amdgcn_ballot_w64(true);
                auto all = [&](int k) { return __builtin_amdgcn_ballot_w64(kind == k) == in_loop; };
                if ((VOTE & 4) != 0 && all(2)) rcode = change<2>(kind, idx, side, tau, treat_done);
                else if ((VOTE & 16) != 0 && all(4)) rcode = change<4>(kind, idx, side, tau, treat_done);
                else if ((VOTE & 8) != 0 && all(3)) {
                    if constexpr (((VOTE >> 5) & 15) != 0) rcode = change_exchange<(VOTE >> 5) & 15>(idx, side, tau, treat_done);
                    else rcode = change<3>(kind, idx, side, tau, treat_done);
                }
                else if ((VOTE & 2) != 0 && all(1)) rcode = change<1>(kind, idx, side, tau, treat_done);
                else rcode = change<0>(kind, idx, side, tau, treat_done);
            } else rcode = change<0>(kind, idx, side, tau, treat_done);
            LSTAMP(9);
            if (treat_done) {      // (see change: no exchange partner at the very end of the homotopy)
                SFOR(l, MV, g[l] = gN[l]; lo[l] = loN[l]; up[l] = upN[l];
                     const double xb = sv[l] == -1 ? loN[l] : upN[l]; xv[l] = sv[l] != 0 ? xb : xv[l];);
                SFOR(i, MC, loA[i] = cloN[i]; upA[i] = cupN[i];);
                status = QPS_SOLVED;
                break;
            }
            if (rcode == RET_INFEASIBLE) { infeasible = 1; break; }
            if (rcode == RET_UNBOUNDED) { unbounded = 1; break; }
            if (rcode != RET_OK) break;
            iter++;
            since_refresh++;
        }
        nWSR = iter;
        return rcode;
    }

    // solved: ONE step of iterative refinement on the final KKT system with residuals from the data, multipliers of the fixed
    // variables from stationarity, A x of the final iterate; returns the objective 0.5 x'Hx + gN'x (refine = false: A x, objective)
    __device__ __forceinline__ double finish(bool refine) {
        double gyx[MV], axx[MC], hxx[MV];
        if (refine) {
            exact_products(gyx, axx, hxx);
            double in[N], o[N];
            SFOR(l, MV, in[l] = (l < nV && sv[l] == 0) ? -(gN[l] - gyx[l]) : 0.0;);
            SFOR(i, MC, in[MV + i] = sc[i] != 0 ? (sc[i] == 1 ? cupN[i] : cloN[i]) - axx[i] : 0.0;);
            g_times(in, o);
            SFOR(l, MV, if (l < nV && sv[l] == 0) xv[l] += o[l];);
            SFOR(i, MC, if (sc[i] != 0) yc[i] -= o[MV + i];);
        }
        exact_products(gyx, axx, hxx);
        double t[MV];
        // (the objective excludes the LP regularisation; mul_alone: a product of its own, as it is behind the select on a run-time nV --
        //  with nV a constant the select folds, and the compiler would contract the product into the sums below: another last bit)
        SFOR(l, MV, if (refine && l < nV) yv[l] = sv[l] != 0 ? gN[l] - gyx[l] : 0.0;
             t[l] = l < nV ? mul_alone(xv[l], fma(0.5, hxx[l] - hreg * xv[l], gN[l])) : 0.0;);
        SFOR(i, MC, ax[i] = i < nC ? axx[i] : 0.0;);
        return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[7] + t[6]) + (t[5] + t[4]));      // (the order of qp_tiny.hip's lane tree)
    }
};

// persistent state of a problem between solves (hot starts): the layout qp_tiny.hip keeps in the problem's state block. This
// kernel WRITES it (KEEP): a hot start on new vectors runs on the 8-lane kernel, which continues from what either kernel left, or in
// the WARM builds of level 2 here, which read 20 doubles of its tail (take_limits) and never its tableau;
// a hot start with new matrices and a warm re-initialisation read no stored tableau and run there too, or in the WARM builds here:
// [N x N tableau, both triangles][6 fields x 8 variable slots: x g lo up gy y][4 fields x 8 constraint slots: A x, loA, upA, y][G_ll (8)]
// [G_{8+l,8+l} (8)][ints: sv (8), sc (8), status, masks, magic, pivots since the tableau was built from the data]
// (Hot starts that READ this block were built for this mapping once -- state block -> LDS -> registers, every mode in one kernel --
// and were 2-3 x slower than the 8-lane kernel (0.23 / 0.25 ms against 0.097 / 0.13 ms for 65 536 members): 1.6 KB of state per
// problem each way with one wave per SIMD to hide the round trips, 100-144 KB of code, 340-960 registers spilled to scratch. Removed;
// the WARM builds take 26 values per problem from the result pools instead: DESIGN.md 4.3b.)
constexpr int LANE_TINY_MAGIC = 0x7a11e;

// the kernel's body; SHV x SHC: the shape as constants (lane_qp_shape_kernel), or -1: run-time words (lane_qp_kernel)
// WARM: the build for hot starts with new matrices (mode 2) and warm re-initialisations (mode 3) of a batch that keeps its state.
// Neither reads the stored tableau: the guess is x, y and the working sets (mode 2: the batch's own result pools, dense and
// member-major, 26 values for 8 x 2; mode 3: the warm-start pools), the tableau is built for it from the new matrices by pivots
// (setup_warm), and the homotopy is the cold start's. The call shape is the launch's (QPPools::guess_mode) or, with
// QPPools::member_mode, a lane's own word: < 0 the member is not in the launch, 0 cold, 2, 3 (level 1: never 1, rsqp_plan_lane_fits).
// WARM == 2 also carries the word 1, the hot start on new vectors: the guess of mode 2 plus the limits the member's last homotopy
// ended on, from the tail of its state block (take_limits); the tableau is built by pivots for the stored working set from the
// unchanged matrices, the auxiliary limits are the stored ones, and the homotopy runs from them to the new targets (its relaxation
// pass for a side that was infinite and is finite now included). The state write is the one of every call shape: the tableau it
// built goes out with the working set it belongs to, whether or not the member changed it
template <int MC, bool KEEP, bool UNI, int HB, int SHV, int SHC, int WARM = 0>
__device__ __forceinline__ void lane_qp_body(const QPPools &P, int nq, int maxWSR) {
    static_assert(UNI || HB == MV, "the block build serves one-pattern batches");
    static_assert(!WARM || (KEEP && SHV < 0), "a hot start continues a batch that keeps its state; no full-shape build of it");
    // the pivots' chunks (sweep_triangle): 14 entries for pivot1, 6 for pivot2 (which holds 40 doubles of vectors beside them) in
    // the headline build; with the state kept or H in full every chunking tried spilled vector registers, so those go pair by pair
    constexpr bool CHUNKS = !KEEP && HB < MV;
    // the ratio test's arms per role (LaneT::ROLES): the same build only -- in the two builds that keep the state with H in full the
    // arms spilled vector registers to scratch memory
    constexpr bool ROLES = CHUNKS;
    // staging in dependency order (stage_matrices): the builds with H as its block -- both compile without a vector register spilled
    // and without scratch memory; the others keep their text, their LDS block and their device code. The results ahead of the
    // objective (below): the headline build only, a kept state keeps its order
    constexpr bool ORDERED = HB < MV;
    // the wave's votes (LaneT::VOTE): the full-shape build without kept state -- the step by `done`, and change() by kinds 3 (both
    // changes of every headline member: a constraint enters by an exchange with a bound) and 2. Kinds 4 and 1 stay on the text by
    // lane: 14 KB more of it, and the headline batch could not tell the builds apart
    // The exchange's votes (bits 5 .. 8, change_exchange() in place of change<3>()): RSQP_LANE_XVOTE, the sums and li
    constexpr int VOTE = (CHUNKS && SHV >= 0) ? (1 | 1 << 2 | 1 << 3 | RSQP_LANE_XVOTE << 5) : 0;
    typedef LaneT<MC, HB, CHUNKS ? 14 : 2, CHUNKS ? 6 : 2, ROLES, SHV, SHC, VOTE, WARM> ENG;
    constexpr int N = ENG::N;
    // (+ the staging table: 32 ints; in the ordered build it lies in the first of the spare slots the vectors pass through)
    constexpr int LDSD = (ENG::NT + ENG::NA) * WL + (ORDERED ? ENG::SPV * WL : 16);
    static_assert(LDSD * sizeof(double) <= 40960, "four waves per CU");
    __shared__ __attribute__((aligned(16))) double lds[LDSD];
    ldouble *T = (ldouble *)lds;
    const int lane = (int)threadIdx.x;
    const int q0 = (int)blockIdx.x * WL, q = q0 + lane;
    const int nqw = nq - q0 < WL ? nq - q0 : WL;
    ENG E;
    E.G = T + lane; E.K = E.G + ENG::NT * WL;
    E.nV = P.uniV; E.nC = P.uniC; E.hreg = P.uni_hreg;
    E.nflips = 0; E.infeasible = E.unbounded = 0; E.status = QPS_NOTINITIALISED; E.fmask = E.amask = 0; E.since_refresh = 0;
    const int nV = E.nV, nC = E.nC;
#ifdef RSQP_STAMPS
    E.tlast = clock64();
    long long &tlast = E.tlast;
#endif
    int rcode = RET_OK, nWSR = 0, setup_pivots = 0;
    bool run = true;                       // WARM: my member is in the launch
    unsigned long long live = ~0ull;       // ... and bit j: the member of lane j is (the wave's stores leave the others' ranges alone)
    unsigned long long live_state = ~0ull; // ... and writes its state block (WARM level 2: not a hot start that found its new bounds inconsistent)
    if constexpr (WARM != 0) {
        // my call shape (a lane beyond the batch runs beside the last member, as everywhere). A member without a solved or stopped
        // QP behind it has nothing to continue from: cold, as qp_tiny.hip decides from the state word (the status pool holds the same)
        const int qown = q0 + (lane < nqw ? lane : nqw - 1);
        int mode = P.member_mode ? P.member_mode[qown] : P.guess_mode;
        run = mode >= 0;
        live = live_state = __builtin_amdgcn_ballot_w64(run);
        const int prev = (mode == 2 || (WARM >= 2 && mode == 1)) ? P.status[qown] : QPS_SOLVED;       // (asked for here, looked at behind the staging)
        // staging as in the cold builds; the guess behind it, through the tableau's slots (setup_warm builds the tableau again)
        typename ENG::Inflight F;
        bool early = false;
        if constexpr (ORDERED) early = E.ordered_wave(P, nqw);
        if constexpr (ORDERED) { if (early) { E.stage_matrices(P, q0, lane, T, F); E.take_bounds(T, lane, F); } }
        if (!early) E.template stage<UNI>(P, q0, lane, nqw, T);
        E.take_guess(P, q0, lane, nqw, T);
        // level 2, a wave with a hot start on new vectors among its members: the stored limits behind the guess (take_limits)
        if constexpr (WARM >= 2) {
            if (__builtin_amdgcn_ballot_w64(mode == 1) != 0) E.take_limits(P.state + (long long)q0 * P.uni_state, P.uni_state, lane, nqw, T);
        }
        if ((mode == 2 || (WARM >= 2 && mode == 1)) && prev % 100 == QPS_NOTINITIALISED) mode = 0;
        const bool hot = WARM >= 2 && mode == 1;
        LSTAMP(0);
        const bool bad = run && E.bounds_inconsistent();
        if constexpr (WARM >= 2) live_state = live & ~__builtin_amdgcn_ballot_w64(bad && hot);
        if (bad || !run) {
            // qpOASES areBoundsConsistent: infeasible before any change. A hot start keeps the stored iterate, an init reports the
            // zero iterate and the empty working set (qp_tiny.hip). A member that sits out: zeros, of which nothing is stored
            // (a hot start on new vectors keeps its state block as well, byte for byte, and the status word it holds: live_state)
            if (bad) { E.infeasible = 1; rcode = RET_INFEASIBLE; }
            if (mode != 2 && !hot) {
                SFOR(l, MV, E.xv[l] = 0.0; E.yv[l] = 0.0; E.sv[l] = 0;);
                SFOR(i, MC, E.yc[i] = 0.0; E.sc[i] = 0;);
            }
            if (hot) E.status = prev % 100;
            SFOR(l, MV, E.g[l] = E.gy[l] = 0.0; E.lo[l] = E.up[l] = 0.0;);
            SFOR(i, MC, E.ax[i] = 0.0; E.loA[i] = E.upA[i] = 0.0;);
            E.g_from_K();
        } else {
            // ONE text of the set-up: the guess of the call shape first, the cold start as the fallback when the guess has no positive
            // definite reduced Hessian (and for the cold members of the launch)
            bool hx = mode == 2 || hot || (mode == 3 && P.guess_x != nullptr), hy = mode == 2 || hot || (mode == 3 && P.guess_y != nullptr);
            bool hg = mode == 2 || hot || (mode == 3 && P.guess_sb != nullptr), hc = mode == 2 || hot, ht = hot;
            bool ok = false;
            for (int attempt = 0; attempt < 2 && !ok; attempt++) {
                ok = E.setup_warm(hx, hy, hg, hc, P.reinit_from_y0 != 0, ht);
                hx = hy = hg = hc = ht = false;
            }
            setup_pivots = E.nFR() + E.nAC();
            if (!ok) rcode = RET_SETUP_FAILED;
        }
        LSTAMP(1);
        if constexpr (ORDERED) { if (early) E.take_g(T, lane, F); }
        if (run && !bad && rcode == RET_OK) rcode = E.homotopy(maxWSR, nWSR);
        LSTAMP(2);
    } else if constexpr (ORDERED) {
        // a full wave of aligned pools: the tableau from A and H while the vectors arrive, the set-up from the bounds while g
        // arrives. The passes of the vectors through LDS are the whole wave's work, so the lanes split (inconsistent bounds,
        // free-variable pivots) only between them
        typename ENG::Inflight F;
        const bool early = E.ordered_wave(P, nqw);
        if (early) { E.stage_matrices(P, q0, lane, T, F); E.take_bounds(T, lane, F); }
        else E.template stage<UNI>(P, q0, lane, nqw, T);
        LSTAMP(0);
        const bool bad = E.bounds_inconsistent();
        bool ok = true;
        if (bad) {
            E.infeasible = 1;
            rcode = RET_INFEASIBLE;
            SFOR(l, MV, E.xv[l] = 0.0; E.yv[l] = 0.0; E.sv[l] = -1; E.g[l] = E.gy[l] = 0.0; E.lo[l] = E.up[l] = 0.0;);
            SFOR(i, MC, E.yc[i] = 0.0; E.sc[i] = 0; E.ax[i] = 0.0; E.loA[i] = E.upA[i] = 0.0;);
            if (!early) E.g_from_K();         // (early: nothing has touched the tableau since it was built)
        } else ok = E.setup_cold(early);
        LSTAMP(1);
        if (early) E.take_g(T, lane, F);
        if (!bad) {
            setup_pivots = E.nFR() + E.nAC();
            if (!ok) rcode = RET_SETUP_FAILED;
            else rcode = E.homotopy(maxWSR, nWSR);
            LSTAMP(2);
        }
    } else {
    E.template stage<UNI>(P, q0, lane, nqw, T);
    LSTAMP(0);
    if (E.bounds_inconsistent()) {
        // qpOASES areBoundsConsistent: infeasible before any change
        E.infeasible = 1;
        rcode = RET_INFEASIBLE;
        SFOR(l, MV, E.xv[l] = 0.0; E.yv[l] = 0.0; E.sv[l] = -1; E.g[l] = E.gy[l] = 0.0; E.lo[l] = E.up[l] = 0.0;);
        SFOR(i, MC, E.yc[i] = 0.0; E.sc[i] = 0; E.ax[i] = 0.0; E.loA[i] = E.upA[i] = 0.0;);
        E.g_from_K();
    } else {
        const bool ok = E.setup_cold();
        LSTAMP(1);
        setup_pivots = E.nFR() + E.nAC();
        if (!ok) rcode = RET_SETUP_FAILED;
        else rcode = E.homotopy(maxWSR, nWSR);
        LSTAMP(2);
    }
    }
    // (the refinement step repairs what the update-only tableau accumulates: with at most 4 pivots there is nothing to repair yet)
    const int pivots = setup_pivots + nWSR;
    const bool refine = run && rcode == RET_OK && pivots > 4;
    // no lane of the wave refines (the headline's members make two pivots): finish() then changes neither x, y nor the working
    // sets, and reads A's dense copy, H's registers and the state, not the slots the results pass through -- the results' stores go
    // out first and the products and the objective run under them. One lane that refines keeps the order for its whole wave
    bool results_first = false;
    if constexpr (ORDERED && !KEEP) results_first = __builtin_amdgcn_ballot_w64(refine) == 0;
    double obj = 0.0;
    if (!results_first) obj = E.finish(refine);
    LSTAMP(3);
    // what a full wave stores write-through (RSQP_LANE_WT)
    constexpr bool WTR = (RSQP_LANE_WT & 1) != 0;
    constexpr bool WTS = (RSQP_LANE_WT & 6) != 0 || (RSQP_LANE_NOSTORE & 2) != 0;
    if constexpr (KEEP) {
        // ---- the state first (its tableau part IS the LDS slots the rest is about to pass through)
        double *sbase = P.state + (long long)q0 * P.uni_state;
        double dg[N];
        SFOR(k, N, dg[k] = E.G[tri(k, k) * WL];);
        // (a full wave, every member in the launch: write-through by the wave's run of the pool; any other wave masks its stores)
        const bool full_state = nqw == WL && (!WARM || live_state == ~0ull) && (((size_t)P.state | (size_t)(P.uni_state << 3)) & 15) == 0;
#define BYFULL(...) do { if (WTS && full_state) { constexpr bool FULL = true; __VA_ARGS__ } else { constexpr bool FULL = false; __VA_ARGS__ } } while (0)
        E.wave_sync();
        BYFULL(E.template state_put_tableau<FULL>(sbase, P.uni_state, nqw, lane, T, live_state););
        E.wave_sync();
        E.template tail_put_half<0>(E.G, dg, pivots);
        E.wave_sync();
        BYFULL(E.template state_put_tail_half<FULL>(sbase, P.uni_state, nqw, lane, T, 0, live_state););
        E.wave_sync();
        E.template tail_put_half<1>(E.G, dg, pivots);
        E.wave_sync();
        BYFULL(E.template state_put_tail_half<FULL>(sbase, P.uni_state, nqw, lane, T, 1, live_state););
        LSTAMP(15);
    }
    // ---- results (x, y = [bounds; constraints], working set, status / nWSR / objective): the member-major vectors leave through the
    // wave's LDS block like the inputs came (a lane storing its own problem's 8-byte pieces touched 64 lines per instruction)
    {
        typedef __attribute__((address_space(3))) int lint;
        constexpr int SX = 0, SY = MV, SB = 2 * MV + MC, SW = 3 * MV + MC;          // slots: x | y | ws_b | ws_c (<= 3 MV + 2 MC <= NT)
        E.wave_sync();
        SFOR(l, MV, E.G[(SX + l) * WL] = E.xv[l]; ((lint *)(E.G + (SB + l) * WL))[0] = E.sv[l];);
        // y of a problem = [nV bound multipliers; nC constraint multipliers]: its slots follow the problem's own nV
        SFOR(l, MV, if (l < nV) E.G[(SY + l) * WL] = E.yv[l];);
        SFOR(i, MC, if (i < nC) E.G[(SY + nV + i) * WL] = E.yc[i]; ((lint *)(E.G + (SW + i) * WL))[0] = E.sc[i];);
        E.wave_sync();
        // (WARM: a wave with a member that is not in the launch stores element by element, each element if its member is in)
        if (nqw == WL && (!WARM || live == ~0ull) && (((size_t)P.x | (size_t)P.y | (size_t)P.ws_b | (size_t)P.ws_c) & 15) == 0) {
            // (a full wave: 16 bytes per lane, as it was staged)
            const int pp = ENG::pair_of(lane);
            BYPARITY(nV, E.template put_pairs<MV, EV, WTR>(P.x + (long long)q0 * nV, nV, pp, T, SX););
            BYPARITY(nV + nC, E.template put_pairs<MV + MC, EV, WTR>(P.y + (long long)q0 * (nV + nC), nV + nC, pp, T, SY););
            E.template put_quads<MV, WTR>(P.ws_b + (long long)q0 * nV, nV, lane, T, SB);
            if (nC > 0) E.template put_quads<MC, WTR>(P.ws_c + (long long)q0 * nC, nC, lane, T, SW);
        } else {
        E.template put_block<MV>(P.x + (long long)q0 * nV, nV, nqw * nV, lane, T, SX, live);
        E.template put_block<MV + MC>(P.y + (long long)q0 * (nV + nC), nV + nC, nqw * (nV + nC), lane, T, SY, live);
        E.template put_block<MV>(P.ws_b + (long long)q0 * nV, nV, nqw * nV, lane, T, SB, live);
        if (nC > 0) E.template put_block<MC>(P.ws_c + (long long)q0 * nC, nC, nqw * nC, lane, T, SW, live);
        }
    }
    if constexpr (ORDERED) {
        LSTAMP(19);
        if (results_first) obj = E.finish(false);
    }
    if (q < nq && run) {
        const int st = E.status;
#if RSQP_LANE_NOSTORE & 1
        if (nqw == WL) {
            const WaveRun<false, true> ws(P.status + q0, 0), wr(P.ret + q0, 0), wn(P.nwsr + q0, 0), wf(P.nflips + q0, 0), wo(P.obj + q0, 0);
            ws.put4(lane, E.infeasible ? 100 + st : (E.unbounded ? 200 + st : st));
            wr.put4(lane, rcode); wn.put4(lane, nWSR); wf.put4(lane, E.nflips); wo.put8(lane, obj);
        } else
#endif
        {
        P.status[q] = E.infeasible ? 100 + st : (E.unbounded ? 200 + st : st);
        P.ret[q] = rcode; P.nwsr[q] = nWSR; P.nflips[q] = E.nflips; P.obj[q] = obj;
        }
    }
    LSTAMP(4);
}

template <int MC, bool KEEP, bool UNI, int HB, int WARM = 0>
__global__ void __launch_bounds__(WL) lane_qp_kernel(QPPools P, int nq, int maxWSR) {
    lane_qp_body<MC, KEEP, UNI, HB, -1, -1, WARM>(P, nq, maxWSR);
}
// the full-shape build: every member NV x NC (the plan's word, SmallPlan::lane_shape); the ragged last wave of such a batch runs it too
template <int MC, bool KEEP, bool UNI, int HB, int NV, int NC>
__global__ void __launch_bounds__(WL) lane_qp_shape_kernel(QPPools P, int nq, int maxWSR) {
    lane_qp_body<MC, KEEP, UNI, HB, NV, NC>(P, nq, maxWSR);
}

}  // namespace

// the plan's build (rsqp_small_plan.h): state kept or not; one pattern or patterns of their own; H as its leading 4 x 4 block or in full;
// SmallPlan::lane_shape: the full-shape build of the one-pattern block builds (8 x 2 as constants), or 0
hipError_t rsqp_launch_lane_qp(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream) {
    static_assert(MV == 8 && WL == kLaneBlock, "rsqp_plan_lane_fits");
    const dim3 grid(pl.grid), block(pl.block);
    if (pl.lane_shape == 8 * 256 + 2 && pl.mc == 2 && pl.uni == 1 && pl.hb == 4) {
        if (pl.keep) hipLaunchKernelGGL((lane_qp_shape_kernel<2, true, true, 4, 8, 2>), grid, block, 0, stream, p, nq, maxWSR);
        else hipLaunchKernelGGL((lane_qp_shape_kernel<2, false, true, 4, 8, 2>), grid, block, 0, stream, p, nq, maxWSR);
        return hipGetLastError();
    }
    if (pl.lane_shape != 0) return hipErrorInvalidValue;
    if (pl.lane_warm && pl.lane_hot) {
        // ... and hot starts on new vectors, alone or among the members' own words (rsqp_plan_lane_fits; rsqp_batch_set_lane_hot)
        switch (pl.mc * 1000 + pl.keep * 100 + pl.uni * 10 + pl.hb) {
        case 2114: hipLaunchKernelGGL((lane_qp_kernel<2, true, true, 4, 2>), grid, block, 0, stream, p, nq, maxWSR); break;
        case 2118: hipLaunchKernelGGL((lane_qp_kernel<2, true, true, 8, 2>), grid, block, 0, stream, p, nq, maxWSR); break;
        case 2108: hipLaunchKernelGGL((lane_qp_kernel<2, true, false, 8, 2>), grid, block, 0, stream, p, nq, maxWSR); break;
        default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    if (pl.lane_hot) return hipErrorInvalidValue;
    if (pl.lane_warm) {
        // hot starts with new matrices / warm re-initialisations (rsqp_plan_lane_fits): the builds that keep the state
        switch (pl.mc * 1000 + pl.keep * 100 + pl.uni * 10 + pl.hb) {
        case 2114: hipLaunchKernelGGL((lane_qp_kernel<2, true, true, 4, 1>), grid, block, 0, stream, p, nq, maxWSR); break;
        case 2118: hipLaunchKernelGGL((lane_qp_kernel<2, true, true, 8, 1>), grid, block, 0, stream, p, nq, maxWSR); break;
        case 2108: hipLaunchKernelGGL((lane_qp_kernel<2, true, false, 8, 1>), grid, block, 0, stream, p, nq, maxWSR); break;
        default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (pl.mc * 1000 + pl.keep * 100 + pl.uni * 10 + pl.hb) {
    case 2114: hipLaunchKernelGGL((lane_qp_kernel<2, true, true, 4>), grid, block, 0, stream, p, nq, maxWSR); break;
    case 2014: hipLaunchKernelGGL((lane_qp_kernel<2, false, true, 4>), grid, block, 0, stream, p, nq, maxWSR); break;
    case 2118: hipLaunchKernelGGL((lane_qp_kernel<2, true, true, 8>), grid, block, 0, stream, p, nq, maxWSR); break;
    case 2018: hipLaunchKernelGGL((lane_qp_kernel<2, false, true, 8>), grid, block, 0, stream, p, nq, maxWSR); break;
    case 2108: hipLaunchKernelGGL((lane_qp_kernel<2, true, false, 8>), grid, block, 0, stream, p, nq, maxWSR); break;
    case 2008: hipLaunchKernelGGL((lane_qp_kernel<2, false, false, 8>), grid, block, 0, stream, p, nq, maxWSR); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
