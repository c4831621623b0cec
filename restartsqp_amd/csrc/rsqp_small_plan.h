// rsqp_small_plan.h -- which kernel a launch of LDS-scale (or HBM-resident) QPs runs, decided ONCE: rsqp_plan_small_launch is a pure
// host function (no HIP call, no environment, no state), the callers (rsqp_solve, launch_batch of rsqp_batch.hip) compute the plan
// of a launch, read from it what they keep on record (state family, reported kernel, mode after the family-change rule) and hand it to
// rsqp_launch_small_qp, which maps it to an instantiation and launches. rsqp_describe_small_launch (rsqp_hip.h) shows a plan without
// a GPU; tests/golden/small_launch_plans.json pins both sides of every threshold below.
#pragma once
#include "rsqp_internal.h"

// what the rules read of a launch's QPPools (rsqp_small_facts), plus whose hot-start state the caller holds
struct SmallFacts {
    int tiny_ok, uniV, uniC, uni_pat, desc, keep_state;
    int skip_mark;        // the CALLER remembers that a launch kept no state (batches: rsqp_batch::state_engine = -1; QPPools::skip_mark)
    int member_mode, done_flag, cert_out, x0, y0, guess_b;      // present or not
    int lane_hblock, uni_hreg;                                  // uni_hreg: != 0.0 or not
    int hbm;              // the batch is HBM-resident (images beyond the LDS of a CU, qp_small_hbm.hip)
    int state_engine;     // family that wrote the stored hot-start state(s): 0 / 1 / 3 as SmallPlan::state_family, < 0 none or mixed
    // the CALLER's word (launch_batch of rsqp_batch.hip; 0 from rsqp_small_facts and rsqp_describe_small_launch): this launch may take a
    // WARM build of the lane-per-problem kernel -- the batch's switch is on (rsqp_batch_set_lane_warm), its result pools hold its
    // own last answer, nothing is handed over, and a launch with member_mode carries no member whose word is 1
    int lane_warm;
    // the CALLER's word beside it (rsqp_batch_set_lane_hot; read only where lane_warm is set): a hot start on new vectors (mode 1), and
    // a launch with member_mode whatever its members' words say, may take the builds that carry the word 1 as well
    int lane_hot;
};
inline SmallFacts rsqp_small_facts(const QPPools &p, bool hbm, int state_engine) {
    return SmallFacts{p.tiny_ok, p.uniV, p.uniC, p.uni_pat, p.desc != nullptr, p.keep_state, p.skip_mark, p.member_mode != nullptr,
                      p.done_flag != nullptr, p.cert_out != nullptr, p.x0 != nullptr, p.y0 != nullptr, p.guess_b != nullptr,
                      p.lane_hblock, p.uni_hreg != 0.0, hbm ? 1 : 0, state_engine};
}

struct SmallPlan {
    int invalid = 0;      // no kernel serves the launch (hipErrorInvalidValue)
    int empty = 0;        // nq <= 0: nothing to launch
    int family = 0;       // as rsqp_batch_get_last_kernel: 0 LDS-resident null-space, 1 8-lane register tableau (qp_tiny.hip),
                          //   2 lane per problem (qp_lane.hip), 3 HBM-resident null-space (qp_small_hbm.hip)
    // ---- the instantiation. Null-space kernels: small_qp_kernel<ENG<L, MAT_LDS[, true]>, L, MAT_LDS, W, SHAPE> / small_qph_kernel<ENG, L, W>
    int engine = 0;       // 0 Engine (Givens / TQ), 1 EngineX (explicit inverses)
    int L = 0, mat_lds = 0, W = 0, shape = 0;       // shape = NVC * 256 + NCC of the compile-time shape build, else 0
    int waves = 0;        // waves per SIMD asked for (W is what the product build instantiates; tools/small_experiment.sh builds more)
    // tiny_qp_kernel<mc, W>; lane_qp_kernel<mc, keep, uni, hb>
    int mc = 0, keep = 0, uni = 0, hb = 0;
    int lane_warm = 0;    // lane_qp_kernel<mc, keep, uni, hb, WARM = true>: a hot start with new matrices / a warm re-initialisation (mode 2 / 3, or
                          //   per-member modes 0 / 2 / 3) on the lane-per-problem kernel; the launcher sets QPPools::guess_* (not among the exported words)
    int lane_hot = 0;     // beside lane_warm: lane_qp_kernel<mc, keep, uni, hb, WARM = 2>, which also carries a hot start on new vectors (mode 1, or a
                          //   member's word 1): the guess plus the stored limits of the state blocks' tails (not among the exported words)
    int lane_shape = 0;   // lane_qp_shape_kernel<mc, keep, uni, hb, NV, NC>: NV * 256 + NC of the lane kernel's full-shape build, else 0 (not
                          //   among the exported words: the build FAMILY stays (keep, uni, hb); rsqp_batch_get_lane_shape reports it)
    int first = 0;       // the mid-size tableau kernel goes first (qp_small_g.h): 1 small_qpg_kernel<3, 1, 9, 4>, 2 <2, 2, 8, 8>; 0 no
    unsigned grid = 0, block = 0;       // of the family's kernel (the tableau kernel that goes first: nq blocks of 256)
    long long lds = 0;    // dynamic LDS bytes
    int stride = 0;       // LDS bytes of one problem (null-space kernels)
    int mode = 0;         // the mode to launch with: the caller's, or cold after the family-change rule
    int state_family = 0; // layout this launch leaves in the state block: 0 LDS-resident kernels, 1 qp_tiny.hip's (families 1 and 2), 3 HBM
    int skip_mark = 0;    // QPPools::skip_mark of the launch: no state kept and no mark left, the caller's record says "no state"
};

constexpr long long kSmallMaxLds = 160 * 1024;
constexpr int kTinyBlock = 256, kLaneBlock = 64;     // threads per workgroup of qp_tiny.hip (8 per problem) / qp_lane.hip (1 per problem)
inline long long rsqp_align16(long long v) { return (v + 15) & ~15LL; }
// the hs071-scale tableau kernels' layout of a state block (qp_tiny.hip, written by qp_lane.hip as well): tiny_state_doubles<MC>()
// doubles -- the (8 + MC)^2 tableau, 6 fields x 8 variable slots, 4 fields x 8 constraint slots, the two diagonals -- then the ints:
// sv (8), sc (8), status [16], masks [17], TINY_MAGIC [18], pivots [19]. A block whose ints say TINY_MAGIC and QPS_NOTINITIALISED is
// one no hot start continues from. MC = SmallPlan::mc of the launch
template <int MC> __host__ __device__ __forceinline__ constexpr long long tiny_state_doubles() { return (long long)(8 + MC) * (8 + MC) + 8LL * 6 + 8LL * 4 + 8LL * 2; }
constexpr int TINY_MAGIC = 0x7a11e;

// 1 if the batch shape is served by the register-resident tableau kernel (qp_tiny.hip: at most 8 variables, 8 constraints)
inline int rsqp_plan_tiny_fits(const SmallKnobs &kn, int nVmax, int nCmax) { return !kn.no_tiny && nVmax <= 8 && nCmax <= 8 && nVmax >= 1; }
// 1 when the launch goes to that kernel (or, rsqp_plan_lane_fits, to the lane-per-problem kernel), whose hot-start state has another
// layout than the LDS-resident kernels'
inline int rsqp_plan_is_tiny(const SmallKnobs &kn, const SmallFacts &f, int nVmax, int nCmax) {
    return (kn.engine < 0 && f.tiny_ok && rsqp_plan_tiny_fits(kn, nVmax, nCmax)) ? 1 : 0;
}
// 1 if a launch that is_tiny is served by the lane-per-problem kernel: a cold start of a one-shape batch of at most 8 x 2 with more members
// (16 384) than 8 lanes per problem hold at a time; no certificate / doorbell of a single-QP handle, no warm re-initialisation
// inputs. A batch that keeps its state gets it written in the 8-lane kernel's layout; one that does not leaves no mark either
// (the handle remembers: QPPools::skip_mark).
// 2 (the WARM builds): with the caller's word SmallFacts::lane_warm, a batch that keeps its state also brings its hot starts with new
// matrices (mode 2), its warm re-initialisations (mode 3, whatever inputs are present) and launches with per-member modes. A hot
// start on new vectors (mode 1) continues from the stored tableau and stays on the 8-lane kernel, unless the caller says
// SmallFacts::lane_hot as well:
// 3 (the WARM builds of level 2): a hot start on new vectors, or a launch with per-member modes one of whose words may be 1
inline int rsqp_plan_lane_fits(const SmallKnobs &kn, const SmallFacts &f, int skip_mark, int nq, int nVmax, int nCmax, int mode) {
    if (kn.lane == 0) return 0;
    // one shape (every member nV x nC); one sparsity pattern (member 0's arrays serve all) or patterns of their own (each lane walks its own)
    if (!(f.uniV >= 1 && f.uniV <= 8 && f.uniC >= 0 && f.uniC <= 2 && nVmax <= 8 && nCmax <= 2 && (f.uni_pat || f.desc))) return 0;
    const bool hot = f.lane_warm && f.lane_hot && f.keep_state && (f.member_mode || mode == 1);
    const bool warm = hot || (f.lane_warm && f.keep_state && (f.member_mode || mode == 2 || mode == 3));
    if (!warm && (mode != 0 || f.member_mode || f.x0 || f.y0 || f.guess_b)) return 0;
    if ((!f.keep_state && !skip_mark) || f.cert_out || f.done_flag || !f.tiny_ok) return 0;
    // (measured, tools/lane_vs_tiny_sweep.py: a launch of this kernel takes 36 us up to 16 384 problems and 43 us at 65 536 -- one
    //  round of waves either way; the 8-lane kernel holds 16 384 problems at a time: 21 us up to 8 192, 26 us at 16 384, 40 us at
    //  20 480 (second round), 47 us at 32 768, 90 us at 65 536. With the state kept, 65 536 members: 0.075 against 0.132 ms)
    return nq >= (kn.lane > 0 ? kn.lane : 16385) ? (hot ? 3 : (warm ? 2 : 1)) : 0;
}

// doubles / 16-bit integers of the LDS image of a formulation, as Engine<L, ML, REGV>::image_doubles (qp_small_engine.h) and
// EngineX<L, ML>::image_doubles (qp_small_x.h) count them (every build of qp_small.hip compares the two once, at its first launch)
inline long long rsqp_plan_image_doubles(int engine, bool regv, int nV, int nC) {
    const long long ld = rsqp_ld(nV), sT = nV < nC ? nV : nC;
    if (engine == 1) return 2 * ld * nV + sT * ld + 19LL * nV + 9LL * nC + 2LL * (nV + nC) + 16 + 4 * (sT + 2);
    return ld * nV + (long long)nV * (nV + 3) / 2 + sT * ld + (regv ? 9LL : 12LL) * nV + 8LL * nC + 2LL * (nV + nC);
}
inline long long rsqp_plan_image_ints(int engine, int nV, int nC) { return nV + 3LL * nC + (engine == 1 ? 8 : 4); }

inline SmallPlan rsqp_plan_small_launch(const SmallKnobs &kn, const SmallFacts &f, int nq, int nVmax, int nCmax, long long mat_bytes_max, int mode) {
    SmallPlan pl;
    const int tiny = rsqp_plan_is_tiny(kn, f, nVmax, nCmax);
    pl.state_family = f.hbm ? 3 : tiny;
    // the kernel families keep different layouts in the same state block: a hot start on another family's state starts cold
    // (per-member modes: the plan kernel of rsqp_batch_optimize.hip was told, and `mode` is not read)
    if (!f.member_mode && (mode == 1 || mode == 2) && f.state_engine != pl.state_family) mode = 0;
    pl.mode = mode;
    // a cold-start-only batch on the tableau kernel keeps no state and leaves no mark: the caller remembers it instead
    pl.skip_mark = (f.skip_mark && !f.hbm && tiny && !f.keep_state) ? 1 : 0;
    // formulation: 0 = Givens / TQ (Engine), 1 = explicit inverses (EngineX, qp_small_x.h), which keeps
    // DENSE copies of A and H in LDS. Measured per shape on the 512-QP hs0xx batch (ms, TQ vs explicit):
    // 5x1 0.14 / 0.16, 8x2 0.045 / 0.051, 8x3 0.25 / 0.21, 12x4 0.49 / 0.42, 16x6 0.73 / 0.55,
    // 23x6 1.26 / 1.01, 37x14 2.57 / 1.51, 69x28 10.8 / 4.1 -- the chains of the TQ form grow with nZ.
    const int forcedE = kn.engine;
    const int eng = forcedE == 0 || forcedE == 1 ? forcedE : (nVmax > 8 ? 1 : 0);
    pl.engine = eng;
    if (f.hbm) {
        // one workgroup per problem, its image in HBM: four waves per problem and dense copies of A and H in the slice (explicit
        // inverses); the Givens / TQ engine has a one-wave build only, sparse matrices from global memory
        pl.family = 3;
        if (nq <= 0) { pl.empty = 1; return pl; }
        if (!(nVmax >= 1 && nCmax >= 0 && nVmax <= RSQP_HBM_MAX_V && nCmax <= RSQP_HBM_MAX_C) || mode < 0 || mode > 3) { pl.invalid = 1; return pl; }
        pl.L = eng == 1 ? 256 : 64; pl.mat_lds = eng == 1 ? 1 : 0; pl.W = pl.waves = eng == 1 ? 1 : 2;
        pl.grid = (unsigned)nq; pl.block = (unsigned)pl.L;
        return pl;
    }
    pl.family = tiny;
    if (nq <= 0) { pl.empty = 1; return pl; }
    if (rsqp_align16(rsqp_image_bytes(nVmax, nCmax)) > kSmallMaxLds) { pl.invalid = 1; return pl; }
    // hs071-scale problems: the register-resident tableau kernel (qp_tiny.hip) serves every call shape
    if (const int lane_fit = tiny ? rsqp_plan_lane_fits(kn, f, pl.skip_mark, nq, nVmax, nCmax, mode) : 0) {
        // the build: H kept as its leading 4 x 4 block, or the full triangle. The block build needs what only a one-pattern launch
        // without regularisation can promise (QPPools::lane_hblock: the host's word on the pattern)
        pl.family = 2;
        pl.mc = 2; pl.keep = f.keep_state ? 1 : 0;
        pl.hb = (f.uni_pat && f.lane_hblock == 4 && !f.uni_hreg) ? 4 : 8;
        pl.uni = (pl.hb == 4 || f.uni_pat) ? 1 : 0;
        // the full shape of that kernel, one pattern, H as its block: the build with nV and nC as constants (RSQP_LANE_SHAPE=0: never)
        pl.lane_warm = lane_fit >= 2 ? 1 : 0; pl.lane_hot = lane_fit == 3 ? 1 : 0;
        if (!pl.lane_warm && kn.lane_shape != 0 && f.uniV == 8 && f.uniC == 2 && f.uni_pat && pl.hb == 4) pl.lane_shape = 8 * 256 + 2;
        pl.grid = (unsigned)((nq + kLaneBlock - 1) / kLaneBlock); pl.block = kLaneBlock;
        return pl;
    }
    if (tiny) {
        // (launches of at most one workgroup per CU -- the single QP of an SQP iteration above all -- get the builds for ONE wave per SIMD:
        //  268 instead of 256 registers, none spilled to scratch, whose round trips sit in the chain of a lone wave: cold solve of the hs071 QP 30.5 ->
        //  28.8 us through the Python loop, the solveQP replay 23.0 -> 22.6 us through the C++ boundary, batches of up to 8 192 QPs 3 % faster)
        pl.mc = nCmax <= 2 ? 2 : (nCmax <= 4 ? 4 : 8);
        pl.W = pl.waves = (pl.mc == 8 || nq <= 32 * 256) ? 1 : 2;
        pl.grid = (unsigned)((nq + kTinyBlock / 8 - 1) / (kTinyBlock / 8)); pl.block = kTinyBlock;
        return pl;
    }
    if (eng == 1 && mat_bytes_max >= 0) mat_bytes_max = 8LL * ((long long)nVmax * nVmax + (long long)nCmax * nVmax);
    // uniform hs071-scale batches (8 x 2 through the QPhandler formulation; parameter scans of one NLP iterate) run
    // the build with the shape as a compile-time constant and the target vectors in registers (see RegVec)
    const int forcedL = kn.lanes, forcedW = kn.waves;
    const bool shape82 = eng == 0 && f.uniV == 8 && f.uniC == 2 && mat_bytes_max >= 0 &&
                         (forcedL < 0 || forcedL == 8);        // only the 8-lane build has the shape instantiation
    // LDS image of the chosen formulation (the persistent copy in HBM is sized for the larger one)
    const long long imgd = rsqp_plan_image_doubles(eng, shape82, nVmax, nCmax), imgi = rsqp_plan_image_ints(eng, nVmax, nCmax);
    const long long img = (8 * imgd + 2 * imgi + 7) & ~7LL;
    const bool mat_lds = mat_bytes_max >= 0 && rsqp_align16(img + mat_bytes_max) <= kSmallMaxLds;
    // LDS of one problem: image, then its staged matrices, 16-byte granular.
    long long stride = rsqp_align16(img + (mat_lds ? mat_bytes_max : 0));
    // (an odd number of 16-byte units would spread the problems of a wave over the banks, but the LDS is
    // allocated in 512-byte steps and the 8-lane build needs 8 x 2880 = 45 x 512 bytes for 7 workgroups per CU)
    // lanes per problem: the vectors of the engine have nV (+ nC) entries, a wave of 64 lanes is
    // mostly idle on hs0xx-scale problems, so 64 / L of them share a wave. Problems in one wave
    // follow their own control flow (exec masking); the LDS capacity bounds the problems in flight.
    const int nmax = nVmax > nCmax ? nVmax : nCmax;
    int L = nmax <= 8 ? 8 : (nmax <= 16 ? 16 : (nmax <= 32 ? 32 : 64));
    if ((forcedL == 8 || forcedL == 16 || forcedL == 32 || forcedL == 64) && forcedL >= L) L = forcedL;   // never fewer lanes than entries
    if (eng == 1 && L < 16) L = 16;   // the explicit-inverse build has no 8-lane instantiation
    if (!mat_lds) L = 64;
    while (L < 64 && (64 / L) * stride > kSmallMaxLds) L *= 2;
    if (L == 64 && stride > kSmallMaxLds) stride = rsqp_align16(mat_lds ? img + mat_bytes_max : img);
    const bool wide0 = eng == 1 && mat_lds && L == 64 && nVmax > 32;
    bool wide = false;
    // several waves per problem: four (256 lanes, one wave per SIMD). The kernel keeps ~430 values live per lane
    // (256 VGPRs + AGPRs), so an eight-wave build spills 233 of them (measured).
    // With one wave per SIMD every wave instruction costs its full 4+ cycles: the four-wave kernel is bound by the
    // instruction count per wave (~350 per 69 x 69 product stage), not by LDS bandwidth or barriers.
    constexpr int wideL = 256;
    if (wide0 && stride + 8 * wideL <= kSmallMaxLds) { stride += 8 * wideL; wide = true; }   // one double per lane of the wide build
    // bank spread of packed waves: a 32-lane LDS access group holds 32 / L problems, each touching 2 L consecutive
    // banks of the 64 (ds_read_b64: bank = dword address mod 64; stores: 16-lane groups, mod 32). Their images must
    // therefore start 2 L dwords apart modulo 64, i.e. stride = 8 L (mod 256) bytes -- with stride = 0 (mod 256)
    // every vector access of an 8-lane build is a 4-way conflict (measured: 54 % of the LDS-array cycles, LDS busy
    // 73 % of the kernel). The stride is padded to the next such value when that does not cost a resident workgroup.
    if (L < 64) {
        long long s1 = stride;
        while ((s1 & 255) != ((8 * L) & 255)) s1 += 16;
        auto wgs = [&](long long st) { const long long a = (((64 / L) * st) + 511) / 512 * 512; return a > 0 ? kSmallMaxLds / a : 0; };
        if (wgs(s1) == wgs(stride) && (64 / L) * s1 <= kSmallMaxLds) stride = s1;
    }
    const int G = 64 / L;
    // minimum resident waves per SIMD = register budget. One problem per wave keeps the uniform
    // state in SGPRs and runs with 4 waves; packed waves hold that state
    // in VGPRs and need ~230 of them, so they run 2 waves/SIMD without spills (measured on
    // 16 384 hs071-scale QPs: L=16 W=2 159 M solves/s, W=3 142 M, W=4 116 M; L=64 W=6 74 M; with the
    // single-trip loop hints L=16 187 M, and on 65 536 QPs L=8 219 M vs L=16 194 M).
    // Packed builds with W=6 (80 VGPRs, ~180 spilled) returned wrong results and are not built.
    // Neither is the one-problem-per-wave Givens / TQ build with W=6 (Engine<64, true>, once the default for nVmax <= 16): on
    // 1 000 random QPs of at most 8 x 15 under RSQP_SMALL_LANES=64 it returned status "solved" with the right nWSR and a
    // wrong x for 128 members, where its W=3 and W=4 builds and the 16- and 32-lane builds were right on all of them
    // (tests/test_gpu_small_builds.py runs that batch on the two builds that stay). RSQP_SMALL_WAVES=6 falls back to W=4.
    int waves = L == 64 ? 4 : 2;
    if (forcedW >= 2 && forcedW <= 4) waves = forcedW;
    // ---- batches of mid-size problems (cold starts and hot starts on new vectors): the tableau kernel first (qp_small_g.h: 3 phases
    // per working-set change instead of ~50); members it cannot carry (non-symmetric H, LP, undecidable tests) come back with
    // ret == RET_BAIL and are solved by the null-space kernel launched right behind it, which skips everybody else
    // 32 row blocks x 8 column blocks of lanes: up to 72 variables x 32 constraints -- the 69 x 28 class of the hs0xx batch;
    // or up to 64 variables x 64 constraints
    // (only where the null-space kernel would give a problem four waves as well: batches of SMALL problems are throughput-bound
    //  and better served by 16 / 32 lanes per problem, several problems per wave)
    // (per-member modes: the kernel itself leaves the members whose mode it does not carry to the null-space kernel)
    // (kn.no_tiny == 2, the LP launches of a batch: every member would come back with RET_BAIL -- no H, hreg != 0)
    if (forcedE < 0 && kn.no_tiny < 2 && eng == 1 && (nVmax > 32 || nCmax > 32) && (f.member_mode || mode == 0 || mode == 1) && !f.done_flag) {
        if (nVmax <= 72 && nCmax <= 32) pl.first = 1;             // EngineG<3, 1, 9, 4>::MAXV x MAXC
        else if (nVmax <= 64 && nCmax <= 64) pl.first = 2;        // EngineG<2, 2, 8, 8>::MAXV x MAXC
    }
    pl.L = L; pl.mat_lds = mat_lds ? 1 : 0; pl.waves = waves; pl.stride = (int)stride;
    pl.grid = (unsigned)((nq + G - 1) / G); pl.block = 64; pl.lds = G * stride;
    if (eng == 1) {
        if (!mat_lds) pl.W = 3;
        else if (L == 16 || L == 32) pl.W = 2;
        else if (wide) { pl.L = 256; pl.W = 1; pl.block = 256; }   // four waves per problem: the O(n^2) phases split over 256 lanes
        else pl.W = 4;
    } else if (!mat_lds) {
        pl.W = 3;
    } else if (L == 8) {
        // shape build: 160 instead of 253 VGPRs, no per-vector address registers, straight-line vector loops; the
        // occupancy of both builds is capped at 2 waves per SIMD by the LDS a wave of 8 problems needs
        pl.W = 2;
        if (shape82) pl.shape = 8 * 256 + 2;
    } else if (shape82) {
        pl.invalid = 1;    // the image was sized for the 8-lane shape build: never launch another one on it
    } else if (L == 16 || L == 32) {
        pl.W = waves == 3 || waves == 4 ? waves : 2;
    } else {
        pl.W = waves == 3 ? 3 : 4;
    }
    return pl;
}
