// rsqp_internal.h -- shared between the HIP translation units of librsqp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#define RSQP_INFTY 1.0e20           // qpOASES INFTY
#define RSQP_EPS 2.221e-16          // qpOASES EPS
#define RSQP_EPS_DEN (1.0e3 * RSQP_EPS)
#define RSQP_BOUND_RELAXATION 1.0e4
#define RSQP_BOUND_TOLERANCE (1.0e6 * RSQP_EPS)
#define RSQP_EPS_LI 1.0e-9
#define RSQP_EPS_PD_REL 1.0e-10
#define RSQP_EPS_PD_ABS 1.0e-25

// solver status codes kept in the per-problem result record (qpOASES QProblemStatus order)
enum { QPS_NOTINITIALISED = 0, QPS_PREPARINGAUXILIARYQP = 1, QPS_AUXILIARYQPSOLVED = 2,
       QPS_PERFORMINGHOMOTOPY = 3, QPS_HOMOTOPYQPSOLVED = 4, QPS_SOLVED = 5 };
enum { RET_OK = 0, RET_MAX_NWSR = 1, RET_INFEASIBLE = 2, RET_UNBOUNDED = 3, RET_SETUP_FAILED = 4,
       RET_BAIL = 9 };   // internal: the KKT-tableau kernel hands the problem to the null-space kernel (never reported)

// one problem of a batch: sizes and offsets into the pooled device arrays
struct QPDesc {
    int nV, nC;
    int offV, offC;       // vector pools: g/lb/ub/x/ws_b at offV, lbA/ubA/ws_c at offC
    int offAjc, offAnz;   // A (CSC): Ajc at offAjc (nV+1 ints), Air/Aval/Aci/Arv at offAnz
    int offArp;           // A (CSR copy): Arp at offArp (nC+1 ints)
    int offHjc, offHnz;   // H (CSC, full symmetric)
    int haveH;
    int annz, hnnz;       // entry counts of A and H when the host knows them (saves a dependent load), else -1
    double hreg;          // H + hreg*I (LP path: qpOASES regularises an all-zero Hessian)
    long long offState;   // persistent engine image (doubles) for hot starts
};

// The RSQP_SMALL_* / RSQP_K_* / RSQP_LANE / RSQP_ARENA_MAPPED / RSQP_NO_SPIN environment switches, read ONCE PER HANDLE (rsqp_create /
// rsqp_batch_create) and kept with it: a handle's behaviour does not depend on what another handle's first use found in the
// environment. Table of every switch: INTEGRATION.md 6.
struct SmallKnobs {
    int engine = -1;          // RSQP_SMALL_ENGINE      0 / 1: force the Givens-TQ / the explicit-inverse LDS kernel (no tableau kernels)
    int k_debug_bail = -1;    // RSQP_K_DEBUG_BAIL      test hook: the mid-size tableau kernel bails out of a hot start before its n-th change
    int lanes = -1;           // RSQP_SMALL_LANES       lanes per problem (8 / 16 / 32 / 64)
    int waves = -1;           // RSQP_SMALL_WAVES       waves per SIMD the build is compiled for
    int no_tiny = 0;          // (set by the single-QP rescue, rsqp_api.hip, and by knobs_of, rsqp_batch.hip) 1: no hs071-scale tableau kernel; 2 (the LP launches of a batch): nor the mid-size one
    int lane = -1;            // RSQP_LANE              0: never the lane-per-problem kernel (qp_lane.hip); n > 0: from n members on (default 16 385)
    int lane_hblock = -1;     // RSQP_LANE_HBLOCK       0: the lane-per-problem kernel always keeps the full triangle of H (never its leading-block build)
    int lane_shape = -1;      // RSQP_LANE_SHAPE        0: never the lane-per-problem kernel's full-shape build (nV = 8, nC = 2 as compile-time constants)
    int arena_mapped = -1;    // RSQP_ARENA_MAPPED     single-QP handles: patterns / plans in host-mapped memory, no upload at set_A / set_H (-1: hs071 scale only)
    int no_spin = 0;          // RSQP_NO_SPIN           single-QP waits block in hipStreamSynchronize instead of spinning on a mapped word
};
SmallKnobs rsqp_small_knobs_from_env();      // qp_small.hip

struct QPPools {
    const QPDesc *desc;
    const int *Ajc, *Air; const double *Aval;
    const int *Arp, *Aci; const double *Arv;
    const int *Hjc, *Hir; const double *Hval;
    const double *g, *lb, *ub, *lbA, *ubA;
    const double *x0, *y0; const int *guess_b;   // warm re-init inputs (may be null)
    double *x, *y; int *ws_b, *ws_c;
    int *status, *ret, *nwsr, *nflips; double *obj;
    double *state;
    int uniV, uniC;   // nV / nC of every problem when the batch is uniform in shape, else -1
    int reinit_from_y0;   // warm re-initialisation (mode 3) without guessed constraints: 1 = sides from sign(y0), 0 = from A x0
    int *done_flag;   // single-QP solves: host-mapped word that receives done_val once the results are out (the host spins
    int done_val;     //   on it instead of sleeping in hipStreamSynchronize); nullptr for batches
    int k_debug_bail; // test hook (RSQP_K_DEBUG_BAIL=n): the KKT-tableau kernel bails out of a HOT start before its n-th change; -1 off
    int only_bailed;  // 1: the null-space kernel runs only the members the KKT-tableau kernel left with ret == RET_BAIL
    double *cert_out; int *cert_Wb, *cert_Wc;   // single-QP handles on the tableau kernel of qp_tiny.hip: the KKT certificate
                      //    (6 doubles: primal, dual, compl, stat, KKT_error, invalid) and the mapped working set are formed at
                      //    the END of the solve kernel -- QPhandler::solveQP always asks for them (src/QPhandler.cpp:470-499); or nullptr
    int tiny_ok;      // 1: every H of the batch is symmetric (or absent): problems of <= 8 variables may take the register-resident
                      //    tableau kernel (qp_tiny.hip), which keeps K symmetric by construction
    int uni_pat;      // 1: every member has the sizes AND the sparsity patterns of member 0 (checked by the host when the batch is
    int uni_annz, uni_hnnz, uni_haveH;   //    created: parameter scans, perturbations of one QP) -- offsets are q * size then, so the kernel
    long long uni_state; double uni_hreg; //    needs no descriptor load, and it reads the PATTERN arrays of member 0 (cache-resident for the
                      //    whole launch) instead of its own copy: two dependent HBM round trips less in front of every solve
                      //    (single-QP handles are the batch of one: set as well; uni_hreg = the LP regularisation, 0 in batches)
    int skip_mark;    // 1 (batches with keep_state = 0 on the hs071-scale tableau kernel): the HOST remembers that no state was kept
                      //    (rsqp_batch::state_engine = -1: the next hot start runs cold), so the kernel does not touch the state block at
                      //    all -- the "not initialised" mark was one scattered 64-byte line per QP
    int lane_hblock;  // 4: one pattern (uni_pat) whose H has every entry in its leading 4 x 4 block (or no entry): the lane-per-problem
                      //    kernel keeps that block alone (SmallPlan::hb, qp_lane.hip); anything else: the full triangle
    int keep_state;   // 1: write the hot-start part of the engine image back to HBM at the end of a solve (what the
                      //    SQProblem object keeps between calls); 0: cold-start-only batches skip that write --
                      //    the image is marked "not initialised", a later hot start falls back to a cold start
    const int *member_mode;   // non-null (rsqp_batch_optimize_qp): member q starts as member_mode[q] says (0..3 as the `mode` argument of the
                      //    kernels, which is then ignored); a negative value = the member is not in this launch and nothing of it is
                      //    touched. In one launch every mode-3 member has the same warm-start inputs present (x0 / y0 / guess_b are
                      //    batch-wide pointers). The lane-per-problem kernel takes such a launch in its WARM builds alone, where the host
                      //    knows that no member's word is 1 (rsqp_plan_lane_fits; rsqp_batch_set_lane_warm), or in those of level 2,
                      //    which carry the word 1 as well (rsqp_batch_set_lane_hot)
    // the WARM builds of the lane-per-problem kernel (qp_lane.hip; set by launch_batch where the plan says SmallPlan::lane_warm): the
    // guess a member's set-up starts from -- x, y = [bounds; constraints], bound statuses, constraint statuses, member-major like
    // the results; any of them null, uniform over the launch. A hot start with new matrices: the batch's own result pools (the
    // kernel reads a wave's members before it writes them); a warm re-initialisation: the warm-start pools, guess_sc null
    const double *guess_x, *guess_y; const int *guess_sb, *guess_sc;
    int guess_mode;   // the call shape of such a launch without member_mode: 2 or 3; level 2 also 1, a hot start on new vectors, whose
                      //    guess is the one of mode 2 plus the limits in the tails of the members' state blocks (`state`, `uni_state`)
};

// optimizeQP's choice of the call shape (src/qpOASESInterface.cpp:150-208) from get_Matrix_change_status (:817-833), stated ONCE for
// rsqp_optimize_qp, rsqp_optimize_lp and the plan kernel of rsqp_batch_optimize_qp. first_solved = firstQPsolved_, updated = the
// matrices changed since the last reset_flags; old_status / new_status (0 UNDEFINED, 1 FIXED, 2 VARIED) are advanced in place.
// Returns the RSQP_MODE_* value: 0 cold, 1 hot start on new vectors, 2 hot start on new matrices, 3 the FIXED <-> VARIED flip
// (re-initialisation; both status words are back at UNDEFINED, :207-208).
__host__ __device__ inline int rsqp_dispatch_mode(bool first_solved, bool updated, int &old_status, int &new_status) {
    if (!first_solved) return 0;
    const int cur = updated ? 2 : 1;
    if (old_status == 0) old_status = cur;
    else {
        if (new_status != 0) old_status = new_status;
        new_status = cur;
    }
    if (new_status == 0) return old_status == 1 ? 1 : 2;
    if (new_status == old_status) return new_status == 1 ? 1 : 2;
    new_status = old_status = 0;
    return 3;
}

// number of doubles / ints of the LDS (and persistent) image of one problem
__host__ __device__ inline int rsqp_ld(int nV) { return nV | 1; }
__host__ __device__ inline long long rsqp_image_doubles(int nV, int nC) {
    long long ld = rsqp_ld(nV), sT = nV < nC ? nV : nC;
    //        Q|Z      R|Wz     T|Y      vectors of nV   vectors of nC   y,dy        scalars
    //        (explicit-inverse engine: Y lives inside Z's array, Minv in the T slot) + four vectors of sT + 2
    return ld * nV + ld * nV + sT * ld + 19LL * nV + 9LL * nC + 2LL * (nV + nC) + 16 + 4 * (sT + 2);
}
__host__ __device__ inline long long rsqp_image_ints(int nV, int nC) { return nV + 3LL * nC + 8; }
__host__ __device__ inline long long rsqp_image_bytes(int nV, int nC) {
    long long b = rsqp_image_doubles(nV, nC) * 8 + rsqp_image_ints(nV, nC) * 4;
    return (b + 15) & ~15LL;
}

// persistent state of one problem in HBM: the image of the null-space engines, followed by the extension of the
// KKT-tableau kernel (qp_small_g.h): G = -SWEEP_S(K) with one slot per variable and constraint, (nV + nC)^2 doubles
__host__ __device__ inline long long rsqp_state_bytes(int nV, int nC) {
    long long b = rsqp_image_bytes(nV, nC) + 8LL * (long long)(nV + nC) * (nV + nC);
    // hs071-scale problems (qp_tiny.hip): the register-resident tableau engine keeps a fixed-slot state of (8 + MC)^2 + 96
    // doubles + 24 ints (<= 2912 B) whatever the problem's own sizes are (MC = 2 / 4 / 8 by the batch's largest nC)
    if (nV <= 8 && nC <= 8 && b < 2944) b = 2944;
    return b;
}

// batches whose images exceed the LDS of a CU (qp_small_hbm.hip): limits of the members' sizes, and the state slice of one
// member -- the image used in place, 8 x 256 bytes of cross-wave partial sums, dense copies of A and H. No KKT-tableau
// extension: the mid-size tableau kernel never sees these batches.
#define RSQP_HBM_MAX_V 512   // = RSQP_BATCH_MAX_V / _C of rsqp_hip.h (checked in rsqp_batch.hip)
#define RSQP_HBM_MAX_C 512
__host__ __device__ inline long long rsqp_hbm_state_bytes(int nV, int nC) {
    return rsqp_image_bytes(nV, nC) + 8LL * 256 + 8LL * ((long long)nV * nV + (long long)nC * nV);
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: set it once per
// (kernel, device) -- `mask` is the kernel's own bitmask of devices already done (thread-safe)
inline void rsqp_allow_full_lds(const void *fn, std::atomic<unsigned long long> &mask, int bytes) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(mask.load(std::memory_order_acquire) & bit)) {
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        mask.fetch_or(bit, std::memory_order_release);
    }
}

// launchers (defined in the .hip files). Which kernel a launch runs is decided in rsqp_small_plan.h and nowhere else: the callers compute
// the SmallPlan of a launch and rsqp_launch_small_qp executes it through the launcher of the plan's family
struct SmallPlan;
hipError_t rsqp_launch_small_qp(const SmallKnobs &kn, const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream);
// the hand-over launch of a batch (rsqp_batch_set_handover), behind a launch of the hs071-scale tableau kernels (plan `tableau`, family
// 1 or 2) on the same stream: the null-space kernel of `pl` -- the plan of the same launch with SmallKnobs::no_tiny = 1, as rsqp_solve
// retries on a handle -- runs the members that launch left with ret == RET_SETUP_FAILED, and nobody else. Such a member starts cold
// where its call shape was a hot start (the stored state is the tableau kernel's), keeps a warm re-initialisation, gets maxWSR
// afresh, and its state block is left as the tableau kernel's "not initialised" (nothing is written where `tableau` keeps no state
// and leaves no mark). handed: nq flags + one count (or null); a member taken over raises its flag, the first time also the count
hipError_t rsqp_launch_small_handover(const SmallKnobs &kn, const SmallPlan &pl, const SmallPlan &tableau, const QPPools &p, int nq,
                                      int maxWSR, int *handed, hipStream_t stream);
long long rsqp_mat_lds_bytes(int nV, int nC, int annz, int hnnz);
int rsqp_small_qp_fits(int nVmax, int nCmax);
// qp_tiny.hip: the register-resident tableau kernel for problems of at most 8 variables and 8 constraints
hipError_t rsqp_launch_tiny_qp(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream);
// qp_lane.hip: one lane per problem, for cold starts of large one-shape batches of at most 8 x 2 (SmallPlan::lane_warm: their hot
// starts with new matrices and warm re-initialisations)
hipError_t rsqp_launch_lane_qp(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream);
// qp_small_hbm.hip: the null-space engines with their images in HBM, one workgroup per problem, for batches beyond
// rsqp_small_qp_fits (every member of such a batch, the small ones included); members up to RSQP_HBM_MAX_V x RSQP_HBM_MAX_C
int rsqp_hbm_qp_fits(int nVmax, int nCmax);
hipError_t rsqp_launch_small_qp_hbm(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream);
