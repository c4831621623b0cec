// qp_small_hbm.hip -- the batched null-space engines of qp_small.hip for batches whose images do not fit the LDS of
// a CU: one workgroup per problem, its image in the problem's own slice of the batch state block in HBM.
//
// The engines are the same source as the LDS-resident kernels (qp_small_engine.h, qp_small_x.h), compiled here with
// RSQP_IMAGE_AS = 1: every image pointer is a global pointer, so the same arithmetic, tie breaks and results run on
// global_load / global_store instead of ds_read / ds_write. The LDS-resident kernels are not compiled in this unit
// and their code does not change.
//
// Slice of one problem (rsqp_hbm_state_bytes): [image of rsqp_image_bytes(nV, nC)][8 L bytes of cross-wave partial
// sums (four-wave build)][dense A (nC x nV) and H (nV x nV), column-major]. The image is used IN PLACE: a hot start
// continues on the factors the previous solve left there (no load, no write-back). Its layout (all doubles of the
// engine, then its 16-bit integers) is not the one the LDS-resident kernels keep in HBM, which is why the host gives
// this kernel a state family of its own (rsqp_batch::state_engine).
//
// MI355X mapping: four waves per problem (L = 256, SYNC() = __syncthreads(), the `wide` shape of the LDS build), one
// problem per workgroup, grid = nq. No dynamic LDS; the working set of a problem's change (its Z / Y / Wz columns
// and the dense matrices, ~1-3 MB at 200 x 100) streams through L2 / the Infinity Cache.
#include <cstdlib>
#include <type_traits>

#include "rsqp_small_plan.h"

#define RSQP_IMAGE_AS 1
#define STAMP(k) do { } while (0)

namespace {

#include "qp_small_engine.h"

#include "qp_small_x.h"

// L = lanes per problem (the whole workgroup), W = waves per SIMD the register allocator leaves room for
template <class ENG, int L, int W>
__global__ void __launch_bounds__(L, W)
small_qph_kernel(QPPools P, int nq, int mode, int maxWSR) {
    const int lane = (int)threadIdx.x;
    const int q = (int)blockIdx.x;
    if (q >= nq) return;
    if (P.member_mode) { mode = P.member_mode[q]; if (mode < 0) return; }   // per-member call shape; < 0: not in this launch
    const QPDesc d = P.desc[q];
    ENG E;
    E.lane = lane;
    lchar *base = (lchar *)(P.state + d.offState);
    const long long ibytes = rsqp_image_bytes(d.nV, d.nC);
    if constexpr (L > 64) E.part = (ldouble *)(base + ibytes);
    E.carve(base, d.nV, d.nC);
    const long long nd = ENG::image_doubles(d.nV, d.nC), ni = ENG::image_ints(d.nV, d.nC);
    const long long np = ENG::persist_doubles(d.nV, d.nC);
    E.haveH = d.haveH;
    E.hreg = d.hreg;
    const int *gAjc = P.Ajc + d.offAjc, *gAir = P.Air + d.offAnz, *gArp = P.Arp + d.offArp, *gAci = P.Aci + d.offAnz;
    const int *gHjc = P.Hjc + d.offHjc, *gHir = P.Hir + d.offHnz;
    const double *gAval = P.Aval + d.offAnz, *gArv = P.Arv + d.offAnz, *gHval = P.Hval + d.offHnz;
    if constexpr (ENG::DENSE_MATS) {
        E.stage_dense(base + ibytes + 8LL * L, gAjc, gAir, gAval, gHjc, gHir, gHval);
    } else {
        E.Ajc = gAjc; E.Air = gAir; E.Aval = gAval; E.Arp = gArp; E.Aci = gAci; E.Arv = gArv;
        E.Hjc = gHjc; E.Hir = gHir; E.Hval = gHval;
    }
    E.nflips = 0; E.infeasible = E.unbounded = 0; E.status = QPS_NOTINITIALISED; E.nFR = E.nAC = 0;
    ldouble *simg = (ldouble *)base;
    lint *siimg = (lint *)(simg + nd);

    int rcode = RET_OK, nWSR = 0;
    if (mode == 0) {
        // (the factor arrays at the head of the image are zeroed by setup_aux itself)
        for (long long k = ENG::factor_doubles(d.nV, d.nC) + lane; k < nd; k += L) simg[k] = 0.0;
        for (int k = lane; k < ni; k += L) siimg[k] = 0;
        SYNC();
    } else {
        // the image of the previous solve is where it was left; its scratch starts from zero as after a reload
        for (long long k = np + lane; k < nd; k += L) simg[k] = 0.0;
        SYNC();
        E.restore(E.iscal[1], E.iscal[2], E.iscal[3]);
        SYNC();
        if (E.status == QPS_NOTINITIALISED) mode = 0;
    }
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
    } else if (mode == 3) {  // warm re-initialisation from (x0, y0, guessed bounds), as the LDS-resident kernel stages it
        if (P.x0) for (int v = lane; v < d.nV; v += L) E.wv4[v] = P.x0[d.offV + v];
        if (P.y0) for (int i = lane; i < d.nV + d.nC; i += L) E.dy[i] = P.y0[d.offV + d.offC + i];
        if (P.guess_b) for (int v = lane; v < d.nV; v += L) E.wq[v] = (double)P.guess_b[d.offV + v];
        SYNC();
        // (no guessed constraints in this call shape, qpOASESInterface.cpp:204-206: their sides come from A x0, or from y0 on request)
        rcode = E.setup_aux(P.x0 != nullptr, P.y0 != nullptr, P.guess_b != nullptr, false, P.reinit_from_y0 != 0);
        if (rcode != RET_OK) rcode = E.setup_aux(false, false, false, false);
    } else {
        E.infeasible = E.unbounded = 0;
        if constexpr (ENG::K_IMAGE) {
            // (only this kernel writes these states, and it marks them as its own factors: kept for symmetry with the
            //  LDS-resident kernel, whose image the tableau kernel may have written)
            if (E.iscal[4] != 0) {
                rcode = E.rebuild_factors();
                if (rcode != RET_OK) rcode = E.setup_aux(false, false, false, false);
            }
        }
    }
    if (rcode == RET_OK) rcode = E.homotopy(maxWSR, nWSR);
    double obj = E.objective();

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
        E.iscal[1] = E.nFR; E.iscal[2] = E.nAC;
        // keep_state = 0: the image is marked "not initialised", a later hot start runs cold
        E.iscal[3] = P.keep_state ? E.status : QPS_NOTINITIALISED;
        if constexpr (ENG::K_IMAGE) E.iscal[4] = 0;      // this engine's factors
    }
}

}  // namespace

int rsqp_hbm_qp_fits(int nVmax, int nCmax) {
    return nVmax >= 1 && nCmax >= 0 && nVmax <= RSQP_HBM_MAX_V && nCmax <= RSQP_HBM_MAX_C;
}

hipError_t rsqp_launch_small_qp_hbm(const SmallPlan &pl, const QPPools &p, int nq, int maxWSR, hipStream_t stream) {
    if (pl.engine == 1 && pl.L == 256 && pl.W == 1)         // four waves per problem, dense copies of A and H in the slice
        hipLaunchKernelGGL((small_qph_kernel<EngineX<256, true>, 256, 1>), dim3(pl.grid), dim3(pl.block), 0, stream, p, nq, pl.mode, maxWSR);
    else if (pl.engine == 0 && pl.L == 64 && pl.W == 2)     // the Givens / TQ engine has a one-wave build only; sparse matrices from global memory
        hipLaunchKernelGGL((small_qph_kernel<Engine<64, false>, 64, 2>), dim3(pl.grid), dim3(pl.block), 0, stream, p, nq, pl.mode, maxWSR);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
