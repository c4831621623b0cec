// qp_small_engine.h -- included by qp_small.hip and qp_small_hbm.hip inside their anonymous namespaces.
//
// The null-space engine of the batched kernels: SYNC / PFOR, the pointer types of the engine image, the reductions and
// Engine (the Givens / TQ formulation). qp_small_x.h (EngineX) builds on it. The image pointer types take their
// address space from RSQP_IMAGE_AS, defined by the including file before it includes this one:
//   3 (LDS, the default): qp_small.hip -- the image of a problem lives in its workgroup's LDS;
//   1 (global): qp_small_hbm.hip -- the image lives in the problem's slice of the HBM state block (problems whose
//     image exceeds the LDS of a CU). Same source, same arithmetic, only the loads and stores differ.
#ifndef RSQP_IMAGE_AS
#define RSQP_IMAGE_AS 3
#endif

// A workgroup is ONE wave: LDS instructions of a wave execute in program order, so making a
// write visible to the other lanes only needs the compiler to keep the order (no s_barrier,
// which would also be illegal inside the per-problem divergent control flow of packed waves).
// (L > 64: a problem owns several waves of its workgroup -- a real barrier.)
#define SYNC()                                                   \
    do {                                                         \
        if constexpr (L > 64) {                                  \
            __syncthreads();                                     \
        } else {                                                 \
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
            __builtin_amdgcn_wave_barrier();                     \
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
        }                                                        \
    } while (0)
#define PFOR(i, n) for (int i = lane; i < (n); i += L)
// packed upper-Hessenberg R of the Givens / TQ engine: element (row r, column c), r <= c + 1
#define RIX(c, r) ((c) * ((c) + 3) / 2 + (r))
// image pointer types in a named address space (LDS unless RSQP_IMAGE_AS says otherwise): guarantees ds_read / ds_write
// (or global_load / global_store) -- a generic pointer would be lowered to flat_load, which is several times slower
#define LDS __attribute__((address_space(3)))
#define RSQP_IMG __attribute__((address_space(RSQP_IMAGE_AS)))
typedef RSQP_IMG double ldouble;
typedef RSQP_IMG short lint;   // working-set arrays of the image: statuses in {-1,0,1}, indices < 32768 (HBM copies stay int)
typedef LDS unsigned short lidx;   // staged matrix indices: every LDS-resident problem has < 65536 rows / entries
typedef RSQP_IMG char lchar;

struct Blocking {
    double tau;
    int kind;  // 0 none, 1 remove constraint, 2 remove bound, 3 add constraint, 4 add bound
    int idx, side;
};

// The target vectors gN / lbN / ubN are only ever read by the lane that owns the entry (and by two uniform-index
// reads in the flipping guard). Builds whose shape is a compile-time constant (nV <= L: one entry per lane) keep
// them in a REGISTER per lane instead of 3 nV doubles of LDS -- which is what brings the hs071-scale image to
// 2368 B = 64 (mod 256): the four problems of a 32-lane LDS access group then sit on disjoint banks.
struct LdsVec {
    ldouble *p;
    __device__ __forceinline__ ldouble &operator[](int i) const { return p[i]; }
    template <int L> __device__ __forceinline__ double bcast(int i) const { return p[i]; }
};
// ---- partner exchange of an all-reduce WITHOUT the LDS crossbar. __shfl_xor compiles to ds_bpermute_b32 (two per
// double, ~100 cycles each and a slot of the LDS pipe the kernel's data also goes through); inside a row of 16 lanes
// a DPP permutation does the same in the VALU. Step S pairs every lane with one that holds the sum of the OTHER
// 2^S-lane block of its 2^(S+1)-lane block: S = 0, 1 quad_perm (xor 1, xor 2), S = 2 row_half_mirror (i <-> 7 - i),
// S = 3 row_mirror (i <-> 15 - i); S = 4, 5 (xor 16, 32) cross rows and stay on ds_bpermute. Steps must run in
// ASCENDING order (the mirrors rely on the blocks below being reduced already); every lane of a block ends with the
// same bits because floating-point addition is commutative.
template <int S> __device__ __forceinline__ int xchg_i32(int x) {
    if constexpr (S == 0) return __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false);       // quad_perm [1,0,3,2]
    else if constexpr (S == 1) return __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
    else if constexpr (S == 2) return __builtin_amdgcn_update_dpp(x, x, 0x141, 0xf, 0xf, false); // row_half_mirror
    else if constexpr (S == 3) return __builtin_amdgcn_update_dpp(x, x, 0x140, 0xf, 0xf, false); // row_mirror
    else return __shfl_xor(x, 1 << S);
}
template <int S> __device__ __forceinline__ double xchg_f64(double x) {
    if constexpr (S >= 4) return __shfl_xor(x, 1 << S);
    else return __hiloint2double(xchg_i32<S>(__double2hiint(x)), xchg_i32<S>(__double2loint(x)));
}
__device__ __forceinline__ double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// A whole wave (NSTEP == 6): after the four DPP steps every lane holds the sum of its row of 16; the four row sums are
// read through scalar registers (v_readlane) and added as (R0 + R1) + (R2 + R3) -- the value the xor-16 / xor-32
// exchanges produce in every lane (addition is commutative), without their four ds_bpermute round trips.
template <int NSTEP, int S = 0> __device__ __forceinline__ double allreduce_sum(double v) {
    if constexpr (NSTEP == 6 && S == 4) {
        const double r0 = readlane_f64(v, 0), r1 = readlane_f64(v, 16), r2 = readlane_f64(v, 32), r3 = readlane_f64(v, 48);
        return (r0 + r1) + (r2 + r3);
    } else if constexpr (S < NSTEP) { v += xchg_f64<S>(v); return allreduce_sum<NSTEP, S + 1>(v); }
    else return v;
}
template <int NSTEP, int S = 0> __device__ __forceinline__ void allreduce_argmin(double &t, int &id) {   // lexicographic min of (t, id)
    if constexpr (NSTEP == 6 && S == 4) {
        double bt = readlane_f64(t, 0);
        int bi = __builtin_amdgcn_readlane(id, 0);
#pragma unroll
        for (int r = 16; r < 64; r += 16) {
            const double t2 = readlane_f64(t, r);
            const int id2 = __builtin_amdgcn_readlane(id, r);
            if (t2 < bt || (t2 == bt && id2 < bi)) { bt = t2; bi = id2; }
        }
        t = bt; id = bi;
    } else if constexpr (S < NSTEP) {
        const double t2 = xchg_f64<S>(t);
        const int id2 = xchg_i32<S>(id);
        if (t2 < t || (t2 == t && id2 < id)) { t = t2; id = id2; }
        allreduce_argmin<NSTEP, S + 1>(t, id);
    }
}
constexpr int ilog2c(int n) { return n <= 1 ? 0 : 1 + ilog2c(n / 2); }

struct RegVec {
    double r;
    __device__ __forceinline__ double &operator[](int) { return r; }                 // index == owning lane by construction
    __device__ __forceinline__ const double &operator[](int) const { return r; }
    template <int L> __device__ __forceinline__ double bcast(int i) const { return __shfl(r, i, L); }   // i uniform over the problem
};
template <bool B> struct MatPtr { typedef const lidx *I; typedef const ldouble *D; };
template <> struct MatPtr<false> { typedef const int *I; typedef const double *D; };

// MAT_LDS: the sparse matrices were staged into LDS behind the image (they fit for every
// hs0xx-scale problem); otherwise they are read from global memory (L2).
template <int L, bool MAT_LDS, bool REGV = false>
struct Engine {
    typedef typename MatPtr<MAT_LDS>::I MI;
    typedef typename MatPtr<MAT_LDS>::D MD;
    // problem
    int nV, nC, ld, sizeT, haveH;
    double hreg;
    MI Ajc, Air; MD Aval;
    MI Arp, Aci; MD Arv;
    MI Hjc, Hir; MD Hval;
    // LDS image
    ldouble *Q, *R, *T;
    ldouble *x, *g, *lb, *ub, *dx, *wq, *wv1, *wv2, *wv3, *wv4, *rc, *rs;
    typedef typename std::conditional<REGV, RegVec, LdsVec>::type TV;
    TV gN, lbN, ubN;
    ldouble *Ax, *lbA, *ubA, *lbAN, *ubAN, *dAx, *wc1, *wc2;
    ldouble *y, *dy;
    lint *Sb, *Sc, *AC, *posAC;
    lint *iscal;    // 8 ints
    static constexpr bool DENSE_MATS = false;
    // uniform over the L lanes of the problem
    int lane;
    int nFR, nAC, status, infeasible, unbounded, nflips;
    long long tlast;

    // ------------------------------------------------------------------ carve
    static constexpr bool K_IMAGE = false;      // (only batches of the explicit-inverse engine are shared with qp_small_g.h)
    // doubles of this formulation's image (<= rsqp_image_doubles, the size of the persistent copy)
    __host__ __device__ static long long image_doubles(int nV, int nC) {
        const long long ld = rsqp_ld(nV), sT = nV < nC ? nV : nC;
        return ld * nV + (long long)nV * (nV + 3) / 2 + sT * ld + (REGV ? 9LL : 12LL) * nV + 8LL * nC + 2LL * (nV + nC);
    }
    __host__ __device__ static long long image_ints(int nV, int nC) { return nV + 3LL * nC + 4; }
    __host__ __device__ static long long factor_doubles(int nV, int nC) {   // Q, R, T: (re)initialised by setup_aux
        const long long ld = rsqp_ld(nV), sT = nV < nC ? nV : nC;
        return ld * nV + (long long)nV * (nV + 3) / 2 + sT * ld;
    }
    // leading part of the image that survives a solve (factors, iterate, auxiliary data, multipliers)
    __host__ __device__ static long long persist_doubles(int nV, int nC) {
        const long long ld = rsqp_ld(nV), sT = nV < nC ? nV : nC;
        return ld * nV + (long long)nV * (nV + 3) / 2 + sT * ld + 4LL * nV + 3LL * nC + (nV + nC);
    }
    __device__ __forceinline__ void carve(lchar *base, int nV_, int nC_) {
        nV = nV_; nC = nC_; ld = rsqp_ld(nV); sizeT = nV < nC ? nV : nC;
        ldouble *p = (ldouble *)base;
        Q = p; p += ld * nV;
        R = p; p += RIX(nV, 0);   // packed upper Hessenberg: column c holds rows 0 .. c + 1 (the sweeps create one sub-diagonal)
        T = p; p += sizeT * ld;
#define CARVE_V(name) name = p; p += nV
#define CARVE_C(name) name = p; p += nC
        // what a hot start needs (persist_doubles, written back to HBM) ...
        CARVE_V(x); CARVE_V(g); CARVE_V(lb); CARVE_V(ub);
        CARVE_C(Ax); CARVE_C(lbA); CARVE_C(ubA);
        y = p; p += nV + nC;
        // ... and the per-solve scratch
        if constexpr (!REGV) { CARVE_V(gN.p); CARVE_V(lbN.p); CARVE_V(ubN.p); }
        CARVE_V(dx); CARVE_V(wq); CARVE_V(wv1); CARVE_V(wv2); CARVE_V(wv3);
        wv4 = wv3;   // the incoming row of an exchange / the staged x0: never alive together with wv3 (Cholesky work vector)
        CARVE_C(lbAN); CARVE_C(ubAN); CARVE_C(dAx); CARVE_C(wc1); CARVE_C(wc2);
#undef CARVE_V
#undef CARVE_C
        dy = p; p += nV + nC;
        // Givens coefficients of a sweep live in dx / dy: the step direction is dead from the homotopy
        // step to the next step_direction(), which is when the working set changes (and in setup_aux,
        // after y0 has been taken out of dy)
        rc = dx; rs = dy;
        lint *ip = (lint *)p;
        Sb = ip; ip += nV;
        Sc = ip; ip += nC;
        AC = ip; ip += nC;
        posAC = ip; ip += nC;
        iscal = ip; ip += 4;
    }

    // ------------------------------------------------------------------ reductions
    // butterflies over the L lanes of this problem (xor offsets < L never leave the group);
    // every lane of the group ends with the same value, so control flow stays group-uniform
    __device__ __forceinline__ double block_sum(double v) { return allreduce_sum<ilog2c(L)>(v); }
    // lexicographic min of (t, id)
    __device__ __forceinline__ void block_argmin(double &t, int &id) { allreduce_argmin<ilog2c(L)>(t, id); }
    __device__ __forceinline__ double dot(const ldouble *a, const ldouble *b, int n) {
        double s = 0.0;
        PFOR(i, n) s += a[i] * b[i];
        return block_sum(s);
    }

    // ------------------------------------------------------------------ sparse products
    // sum_k val[k] * v[idx[k]] over [k0, k1), accumulated in entry order. Four entries per trip:
    // their index / value / gather loads are independent, so the LDS latencies overlap instead of
    // chaining two round trips per entry.
    template <class IP, class DP>
    __device__ __forceinline__ static double sparse_dot(IP idx, DP val, const ldouble *v, int k0, int k1) {
        double s = 0.0;
        int k = k0;
        if constexpr (!MAT_LDS) {
            // matrices in global memory (the image alone nearly fills the LDS): 8 entries per trip, so
            // that 16 L2 round trips are in flight at once instead of 2
            for (; k + 8 <= k1; k += 8) {
                int c[8]; double a[8], w[8];
#pragma unroll
                for (int u = 0; u < 8; u++) { c[u] = idx[k + u]; a[u] = val[k + u]; }
#pragma unroll
                for (int u = 0; u < 8; u++) w[u] = v[c[u]];
#pragma unroll
                for (int u = 0; u < 8; u++) s += a[u] * w[u];
            }
        }
        for (; k + 4 <= k1; k += 4) {
            const int c0 = idx[k], c1 = idx[k + 1], c2 = idx[k + 2], c3 = idx[k + 3];
            const double a0 = val[k], a1 = val[k + 1], a2 = val[k + 2], a3 = val[k + 3];
            const double v0 = v[c0], v1 = v[c1], v2 = v[c2], v3 = v[c3];
            s += a0 * v0; s += a1 * v1; s += a2 * v2; s += a3 * v3;
        }
        if (k + 2 <= k1) {
            const int c0 = idx[k], c1 = idx[k + 1];
            const double a0 = val[k], a1 = val[k + 1];
            const double v0 = v[c0], v1 = v[c1];
            s += a0 * v0; s += a1 * v1;
            k += 2;
        }
        if (k < k1) s += val[k] * v[idx[k]];
        return s;
    }
    __device__ __forceinline__ void A_times(const ldouble *v, ldouble *out) {
        PFOR(r, nC) out[r] = sparse_dot(Aci, Arv, v, Arp[r], Arp[r + 1]);
        SYNC();
    }
    __device__ __forceinline__ void AT_times(const ldouble *yc, ldouble *out) {
        PFOR(c, nV) out[c] = sparse_dot(Air, Aval, yc, Ajc[c], Ajc[c + 1]);
        SYNC();
    }
    __device__ __forceinline__ void H_times(const ldouble *v, ldouble *out) {
        PFOR(c, nV) {
            const double s = haveH ? sparse_dot(Hir, Hval, v, Hjc[c], Hjc[c + 1]) : 0.0;
            out[c] = s + hreg * v[c];
        }
        SYNC();
    }
    // a[v] = A[i][v] for free v, 0 otherwise (all==true: every variable)
    __device__ __forceinline__ void row_of_A(int i, ldouble *a, bool all) {
        PFOR(v, nV) a[v] = 0.0;
        SYNC();
        for (int k = Arp[i] + lane; k < Arp[i + 1]; k += L) {
            int c = Aci[k];
            if (all || Sb[c] == 0) a[c] = Arv[k];
        }
        SYNC();
    }
    // w[c] = Q[:,c] . a   for c < nFR
    __device__ __forceinline__ void QT_times(const ldouble *a, ldouble *w) {
        PFOR(c, nFR) {
            const ldouble *qc = Q + c * ld;
            double s = 0.0;
            for (int v = 0; v < nV; v++) s += qc[v] * a[v];
            w[c] = s;
        }
        SYNC();
    }

    // ------------------------------------------------------------------ Givens helpers
    __device__ __forceinline__ static void givens(double a_elim, double b_keep, double &c, double &s) {
        if (a_elim == 0.0) { c = 1.0; s = 0.0; return; }
        double r = hypot(a_elim, b_keep);
        c = b_keep / r;
        s = a_elim / r;
    }
    // rotations (j, j+1), j = j0 .. j1-1, left to right, coefficients rc/rs[j], applied
    // to the vector w (thread 0 computes them: the chain is sequential)
    __device__ __forceinline__ void plan_sweep(ldouble *w, int j0, int j1, int jskip_below) {
        if (lane == 0) {
            for (int j = j0; j < j1; j++) {
                double c = 1.0, s = 0.0;
                if (j >= jskip_below) givens(w[j], w[j + 1], c, s);
                double a = w[j], b = w[j + 1];
                w[j] = c * a - s * b;
                w[j + 1] = s * a + c * b;
                rc[j] = c; rs[j] = s;
            }
        }
        SYNC();
    }
    // apply the planned sweep to the columns of Q (lane per variable, value carried)
    __device__ __forceinline__ void sweep_Q(int j0, int j1) {
        if (j1 <= j0) return;
        PFOR(v, nV) {
            double carry = Q[j0 * ld + v];
            for (int j = j0; j < j1; j++) {
                double b = Q[(j + 1) * ld + v], c = rc[j], s = rs[j];
                Q[j * ld + v] = c * carry - s * b;
                carry = s * carry + c * b;
            }
            Q[j1 * ld + v] = carry;
        }
        SYNC();
    }
    // same sweep on the columns of T (lane per active row)
    __device__ __forceinline__ void sweep_T(int j0, int j1) {
        if (j1 <= j0) return;
        PFOR(i, nAC) {
            ldouble *row = T + i * ld;
            double carry = row[j0];
            for (int j = j0; j < j1; j++) {
                double b = row[j + 1], c = rc[j], s = rs[j];
                row[j] = c * carry - s * b;
                carry = s * carry + c * b;
            }
            row[j1] = carry;
        }
        SYNC();
    }
    // column sweep (j, j+1), j = 0..nZ-2, on R followed by the row rotations that make
    // it upper triangular again
    __device__ __forceinline__ void sweep_R(int nZ) {
        if (nZ < 2) return;
        PFOR(r, nZ) {
            int j0 = r > 0 ? r - 1 : 0;
            double carry = R[RIX(j0, r)];
            for (int j = j0; j + 1 < nZ; j++) {
                double b = R[RIX(j + 1, r)], c = rc[j], s = rs[j];
                R[RIX(j, r)] = c * carry - s * b;
                carry = s * carry + c * b;
            }
            R[RIX(nZ - 1, r)] = carry;
        }
        SYNC();
        for (int j = 0; j + 1 < nZ; j++) {
            double diag = R[RIX(j, j)], sub = R[RIX(j, j + 1)];
            if (sub != 0.0) {  // uniform: every lane read the same LDS words
                double r = hypot(diag, sub), cc = diag / r, ss = sub / r;
                SYNC();
                for (int col = j + lane; col < nZ; col += L) {
                    ldouble *pc = R + RIX(col, 0);
                    double a = pc[j], b = pc[j + 1];
                    pc[j] = cc * a + ss * b;
                    pc[j + 1] = col == j ? 0.0 : -ss * a + cc * b;
                }
                SYNC();
            }
        }
    }

    // ------------------------------------------------------------------ independence tests
    __device__ __forceinline__ bool constraint_is_LI(int i) {
        int nZ = nFR - nAC;
        if (nZ <= 0) return false;
        row_of_A(i, wv1, false);
        double na2 = dot(wv1, wv1, nV);
        if (na2 == 0.0) return false;
        double s = 0.0;
        PFOR(c, nZ) {
            const ldouble *qc = Q + c * ld;
            double d = 0.0;
            for (int v = 0; v < nV; v++) d += qc[v] * wv1[v];
            s += d * d;
        }
        s = block_sum(s);
        return sqrt(s) > RSQP_EPS_LI * sqrt(na2);
    }
    __device__ __forceinline__ bool bound_is_LI(int v) {
        int nZ = nFR - nAC;
        if (nZ <= 0) return false;
        double s = 0.0;
        PFOR(c, nZ) { double d = Q[c * ld + v]; s += d * d; }
        s = block_sum(s);
        return sqrt(s) > RSQP_EPS_LI;
    }

    // ------------------------------------------------------------------ working-set updates
    __device__ __forceinline__ void add_constraint(int i, int st, bool upd_chol, bool skipZ) {
        int nZ = nFR - nAC;
        row_of_A(i, wv1, false);
        QT_times(wv1, wq);
        int j1 = nZ - 1 > 0 ? nZ - 1 : 0;
        plan_sweep(wq, 0, j1, skipZ ? j1 : 0);
        if (!skipZ) {
            sweep_Q(0, j1);
            if (upd_chol) sweep_R(nZ);
        }
        ldouble *row = T + nAC * ld;
        PFOR(c, nV) row[c] = (c >= nZ - 1 && c < nFR) ? wq[c] : 0.0;
        if (lane == 0) { AC[nAC] = i; posAC[i] = nAC; Sc[i] = st; }
        nAC++;
        SYNC();
    }

    __device__ __forceinline__ void add_bound(int v, int st, bool upd_chol, bool skipZ) {
        int nZ = nFR - nAC;
        PFOR(c, nFR) wq[c] = Q[c * ld + v];
        SYNC();
        int jz = nZ - 1 > 0 ? nZ - 1 : 0;
        plan_sweep(wq, 0, nFR - 1, skipZ ? jz : 0);
        sweep_Q(skipZ ? jz : 0, nFR - 1);
        if (!skipZ && upd_chol) sweep_R(nZ);
        sweep_T(jz, nFR - 1);
        // row v is now +-e_{nFR-1}: drop that row and column
        PFOR(c, nFR) Q[c * ld + v] = 0.0;
        PFOR(u, nV) Q[(nFR - 1) * ld + u] = 0.0;
        PFOR(i, nAC) T[i * ld + nFR - 1] = 0.0;
        if (lane == 0) Sb[v] = st;
        nFR--;
        SYNC();
    }

    // append the Cholesky column of the new null-space column zc; false = not pos. def.
    __device__ __forceinline__ bool chol_append(int zc) {
        const ldouble *z = Q + zc * ld;
        H_times(z, wv2);
        double zHz = dot(z, wv2, nV);
        PFOR(j, zc) {
            const ldouble *qj = Q + j * ld;
            double s = 0.0;
            for (int v = 0; v < nV; v++) s += qj[v] * wv2[v];
            wv3[j] = s;
        }
        SYNC();
        // R' r = rhs, column oriented
        for (int j = 0; j < zc; j++) {
            double rj = wv3[j] / R[RIX(j, j)];
            SYNC();
            if (lane == 0) wv3[j] = rj;
            for (int k = j + 1 + lane; k < zc; k += L) wv3[k] -= R[RIX(k, j)] * rj;
            SYNC();
        }
        double rr = dot(wv3, wv3, zc);
        double rho2 = zHz - rr;
        if (!(rho2 > RSQP_EPS_PD_REL * (fabs(zHz) + rr) + RSQP_EPS_PD_ABS)) return false;
        PFOR(j, zc + 2) R[RIX(zc, j)] = j < zc ? wv3[j] : (j == zc ? sqrt(rho2) : 0.0);   // rows 0 .. zc + 1 of the packed column
        SYNC();
        return true;
    }

    // right-to-left sweep used by the two removals: rotation t acts on columns
    // (cfirst - t, cfirst - t + 1) and is fixed by row (row0 + t) of T
    __device__ __forceinline__ void removal_sweep(int row0, int nrot, int cfirst) {
        for (int t = 0; t < nrot; t++) {
            int i = row0 + t, c0 = cfirst - t;
            ldouble *ri = T + i * ld;
            double c, s;
            givens(ri[c0], ri[c0 + 1], c, s);  // uniform
            SYNC();
            if (lane == 0) { rc[t] = c; rs[t] = s; }
            if (s != 0.0) {
                for (int ii = i + lane; ii < nAC; ii += L) {
                    ldouble *row = T + ii * ld;
                    double a = row[c0], b = row[c0 + 1];
                    row[c0] = ii == i ? 0.0 : c * a - s * b;
                    row[c0 + 1] = s * a + c * b;
                }
            }
            SYNC();
        }
        if (nrot <= 0) return;
        PFOR(v, nV) {
            double keep = Q[(cfirst + 1) * ld + v];
            for (int t = 0; t < nrot; t++) {
                int c0 = cfirst - t;
                double a = Q[c0 * ld + v], c = rc[t], s = rs[t];
                Q[(c0 + 1) * ld + v] = s * a + c * keep;
                keep = c * a - s * keep;
            }
            Q[(cfirst - nrot + 1) * ld + v] = keep;
        }
        SYNC();
    }

    __device__ __forceinline__ int remove_constraint_tq(int k) {
        int cons = AC[k];
        SYNC();
        PFOR(c, nV)
            for (int i = k; i + 1 < nAC; i++) T[i * ld + c] = T[(i + 1) * ld + c];
        if (lane == 0) {
            for (int i = k; i + 1 < nAC; i++) { AC[i] = AC[i + 1]; posAC[AC[i]] = i; }
            posAC[cons] = -1;
            Sc[cons] = 0;
        }
        nAC--;
        SYNC();
        PFOR(c, nV) T[nAC * ld + c] = 0.0;
        SYNC();
        removal_sweep(k, nAC - k, nFR - 2 - k);
        return nFR - nAC - 1;
    }

    __device__ __forceinline__ int remove_bound_tq(int v) {
        int cn = nFR;
        nFR++;
        PFOR(u, nV) Q[cn * ld + u] = u == v ? 1.0 : 0.0;
        PFOR(c, cn) Q[c * ld + v] = 0.0;
        PFOR(i, nAC) T[i * ld + cn] = 0.0;
        if (lane == 0) Sb[v] = 0;
        SYNC();
        for (int k = Ajc[v] + lane; k < Ajc[v + 1]; k += L) {
            int r = Air[k];
            if (Sc[r] != 0) T[posAC[r] * ld + cn] = Aval[k];
        }
        SYNC();
        removal_sweep(0, nAC, cn - 1);
        return nFR - nAC - 1;
    }

    __device__ __forceinline__ bool chol_setup() {
        int nZ = nFR - nAC;
        for (int c = 0; c < nZ; c++)
            if (!chol_append(c)) return false;
        return true;
    }

    // ------------------------------------------------------------------ auxiliary QP
    __device__ __forceinline__ static double clampinf(double v) {
        return v > RSQP_INFTY ? RSQP_INFTY : (v < -RSQP_INFTY ? -RSQP_INFTY : v);
    }
    __device__ __forceinline__ void store_targets(const double *g_, const double *lb_, const double *ub_,
                                  const double *lbA_, const double *ubA_) {
        PFOR(v, nV) { gN[v] = g_[v]; lbN[v] = clampinf(lb_[v]); ubN[v] = clampinf(ub_[v]); }
        PFOR(i, nC) { lbAN[i] = clampinf(lbA_[i]); ubAN[i] = clampinf(ubA_[i]); }
        SYNC();
    }

    // warm-start inputs are staged by the caller: x0 in wv4, y0 in dy, guessed bound status in
    // wq and guessed constraint status in wc1 (as doubles); the flags say which are present
    __device__ __forceinline__ int setup_aux(bool x0, bool y0, bool guess_b, bool guess_c, bool cy0 = false) {
        status = QPS_PREPARINGAUXILIARYQP;
        infeasible = unbounded = 0;
        PFOR(v, nV) {
            double xv = x0 ? wv4[v] : 0.0;
            int s;
            if (guess_b) s = (int)wq[v];
            else if (x0) s = xv <= lbN[v] + RSQP_BOUND_TOLERANCE ? -1 : (xv >= ubN[v] - RSQP_BOUND_TOLERANCE ? 1 : 0);
            else if (y0) s = dy[v] > RSQP_EPS ? -1 : (dy[v] < -RSQP_EPS ? 1 : 0);
            else s = -1;
            if (s == -1 && lbN[v] <= -RSQP_INFTY) s = (ubN[v] < RSQP_INFTY && !x0 && !guess_b) ? 1 : 0;
            if (s == 1 && ubN[v] >= RSQP_INFTY) s = 0;
            wv4[v] = xv;
            wq[v] = (double)s;
        }
        if (!y0) { PFOR(i, nV + nC) dy[i] = 0.0; }
        if (!guess_c) { PFOR(i, nC) wc1[i] = 0.0; }
        SYNC();
        PFOR(v, nV) { x[v] = wv4[v]; Sb[v] = (int)wq[v]; }
        PFOR(i, nV + nC) y[i] = dy[i];
        for (int k = lane; k < ld * nV; k += L) Q[k] = 0.0;
        for (int k = lane; k < RIX(nV, 0); k += L) R[k] = 0.0;
        for (int k = lane; k < sizeT * ld; k += L) T[k] = 0.0;
        PFOR(i, nC) { Sc[i] = 0; posAC[i] = -1; }
        SYNC();
        if (lane == 0) {
            int n = 0;
            for (int v = 0; v < nV; v++)
                if (Sb[v] == 0) Q[(n++) * ld + v] = 1.0;
            iscal[0] = n;
        }
        SYNC();
        nFR = iscal[0];
        nAC = 0;
        // products with x = 0 / y = 0 (a cold start) are zero vectors: no need to walk the matrices
        if (x0) A_times(x, Ax); else { PFOR(i, nC) Ax[i] = 0.0; SYNC(); }
        for (int i = 0; i < nC; i++) {
            int s = 0;
            if (guess_c) s = (int)wc1[i];
            else if (y0 && (!x0 || cy0)) s = y[nV + i] > RSQP_EPS ? -1 : (y[nV + i] < -RSQP_EPS ? 1 : 0);
            else if (x0) s = Ax[i] <= lbAN[i] + RSQP_BOUND_TOLERANCE ? -1 : (Ax[i] >= ubAN[i] - RSQP_BOUND_TOLERANCE ? 1 : 0);
            if (s == -1 && lbAN[i] <= -RSQP_INFTY) s = 0;
            if (s == 1 && ubAN[i] >= RSQP_INFTY) s = 0;
            if (s != 0 && constraint_is_LI(i)) add_constraint(i, s, false, false);
        }
        PFOR(v, nV) {
            double yv = y[v];
            if (Sb[v] == 0 || (Sb[v] == -1 && yv < 0.0) || (Sb[v] == 1 && yv > 0.0)) y[v] = 0.0;
        }
        PFOR(i, nC) {
            double yi = y[nV + i];
            if (Sc[i] == 0 || (Sc[i] == -1 && yi < 0.0) || (Sc[i] == 1 && yi > 0.0)) y[nV + i] = 0.0;
        }
        SYNC();
        if (y0) AT_times(y + nV, wv1); else { PFOR(v, nV) wv1[v] = 0.0; }
        if (x0) H_times(x, wv2); else { PFOR(v, nV) wv2[v] = 0.0; }
        SYNC();
        PFOR(v, nV) {
            double xv = x[v];
            g[v] = wv1[v] + y[v] - wv2[v];
            lb[v] = Sb[v] == -1 ? xv : fmin(lbN[v], xv - RSQP_BOUND_RELAXATION);
            ub[v] = Sb[v] == 1 ? xv : fmax(ubN[v], xv + RSQP_BOUND_RELAXATION);
        }
        PFOR(i, nC) {
            double ax = Ax[i];
            lbA[i] = Sc[i] == -1 ? ax : fmin(lbAN[i], ax - RSQP_BOUND_RELAXATION);
            ubA[i] = Sc[i] == 1 ? ax : fmax(ubAN[i], ax + RSQP_BOUND_RELAXATION);
        }
        SYNC();
        if (!chol_setup()) return RET_SETUP_FAILED;
        status = QPS_AUXILIARYQPSOLVED;
        return RET_OK;
    }

    // ------------------------------------------------------------------ step direction
    __device__ __forceinline__ static double delta_of(double target, double cur) {
        return (fabs(target) >= RSQP_INFTY && fabs(cur) >= RSQP_INFTY) ? 0.0 : target - cur;
    }

    __device__ __forceinline__ void step_direction() {
        int nZ = nFR - nAC;
        PFOR(v, nV) dx[v] = Sb[v] == -1 ? delta_of(lbN[v], lb[v]) : (Sb[v] == 1 ? delta_of(ubN[v], ub[v]) : 0.0);
        PFOR(i, nV + nC) dy[i] = 0.0;
        SYNC();
        A_times(dx, wc2);
        // without a null space (nZ == 0: every free direction is pinned by an active constraint -- the
        // whole cold-start phase of hs0xx-scale problems) the projected-gradient part below is empty:
        // its two Hessian products are skipped, nothing else depends on them
        if (nZ > 0) H_times(dx, wv2);
        PFOR(i, nAC) {
            int r = AC[i];
            wc1[i] = (Sc[r] == -1 ? delta_of(lbAN[r], lbA[r]) : delta_of(ubAN[r], ubA[r])) - wc2[r];
        }
        if (nZ > 0) { PFOR(v, nV) wv1[v] = (gN[v] - g[v]) + wv2[v]; }  // tmpg
        PFOR(c, nFR) wq[c] = 0.0;
        SYNC();
        // range space: T wY = bA (column oriented)
        for (int i = 0; i < nAC; i++) {
            int c = nFR - 1 - i;
            double w = wc1[i] / T[i * ld + c];
            SYNC();
            if (lane == 0) wq[c] = w;
            for (int ii = i + 1 + lane; ii < nAC; ii += L) wc1[ii] -= T[ii * ld + c] * w;
            SYNC();
        }
        PFOR(v, nV) {
            double s = 0.0;
            for (int c = nZ; c < nFR; c++) s += Q[c * ld + v] * wq[c];
            wv3[v] = s;  // xY
        }
        SYNC();
        // null space: R'R wZ = -Z'(tmpg + H xY)
        if (nZ > 0) {
            H_times(wv3, wv2);
            PFOR(v, nV) wv2[v] += wv1[v];
            SYNC();
        }
        PFOR(j, nZ) {
            const ldouble *qj = Q + j * ld;
            double s = 0.0;
            for (int v = 0; v < nV; v++) s += qj[v] * wv2[v];
            wq[j] = -s;
        }
        SYNC();
        for (int j = 0; j < nZ; j++) {
            double u = wq[j] / R[RIX(j, j)];
            SYNC();
            if (lane == 0) wq[j] = u;
            for (int k = j + 1 + lane; k < nZ; k += L) wq[k] -= R[RIX(k, j)] * u;
            SYNC();
        }
        for (int j = nZ - 1; j >= 0; j--) {
            double w = wq[j] / R[RIX(j, j)];
            SYNC();
            if (lane == 0) wq[j] = w;
            for (int k = lane; k < j; k += L) wq[k] -= R[RIX(j, k)] * w;
            SYNC();
        }
        PFOR(v, nV) {
            if (Sb[v] == 0) {
                double s = wv3[v];
                for (int j = 0; j < nZ; j++) s += Q[j * ld + v] * wq[j];
                dx[v] = s;
            }
        }
        SYNC();
        // multipliers of the active constraints: T' dyAC = Y'(H dx + dg)
        H_times(dx, wv2);
        PFOR(v, nV) wv2[v] += gN[v] - g[v];
        SYNC();
        for (int c = nZ + lane; c < nFR; c += L) {
            const ldouble *qc = Q + c * ld;
            double s = 0.0;
            for (int v = 0; v < nV; v++) s += qc[v] * wv2[v];
            wq[c] = s;
        }
        SYNC();
        for (int m = 0; m < nAC; m++) {
            int i = nAC - 1 - m, c = nZ + m;
            const ldouble *ri = T + i * ld;
            double d = wq[c] / ri[c];
            SYNC();
            if (lane == 0) dy[nV + AC[i]] = d;
            for (int cc = c + 1 + lane; cc < nFR; cc += L) wq[cc] -= ri[cc] * d;
            SYNC();
        }
        if (nAC > 0) AT_times(dy + nV, wv3); else { PFOR(v, nV) wv3[v] = 0.0; SYNC(); }   // no active constraint: dy_C = 0
        PFOR(v, nV) dy[v] = Sb[v] != 0 ? wv2[v] - wv3[v] : 0.0;
        A_times(dx, dAx);
    }

    // ------------------------------------------------------------------ ratio tests
    __device__ __forceinline__ static void cand(double num, double den, int id, double &bt, int &bid) {
        // the quotient does not wait for the comparison with the running minimum (two candidates of a
        // lane divide back to back); a rejected denominator only wastes a division
        const double t = (num > 0.0 ? num : 0.0) / den;
        if (den >= RSQP_EPS_DEN && (t < bt || (t == bt && id < bid))) { bt = t; bid = id; }
    }
    // candidate ids: [0,nC) active constr. duals, [nC,nC+nV) fixed-variable duals,
    // then inactive constr. lower / upper, then free variables lower / upper
    __device__ __forceinline__ Blocking ratio_tests() {
        double bt = 1.0;
        int bid = 0x7fffffff;
        PFOR(i, nC) {
            double Axi = Ax[i], dA = dAx[i];
            if (Sc[i] != 0) {
                double yi = y[nV + i], d = dy[nV + i];
                if (Sc[i] == -1) cand(yi, -d, i, bt, bid); else cand(-yi, d, i, bt, bid);
            } else {
                if (lbAN[i] > -RSQP_INFTY) cand(Axi - lbA[i], delta_of(lbAN[i], lbA[i]) - dA, nC + nV + i, bt, bid);
                if (ubAN[i] < RSQP_INFTY) cand(ubA[i] - Axi, dA - delta_of(ubAN[i], ubA[i]), 2 * nC + nV + i, bt, bid);
            }
        }
        PFOR(v, nV) {
            if (Sb[v] != 0) {
                double yi = y[v], d = dy[v];
                if (Sb[v] == -1) cand(yi, -d, nC + v, bt, bid); else cand(-yi, d, nC + v, bt, bid);
            } else {
                if (lbN[v] > -RSQP_INFTY) cand(x[v] - lb[v], delta_of(lbN[v], lb[v]) - dx[v], 3 * nC + nV + v, bt, bid);
                if (ubN[v] < RSQP_INFTY) cand(ub[v] - x[v], dx[v] - delta_of(ubN[v], ub[v]), 3 * nC + 2 * nV + v, bt, bid);
            }
        }
        // a candidate only blocks if it is strictly inside the step (t < 1)
        if (!(bt < 1.0)) { bt = 1.0; bid = 0x7fffffff; }
        block_argmin(bt, bid);
        Blocking b;
        b.tau = bt; b.kind = 0; b.idx = -1; b.side = 0;
        if (bid != 0x7fffffff) {
            if (bid < nC) { b.kind = 1; b.idx = bid; }
            else if (bid < nC + nV) { b.kind = 2; b.idx = bid - nC; }
            else if (bid < 2 * nC + nV) { b.kind = 3; b.idx = bid - nC - nV; b.side = -1; }
            else if (bid < 3 * nC + nV) { b.kind = 3; b.idx = bid - 2 * nC - nV; b.side = 1; }
            else if (bid < 3 * nC + 2 * nV) { b.kind = 4; b.idx = bid - 3 * nC - nV; b.side = -1; }
            else { b.kind = 4; b.idx = bid - 3 * nC - 2 * nV; b.side = 1; }
        }
        return b;
    }

    // ------------------------------------------------------------------ removal with guard
    __device__ __forceinline__ int remove_with_guard(bool is_bound, int idx) {
        if (is_bound) {
            int old = Sb[idx];
            SYNC();
            int zc = remove_bound_tq(idx);
            if (lane == 0) y[idx] = 0.0;
            SYNC();
            if (chol_append(zc)) return RET_OK;
            if ((old == -1 && ubN.template bcast<L>(idx) >= RSQP_INFTY) || (old == 1 && lbN.template bcast<L>(idx) <= -RSQP_INFTY)) {
                add_bound(idx, old, false, true);
                return RET_UNBOUNDED;
            }
            add_bound(idx, -old, false, true);
            if (lane == 0) { if (old == -1) ub[idx] = x[idx]; else lb[idx] = x[idx]; }
            nflips++;
            SYNC();
            return RET_OK;
        } else {
            int old = Sc[idx], k = posAC[idx];
            SYNC();
            int zc = remove_constraint_tq(k);
            if (lane == 0) y[nV + idx] = 0.0;
            SYNC();
            if (chol_append(zc)) return RET_OK;
            if ((old == -1 && ubAN[idx] >= RSQP_INFTY) || (old == 1 && lbAN[idx] <= -RSQP_INFTY)) {
                add_constraint(idx, old, false, true);
                return RET_UNBOUNDED;
            }
            add_constraint(idx, -old, false, true);
            if (lane == 0) { if (old == -1) ubA[idx] = Ax[idx]; else lbA[idx] = Ax[idx]; }
            nflips++;
            SYNC();
            return RET_OK;
        }
    }

    // ------------------------------------------------------------------ exchange
    // a_full in wv4. Shifts the multipliers; returns partner in (pkind, pidx)
    __device__ __forceinline__ int ensure_LI(int side, double &y_new, int &pkind, int &pidx) {
        int nZ = nFR - nAC;
        PFOR(v, nV) wv1[v] = Sb[v] == 0 ? wv4[v] : 0.0;
        PFOR(i, nC) wc2[i] = 0.0;
        SYNC();
        QT_times(wv1, wq);
        for (int m = 0; m < nAC; m++) {
            int i = nAC - 1 - m, c = nZ + m;
            const ldouble *ri = T + i * ld;
            double d = wq[c] / ri[c];
            SYNC();
            if (lane == 0) wc2[AC[i]] = d;
            for (int cc = c + 1 + lane; cc < nFR; cc += L) wq[cc] -= ri[cc] * d;
            SYNC();
        }
        if (nAC > 0) AT_times(wc2, wv2); else { PFOR(v, nV) wv2[v] = 0.0; SYNC(); }   // xi_C = 0 without active constraints
        PFOR(v, nV) wv2[v] = Sb[v] != 0 ? wv4[v] - wv2[v] : 0.0;  // xiB
        SYNC();
        double sgn = side == 1 ? -1.0 : 1.0;
        double bt = RSQP_INFTY;
        int bid = 0x7fffffff;
        PFOR(i, nC) {
            if (Sc[i] != 0) {
                double xi = sgn * wc2[i], yi = y[nV + i];
                double num = Sc[i] == -1 ? yi : -yi, den = Sc[i] == -1 ? xi : -xi;
                if (den > RSQP_EPS_DEN) {
                    double t = (num > 0.0 ? num : 0.0) / den;
                    if (t < bt || (t == bt && i < bid)) { bt = t; bid = i; }
                }
            }
        }
        PFOR(v, nV) {
            if (Sb[v] != 0) {
                double xi = sgn * wv2[v], yi = y[v];
                double num = Sb[v] == -1 ? yi : -yi, den = Sb[v] == -1 ? xi : -xi;
                if (den > RSQP_EPS_DEN) {
                    double t = (num > 0.0 ? num : 0.0) / den;
                    if (t < bt || (t == bt && nC + v < bid)) { bt = t; bid = nC + v; }
                }
            }
        }
        block_argmin(bt, bid);
        if (bid == 0x7fffffff) return RET_INFEASIBLE;
        PFOR(i, nC) if (Sc[i] != 0) y[nV + i] -= bt * sgn * wc2[i];
        PFOR(v, nV) if (Sb[v] != 0) y[v] -= bt * sgn * wv2[v];
        SYNC();
        y_new = sgn * bt;
        pkind = bid < nC ? 1 : 2;
        pidx = bid < nC ? bid : bid - nC;
        return RET_OK;
    }

    __device__ __forceinline__ bool remove_partner(int pkind, int pidx) {
        int zc;
        if (pkind == 1) {
            int k = posAC[pidx];
            SYNC();
            zc = remove_constraint_tq(k);
            if (lane == 0) y[nV + pidx] = 0.0;
        } else {
            zc = remove_bound_tq(pidx);
            if (lane == 0) y[pidx] = 0.0;
        }
        SYNC();
        return chol_append(zc);
    }

    __device__ __forceinline__ int change_active_set(const Blocking &b) {
        if (b.kind == 1) return remove_with_guard(false, b.idx);
        if (b.kind == 2) return remove_with_guard(true, b.idx);
        if (b.kind == 3 || b.kind == 4) {
            double ynew = 0.0;
            bool full = true;
            bool li = b.kind == 3 ? constraint_is_LI(b.idx) : bound_is_LI(b.idx);
            if (!li) {
                int pkind = 0, pidx = -1;
                if (b.kind == 3) row_of_A(b.idx, wv4, true);
                else { PFOR(v, nV) wv4[v] = v == b.idx ? 1.0 : 0.0; SYNC(); }
                int rc_ = ensure_LI(b.side, ynew, pkind, pidx);
                if (rc_ != RET_OK) return rc_;
                full = remove_partner(pkind, pidx);
            }
            if (b.kind == 3) {
                add_constraint(b.idx, b.side, full, !full);
                if (lane == 0) y[nV + b.idx] = ynew;
            } else {
                add_bound(b.idx, b.side, full, !full);
                if (lane == 0) y[b.idx] = ynew;
            }
            SYNC();
        }
        return RET_OK;
    }

    // ------------------------------------------------------------------ homotopy
    __device__ __forceinline__ void drift_correction() {
        PFOR(v, nV) if (Sb[v] != 0) x[v] = Sb[v] == -1 ? lb[v] : ub[v];
        SYNC();
        A_times(x, Ax);
        PFOR(i, nC) { if (Sc[i] == -1) lbA[i] = Ax[i]; else if (Sc[i] == 1) ubA[i] = Ax[i]; }
        PFOR(v, nV) {   // A'y_C and H x of variable v in one pass, then the gradient from stationarity
            const double aty = sparse_dot(Air, Aval, y + nV, Ajc[v], Ajc[v + 1]);
            const double hx = (haveH ? sparse_dot(Hir, Hval, x, Hjc[v], Hjc[v + 1]) : 0.0) + hreg * x[v];
            g[v] = aty + y[v] - hx;
        }
        SYNC();
    }

    __device__ __forceinline__ int homotopy(int maxit, int &nWSR) {
        int iter = 0, rcode = RET_OK;
        status = QPS_PERFORMINGHOMOTOPY;
        PFOR(v, nV) {
            if (Sb[v] != -1 && lb[v] <= -RSQP_INFTY && lbN[v] > -RSQP_INFTY) lb[v] = fmin(lbN[v], x[v] - RSQP_BOUND_RELAXATION);
            if (Sb[v] != 1 && ub[v] >= RSQP_INFTY && ubN[v] < RSQP_INFTY) ub[v] = fmax(ubN[v], x[v] + RSQP_BOUND_RELAXATION);
        }
        PFOR(i, nC) {
            if (Sc[i] != -1 && lbA[i] <= -RSQP_INFTY && lbAN[i] > -RSQP_INFTY) lbA[i] = fmin(lbAN[i], Ax[i] - RSQP_BOUND_RELAXATION);
            if (Sc[i] != 1 && ubA[i] >= RSQP_INFTY && ubAN[i] < RSQP_INFTY) ubA[i] = fmax(ubAN[i], Ax[i] + RSQP_BOUND_RELAXATION);
        }
        SYNC();
        for (;;) {
            STAMP(7);
            step_direction();
            STAMP(3);
            Blocking b = ratio_tests();
            STAMP(4);
            double tau = b.tau;
            bool done = b.kind == 0;
            PFOR(v, nV) {
                if (done) {
                    g[v] = gN[v]; lb[v] = lbN[v]; ub[v] = ubN[v];
                    x[v] = Sb[v] == -1 ? lb[v] : (Sb[v] == 1 ? ub[v] : x[v] + tau * dx[v]);
                } else {
                    x[v] += tau * dx[v];
                    g[v] += tau * (gN[v] - g[v]);
                    lb[v] += tau * delta_of(lbN[v], lb[v]);
                    ub[v] += tau * delta_of(ubN[v], ub[v]);
                }
            }
            PFOR(i, nV + nC) y[i] += tau * dy[i];
            PFOR(i, nC) {
                if (done) { lbA[i] = lbAN[i]; ubA[i] = ubAN[i]; }
                else {
                    lbA[i] += tau * delta_of(lbAN[i], lbA[i]); ubA[i] += tau * delta_of(ubAN[i], ubA[i]);
                    // A x follows the step by its increment (dAx, a by-product of the step direction). Until the exact
                    // product in drift_correction only Ax[blocking] / Ax[flipped] are read, and only into bounds that
                    // drift_correction overwrites with the exact product once the constraint is active
                    Ax[i] += tau * dAx[i];
                }
            }
            SYNC();
            if (done) A_times(x, Ax);
            STAMP(5);
            if (done) { status = QPS_SOLVED; break; }
            if (iter >= maxit) { rcode = RET_MAX_NWSR; break; }
            if (lane == 0) {
                if (b.kind == 3) { if (b.side == -1) lbA[b.idx] = Ax[b.idx]; else ubA[b.idx] = Ax[b.idx]; }
                else if (b.kind == 4) { if (b.side == -1) lb[b.idx] = x[b.idx]; else ub[b.idx] = x[b.idx]; }
            }
            SYNC();
            rcode = change_active_set(b);
            STAMP(6);
            if (rcode == RET_INFEASIBLE) { infeasible = 1; break; }
            if (rcode == RET_UNBOUNDED) { unbounded = 1; break; }
            iter++;
            drift_correction();
        }
        nWSR = iter;
        return rcode;
    }

    __device__ __forceinline__ bool bounds_inconsistent() {
        double bad = 0.0;
        PFOR(v, nV) if (lbN[v] > ubN[v] + RSQP_EPS) bad += 1.0;
        PFOR(i, nC) if (lbAN[i] > ubAN[i] + RSQP_EPS) bad += 1.0;
        return block_sum(bad) > 0.0;
    }
    __device__ __forceinline__ void restore(int nFR_, int nAC_, int status_) { nFR = nFR_; nAC = nAC_; status = status_; }

    __device__ __forceinline__ double objective() {
        H_times(x, wv2);
        double bs = 0.0;
        PFOR(i, nV) bs += gN[i] * x[i];
        double a = dot(x, wv2, nV), b = block_sum(bs), c = dot(x, x, nV);
        return 0.5 * (a - hreg * c) + b;
    }
};
