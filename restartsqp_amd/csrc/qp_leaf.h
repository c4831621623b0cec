// qp_leaf.h -- leaf helpers of the tableau kernels (qp_tiny.hip, qp_lane.hip, qp_small_g.h), one copy. Included inside the unit's
// namespace. (The null-space engines keep clampinf as a member, and their lane exchanges serve more lanes: qp_small_engine.h.)
// a value the compiler must not look through: a one-hot weight (a == k ? 1.0 : 0.0) that multiplies register-array entries is
// otherwise recognised as a select and turned into an INDEXED load from a copy of the array in scratch memory
__device__ __forceinline__ double opaque(double v) { asm volatile("" : "+v"(v)); return v; }
__device__ __forceinline__ double clampinf(double v) { return v > RSQP_INFTY ? RSQP_INFTY : (v < -RSQP_INFTY ? -RSQP_INFTY : v); }
__device__ __forceinline__ double recip(double x) {      // v_rcp_f64 + two Newton steps: ~2^-52 relative, the same bits in every lane
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0); y = fma(y, e, y);
    e = fma(-x, y, 1.0); y = fma(y, e, y);
    return y;
}
