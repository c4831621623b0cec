// qp_band_check.h -- the check entry points of include/rsqp_hip_band_check.h: the banded H^-1 operator called the way the engine
// calls it. Included by qp_large.hip behind qp_rs_path.h, whose band_factor_host / band_build_of / band_dispatch do the work: nothing
// of the operator is restated here. Every argument is judged on the host before the first device call.
#pragma once
#include "../../include/rsqp_hip_band_check.h"

static_assert(RSQP_BAND_MAX_N == BAND_MAX_N && RSQP_BAND_THREADS == BAND_TH, "rsqp_hip_band_check.h states the kernels' sizes");

struct rsqp_band_check {
    BandFactor f;               // the host's image; it goes up with the first product (create needs no device)
    BandOp op{};
    double *buf = nullptr;      // the factor's image + agg, as Impl::band_buf
    int *err = nullptr;
    double seq = 0.0;           // as Impl::band_seq
};

namespace {
#define BCHK(call) do { if ((call) != hipSuccess) return -2; } while (0)
struct BandDev {      // device memory of one call
    void *p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 8)); }
    template <class T> hipError_t put(const T *host, size_t n) {
        hipError_t e = alloc(sizeof(T) * n);
        return e != hipSuccess ? e : hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice);
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
    ~BandDev() { if (p) (void)hipFree(p); }
};
// ncols columns of n rows at `off` with leading dimension ld lie inside a buffer of len doubles
bool band_window_ok(const double *buf, long long len, long long off, long long ld, long long n, long long ncols) {
    if (!buf || len < 1 || off < 0 || off > len || n < 1 || ncols < 1 || ld < n) return false;
    return (ncols - 1) <= (len - off - n) / ld && off + (ncols - 1) * ld + n <= len;
}
// the factor, a zero-filled agg and a zero err word on the device, once per handle (as Impl::rs_build_band leaves them)
hipError_t band_check_upload(rsqp_band_check *h) {
    if (h->buf) return hipSuccess;
    const BandFactor &f = h->f;
    double *buf = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&buf), sizeof(double) * f.buf.size());
    if (e != hipSuccess) return e;
    if (!h->err) e = hipMalloc(reinterpret_cast<void **>(&h->err), sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(buf, f.buf.data(), sizeof(double) * f.buf.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->err, 0, sizeof(int));
    if (e == hipSuccess) e = band_set_attributes();
    if (e != hipSuccess) { (void)hipFree(buf); return e; }
    h->buf = buf;
    h->op.m1i = buf; h->op.m2i = buf + f.off_m2i(); h->op.sinv = buf + f.off_sinv(); h->op.agg = buf + f.off_agg();
    h->op.err = h->err;
    return hipSuccess;
}
int band_check_finish(rsqp_band_check *h, int *err, long long *seq) {
    BCHK(hipDeviceSynchronize());
    BCHK(hipMemcpy(err, h->err, sizeof(int), hipMemcpyDeviceToHost));
    *seq = (long long)h->seq;
    return 0;
}
}  // namespace

extern "C" int rsqp_band_check_factor(int n, const double *d0, const double *e1, const double *e2, int *built, int *c, int *build,
                                      double *growth, double *m1i, long long len1, double *m2i, long long len2, double *sinv,
                                      long long lens) {
    if (!built || !c || !build || !growth) return -1;
    if (n < 1 || n > BAND_MAX_N) { *built = 0; *c = 0; *build = 0; *growth = -1.0; return 0; }
    const long long cc = (n + BAND_TH - 1) / BAND_TH;
    if (!d0 || !e1 || !e2 || !m1i || !m2i || !sinv || len1 < BAND_TH * (cc + 1) || len2 < BAND_TH * (cc + 2) || lens < n) return -1;
    BandFactor f;
    band_factor_host(n, d0, e1, e2, &f);
    *built = f.built ? 1 : 0; *c = f.c; *build = band_build_of(f.c); *growth = f.growth;
    if (f.built) {
        std::copy(f.buf.begin(), f.buf.begin() + f.off_m2i(), m1i);
        std::copy(f.buf.begin() + f.off_m2i(), f.buf.begin() + f.off_sinv(), m2i);
        std::copy(f.buf.begin() + f.off_sinv(), f.buf.begin() + f.off_agg(), sinv);
    }
    return 0;
}

extern "C" int rsqp_band_check_create(int n, const double *d0, const double *e1, const double *e2, rsqp_band_check **out) {
    if (!out || !d0 || !e1 || !e2 || n < 1 || n > BAND_MAX_N) return -1;
    rsqp_band_check *h = new rsqp_band_check();
    band_factor_host(n, d0, e1, e2, &h->f);
    if (!h->f.built) { delete h; return -1; }
    h->op.n = n; h->op.c = h->f.c;
    *out = h;
    return 0;
}

extern "C" int rsqp_band_check_destroy(rsqp_band_check *h) {
    if (!h) return -1;
    if (h->buf) (void)hipFree(h->buf);
    if (h->err) (void)hipFree(h->err);
    delete h;
    return 0;
}

extern "C" int rsqp_band_check_apply(rsqp_band_check *h, int kernel, int ncols, long long ld, int inplace, double *in,
                                     long long len_in, long long off_in, const double *sub, long long len_sub, long long off_sub,
                                     double *out, long long len_out, long long off_out, int *err, long long *seq) {
    if (!h || !err || !seq || (kernel != RSQP_BAND_KERNEL_ENGINE && kernel != RSQP_BAND_KERNEL_1WG)) return -1;
    const int n = h->op.n;
    if (!band_window_ok(in, len_in, off_in, ld, n, ncols)) return -1;
    if (!inplace && !band_window_ok(out, len_out, off_out, ld, n, ncols)) return -1;
    if (sub && !band_window_ok(sub, len_sub, off_sub, n, n, 1)) return -1;
    BCHK(band_check_upload(h));
    BandDev di, ds, dout;
    BCHK(di.put(in, (size_t)len_in));
    if (sub) BCHK(ds.put(sub, (size_t)len_sub));
    if (!inplace) BCHK(dout.put(out, (size_t)len_out));
    const double *pin = di.as<double>() + off_in, *psub = sub ? ds.as<double>() + off_sub : nullptr;
    double *pout = inplace ? di.as<double>() + off_in : dout.as<double>() + off_out;
    band_dispatch(h->op, &h->seq, kernel == RSQP_BAND_KERNEL_1WG, ncols, pin, psub, pout, ld, BandQ{}, nullptr);
    BCHK(hipGetLastError());
    const int rc = band_check_finish(h, err, seq);
    if (rc != 0) return rc;
    BCHK(hipMemcpy(in, di.p, sizeof(double) * (size_t)len_in, hipMemcpyDeviceToHost));
    if (!inplace) BCHK(hipMemcpy(out, dout.p, sizeof(double) * (size_t)len_out, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rsqp_band_check_apply_q(rsqp_band_check *h, int kernel, const int *Sb, const double *ATdy, const double *dy,
                                       const double *gN, const double *g, double *Hdx, long long len_h, long long off_h, double *dx,
                                       long long len_x, long long off_x, int *err, long long *seq) {
    if (!h || !err || !seq || !Sb || !ATdy || !dy || !gN || !g) return -1;
    if (kernel != RSQP_BAND_KERNEL_ENGINE && kernel != RSQP_BAND_KERNEL_1WG) return -1;
    const int n = h->op.n;
    if (!band_window_ok(Hdx, len_h, off_h, n, n, 1) || !band_window_ok(dx, len_x, off_x, n, n, 1)) return -1;
    BCHK(band_check_upload(h));
    BandDev dSb, dA, dY, dN, dG, dH, dX;
    BCHK(dSb.put(Sb, (size_t)n)); BCHK(dA.put(ATdy, (size_t)n)); BCHK(dY.put(dy, (size_t)n)); BCHK(dN.put(gN, (size_t)n));
    BCHK(dG.put(g, (size_t)n)); BCHK(dH.put(Hdx, (size_t)len_h)); BCHK(dX.put(dx, (size_t)len_x));
    BandQ q{};
    q.Sb = dSb.as<int>(); q.ATdy = dA.as<double>(); q.dy = dY.as<double>(); q.gN = dN.as<double>(); q.g = dG.as<double>();
    q.Hdx = dH.as<double>() + off_h;
    // (the engine's call: band_launch(1, in, sub, out, 0, true) -- in and sub are not read in this form)
    band_dispatch(h->op, &h->seq, kernel == RSQP_BAND_KERNEL_1WG, 1, nullptr, nullptr, dX.as<double>() + off_x, 0LL, q, nullptr);
    BCHK(hipGetLastError());
    const int rc = band_check_finish(h, err, seq);
    if (rc != 0) return rc;
    BCHK(hipMemcpy(Hdx, dH.p, sizeof(double) * (size_t)len_h, hipMemcpyDeviceToHost));
    BCHK(hipMemcpy(dx, dX.p, sizeof(double) * (size_t)len_x, hipMemcpyDeviceToHost));
    return 0;
}
#undef BCHK
