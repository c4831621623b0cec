"""What deciding a batch's SQP steps costs on 65 536 one-pattern hs071 members (n = 4, m = 2), on the device and through the host.

    python tools/nlp_step_sweep.py [--nq 65536] [--iters 30] > profiles/nlp_step_sweep.txt

device  one rsqp_batch_handler_ratio_test plus one rsqp_batch_handler_check_optimality with device pointers: the device time of each,
        taken with the batch's own stopwatch (rsqp_batch_timer_start / _stop_ms around the one library call, its argument struct
        built beforehand: the stopwatch counts the host's way to the launch as well), median over --iters; and the wall time of
        the two calls through the binding. With the bytes each kernel has to move per member (every input read once, every output written
        once; the pattern arrays of the one-pattern batch are cache-resident and not counted) that gives the achieved bytes per
        second, set against the HBM peak of 8.0 TB/s (6.29 TB/s measured for a float4 copy).
host    what the host route cannot avoid around the same decision, whatever the CPU arithmetic costs: the wall time of
        handler_step(on_device=False) -- p, lam_c, lam_x, norm_p, infea_model down -- plus handler_update with host what, delta,
        rho, x_k, c_k (DELTA words: the smallest update a decision leads to). These two calls are the parent commit's, unchanged.
One JSON line per route, then a summary line. torch is imported first (capi.device_torch)."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (before anything loads librsqp_hip.so)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
from restartsqp_amd import capi, problems  # noqa: E402

WARMUP = 3
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    nq, n, m = a.nq, 4, 2
    rng = np.random.default_rng(17)
    base, nlp = problems.hs071_first_qp(), problems.hs071_nlp()
    b = capi.Batch([base] * nq)
    b.handler_set_problem(*[np.tile(nlp[k], nq) for k in ("x_l", "x_u", "c_l", "c_u")])
    x0, c0, g0 = np.array([1.0, 5.0, 5.0, 1.0]), np.array([25.0, 52.0]), np.array([12.0, 1.0, 2.0, 11.0])
    x_k = np.clip(x0 * (1.0 + 0.02 * rng.normal(size=(nq, n))), 1.0, 5.0).reshape(-1)
    c_k = (c0 * (1.0 + 0.02 * rng.normal(size=(nq, m)))).reshape(-1)
    grad = (g0 * (1.0 + 0.02 * rng.normal(size=(nq, n)))).reshape(-1)
    ones = np.ones(nq)
    b.handler_update(np.full(nq, capi.HU_SET, np.int32), ones, ones, x_k, c_k, grad)
    b.optimize_qp()
    solved = sum(1 for s in b.results()[:256] if s["status"] == 20)
    med = lambda v: float(np.median(v))

    # ---- device route ----
    dev = lambda v, dt=np.float64: torch.as_tensor(np.ascontiguousarray(v, dtype=dt), device="cuda")
    what = dev(np.ones(nq), np.int32)
    infea = b.handler_infeasibility(dev(c_k), on_device=True)
    # every second member's trial point is better by 1 with the same constraint values (accepted: x_k, c_k, f_k, infea_k are
    # rewritten), the others' worse by 1 (rejected: delta alone); f_k is put back before every call, so each decides the same way
    f_k = 16.0 + 0.1 * rng.normal(size=nq)
    trial = dict(what=what, rho=dev(ones), f_trial=dev(f_k + np.where(np.arange(nq) % 2 == 0, -1.0, 1.0)), c_trial=dev(c_k),
                 x_k=dev(x_k), c_k=dev(c_k), f_k=dev(f_k), infea_k=infea.clone(), delta=dev(ones))
    point = dict(what=what, x_k=trial["x_k"], grad=dev(grad), c_k=trial["c_k"], infea=trial["infea_k"])
    out = {k: torch.zeros(nq, dtype=torch.int32 if k in capi.NlpTrial.INTS else torch.float64, device="cuda") for k in capi.NlpTrial.OUT}
    st, verdict = torch.zeros((nq, 5), dtype=torch.float64, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda")
    o = capi.NlpStepOptions(refresh_ubA=1)
    torch.cuda.synchronize()
    # the stopwatch covers the stream time between its two events, the host's way to the launch included: the argument structs are
    # therefore built once, outside it, and the library is called directly; the wall time is that of the binding's calls as a
    # driver makes them
    import ctypes as C
    L = capi.lib()
    ct = capi.NlpTrial(**{k: v.data_ptr() for k, v in dict(trial, **out).items()})
    cp = capi.NlpPoint(**{k: v.data_ptr() for k, v in point.items()})
    a_t, a_p, a_o = C.addressof(ct), C.addressof(cp), C.addressof(o)
    ms_ratio, ms_kkt, wall = [], [], []
    f_k0 = trial["f_k"].clone()
    for k in range(WARMUP + a.iters):
        trial["f_k"].copy_(f_k0); torch.cuda.synchronize()
        b.timer_start()
        capi.check(L.rsqp_batch_handler_ratio_test(b._h, a_t, a_o, 1))
        r = b.timer_stop_ms()
        b.timer_start()
        capi.check(L.rsqp_batch_handler_check_optimality(b._h, a_p, a_o, st.data_ptr(), verdict.data_ptr(), 1))
        c = b.timer_stop_ms()
        trial["f_k"].copy_(f_k0); torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.handler_ratio_test(options=o, on_device=True, out=out, **trial)
        b.handler_check_optimality(options=o, on_device=True, out=st, verdict=verdict, **point)
        t1 = time.perf_counter()
        if k >= WARMUP:
            ms_ratio.append(r); ms_kkt.append(c); wall.append(1e3 * (t1 - t0))
    accepted = int(out["accept"].sum().item())
    # bytes per member, every array once: (what, rho, f_trial, obj | c_trial, c_l, c_u | p, x_k in and out | c_k out | f_k, infea_k,
    # delta in and out | 3 doubles and 4 ints out), (what, infea | x_k, grad, x_l, x_u, lam_x | c_k, c_l, c_u, lam_c | J | 5 doubles, 1 int out)
    bytes_ratio = (4 + 3 * 8) + 3 * 8 * m + 3 * 8 * n + 8 * m + 6 * 8 + (3 * 8 + 4 * 4)
    bytes_kkt = (4 + 8) + 5 * 8 * n + 4 * 8 * m + 8 * n * m + (5 * 8 + 4)
    rate = lambda byts, ms: nq * byts / (1e-3 * ms)
    device = dict(route="device", nq=nq, iters=a.iters, solved_of_first_256=solved, accepted=accepted,
                  ms_device_median=dict(ratio_test=round(med(ms_ratio), 5), check_optimality=round(med(ms_kkt), 5),
                                        both=round(med(ms_ratio) + med(ms_kkt), 5)),
                  ms_wall_median_both_calls=round(med(wall), 4), bytes_per_member=dict(ratio_test=bytes_ratio, check_optimality=bytes_kkt),
                  TB_per_s=dict(ratio_test=round(rate(bytes_ratio, med(ms_ratio)) / 1e12, 4), check_optimality=round(rate(bytes_kkt, med(ms_kkt)) / 1e12, 4)),
                  fraction_of_hbm_peak_8TBs=dict(ratio_test=round(rate(bytes_ratio, med(ms_ratio)) / HBM_PEAK, 4),
                                                 check_optimality=round(rate(bytes_kkt, med(ms_kkt)) / HBM_PEAK, 4)),
                  fraction_of_measured_copy_6_29TBs=dict(ratio_test=round(rate(bytes_ratio, med(ms_ratio)) / HBM_COPY, 4),
                                                         check_optimality=round(rate(bytes_kkt, med(ms_kkt)) / HBM_COPY, 4)))
    print(json.dumps(device), flush=True)

    # ---- host route: the transfers around a decision on the CPU ----
    hx, hc, hd = trial["x_k"].cpu().numpy(), trial["c_k"].cpu().numpy(), trial["delta"].cpu().numpy()
    words = np.full(nq, capi.HU_DELTA, np.int32)
    ms_step, ms_update = [], []
    for k in range(WARMUP + a.iters):
        t0 = time.perf_counter()
        s = b.handler_step(on_device=False)
        t1 = time.perf_counter()
        b.handler_update(words, hd, ones, hx, hc)
        t2 = time.perf_counter()
        if k >= WARMUP:
            ms_step.append(1e3 * (t1 - t0)); ms_update.append(1e3 * (t2 - t1))
    host = dict(route="host", nq=nq, iters=a.iters, checksum=float(s["norm_p"].sum()),
                ms_wall_median=dict(handler_step=round(med(ms_step), 4), handler_update=round(med(ms_update), 4),
                                    both=round(med(ms_step) + med(ms_update), 4)))
    print(json.dumps(host), flush=True)
    print(json.dumps(dict(summary="host transfers / device decision", wall_ratio=round((med(ms_step) + med(ms_update)) / med(wall), 2),
                          host_wall_ms=round(med(ms_step) + med(ms_update), 4), device_wall_ms=round(med(wall), 4),
                          device_kernel_ms=round(med(ms_ratio) + med(ms_kkt), 5))), flush=True)
    b.close()


if __name__ == "__main__":
    main()
