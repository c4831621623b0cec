"""What the ratio test with second_order_correction costs on 65 536 hs071 members (n = 4, m = 2), decided on the device and driven
from the host.

    python tools/soc_sweep.py [--nq 65536] [--iters 10] > profiles/soc_sweep.txt

The even members are member 0 of the hs071 batch of the GPU tests (tests/penalty_cases.members_of("hs071_gpu")) with trial values
the model predicts (accepted at the first test), the odd members its member 2 with an objective that rises with |step|^2 (bias (3, 0) of tests/soc_cases.trial_values: rejected, corrected,
rejected again, the first solve put back), alternating, so every wave of the 8-lane kernels holds both. refresh_ubA = 1, without
which the correction QP of hs071's equality constraint is infeasible.

device  rsqp_batch_handler_soc_begin + rsqp_batch_handler_soc_end with device pointers (torch tensors): wall time of the binding's
        two calls, each ending in the call's own wait; median over --iters of their sum.
host    the same work with the entry points of the parent commit plus rsqp_batch_set_objective, vectorised over the batch: status,
        objective, x and handler_step down, the tests and H_k p + grad in numpy, handler_ratio_test for the members accepted at once,
        one handler_update (bounds and gradient words), set_members, optimize_qp, results down, set_results up; then the second
        test, set_results / set_objective for the restore and the radius in numpy. Wall time of the two phases, median of their sum.
The driver's own evaluation of f and c at x_trial lies between the two calls on both routes and is not timed. Before every timed
iteration, untimed: the QP vectors set again (RSQP_HU_SET) and the QP solved again, so each route meets a batch that has just
solved its QP. Both routes take the same decisions, which is checked. torch is imported first (capi.device_torch)."""
import argparse
import json
import os
import sys
import time

import torch  # noqa: F401  (before anything loads librsqp_hip.so)

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tests")]
import numpy as np  # noqa: E402
from restartsqp_amd import capi  # noqa: E402
import penalty_cases as PC  # noqa: E402
import soc_cases as SC  # noqa: E402

WARMUP = 2
DRAWS = ((0, (0.0, 0.0)), (2, (3.0, 0.0)))      # (draw, bias) of the even and of the odd members
N, M = 4, 2


class Evaluators:
    """tests/soc_cases.trial_values for the whole batch at once: f and c at x_k + step, step [nq, 4]"""

    def __init__(self, members, bias):
        dense = [SC.dense_of(d) for d in members[:2]]
        nq = len(members)
        rep = lambda two: np.stack([np.asarray(two[0], float), np.asarray(two[1], float)])[np.arange(nq) % 2]
        self.J, self.H = rep([dense[0][0], dense[1][0]]), rep([dense[0][1], dense[1][1]])
        self.grad = rep([np.asarray(d["qp"].g, float)[:N] for d in members[:2]])
        self.c_k, self.f_k = rep([d["c_k"] for d in members[:2]]), rep([SC.f_k_of(d) for d in members[:2]])
        d2 = [d["delta"] ** 2 for d in members[:2]]
        infea = [float(PC.handler.cal_infea_reference(*d["c_infea"], 8)) for d in members[:2]]
        self.inv_d2 = rep([1.0 / v for v in d2])
        self.sf = rep([bias[k][0] * (float(np.abs(self.grad[k]).sum()) * members[k]["delta"] + members[k]["rho"] * infea[k]) for k in range(2)])
        self.sc = rep([bias[k][1] * np.abs(dense[k][0]).sum(axis=1) * members[k]["delta"] for k in range(2)])

    def __call__(self, step):
        ss = np.einsum("qi,qi->q", step, step) * self.inv_d2
        f = self.f_k + np.einsum("qi,qi->q", self.grad, step) + 0.5 * np.einsum("qi,qij,qj->q", step, self.H, step) + ss * self.sf
        c = self.c_k + np.einsum("qij,qj->qi", self.J, step) + ss[:, None] * self.sc
        return f, c.reshape(-1)


def pools(b, x=True):
    nq = b.nq
    st, obj, xs = np.zeros(nq, np.int32), np.zeros(nq), (np.zeros(nq * (N + 2 * M)) if x else None)
    capi.check(capi.lib().rsqp_batch_get_results(b._h, capi._dp(xs), None, None, None, capi._ip(st), None, capi._dp(obj)))
    return st, obj, (xs.reshape(nq, -1) if x else None)


def infea_of(c, c_l, c_u):
    """cal_infea of every member: two constraints, the tree sum of two terms is their sum"""
    c = c.reshape(-1, M)
    t = np.where(c < c_l, c_l - c, np.where(c > c_u, c - c_u, 0.0))
    return t[:, 0] + t[:, 1]


def ratio(S, o, f_t, it, qp_obj):
    actual = (S["f_k"] + S["rho"] * S["infea_k"]) - (f_t + S["rho"] * it)
    pred = S["rho"] * S["infea_k"] - qp_obj
    return actual, pred, (actual >= o["eta_s"] * pred) & (actual >= -o["tol"])


def radius(S, o, who, actual, pred, norm_p):
    d = S["delta"]
    shrink = who & (actual < o["eta_c"] * pred)
    grow = who & ~shrink & (actual > o["eta_e"] * pred) & (o["tol"] > np.abs(d - norm_p))
    S["delta"] = np.where(shrink, o["gamma_c"] * d, np.where(grow, np.minimum(o["gamma_e"] * d, o["delta_max"]), d))


def host_route(b, ev, S, o, opts, f_t, c_t, c_l, c_u):
    """one iteration driven from the host; S is written in place. Returns (ms of the two phases, accept, went)"""
    nq = b.nq
    t0 = time.perf_counter()
    st0, obj0, x0 = pools(b)
    step = b.handler_step()
    p = step["p"].reshape(nq, N)
    actual, pred, acc = ratio(S, o, f_t, infea_of(c_t, c_l, c_u), obj0)
    corr = ~acc
    b.handler_ratio_test(acc.astype(np.int32), S["rho"], f_t, c_t, S["x_k"], S["c_k"], S["f_k"], S["infea_k"], S["delta"], options=opts)
    gs = (np.einsum("qij,qj->qi", ev.H, p) + S["grad"].reshape(nq, N)).reshape(-1)
    xt = S["x_k"] + step["p"]
    b.handler_update((corr * (capi.HU_BOUNDS | capi.HU_UBA | capi.HU_GRAD)).astype(np.int32), S["delta"], S["rho"], xt, c_t, grad=gs)
    b.set_members(corr)
    b.optimize_qp()
    st1, obj1, x1 = pools(b)
    went = corr & (st1 == capi.QP_OPTIMAL)
    both = p + x1[:, :N]
    x_new = x1.copy()
    x_new[went, :N] = both[went]
    b.set_results(x=x_new.reshape(-1))
    x_trial = S["x_k"].reshape(nq, N) + both
    qp_obj = obj1 + (obj0 - S["rho"] * step["infea_model"])
    t1 = time.perf_counter()
    f2, c2 = ev(np.where(went[:, None], both, 0.0))          # the driver's evaluators at x_trial: not timed
    t2 = time.perf_counter()
    actual2, pred2, acc2 = ratio(S, o, f2, infea_of(c2, c_l, c_u), obj1)
    ok, rej = went & acc2, went & ~acc2
    S["x_k"] = np.where(np.repeat(ok, N), x_trial.reshape(-1), S["x_k"])
    S["c_k"] = np.where(np.repeat(ok, M), c2, S["c_k"])
    S["f_k"], S["infea_k"] = np.where(ok, f2, S["f_k"]), np.where(ok, infea_of(c2, c_l, c_u), S["infea_k"])
    if rej.any():
        x_new[rej] = x0[rej]
        b.set_results(x=x_new.reshape(-1))
        b.set_objective(obj0, members=rej)
    norm_p = np.where(ok, np.abs(both).max(axis=1), np.abs(p).max(axis=1))
    radius(S, o, went, actual2, pred2, norm_p)
    t3 = time.perf_counter()
    accept = np.where(went, acc2, acc).astype(np.int32)
    return 1e3 * (t1 - t0), 1e3 * (t3 - t2), accept, went, qp_obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    nq = a.nq
    draws = PC.members_of("hs071_gpu")
    members = [draws[DRAWS[q % 2][0]] for q in range(nq)]
    bias = [DRAWS[0][1], DRAWS[1][1]]
    ev = Evaluators(members, bias)
    S0 = SC.pooled(members[:2])
    S0 = {k: np.tile(v.reshape(2, -1), (nq // 2, 1)).reshape(-1).astype(v.dtype) for k, v in S0.items()}
    S0["what"] = np.full(nq, capi.SOC_TEST | capi.SOC_CORRECT, np.int32)
    c_l, c_u = np.stack([members[q]["c_l"] for q in range(2)])[np.arange(nq) % 2], np.stack([members[q]["c_u"] for q in range(2)])[np.arange(nq) % 2]
    opts, sopts = capi.NlpStepOptions(refresh_ubA=1), capi.SocOptions()
    o = opts.as_dict()
    words = np.full(nq, capi.HU_SET, np.int32)
    med = lambda v: float(np.median(v))
    results = {}
    for route in ("device", "host"):
        b = SC.make_batch(capi, members)
        first, second, S, accept, went = [], [], None, None, None
        for k in range(WARMUP + a.iters):
            b.set_members(None)
            b.handler_update(words, S0["delta"], S0["rho"], S0["x_k"], S0["c_k"], grad=S0["grad"])
            b.optimize_qp()
            S = {key: v.copy() for key, v in S0.items()}
            f_t, c_t = ev(pools(b)[2][:, :N])
            if route == "device":
                T = lambda v: torch.as_tensor(v, device="cuda")
                it = {key: T(S[key]) for key in SC.ITERATE}
                out = {key: torch.zeros(nq * N if key == "x_trial" else nq, dtype=torch.int32 if key in capi.SocTrial.INTS else torch.float64,
                                        device="cuda") for key in capi.SocTrial.OUT}
                d_in = [T(S["what"]), T(S["rho"]), T(f_t), T(c_t)]
                d_grad = T(S["grad"])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.handler_soc_begin(*d_in, **it, grad=d_grad, options=opts, soc_options=sopts, on_device=True, out=out)
                t1 = time.perf_counter()
                went = out["soc"].cpu().numpy() == 1
                both = pools(b)[2][:, :N]
                f2, c2 = ev(np.where(went[:, None], both, 0.0))      # the driver's evaluators at x_trial: not timed
                d_f2, d_c2 = T(f2), T(c2)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                b.handler_soc_end(d_in[1], d_f2, d_c2, **it, out=out, options=opts, soc_options=sopts, on_device=True)
                t3 = time.perf_counter()
                S.update({key: it[key].cpu().numpy() for key in it})
                accept = out["accept"].cpu().numpy()
                ms1, ms2 = 1e3 * (t1 - t0), 1e3 * (t3 - t2)
            else:
                ms1, ms2, accept, went, _ = host_route(b, ev, S, o, opts, f_t, c_t, c_l, c_u)
            if k >= WARMUP:
                first.append(ms1); second.append(ms2)
        total = [u + v for u, v in zip(first, second)]
        results[route] = dict(route=route, nq=nq, iters=a.iters, rejected_at_first_test=int(np.sum(went | (accept == 0))),
                              corrected=int(went.sum()), accepted_after_correction=int(accept[went].sum()),
                              ms_wall_median=round(med(total), 4), ms_wall_min=round(min(total), 4), ms_wall_max=round(max(total), 4),
                              ms_first_phase_median=round(med(first), 4), ms_second_phase_median=round(med(second), 4))
        results[route + "_state"] = (S, accept, went)
        print(json.dumps(results[route]), flush=True)
        b.close()
    (Sd, ad, wd), (Sh, ah, wh) = results["device_state"], results["host_state"]
    same = bool(np.array_equal(ad, ah) and np.array_equal(wd, wh) and np.array_equal(Sd["delta"], Sh["delta"]))
    print(json.dumps(dict(summary="host-driven loop / device calls", routes_agree=same,
                          wall_ratio=round(results["host"]["ms_wall_median"] / results["device"]["ms_wall_median"], 2),
                          host_wall_ms=results["host"]["ms_wall_median"], device_wall_ms=results["device"]["ms_wall_median"])), flush=True)


if __name__ == "__main__":
    main()
