"""What update_penalty_parameter costs on 65 536 hs071 members (n = 4, m = 2), decided on the device and driven from the host.

    python tools/penalty_sweep.py [--nq 65536] [--iters 10] > profiles/penalty_update_sweep.txt

Half of the members are draw 15 of tests/penalty_cases.hs071_members() (delta 0.25, rho 1: the LP is feasible, one round at rho 10
succeeds -- branch A), the other half draw 1 (rho 1e5: the model is feasible, nothing happens), alternating, so every wave of the
8-lane kernels holds both.

device  one rsqp_batch_handler_update_penalty with device pointers (torch tensors): wall time of the binding's call, median over
        --iters. Inside it: penalty_begin, setupLP (handler_update + the J launch), optimize_lp, penalty_after_lp, optimize_qp,
        penalty_round for half of the members.
host    the same work with the entry points of the parent commit: status and objective down (rsqp_batch_get_results), handler_step
        down, the decisions in numpy (vectorised over the batch), set_members + handler_update / handler_set_matrices + optimize up,
        for the LP and for each round. Wall time, median over --iters. Both routes end on the same rho and counters, which is checked.
Before every timed call, untimed: g[n..) = rho again and the QP solved again, so each call meets a batch that has just solved its QP;
the LP batch's first solve is cold, the later ones hot starts with new matrices (the first timed iteration is behind the warm-up).
A third line times the call when nobody exceeds the tolerance (one launch). torch is imported first (capi.device_torch)."""
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

WARMUP = 2
DRAW_A, DRAW_NOTHING = 15, 1


def status_and_objective(b):
    st, obj = np.zeros(b.nq, np.int32), np.zeros(b.nq)
    capi.check(capi.lib().rsqp_batch_get_results(b._h, None, None, None, None, capi._ip(st), None, capi._dp(obj)))
    return st, obj


def host_route(qp, lp, S, o):
    """update_penalty_parameter driven from the host, vectorised over the batch; S is written in place. The x / objective restore of
    the failure path has no setter and is left out (nobody fails in this batch)"""
    nq = qp.nq
    tol, inc, rho_max, it_max = o["penalty_update_tol"], o["increase_parm"], o["rho_max"], o["penalty_iter_max"]
    ik = S["infea_k"]
    status, obj = status_and_objective(qp)
    model = qp.handler_step()["infea_model"]
    take = (S["what"] != 0) & (status == capi.QP_OPTIMAL) & (model > tol)
    rounds = 0
    if take.any():
        lp.handler_update((take * capi.HU_SET).astype(np.int32), S["delta"], S["rho"], S["x_k"], S["c_k"], grad=None)
        A = qp.get_matrix_values()[0]
        jac = A.reshape(nq, -1)[:, :int(qp.jnz[0])].reshape(-1)            # (one pattern: the J entries lead every member's values)
        lp.handler_set_matrices((take * capi.HM_JAC).astype(np.int32), jac=jac)
        lp.set_members(take)
        lp.optimize_lp()
        lstatus, _ = status_and_objective(lp)
        infty = lp.handler_step()["infea_model"]
        ok = take & (lstatus == capi.QP_OPTIMAL)
        in_a = ok & (infty <= tol)
        rho_trial, broke = S["rho"].copy(), np.zeros(nq, bool)

        def goes_on(who):
            cond = np.where(in_a, model > tol, ((ik - model) < S["eps1"] * (ik - infty)) & (S["trial"] < it_max))
            return who & cond & ~(rho_trial >= rho_max)

        loop = goes_on(ok)
        while loop.any():
            rho_trial[loop] = np.minimum(rho_max, rho_trial[loop] * inc)
            S["trial"][loop] += 1
            qp.handler_update((loop * capi.HU_PENALTY).astype(np.int32), S["delta"], rho_trial, S["x_k"], S["c_k"])
            qp.set_members(loop)
            qp.optimize_qp()
            rounds += 1
            status, obj = status_and_objective(qp)
            solved = status == capi.QP_OPTIMAL
            broke |= loop & ~solved
            model = np.where(loop & solved, qp.handler_step()["infea_model"], model)
            loop = goes_on(loop & solved)
        changed = ok & (rho_trial > S["rho"])
        good = changed & ~broke & (rho_trial * ik - obj >= o["eps2"] * rho_trial * (ik - model))
        S["succ"][good] += 1; S["fail"][changed & ~good] += 1
        S["eps1"][good] = S["eps1"][good] + (1 - S["eps1"][good]) * o["eps1_change_parm"]
        S["rho"][good] = rho_trial[good]
    return rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    nq = a.nq
    draws = PC.hs071_members()
    members = [draws[DRAW_A if q % 2 == 0 else DRAW_NOTHING] for q in range(nq)]
    S0 = PC.pooled(members, PC.EPS1, what=np.ones(nq, np.int32))
    o = capi.PenaltyOptions()
    od = o.as_dict()
    words = np.full(nq, capi.HU_PENALTY, np.int32)
    med = lambda v: float(np.median(v))
    results = {}
    for route in ("device", "host"):
        qp, lp = PC.make_pair(capi, members)
        if route == "device":
            qp.handler_pair_lp(lp)
        wall, S = [], None
        for k in range(WARMUP + a.iters):
            qp.set_members(None)
            qp.handler_update(words, S0["delta"], S0["rho"], S0["x_k"], S0["c_k"])
            qp.optimize_qp()
            S = {key: v.copy() for key, v in S0.items()}
            if route == "device":
                dS = {key: torch.as_tensor(v, device="cuda") for key, v in S.items()}
                out = {key: torch.zeros(nq, dtype=torch.int32 if key in capi.PenaltyState.INTS else torch.float64, device="cuda")
                       for key in capi.PenaltyState.OUT}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                qp.handler_update_penalty(**dS, options=o, on_device=True, out=out)
                t1 = time.perf_counter()
                S = {key: dS[key].cpu().numpy() for key in S}
                rounds = int(out["rounds"].max().item())
            else:
                t0 = time.perf_counter()
                rounds = host_route(qp, lp, S, od)
                t1 = time.perf_counter()
            if k >= WARMUP:
                wall.append(1e3 * (t1 - t0))
        results[route] = dict(route=route, nq=nq, iters=a.iters, rounds=rounds, raised_rho=int(np.sum(S["rho"] > S0["rho"])),
                              succ=int(np.sum(S["succ"] - S0["succ"])), fail=int(np.sum(S["fail"] - S0["fail"])),
                              ms_wall_median=round(med(wall), 4), ms_wall_min=round(min(wall), 4), ms_wall_max=round(max(wall), 4))
        results[route + "_state"] = S
        print(json.dumps(results[route]), flush=True)
        if route == "device":
            # nobody exceeds the tolerance: one launch
            idle = capi.PenaltyOptions(penalty_update_tol=1.0e30)
            quiet = []
            for k in range(WARMUP + a.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                qp.handler_update_penalty(**dS, options=idle, on_device=True, out=out)
                quiet.append(1e3 * (time.perf_counter() - t0))
            print(json.dumps(dict(route="device, nobody exceeds the tolerance", nq=nq, ms_wall_median=round(med(quiet[WARMUP:]), 4))), flush=True)
            qp.handler_pair_lp(None)
        qp.close(); lp.close()
    same = all(np.array_equal(results["device_state"][k], results["host_state"][k]) for k in ("rho", "eps1", "trial", "succ", "fail"))
    print(json.dumps(dict(summary="host-driven loop / device call", routes_agree=bool(same),
                          wall_ratio=round(results["host"]["ms_wall_median"] / results["device"]["ms_wall_median"], 2),
                          host_wall_ms=results["host"]["ms_wall_median"], device_wall_ms=results["device"]["ms_wall_median"])), flush=True)


if __name__ == "__main__":
    main()
