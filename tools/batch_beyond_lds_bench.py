"""Device time of batches beyond the LDS image (qp_small_hbm.hip, rsqp_batch_get_last_kernel() == 3) against two baselines.

    python tools/batch_beyond_lds_bench.py [--nq 512] [--reps 5] [--single 4] [--cpu-seconds 5] [--out FILE]

Workloads: nq handler-shaped members (batch_problems.handler_batch: A = [J I -I], H = blkdiag(H_k, 0), every third H_k
indefinite) of two shapes, nV x nC = (n + 2m) x m:
  120 x 30  (n = 60, m = 30)
  200 x 80  (n = 40, m = 80; the handler shape cannot give 200 x 100, which would need n = 0)
Figures per shape:
  gpu_batch        device ms per cold batch solve (HIP events around the one launch), median of --reps
  cpu_all_cores    the CPU oracle on the same members, one pinned process per core (as bench.py --full times the hs0xx
                   batch), converted to ms per nq members
  single_handles   --single members solved one after another through single rsqp_solver handles (the HBM-resident engine
                   of qp_large.hip, wall time of the cold optimize_qp of a fresh handle), extrapolated to nq members
  bytes            per working-set change, the image columns and matrices the explicit-inverse engine streams (Z|Y, Wz, dense
                   A and the Hessian block: 8 (2 ld nV + nC nV + n^2) bytes), summed over the members' nWSR, over the device time
Every GPU step runs in a child process under `timeout -k 10`, so a hang ends that step and nothing more starts on the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"120x30": (60, 30), "200x80": (40, 80)}


def members(shape, nq):
    from restartsqp_amd import batch_problems
    n, m = SHAPES[shape]
    return batch_problems.handler_batch(nq, n, m)


def step_batch(shape, nq, reps):
    from restartsqp_amd import capi
    probs = members(shape, nq)
    b = capi.Batch(probs)
    b.set_keep_state(False)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == 3, b.last_kernel()
    ms = []
    for _ in range(reps):
        b.solve(capi.MODE_COLD, 1000)
        ms.append(b.last_solve_ms())
    ok, kkt = b.test_optimality()
    res = b.results()
    n, m = SHAPES[shape]
    nV, nC = n + 2 * m, m
    ld = nV | 1
    per_change = 8 * (2 * ld * nV + nC * nV + n * n)
    nwsr = np.array([r["nWSR"] for r in res], dtype=float)
    med = float(np.median(ms))
    b.close()
    return {"ms_per_batch": med, "ms_all": ms, "kernel": 3, "nq": nq, "shape": [nV, nC],
            "solved": int(sum(r["status"] == 20 for r in res)), "certified": int(sum(o == 1 for o in ok)),
            "mean_nWSR": float(nwsr.mean()), "max_nWSR": float(nwsr.max()), "bytes_per_change": per_change,
            "streamed_GB_per_s": float(per_change * nwsr.sum() / (med * 1e-3) / 1e9)}


def step_single(shape, nq, k):
    from restartsqp_amd import capi
    probs = members(shape, nq)[:k + 1]
    times, nw = [], []
    for j, q in enumerate(probs):
        # the first solve of a fresh handle is the cold start (a second optimize_qp on unchanged data is a hot start that
        # changes nothing); member 0 only warms the engine's code paths and is not counted
        s = capi.Solver(q.nV, q.nC)
        s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
            s.set_vector(w, v)
        t0 = time.perf_counter()
        n = s.optimize_qp()
        if j > 0:
            times.append(time.perf_counter() - t0)
            nw.append(n)
        s.close()
    mean_ms = 1e3 * float(np.mean(times))
    return {"sample": k, "ms_per_qp": [1e3 * t for t in times], "nWSR": nw, "mean_ms_per_qp": mean_ms,
            "extrapolated_ms_per_batch": mean_ms * nq}


def _pin(core):
    try:
        allowed = sorted(os.sched_getaffinity(0))
        os.sched_setaffinity(0, {allowed[core % len(allowed)]})
    except (AttributeError, OSError):
        pass


def _cpu_worker(args):
    shape, nq, seconds, core = args
    _pin(core)
    import oracle as O
    probs = members(shape, nq)
    handles = []
    for q in probs:
        qp = O.OracleQP(q.nV, q.nC)
        qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        handles.append((qp, q))
    n, t0, k = 0, time.perf_counter(), core          # each core starts at another member
    while True:
        qp, q = handles[k % len(handles)]
        qp.init_repeat(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000, 1)
        n += 1; k += 1
        t = time.perf_counter() - t0
        if t >= seconds:
            return n, t


def cpu_all_cores(shape, nq, seconds):
    import multiprocessing as mp
    import oracle as O
    O.build()
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = min(cores, int(os.environ.get("OMP_NUM_THREADS", cores)))
    with mp.get_context("fork").Pool(cores) as pool:
        rs = pool.map(_cpu_worker, [(shape, nq, seconds, c) for c in range(cores)])
    rate = sum(n / t for n, t in rs)
    return {"cores": cores, "qp_per_s": rate, "ms_per_batch": 1e3 * nq / rate,
            "note": "one independent stream of the members per core, each pinned; in-repo C oracle"}


def run_step(args, step, shape, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--shape", shape,
           "--nq", str(args.nq), "--reps", str(args.reps), "--single", str(args.single)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        return {"error": "exit %d" % r.returncode, "stderr": r.stderr[-1500:]}, r.returncode
    return json.loads(r.stdout.strip().splitlines()[-1]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", type=int, default=4)
    ap.add_argument("--cpu-seconds", type=float, default=5.0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="")
    ap.add_argument("--shape", default="")
    args = ap.parse_args()
    if args.step == "batch":
        print(json.dumps(step_batch(args.shape, args.nq, args.reps)))
        return 0
    if args.step == "single":
        print(json.dumps(step_single(args.shape, args.nq, args.single)))
        return 0
    out = {"nq": args.nq}
    for shape in args.shapes.split(","):
        row = {}
        row["gpu_batch"], rc = run_step(args, "batch", shape, 300)
        if rc != 0:           # a failed or hung GPU step: nothing more starts on the GPU
            out[shape] = row
            break
        row["single_handles"], rc = run_step(args, "single", shape, 300)
        row["cpu_all_cores"] = cpu_all_cores(shape, args.nq, args.cpu_seconds)
        g = row["gpu_batch"]["ms_per_batch"]
        row["speedup_vs_cpu_all_cores"] = row["cpu_all_cores"]["ms_per_batch"] / g
        if rc == 0:
            row["speedup_vs_single_handles"] = row["single_handles"]["extrapolated_ms_per_batch"] / g
        out[shape] = row
        print(shape, json.dumps({k: v for k, v in row.items()}), flush=True)
        if rc != 0:
            break
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
    return 0 if all("error" not in json.dumps(out[s]) for s in out if s != "nq") else 1


if __name__ == "__main__":
    sys.exit(main())
