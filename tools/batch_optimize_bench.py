"""Cost of optimizeQP per member of a batch (rsqp_batch_optimize_qp); figures in profiles/r07_batch_optimize.json, DESIGN.md 4.7.

    python tools/batch_optimize_bench.py m1_tiny | m1_hs512 | m2 | trace  [reps]

m1_*:  steady FIXED state (every member hot-starts on new vectors, nobody is rescued): wall time of one rsqp_batch_optimize_qp
       against rsqp_batch_solve(HOT_VECTORS) + rsqp_batch_sync on the same batch and vectors -- 65 536 hs071-scale members
       (m1_tiny), the 512-member hs0xx batch (m1_hs512); and the same call with every second member sitting out
       (rsqp_batch_set_members), where the library has it.
m2:    the seven-step sequence of tests/test_gpu_batch_optimize.py on hs_batch(512): one batch against 512 single handles.
trace: three calls per batch and nothing else, to run under `rocprofv3 --kernel-trace --stats`.
TREE=<checkout> imports restartsqp_amd from another checkout (one that lacks the entry point measures its rsqp_batch_solve and
its single handles only), so that two revisions can alternate in one job. One JSON line per measurement."""
import json, os, sys, time
TREE = os.environ.get("TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import numpy as np
from restartsqp_amd import capi, problems
side = "with optimize" if "rsqp_batch_optimize_qp" in capi.SYMBOLS else "without"
what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 40


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts[0]), max_ms=float(ts[-1]), q1_ms=float(np.percentile(ts, 25)), q3_ms=float(np.percentile(ts, 75)), n=len(ts))


def cat(ps, name):
    return np.concatenate([getattr(p, name) for p in ps] + [np.zeros(0)])


def m1(label, base):
    rng = np.random.default_rng(1)
    sets = []
    for k in range(2):
        ps = [problems.perturb(rng, q, 0.01) for q in base]
        sets.append(tuple(cat(ps, n) for n in ("g", "lb", "ub", "lbA", "ubA")))
    b = capi.Batch(base)
    out = {}
    # (a) the parent's way: one mode for everybody + a wait
    b.solve(capi.MODE_COLD, 1000)
    ts = []
    for r in range(reps + 5):
        b.set_vectors(*sets[r % 2])
        t0 = time.perf_counter(); b.solve(capi.MODE_HOT_VECTORS, 1000); t1 = time.perf_counter()
        if r >= 5: ts.append(t1 - t0)
    out["solve_hot_vectors_plus_sync"] = stats(ts)
    res = b.results(); out["solved"] = int(sum(r["status"] == 20 for r in res)); out["kernel"] = b.last_kernel()
    if side == "with optimize":
        b2 = capi.Batch(base)
        b2.optimize_qp()
        ts = []
        for r in range(reps + 5):
            b2.set_vectors(*sets[r % 2])
            t0 = time.perf_counter(); used = b2.optimize_qp(); t1 = time.perf_counter()
            if r >= 5: ts.append(t1 - t0)
        mode, rescue = b2.dispatch()
        assert np.all(mode == 1) and np.all(rescue == 0), (np.bincount(mode), np.bincount(rescue))
        out["optimize_qp"] = stats(ts); out["optimize_kernel"] = b2.last_kernel()
        ts = []
        for r in range(reps + 5):       # (the same call without its nWSR_used output: no copy to the host behind the wait)
            b2.set_vectors(*sets[r % 2])
            t0 = time.perf_counter(); capi.check(capi.lib().rsqp_batch_optimize_qp(b2._h, None)); t1 = time.perf_counter()
            if r >= 5: ts.append(t1 - t0)
        out["optimize_qp_without_nWSR_used"] = stats(ts)
        r2 = b2.results()
        out["same_as_solve"] = bool(all(np.array_equal(a["x"], c["x"]) and a["nWSR"] == c["nWSR"] for a, c in zip(res, r2)))
        if "rsqp_batch_set_members" in capi.SYMBOLS:       # every second member sits out (rsqp_batch_set_members): against the full call above
            half = (np.arange(len(base)) % 2 == 0).astype(np.int32)
            b2.set_members(half)
            ts = []
            for r in range(reps + 5):
                b2.set_vectors(*sets[r % 2])
                t0 = time.perf_counter(); used = b2.optimize_qp(); t1 = time.perf_counter()
                if r >= 5: ts.append(t1 - t0)
            mode, rescue = b2.dispatch()
            assert np.all(mode[half == 1] == 1) and np.all(mode[half == 0] == -1) and np.all(used[half == 0] == 0)
            out["optimize_qp_every_second_member_sits_out"] = stats(ts)
        b2.close()
    b.close()
    print(json.dumps(dict(measurement="M1", side=side, batch=label, nq=len(base), **out)), flush=True)


def m2():
    sys.path.insert(0, os.path.join(HERE, "tests")); sys.path.insert(0, HERE)
    import test_gpu_batch_optimize as T
    T.BATCHES["hs512"] = (lambda: problems.hs_batch(512), 12, 20, None)
    steps, budget, _ = T.sequence("hs512")
    steps = [st[:-1] for st in steps]      # (without the inconsistent extra member)
    nq = len(steps[0])
    if side == "with optimize":
        b = capi.Batch(steps[0]); b.set_options(qp_maxiter=budget)
        t0 = time.perf_counter(); tot = 0
        for k, (kind, members) in enumerate(zip(T.STEP_KIND, steps)):
            if k == 5: b.set_options(qp_maxiter=1000)
            if k > 0: T.upload(b, members, kind == "newmats")
            tot += int(b.optimize_qp().sum())
        el = time.perf_counter() - t0
        print(json.dumps(dict(measurement="M2", side=side, how="one batch, 7 x rsqp_batch_optimize_qp (uploads included)", nq=nq, seconds=el, nWSR_used=tot)), flush=True)
    hs = []
    for q in steps[0]:
        s = capi.Solver(q.nV, q.nC); s.set_options(qp_maxiter=budget); hs.append(s)
    t0 = time.perf_counter(); tot = 0
    for k, (kind, members) in enumerate(zip(T.STEP_KIND, steps)):
        for s, m in zip(hs, members):
            if k == 5: s.set_options(qp_maxiter=1000)
            if k == 0 or kind == "newmats":
                s.set_A_csc(m.A_jc, m.A_ir, m.A_val); s.set_H_csc(m.H_jc, m.H_ir, m.H_val)
            for w, v in zip(range(5), (m.g, m.lb, m.ub, m.lbA, m.ubA)):
                s.set_vector(w, v)
            tot += s.optimize_qp()
    el = time.perf_counter() - t0
    print(json.dumps(dict(measurement="M2", side=side, how="512 single handles, 7 x rsqp_optimize_qp each (setters included)", nq=nq, seconds=el, nWSR_used=tot)), flush=True)


if what == "m1_tiny":
    m1("hs071_scale_batch(65536)", problems.hs071_scale_batch(65536))
elif what == "m1_hs512":
    m1("hs_batch(512)", problems.hs_batch(512))
elif what == "m2":
    m2()
elif what == "trace":
    for label, base in (("tiny", problems.hs071_scale_batch(65536)), ("hs512", problems.hs_batch(512))):
        rng = np.random.default_rng(1)
        ps = [problems.perturb(rng, q, 0.01) for q in base]
        b = capi.Batch(base); b.optimize_qp(); b.set_vectors_from(ps); b.optimize_qp(); b.set_vectors_from(base); b.optimize_qp(); b.close()
