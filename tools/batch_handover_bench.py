"""Cost of the hand-over switch of a batch (rsqp_batch_set_handover) where nobody needs it; figures in
profiles/batch_handover_cost.json, DESIGN.md 4.12.

    python tools/batch_handover_bench.py cold | fixed | stiff  [reps]  [off | on]

cold:   65 536 hs071-scale cold solves, no state kept (the lane-per-problem kernel, bench.py's headline launch): device time of
        the launch (rsqp_batch_last_solve_ms: the events around it) and wall time of solve + sync, switch off against on.
fixed:  the steady FIXED state of DESIGN.md 4.7 (every member hot-starts on new vectors, nobody is rescued): wall time of one
        rsqp_batch_optimize_qp on 65 536 hs071-scale members, off against on.
stiff:  what the switch buys: problems.stiff_free_batch(8, 2) with 65 536 members, every third one given up on by the tableau
        kernel -- solved members and device time of the cold launch, off against on.
One batch at a time: a leg is measured on a batch of its own, which is closed before the next leg's is created (two batches of
65 536 members alternating call by call evict each other's state blocks from the last-level cache and each other's kernels from
the instruction caches: the off leg then read 1-1.5 us (cold) and 9-19 us (fixed) slower than the same library did alone). A third
argument runs one leg only.
TREE=<checkout> imports restartsqp_amd from another checkout; one that lacks the entry point measures the off leg only, so that two
revisions can alternate in one job. One JSON line per measurement."""
import json, os, sys, time
TREE = os.environ.get("TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import numpy as np
from restartsqp_amd import capi, problems
have = hasattr(capi, "HANDOVER_SYMBOLS")
side = "with hand-over" if have else "without"
what = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
legs = (False, True) if have else (False,)
if len(sys.argv) > 3:
    legs = tuple(on for on in legs if on == (sys.argv[3] == "on"))


def stats(ts):
    ts = np.sort(np.asarray(ts))
    return dict(median=float(np.median(ts)), min=float(ts[0]), q1=float(np.percentile(ts, 25)), q3=float(np.percentile(ts, 75)), max=float(ts[-1]), n=len(ts))


def cat(ps, name):
    return np.concatenate([getattr(p, name) for p in ps] + [np.zeros(0)])


def batch(base, keep, on):
    b = capi.Batch(base)
    b.set_keep_state(keep)
    if have:
        b.set_handover(on)
    return b


def cold(label, base):
    out = {}
    for on in legs:
        b = batch(base, False, on)
        dev, wall = [], []
        for r in range(reps + 5):
            t0 = time.perf_counter(); b.solve(capi.MODE_COLD, 1000); t1 = time.perf_counter()
            if r >= 5:
                dev.append(b.last_solve_ms() * 1e3); wall.append((t1 - t0) * 1e6)
        res = b.results()
        out["on" if on else "off"] = dict(device_us=stats(dev), wall_us=stats(wall), kernel=b.last_kernel(),
                                          solved=int(sum(r["status"] == 20 for r in res)), handed=int(b.handover()[1]) if have else 0)
        b.close()
    print(json.dumps(dict(measurement=what, side=side, batch=label, nq=len(base), **out)), flush=True)


def fixed(label, base):
    rng = np.random.default_rng(1)
    sets = []
    for k in range(2):
        ps = [problems.perturb(rng, q, 0.01) for q in base]
        sets.append(tuple(cat(ps, n) for n in ("g", "lb", "ub", "lbA", "ubA")))
    out = {}
    for on in legs:
        b = batch(base, True, on)
        b.optimize_qp()
        wall = []
        for r in range(reps + 5):
            b.set_vectors(*sets[r % 2])
            t0 = time.perf_counter(); b.optimize_qp(); t1 = time.perf_counter()
            if r >= 5:
                wall.append((t1 - t0) * 1e6)
        mode, rescue = b.dispatch()
        assert np.all(mode == 1) and np.all(rescue == 0)
        out["on" if on else "off"] = dict(wall_us=stats(wall), kernel=b.last_kernel(), handed=int(b.handover()[1]) if have else 0)
        b.close()
    print(json.dumps(dict(measurement=what, side=side, batch=label, nq=len(base), **out)), flush=True)


if what == "cold":
    cold("hs071_scale_batch(65536)", problems.hs071_scale_batch(65536))
elif what == "fixed":
    fixed("hs071_scale_batch(65536)", problems.hs071_scale_batch(65536))
elif what == "stiff":
    cold("stiff_free_batch(8, 2, 65536)", problems.stiff_free_batch(np.random.default_rng(5082), 8, 2, 65536))
