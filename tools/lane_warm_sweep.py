"""Tuning: hs071-scale batches that keep their state -- hot start with new matrices (mode 2) and warm re-initialisation from
(x0, y0, guess_b) (mode 3) of 65 536 members, with rsqp_batch_set_lane_warm off (the 8-lane kernel) and on (the lane-per-problem
kernel's WARM build): launch time by HIP events, the median of 10 launches alternating between two sets of vectors, REPEATS times
per call shape in one process -- the spread of the repeats is the margin of a comparison.
    python tools/lane_warm_sweep.py [nq] [--root TREE]
--root: import restartsqp_amd from another checkout (the parent commit, built there): a tree without the switch times "off" alone."""
import os, sys
import numpy as np
args = sys.argv[1:]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in args:
    k = args.index("--root")
    ROOT = os.path.abspath(args[k + 1])
    del args[k:k + 2]
sys.path.insert(0, ROOT)
from restartsqp_amd import capi, problems
nq = int(args[0]) if args else 65536
REPEATS = 5
rng = np.random.default_rng(5)
probs = problems.hs071_scale_batch(nq)
alt = [[problems.perturb(rng, q, 0.05) for q in probs] for _ in range(2)]
os.environ["RSQP_LANE"] = "1"
has_switch = hasattr(capi, "LANE_WARM_SYMBOLS")
print("tree %s (%s), %d members" % (ROOT, "with the switch" if has_switch else "without the switch", nq))
for warm in ((False, True) if has_switch else (False,)):
    b = capi.Batch(probs)
    b.set_keep_state(True)
    if has_switch:
        b.set_lane_warm(warm)
    b.solve(capi.MODE_COLD, 1000)
    first = b.results()
    b.set_warm_start(np.concatenate([r["x"] for r in first]), np.concatenate([r["y"] for r in first]),
                     np.concatenate([r["ws_b"] for r in first]))
    for name, mode in (("cold start, state kept", capi.MODE_COLD), ("hot start, new matrices", capi.MODE_HOT_MATRICES),
                       ("warm re-initialisation", capi.MODE_WARM_REINIT)):
        meds = []
        for rep in range(REPEATS):
            ms = []
            for k in range(10):
                b.set_vectors_from(alt[k % 2])
                b.solve(mode, 1000, sync=True)
                ms.append(b.last_solve_ms())
            meds.append(float(np.median(ms)))
        res = b.results()
        print("switch %s, %s: kernel %d, medians of %d x 10 launches %s ms (min %.4f max %.4f), mean nWSR %.2f, %d solved"
              % ("on" if warm else "off", name, b.last_kernel(), REPEATS, " ".join("%.4f" % m for m in meds), min(meds), max(meds),
                 float(np.mean([r["nWSR"] for r in res])), int(sum(r["status"] == 20 for r in res))))
    b.close()
