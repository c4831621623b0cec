"""Tuning: hs071-scale batches that keep their state -- the hot start on new vectors (mode 1) of 65 536 members, with
rsqp_batch_set_lane_warm / rsqp_batch_set_lane_hot both off (the 8-lane kernel) and both on (the lane-per-problem kernel's WARM
build of level 2). Legs:
  (i)   new vectors that change next to no working set: the base's vectors perturbed by 0.02;
  (ii)  the same with 0.3: most members change their working set -- and a few members in a thousand cycle until the iteration limit
        of 1 000 on either kernel, so this leg times the sequential cost of 1 000 changes of one member, not a typical step;
  (ii') the same with 0.05, between the two: a few per cent of the members change their working set, nobody cycles;
  (iii) one rsqp_batch_optimize_qp call with per-member update marks alone: every second member is named by
        rsqp_batch_set_matrix_values_of before every call and hot-starts with new matrices (mode 2), the others hot-start on new
        vectors (mode 1).
Time by HIP events: around the solve launch for (i) and (ii), around the whole call (plan kernel, first solve, rescue plan, rescue
launch, count) for (iii). Beside the time: the mean and the largest nWSR of the last launch. Every launch gets other inputs than the one before (two sets, alternating), so no hot start repeats a
solved QP. The median of 10 launches, REPEATS times per leg in one process -- the spread of the repeats is the margin of a comparison.
    python tools/lane_hot_vectors_sweep.py [nq] [--root TREE]
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
rng = np.random.default_rng(6)
probs = problems.hs071_scale_batch(nq)
cat = lambda members, name: np.concatenate([getattr(q, name) for q in members])
vectors = lambda members: tuple(cat(members, n) for n in ("g", "lb", "ub", "lbA", "ubA"))
sets = {rel: [vectors([problems.perturb(rng, q, rel) for q in probs]) for _ in range(2)] for rel in (0.02, 0.3, 0.05)}
Aval, Hval = cat(probs, "A_val"), cat(probs, "H_val")
mats = [(Aval * (1.0 + 0.01 * rng.normal(size=Aval.shape)), Hval * s) for s in (1.0, 1.05)]
named = np.zeros(nq, np.int32); named[1::2] = 1
os.environ["RSQP_LANE"] = "1"
has_switch = hasattr(capi, "LANE_HOT_SYMBOLS")
print("tree %s (%s), %d members" % (ROOT, "with the switch" if has_switch else "without the switch", nq))


def timed(b, launch):
    meds = []
    for rep in range(REPEATS):
        ms = []
        for k in range(10):
            launch(k)
            ms.append(b.last_solve_ms())
        meds.append(float(np.median(ms)))
    return meds


def report(b, on, name, meds, extra=""):
    res = b.results()
    print("switches %s, %s: kernel %d, medians of %d x 10 launches %s ms (min %.4f max %.4f), nWSR mean %.2f max %d, %d without a change, "
          "%d solved%s" % ("on" if on else "off", name, b.last_kernel(), REPEATS, " ".join("%.4f" % m for m in meds), min(meds), max(meds),
                           float(np.mean([r["nWSR"] for r in res])), max(r["nWSR"] for r in res), int(sum(r["nWSR"] == 0 for r in res)),
                           int(sum(r["status"] == 20 for r in res)), extra))


for on in ((False, True) if has_switch else (False,)):
    b = capi.Batch(probs)
    b.set_keep_state(True)
    if has_switch:
        b.set_lane_warm(on); b.set_lane_hot(on)
    b.solve(capi.MODE_COLD, 1000)
    for name, rel in (("(i) new vectors, 0.02", 0.02), ("(ii) new vectors, 0.3", 0.3), ("(ii') new vectors, 0.05", 0.05)):
        def launch(k, rel=rel):
            b.set_vectors(*sets[rel][k % 2])
            b.solve(capi.MODE_HOT_VECTORS, 1000, sync=True)
        launch(1)                           # (the first hot start of a leg comes from another leg's answer)
        report(b, on, name, timed(b, launch))

    def call(k):
        b.set_vectors(*sets[0.02][k % 2])
        b.set_matrix_values(*mats[k % 2], members=named)
        b.optimize_qp()
    for k in range(4):                      # (the first call is the cold one, the next ones hold the FIXED <-> VARIED flips)
        call(k)
    meds = timed(b, call)
    mode, rescue = b.dispatch()
    report(b, on, "(iii) optimize_qp, per-member marks", meds,
           "; modes %s, %d rescued" % (" ".join("%d: %d" % (m, int((mode == m).sum())) for m in sorted(set(mode))), int((rescue != 0).sum())))
    b.close()
