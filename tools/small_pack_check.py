"""Check that every lanes-per-problem / waves build of the batch kernel returns identical results (bitwise: the arithmetic order
does not depend on the packing).

    python tools/small_pack_check.py [--quick]

Every variant runs in a process of its own (--one) under RSQP_SMALL_LANES / RSQP_SMALL_WAVES and writes, next to its results, the
build its launches ran (Batch.last_plan -> capi.plan_builds). A variant FAILS when that build is not the (L, W) it asked for, or
is the build of the kind's reference variant: a comparison of a kernel with itself proves nothing. The kinds are chosen so that
the variants are real:
  hs071    4 099 QPs of the hs071 shape under RSQP_SMALL_ENGINE=0: 8 lanes = the compile-time shape build, 16 / 32 / 64 lanes the
           Givens / TQ builds (without the switch every variant would run the register-resident tableau kernel)
  random   mixed shapes of at most 8 variables and 15 constraints (+ degenerate ones of the same size): Givens / TQ, whose W builds
           differ -- 16 / 32 lanes at W 2, 3, 4; 64 lanes at W 3, 4 (this kind found the W 6 build of 64 lanes wrong: it is not
           built any more)
  randomx  mixed shapes of up to 14 variables: explicit inverses, whose W is fixed by L -- (16, 2), (32, 2), (64, 4)
--quick keeps at least one variant per L on each engine."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "--one":
    sys.path.insert(0, ROOT)
    import numpy as np
    from restartsqp_amd import capi, problems
    kind, out = sys.argv[2], sys.argv[3]
    if kind == "hs071":
        probs = problems.hs071_scale_batch(4099)
    else:
        rng = np.random.default_rng(5)
        vmax, cmax = (8, 15) if kind == "random" else (14, 11)
        probs = [problems.random_qp(rng, int(rng.integers(2, vmax + 1)), int(rng.integers(1, cmax + 1))) for k in range(1000)]
        while len(probs) < 1200:
            q = problems.degenerate_qp(rng, len(probs) % 5)
            if q.nV <= vmax and q.nC <= cmax:
                probs.append(q)
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    builds = [capi.plan_builds(b.last_plan())]
    res = b.results()
    # hot start on perturbed vectors
    prng = np.random.default_rng(11)
    pert = [problems.perturb(prng, p, 0.05) for p in probs]
    b.set_vectors_from(pert)
    b.solve(capi.MODE_HOT_VECTORS, 1000)
    builds.append(capi.plan_builds(b.last_plan()))
    res2 = b.results()
    cat = lambda rs, k: np.concatenate([np.atleast_1d(np.asarray(r[k], dtype=float)) for r in rs])
    np.savez(out, **{k + s: cat(rs, k) for s, rs in (("_c", res), ("_h", res2)) for k in ("x", "y", "ws_b", "ws_c", "status", "nWSR", "obj")})
    json.dump(builds, open(out + ".json", "w"))
    sys.exit(0)
import numpy as np
quick = "--quick" in sys.argv
GIVENS_W = ((64, 4), (64, 3), (32, 2), (32, 3), (32, 4), (16, 2), (16, 3), (16, 4))
KINDS = {   # kind: (environment, variants; the first is the reference)
    "hs071": ({"RSQP_SMALL_ENGINE": "0"}, ((64, 4), (32, 2), (16, 2), (8, 2)) if quick else GIVENS_W + ((8, 2),)),
    "random": ({}, ((64, 4), (32, 3), (16, 4), (16, 2)) if quick else GIVENS_W),
    "randomx": ({}, ((64, 4), (32, 2), (16, 2))),
}
bad = 0
tmp = tempfile.mkdtemp(prefix="small_pack_")
for kind, (kenv, variants) in KINDS.items():
    ref = ref_build = None
    for L, W in variants:
        env = dict(os.environ, RSQP_SMALL_LANES=str(L), RSQP_SMALL_WAVES=str(W), **kenv)
        out = os.path.join(tmp, "pack_%s_%d_%d.npz" % (kind, L, W))
        r = subprocess.run([sys.executable, __file__, "--one", kind, out], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print(kind, L, W, "FAILED", r.stderr[-400:]); bad += 1; continue
        d = dict(np.load(out))
        builds = [[tuple(b) for b in bs] for bs in json.load(open(out + ".json"))]
        # one null-space build, the same cold and hot, with the lanes and waves asked for
        mine = builds[0][0] if all(len(bs) == 1 and bs == builds[0] and bs[0][0] == "qp" for bs in builds) else None
        if mine is None or (mine[2], mine[4]) != (L, W):
            print(kind, "L=%d W=%d" % (L, W), "RAN ANOTHER BUILD:", builds, flush=True); bad += 1; continue
        if ref is None:
            ref, ref_build = d, mine
            print(kind, "reference L=%d W=%d %s: nWSR cold %d hot %d, solved %d/%d" % (L, W, mine, d["nWSR_c"].sum(), d["nWSR_h"].sum(), (d["status_c"] == 20).sum(), len(d["status_c"])), flush=True)
            continue
        if mine == ref_build:
            print(kind, "L=%d W=%d" % (L, W), "IS THE REFERENCE'S BUILD:", mine, flush=True); bad += 1; continue
        diffs = [k for k in ref if not np.array_equal(ref[k], d[k], equal_nan=True)]
        nan = [k for k in d if np.isnan(d[k]).any()]
        print(kind, "L=%d W=%d" % (L, W), mine, "identical" if not diffs else "DIFFERS in %s" % diffs, ("NaN in %s" % nan) if nan else "", flush=True)
        if diffs:
            bad += 1
            for k in diffs[:3]:
                idx = np.flatnonzero(~((ref[k] == d[k]) | (np.isnan(ref[k]) & np.isnan(d[k]))))
                print("   ", k, "first idx", idx[:5], ref[k][idx[:3]], d[k][idx[:3]])
print("BAD" if bad else "ALL IDENTICAL")
sys.exit(1 if bad else 0)
