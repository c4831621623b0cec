"""The 31 kernel instantiations of the small-QP layer (qp_small.hip 16 + 2, qp_small_hbm.hip 2, qp_tiny.hip 5, qp_lane.hip 6), at
least one case each (a 32nd, Engine<64, true> at six waves per SIMD, failed its case here and was taken out of the product): the environment switches, the batch and the build the batch must reach. Shared by tests/test_gpu_small_builds.py (every
case against the oracle on the GPU) and tests/test_small_launch_plan.py (the golden table names the same 31 builds).

qp_lane.hip holds 11 builds by now. The table covers its six cold run-time-shape builds; the two full-shape builds and the three WARM
builds are covered in tests/test_gpu_lane_shape.py and tests/test_gpu_lane_warm.py (shared pieces: tests/lane_cases.py).

A build is told from its neighbours by the plan words capi.plan_builds projects: ("qp", engine, L, mat_lds, W, shape),
("qpg", first), ("tiny", mc, W), ("lane", keep, uni, hb), ("qph", engine).

The batches are the smallest that reach and stress a build: shapes drawn below the class maximum (nV = 1 and nC = 0 included where
the class allows), one member pinned at the maximum, a member count that is no multiple of the 64 / L problems of a wave. The
oracle's answers are computed once per case (reference) and never changed."""
import numpy as np

from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc

PERTURB = 0.3            # of the hot starts: with the parity tests' 0.05 most small members keep their working set
COLD_SHARE, HOT_SHARE = 0.8, 0.4      # of a case's members: >= 2 working-set changes cold, >= 1 in each hot start (oracle's counts)


def kernel_name(build):
    """the instantiation behind a build, as the golden table's `kernels` field spells it"""
    b = lambda v: "true" if v else "false"
    if build[0] == "qp":
        _, e, L, ml, W, shape = build
        eng = "%s<%d, %s%s>" % ("EngineX" if e else "Engine", L, b(ml), ", true" if shape else "")
        return "void small_qp_kernel(QPPools, int, int, int, int) [ENG = %s, L = %d, ML = %s, W = %d, SHAPE = %d]" % (eng, L, b(ml), W, shape)
    if build[0] == "qpg":
        return "void small_qpg_kernel(QPPools, int, int, int) [RV = %d, RC = %d, CV = %d, CC = %d]" % {1: (3, 1, 9, 4), 2: (2, 2, 8, 8)}[build[1]]
    if build[0] == "tiny":
        return "void tiny_qp_kernel(QPPools, int, int, int) [MC = %d, W = %d, GL = false]" % build[1:]
    if build[0] == "lane":
        return "void lane_qp_kernel(QPPools, int, int) [MC = 2, KEEP = %s, UNI = %s, HB = %d]" % (b(build[1]), b(build[2]), build[3])
    assert build[0] == "qph"
    return "void small_qph_kernel(QPPools, int, int, int) [ENG = %s]" % ("EngineX<256, true>, L = 256, W = 1" if build[1] else "Engine<64, false>, L = 64, W = 2")


# ------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------
def mixed(seed, n, vmax, cmax, vmin=1, cmin=0, density=0.5, one_var=True, no_con=True):
    """n random convex QPs of vmin..vmax variables and cmin..cmax constraints: member n // 2 has the maximum shape, one member a
    single variable and one no constraint (where the class allows)"""
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.integers(vmin, vmax + 1)), int(rng.integers(cmin, cmax + 1))) for _ in range(n)]
    shapes[n // 2] = (vmax, cmax)
    if one_var and vmin <= 1:
        shapes[1] = (1, shapes[1][1])
    if no_con and cmin <= 0:
        shapes[n - 2] = (shapes[n - 2][0], 0)
    return [problems.random_qp(rng, v, c, density=density, name="%dx%d" % (v, c)) for v, c in shapes]


def one_shape(seed, n, nV=8, nC=2):
    """n random convex QPs of one shape, patterns of their own"""
    rng = np.random.default_rng(seed)
    return [problems.random_qp(rng, nV, nC) for _ in range(n)]


def small_on_a_wave(seed, n):
    """n random convex QPs of 2..8 variables and 1..15 constraints: 16 lanes would do, RSQP_SMALL_LANES=64 gives each a wave"""
    rng = np.random.default_rng(seed)
    return [problems.random_qp(rng, int(rng.integers(2, 9)), int(rng.integers(1, 16))) for _ in range(n)]


def with_H(q, H):
    return QPData(q.nV, q.nC, *dense_to_csc(H), q.A_jc, q.A_ir, q.A_val, q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name)


def _varied(rng, base, n):
    """n members on the patterns of `base`: vectors drawn anew around the base's, every matrix value rescaled"""
    out = []
    for _ in range(n):
        q = problems.perturb(rng, base, 1.0)
        q.A_val = q.A_val * (1.0 + 0.3 * rng.normal(size=q.A_val.shape))
        out.append(q)
    return out


def lane_batch(seed, n, uni, hb):
    """8 x 2 members for the lane-per-problem kernel (the recipes of test_gpu_lane.py / test_gpu_lane_hblock.py): one pattern
    (uni) or two patterns interleaved; H inside its leading 4 x 4 block (hb = 4) or dense"""
    rng = np.random.default_rng(seed)

    def base():
        q = problems.random_qp(rng, 8, 2, density=1.0)
        if hb == 4:
            H = np.zeros((8, 8))
            H[:4, :4] = q.dense_H()[:4, :4]
            q = with_H(q, H)
        return q
    a = base()
    if uni:
        return _varied(rng, a, n)
    c = base()
    A = c.dense_A(); A[0, 2] = 0.0; A[1, 5] = 0.0
    c.A_jc, c.A_ir, c.A_val = dense_to_csc(A)
    va, vc = _varied(rng, a, n), _varied(rng, c, n)
    return [(va, vc)[k % 2][k] for k in range(n)]


def hot_vectors(seed, probs):
    rng = np.random.default_rng(seed)
    return [problems.perturb(rng, q, PERTURB) for q in probs]


def hot_matrices(seed, probs):
    """new vectors and new values on the same patterns (H scaled: it stays symmetric)"""
    rng = np.random.default_rng(seed)
    out = [problems.perturb(rng, q, PERTURB) for q in probs]
    for q in out:
        q.A_val = q.A_val * (1.0 + 0.05 * rng.normal(size=q.A_val.shape))
        q.H_val = q.H_val * 1.05
    return out


# ------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------
class Case:
    """name; build: what the batch must reach; env: the switches (read per handle, at rsqp_batch_create); seed, make(seed) -> the
    distinct members; tile: the member count the distinct ones are repeated to (0: as they are); hot: the family keeps state, so
    both hot starts run; keep: set_keep_state (None: the default); hbm: the batch lies beyond the LDS image; group: cases that
    differ only in W share a batch and must give the same bits. The seeds were chosen on the CPU oracle so that the shares of
    COLD_SHARE / HOT_SHARE hold with room to spare (profiles/HISTORY.md lists them)"""

    def __init__(self, name, build, env, seed, make, tile=0, hot=True, keep=None, hbm=0, group=None):
        self.name, self.build, self.env, self.seed, self.make, self.tile, self.hot, self.keep, self.hbm, self.group = \
            name, build, env, seed, make, tile, hot, keep, hbm, group

    def members(self, distinct):
        return [distinct[k % len(distinct)] for k in range(self.tile)] if self.tile else list(distinct)


def _waves(W, default):
    return {} if W == default else {"RSQP_SMALL_WAVES": str(W)}


E0, E1 = {"RSQP_SMALL_ENGINE": "0"}, {"RSQP_SMALL_ENGINE": "1"}
CASES = [
    Case("Engine<8> shape 8 x 2", ("qp", 0, 8, 1, 2, 8 * 256 + 2), E0, 2039, lambda s: one_shape(s, 37)),
    Case("Engine<8>", ("qp", 0, 8, 1, 2, 0), E0, 2062, lambda s: mixed(s, 37, 8, 8)),
]
CASES += [Case("Engine<16> W %d" % W, ("qp", 0, 16, 1, W, 0), _waves(W, 2), 2011, lambda s: mixed(s, 37, 8, 12), group="Engine<16>") for W in (2, 3, 4)]
CASES += [Case("Engine<32> W %d" % W, ("qp", 0, 32, 1, W, 0), _waves(W, 2), 2025, lambda s: mixed(s, 19, 8, 24), group="Engine<32>") for W in (2, 3, 4)]
CASES += [Case("Engine<64, true> W %d" % W, ("qp", 0, 64, 1, W, 0), _waves(W, 4), 2071, lambda s: mixed(s, 9, 8, 40), group="Engine<64, true>")
          for W in (4, 3)]
# (its W = 6 build, once the default here, is not built any more: on the batch of the next two cases -- the head of the `random`
#  kind of tools/small_pack_check.py, which found it -- it answered "solved" with a wrong x for 11 of the first 40 members, where
#  it matched the oracle on all 9 of the batch above. RSQP_SMALL_WAVES=6 gets the W = 4 build: rsqp_small_plan.h)
CASES += [Case("Engine<64, true> W %d, small members on a wave of their own" % W, ("qp", 0, 64, 1, W, 0), dict(_waves(W, 4), RSQP_SMALL_LANES="64"),
               5, lambda s: small_on_a_wave(s, 41), group="Engine<64, true> by RSQP_SMALL_LANES") for W in (4, 3)]
CASES += [
    # dense 66 x 32: at 32 constraints the first nV whose image fits 160 KiB while image + staged matrices do not (describe_small_launch)
    Case("Engine<64, false>", ("qp", 0, 64, 0, 3, 0), E0, 1106, lambda s: mixed(s, 3, 66, 32, vmin=40, cmin=10, density=1.0)),
    Case("EngineX<16>", ("qp", 1, 16, 1, 2, 0), E1, 2009, lambda s: mixed(s, 37, 12, 6)),
    Case("EngineX<32>", ("qp", 1, 32, 1, 2, 0), E1, 2036, lambda s: mixed(s, 19, 24, 10)),
    Case("EngineX<64, true>", ("qp", 1, 64, 1, 4, 0), dict(E1, RSQP_SMALL_LANES="64"), 2036, lambda s: mixed(s, 9, 32, 14)),
    Case("EngineX<256>", ("qp", 1, 256, 1, 1, 0), E1, 1110, lambda s: mixed(s, 5, 40, 14, one_var=False, no_con=False)),
    Case("EngineX<64, false>", ("qp", 1, 64, 0, 3, 0), E1, 1111, lambda s: mixed(s, 3, 72, 32, vmin=40, cmin=10, density=1.0)),
    Case("small_qpg<3, 1, 9, 4>", ("qpg", 1), {}, 1112, lambda s: mixed(s, 5, 40, 14, one_var=False, no_con=False)),
    Case("small_qpg<2, 2, 8, 8>", ("qpg", 2), {}, 1113, lambda s: mixed(s, 5, 40, 40, one_var=False, no_con=False)),
    # (the smallest shapes of test_gpu_batch_beyond_lds.py: 96 variables and up)
    Case("small_qph EngineX<256>", ("qph", 1), {}, 1114, lambda s: mixed(s, 3, 104, 40, vmin=96, no_con=False), hbm=1),
    Case("small_qph Engine<64>", ("qph", 0), E0, 1115, lambda s: mixed(s, 3, 104, 40, vmin=96, no_con=False), hbm=1),
]
CASES += [Case("tiny MC %d W 1" % mc, ("tiny", mc, 1), {}, seed, (lambda mc: lambda s: mixed(s, 67, 8, mc))(mc))
          for mc, seed in ((2, 2061), (4, 2010), (8, 2004))]
# more than 8 192 members: 67 distinct QPs (coprime to the 32 problems of a workgroup) tiled, every copy bit-identical to its first
CASES += [Case("tiny MC %d W 2" % mc, ("tiny", mc, 2), {}, seed, (lambda mc: lambda s: mixed(s, 67, 8, mc))(mc), tile=8193)
          for mc, seed in ((2, 2057), (4, 2066))]
# 67 distinct 8 x 2 QPs tiled to 131 members: three workgroups of 64, the last with 3 lanes. Cold solves only
CASES += [Case("lane KEEP %d UNI %d HB %d" % (keep, uni, hb), ("lane", keep, uni, hb), {"RSQP_LANE": "64"}, seed,
               (lambda uni, hb: lambda s: lane_batch(s, 67, uni, hb))(uni, hb), tile=131, hot=False, keep=bool(keep))
          for keep in (1, 0) for uni, hb, seed in ((1, 4, 2027), (1, 8, 2014), (0, 8, 2000))]
BY_NAME = {c.name: c for c in CASES}
BUILDS = sorted({c.build for c in CASES})      # 31: two builds have a second case
SWITCHES = ("RSQP_SMALL_ENGINE", "RSQP_SMALL_LANES", "RSQP_SMALL_WAVES", "RSQP_LANE", "RSQP_LANE_HBLOCK", "RSQP_K_DEBUG_BAIL")


# ------------------------------------------------------------------------------------
# the plan a batch gets, from its members alone (what rsqp_batch_create reads of them): needs no GPU
# ------------------------------------------------------------------------------------
def mat_lds_bytes(q):
    annz, hnnz = len(q.A_val), len(q.H_val)
    idx = 2 * (q.nV + 1) + (q.nC + 1) + 2 * annz + hnnz
    return ((idx * 2 + 7) & ~7) + (2 * annz + hnnz) * 8


def predicted_plan(capi, case, probs, mode=0, state_engine=-1):
    """probs: the distinct members (tiling changes the count alone)"""
    nVmax, nCmax = max(q.nV for q in probs), max(q.nC for q in probs)
    uniV = probs[0].nV if all(q.nV == probs[0].nV for q in probs) else -1
    uniC = probs[0].nC if all(q.nC == probs[0].nC for q in probs) else -1
    p0 = probs[0]
    same = lambda a, c: len(a) == len(c) and np.array_equal(a, c)
    uni_pat = int(uniV > 0 and uniC >= 0 and all(same(q.A_jc, p0.A_jc) and same(q.A_ir, p0.A_ir) and same(q.H_jc, p0.H_jc) and
                                                 same(q.H_ir, p0.H_ir) for q in probs))
    inside = all(int(r) < 4 for r in p0.H_ir) and int(p0.H_jc[min(4, p0.nV)]) == int(p0.H_jc[p0.nV])
    sym = nVmax <= 8 and all(np.array_equal(q.dense_H(), q.dense_H().T) for q in probs)
    env = lambda k: int(case.env.get(k, -1))
    keep = 1 if case.keep is None else int(case.keep)
    words = dict(engine=env("RSQP_SMALL_ENGINE"), lanes=env("RSQP_SMALL_LANES"), waves=env("RSQP_SMALL_WAVES"), no_tiny=0, lane=env("RSQP_LANE"),
                 nq=case.tile or len(probs), nVmax=nVmax, nCmax=nCmax, mat_bytes_max=max(mat_lds_bytes(q) for q in probs), mode=mode, hbm=case.hbm,
                 state_engine=state_engine, tiny_ok=int(sym), uniV=uniV, uniC=uniC, uni_pat=uni_pat, desc=1, keep_state=keep, skip_mark=1,
                 member_mode=0, done_flag=0, cert_out=0, x0=0, y0=0, guess_b=0, lane_hblock=4 if (uni_pat and inside) else 8, uni_hreg=0)
    return capi.describe_small_launch(**words)


# ------------------------------------------------------------------------------------
# the oracle's answers, once per case
# ------------------------------------------------------------------------------------
def _record(qp, n):
    return dict(status=qp.exitflag(), nWSR=int(n), ws_b=np.array(qp.ws_bounds), ws_c=np.array(qp.ws_constraints), x=np.array(qp.x),
                y=np.array(qp.y), obj=float(qp.objective))


_REFERENCE = {}


def reference(O, case):
    """{"cold": (problems, oracle records)[, "hot_vectors": ..., "hot_matrices": ...]} over the DISTINCT members of the case"""
    key = case.group or case.name
    if key in _REFERENCE:
        return _REFERENCE[key]
    probs = case.make(case.seed)
    qps, cold = [], []
    for q in probs:
        qp = O.OracleQP(q.nV, q.nC)
        qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        rc, n = qp.init(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
        qps.append(qp); cold.append(_record(qp, n))
    ref = {"cold": (probs, cold)}
    if case.hot:
        seed = case.seed + 50000
        p2 = hot_vectors(seed, probs)
        rec = []
        for q, qp in zip(p2, qps):
            rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            rec.append(_record(qp, n))
        ref["hot_vectors"] = (p2, rec)
        p3 = hot_matrices(seed + 1, p2)
        rec = []
        for q, qp in zip(p3, qps):
            qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
            rc, n = qp.hotstart_matrices(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            rec.append(_record(qp, n))
        ref["hot_matrices"] = (p3, rec)
    _REFERENCE[key] = ref
    return ref


def activity(ref):
    """share of the members with >= 2 working-set changes cold, >= 1 in each hot start: from the oracle's counts alone"""
    out = {"cold": float(np.mean([r["nWSR"] >= 2 for r in ref["cold"][1]]))}
    for k in ("hot_vectors", "hot_matrices"):
        if k in ref:
            out[k] = float(np.mean([r["nWSR"] >= 1 for r in ref[k][1]]))
    return out
