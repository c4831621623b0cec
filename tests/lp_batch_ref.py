"""Shared by tests/test_gpu_batch_optimize_lp.py and tests/test_batch_optimize_lp_args.py: the reference of optimizeLP per member of
a batch (rsqp_batch_optimize_lp, restartsqp_amd/csrc/rsqp_batch_optimize.hip) and the inputs of its tests.

`LPRef` restates rsqp_optimize_lp (restartsqp_amd/csrc/rsqp_api.hip; reference src/qpOASESInterface.cpp:227-284 and the LP branch of
handle_error, :688-717) over oracle.OracleQP, the way `Ref` of tests/test_gpu_batch_optimize.py restates rsqp_optimize_qp. The six-step
sequence puts the members of one batch into different states; which branches occur is a condition on the INPUTS and is asserted from
the oracle run alone (assert_inputs_cover_the_branches), so a generator change cannot silently empty one.
"""
import functools

import numpy as np

from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc

TOL = 1e-8           # the tolerance test_gpu_parity.test_optimize_lp uses for the x of an LP: relative to max(1, |.|_inf)
EPS = 2.221e-16      # RSQP_EPS (qpOASES EPS)
MODES = {"cold": 0, "hot_vectors": 1, "hot_matrices": 2, "reinit": 3}
RESCUES = {None: 0, "rescue_cold": 1, "rescue_slack": 2}
STEP_KIND = ("first", "perturb", "newA", "newA", "perturb", "perturb")
FULL_BUDGET_FROM = 5     # index of the step from which lp_maxiter is 1000 again


class LPRef:
    """rsqp_optimize_lp over oracle.OracleQP; s.log = what the last optimize ran (the flip is logged as "reinit": it runs as a plain
    init)"""

    def __init__(s, O, q, maxit):
        s.qp = O.OracleQP(q.nV, q.nC); s.maxit = maxit
        s.qp.set_A_csc(q.A_jc, q.A_ir, q.A_val)
        s.first = s.upd = False; s.old = s.new = 0; s.reg = 0.0; s.log = []

    def set_mats(s, q):
        if s.first:
            s.upd = True
        s.qp.set_A_csc(q.A_jc, q.A_ir, q.A_val)

    def reg_for_init(s, q):
        ng = float(np.sqrt(np.sum(q.g * q.g)))
        s.reg = (ng if ng > 0.0 else 1.0) * 1.0e3 * EPS
        s.qp.set_H_csc(None, None, None); s.qp.set_regularisation(s.reg)

    def rescue(s, q):
        v = (q.g, q.lb, q.ub, q.lbA, q.ubA)
        s.reg_for_init(q)
        if s.qp.is_infeasible() and q.nV >= 2 * q.nC:
            x0 = s.qp.x.copy()                      # x_0 := x of the failed solve, slack entries overwritten (:693-699)
            for i in range(q.nC):
                x0[i + q.nV - 2 * q.nC] = max(0.0, q.lbA[i]); x0[i + q.nV - q.nC] = -min(0.0, q.ubA[i])
            rc, n = s.qp.init(*v, s.maxit, x0=x0); s.log.append("rescue_slack")
        else:
            rc, n = s.qp.init(*v, s.maxit); s.log.append("rescue_cold")
        s.old = s.new = 0
        return n

    def optimize(s, q):
        qp, N, total = s.qp, s.maxit, 0
        s.log = []
        v = (q.g, q.lb, q.ub, q.lbA, q.ubA)
        if not s.first:
            s.reg_for_init(q)
            rc, n = qp.init(*v, N); s.log.append("cold")
            if qp.is_solved():
                s.first = True
            else:
                total += s.rescue(q)
                if not qp.is_solved():
                    return total
        else:
            cur = 2 if s.upd else 1
            if s.old == 0:
                s.old = cur
            else:
                if s.new != 0:
                    s.old = s.new
                s.new = cur
            if s.new == 0 or s.new == s.old:
                if (s.old if s.new == 0 else s.new) == 1:
                    rc, n = qp.hotstart(*v, N); s.log.append("hot_vectors")
                else:
                    rc, n = qp.hotstart_matrices(*v, N); s.log.append("hot_matrices")
            else:
                s.reg_for_init(q)
                rc, n = qp.init(*v, N); s.log.append("reinit")      # :266-270: a plain init, no warm-start inputs
                s.new = s.old = 0
            s.upd = False
            if not qp.is_solved():
                total += s.rescue(q)
                if not qp.is_solved():
                    return total
        total += n
        # one regularisation step: a hot start on the gradient g - regVal x with a fresh budget
        rc, n2 = qp.hotstart(q.g - s.reg * qp.x, q.lb, q.ub, q.lbA, q.ubA, N)
        return total + n2


def random_lp(rng, nV, nC, H=None, name=""):
    """the members of test_gpu_parity.test_optimize_lp; H: None = an empty pattern, else a dense matrix (which an LP call ignores)"""
    A = rng.normal(size=(nC, nV)); g = rng.normal(size=nV); xh = rng.normal(size=nV)
    lb = xh - np.abs(rng.normal(size=nV)) - 0.1; ub = xh + np.abs(rng.normal(size=nV)) + 0.1
    lbA = A @ xh - np.abs(rng.normal(size=nC)) - 0.1; ubA = A @ xh + np.abs(rng.normal(size=nC)) + 0.1
    Hc = dense_to_csc(H) if H is not None else (np.zeros(nV + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    return QPData(nV, nC, *Hc, *dense_to_csc(A), g, lb, ub, lbA, ubA, name=name)


def spd(rng, nV):
    M = rng.normal(size=(nV, nV))
    return M @ M.T / nV + np.eye(nV)


def inconsistent(q):
    """lbA[0] > ubA[0]: infeasible before any change, in every call"""
    q.lbA = q.lbA.copy(); q.lbA[0] = q.ubA[0] + 1.0
    return q


# name -> (random members, (nV range), (nC range), with H, shapes of the inconsistent members (the first has nV >= 2 nC: slack-point
#          rescue; the second nC = nV: rescue from scratch), seed, lp_maxiter of steps 1-5, sum of nWSR_used per step on the CPU oracle)
BATCHES = {
    "tiny": (38, (2, 9), (1, 9), False, ((8, 3), (5, 5)), 102, 16, (321, 50, 312, 43, 323, 47)),
    "mid": (30, (9, 40), (1, 30), True, ((20, 8), (12, 12)), 101, 70, (1626, 736, 1499, 603, 1623, 899)),
    "hbm": (5, (96, 131), (10, 60), False, ((120, 40),), 115, 400, (1896, 823, 1528, 521, 1899, 526)),
}


@functools.lru_cache(maxsize=None)
def sequence(name):
    """the members of every step, [step][member], and the budget. ONE generator feeds every step in member order; the inconsistent
    members, at the end, keep their data (a perturbation would make their bounds consistent)"""
    nq, rV, rC, withH, extra_shapes, seed, budget, sums = BATCHES[name]
    rng = np.random.default_rng(seed)
    hrng = np.random.default_rng(seed + 1000)
    base = []
    for k in range(nq):
        nV, nC = int(rng.integers(*rV)), int(rng.integers(*rC))
        base.append(random_lp(rng, nV, nC, spd(hrng, nV) if withH else None, name="%s%d" % (name, k)))
    extra = [inconsistent(random_lp(rng, nV, nC, spd(hrng, nV) if withH else None, name="%s_inconsistent%d" % (name, k)))
             for k, (nV, nC) in enumerate(extra_shapes)]
    steps = [base]
    for kind in STEP_KIND[1:]:
        nxt = [problems.perturb(rng, q, 0.05) for q in steps[-1]]
        if kind == "newA":
            for q in nxt:
                q.A_val = q.A_val * (1.0 + 0.01 * rng.normal(size=q.A_val.shape))
        steps.append(nxt)
    return [st + extra for st in steps], budget, sums


def row_of(r, used, q):
    resc = [e for e in r.log if e.startswith("rescue")]
    x = r.qp.x.copy()
    return dict(used=used, mode=MODES[r.log[0]], rescue=RESCUES[resc[0] if resc else None], flag=r.qp.exitflag(),
                solved=bool(r.qp.is_solved()), x=x, y=r.qp.y.copy(), ws_b=r.qp.ws_bounds.copy(), ws_c=r.qp.ws_constraints.copy(),
                obj=float(q.g @ x), first=r.first)


_RUNS = {}


def oracle_run(O, name):
    """(steps, budget, sums, per step: list over members of dict(used, mode, rescue, flag, solved, x, y, ws_b, ws_c, obj, first));
    computed once per session and shared -- nobody changes it"""
    if name not in _RUNS:
        steps, budget, sums = sequence(name)
        refs = [LPRef(O, q, budget) for q in steps[0]]
        out = []
        for k, (kind, members) in enumerate(zip(STEP_KIND, steps)):
            if k == FULL_BUDGET_FROM:
                for r in refs:
                    r.maxit = 1000
            rows = []
            for r, q in zip(refs, members):
                if kind == "newA":
                    r.set_mats(q)
                rows.append(row_of(r, r.optimize(q), q))
            out.append(rows)
        _RUNS[name] = (steps, budget, sums, out)
    return _RUNS[name]


def count(rows, mode=None, rescue=None, solved=None):
    return sum(1 for r in rows if (mode is None or r["mode"] == mode) and (rescue is None or r["rescue"] == rescue) and
               (solved is None or r["solved"] == solved))


def is_vertex(r):
    return int(np.count_nonzero(r["ws_b"]) + np.count_nonzero(r["ws_c"])) == r["x"].size


def assert_inputs_cover_the_branches(name, sums, ora):
    """conditions on the INPUTS, from the oracle run alone"""
    assert tuple(sum(r["used"] for r in rows) for rows in ora) == sums, tuple(sum(r["used"] for r in rows) for rows in ora)
    # the working set of every solved member is unique: a vertex (another seed if this fails, never a looser comparison)
    assert all(is_vertex(r) for rows in ora for r in rows if r["solved"])
    s1, s2, s3, s4, s5, s6 = ora
    assert all(r["mode"] == 0 for r in s1)
    # members in different states within single calls: cold next to hot-vectors; cold, hot-matrices and the flip side by side
    assert count(s2, mode=0) > 0 and count(s2, mode=1) > 0
    assert count(s3, mode=0) > 0 and count(s3, mode=2) > 0 and count(s3, mode=3) > 0
    assert count(s4, mode=2) > 0 and count(s5, mode=3) > 0 and count(s6, mode=1) > 0
    every = {(r["mode"], r["rescue"]) for rows in ora for r in rows}
    # rescues from scratch after a cold start and after a flip, the slack-point rescue
    assert {(0, 1), (3, 1), (0, 2)} <= every, every
    # the inconsistent member with nV >= 2 nC takes the slack-point rescue in every call and stays unsolved
    n_extra = len(BATCHES[name][4])
    for rows in ora:
        r = rows[len(rows) - n_extra]
        assert (r["mode"], r["rescue"], r["solved"], r["first"]) == (0, 2, False, False)
        if n_extra == 2:
            assert (rows[-1]["mode"], rows[-1]["rescue"], rows[-1]["solved"]) == (0, 1, False)
    # members that hit the iteration limit: rescued from scratch, some of them still unsolved behind the rescue
    assert any(count(rows[:len(rows) - n_extra], rescue=1, solved=False) > 0 for rows in ora[:FULL_BUDGET_FROM])
    # with the full budget the members that never had a solved first LP run cold and solve
    assert count(s6[:len(s6) - n_extra], mode=0, solved=True) > 0 and count(s6[:len(s6) - n_extra], solved=False) == 0


def one_pattern_members(nq=70, seed=7):
    """nq members of ONE pattern: one 8 x 2 LP and its perturbations; a second step perturbs every member again"""
    rng = np.random.default_rng(seed)
    base = random_lp(rng, 8, 2, name="lp8x2")
    first = [base] + [problems.perturb(rng, base, 0.05) for _ in range(nq - 1)]
    return first, [problems.perturb(rng, q, 0.05) for q in first]


def assert_member(tag, r, o, used, mode, rescue):
    """one member of one step against LPRef"""
    assert r["status"] == o["flag"], (tag, "flag", r["status"], o["flag"])
    assert int(used) == o["used"], (tag, "nWSR_used", int(used), o["used"])
    assert (int(mode), int(rescue)) == (o["mode"], o["rescue"]), (tag, "dispatch", int(mode), int(rescue), o["mode"], o["rescue"])
    assert np.array_equal(r["ws_b"], o["ws_b"]) and np.array_equal(r["ws_c"], o["ws_c"]), (tag, "working set")
    xs, ys = max(1.0, np.abs(o["x"]).max()), max(1.0, np.abs(o["y"]).max())
    assert np.abs(o["x"] - r["x"]).max() <= TOL * xs, (tag, "x", np.abs(o["x"] - r["x"]).max() / xs)
    assert np.abs(o["y"] - r["y"]).max() <= TOL * ys, (tag, "y", np.abs(o["y"] - r["y"]).max() / ys)
    if "obj" in o:
        assert abs(o["obj"] - r["obj"]) <= TOL * max(1.0, abs(o["obj"])), (tag, "objective", r["obj"], o["obj"])
