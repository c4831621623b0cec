"""Members of a batch on their own (rsqp_batch_set_members, rsqp_batch_set_matrix_values_of, rsqp_batch_set_vectors_of;
restartsqp_amd/csrc/rsqp_batch_optimize.hip, rsqp_batch_handler.hip): a member sits out optimize calls, takes new matrices alone,
and behaves as a single rsqp_solver that received only the calls it was named in or took part in.

The sequences, references and tolerances are those of tests/test_gpu_batch_optimize.py (`T`) and tests/lp_batch_ref.py (`R`); what is
new is a SCHEDULE from one seeded generator: per step and member `takes_part` (p = 0.7, the first step included), and per step that
brings new matrices `named` (p = 0.7, independent of takes_part). The reference of member q is one T.Ref / R.LPRef over the CPU oracle
that gets set_mats only when q is named and optimize only when q takes part. The batch gets NaN in every entry of a member that is not
named, so a copy that leaks shows. Which situations occur is a condition on the INPUTS and is asserted from the oracle run alone.

Schedule seeds: chosen on the CPU oracle from 1..8, the first that meets the conditions of its test (SEEDS / LP_SEEDS; the seeds
tried are listed there)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData

import lp_batch_ref as R
import test_gpu_batch_optimize as T

pytestmark = pytest.mark.gpu

P_TAKE = P_NAMED = 0.7
# batch -> schedule seed. Tried in order 1, 2, ...; the first seed whose oracle run meets assert_schedule_covers_the_cases
# (seed 1 of hs64 and hs64_small: the inconsistent member never sits out directly after an infeasible answer)
SEEDS = {"hs64": 2, "hs64_small": 2, "hbm12": 1}
SEEDS_TRIED = {"hs64": (1, 2), "hs64_small": (1, 2), "hbm12": (1,)}
LP_SEEDS = {"tiny": 1, "hbm": 1}
LP_SEEDS_TRIED = {"tiny": (1,), "hbm": (1,)}


def schedule(seed, kinds, nq, mats_kinds):
    """(takes[step][member], named[step][member]) as bool arrays; named is drawn for the steps that bring matrices only (all False
    elsewhere)"""
    rng = np.random.default_rng(seed)
    takes = np.zeros((len(kinds), nq), bool); named = np.zeros((len(kinds), nq), bool)
    for k, kind in enumerate(kinds):
        takes[k] = rng.random(nq) < P_TAKE
        if kind in mats_kinds:
            named[k] = rng.random(nq) < P_NAMED
    return takes, named


def nan_where(arrays, keep):
    """the members' arrays concatenated, NaN in every entry of a member with keep[q] false"""
    return np.concatenate([a if k else np.full(a.shape, np.nan) for a, k in zip(arrays, keep)] + [np.zeros(0)])


def masked_vectors(b, members, keep):
    b.set_vectors(*[nan_where([getattr(q, n) for q in members], keep) for n in ("g", "lb", "ub", "lbA", "ubA")], members=keep)


def same_bytes(a, c):
    return (all(np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes() for k in ("x", "y", "ws_b", "ws_c")) and
            a["status"] == c["status"] and a["nWSR"] == c["nWSR"] and np.float64(a["obj"]).tobytes() == np.float64(c["obj"]).tobytes())


def assert_sitter(tag, before, after, used, mode, rescue):
    assert int(used) == 0 and (int(mode), int(rescue)) == (-1, 0), (tag, "sitter", int(used), int(mode), int(rescue))
    assert same_bytes(before, after), (tag, "a member that sat out has other results")


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the seven-step sequences of T with a schedule
# ---------------------------------------------------------------------------------------------------------------------------------
_QP_RUNS = {}


def masked_oracle_run(O, name, seed):
    """(steps, budget, takes, named, rows): rows[step][member] = the dict of T.oracle_run, or None where the member sat out"""
    if (name, seed) not in _QP_RUNS:
        steps, budget, sums = T.sequence(name)
        nq = len(steps[0])
        takes, named = schedule(seed, T.STEP_KIND, nq, ("newmats",))
        refs = [T.Ref(O, q, budget) for q in steps[0]]
        out = []
        for k, members in enumerate(steps):
            if k == 5:
                for r in refs:
                    r.maxit = 1000
            rows = []
            for q, (r, m) in enumerate(zip(refs, members)):
                if named[k, q]:
                    r.set_mats(m)
                if not takes[k, q]:
                    rows.append(None)
                    continue
                used = r.optimize(m)
                resc = [e for e in r.log if e.startswith("rescue")]
                rows.append(dict(used=used, mode=T.MODES[r.log[0]], rescue=T.RESCUES[resc[0] if resc else None], flag=r.qp.exitflag(),
                                 solved=bool(r.qp.is_solved()), x=r.qp.x.copy(), y=r.qp.y.copy(), ws_b=r.qp.ws_bounds.copy(),
                                 ws_c=r.qp.ws_constraints.copy()))
            out.append(rows)
        _QP_RUNS[name, seed] = (steps, budget, takes, named, out)
    return _QP_RUNS[name, seed]


def inconsistent_index(members):
    """where T.sequence put T.inconsistent_member(): the one member whose constraint bounds cross"""
    e = [q for q, m in enumerate(members) if np.any(m.lbA > m.ubA)]
    assert len(e) == 1, e
    return e[0]


def schedule_gaps(takes, named, rows, e):
    """what of the list below the oracle run of one schedule does NOT hold (empty: the schedule serves); e: the inconsistent member"""
    nsteps, nq = takes.shape
    miss = []
    if not all(0 < takes[k].sum() < nq for k in range(nsteps)):
        miss.append("every step has a sitter and a participant")
    firsts = [int(np.argmax(takes[:, q])) if takes[:, q].any() else -1 for q in range(nq)]
    if not any(firsts[q] > 0 and any(o is not None and o["mode"] in (1, 2) for o in rows[firsts[q]]) for q in range(nq)):
        miss.append("a first solve in a call where others hot-start")
    waited = unnamed_hot = False
    for q in range(nq):
        for k in range(nsteps):
            if named[k, q] and not takes[k, q]:
                later = [p for p in range(k + 1, nsteps) if takes[p, q]]
                if later and not named[later[0], q] and rows[later[0]][q]["mode"] in (2, 3):
                    waited = True
            if T.STEP_KIND[k] == "newmats" and takes[k, q] and not named[k, q] and rows[k][q]["mode"] == 1:
                unnamed_hot = True
    if not waited:
        miss.append("named while sitting out, mode 2 or 3 at the next participation (not named there)")
    if not unnamed_hot:
        miss.append("a participant of a newmats step that is not named runs mode 1")
    if not any(takes[k, e] and not rows[k][e]["solved"] and rows[k][e]["flag"] == 22 and not takes[k + 1, e] and takes[k + 2:, e].any()
               for k in range(nsteps - 2)):
        miss.append("the inconsistent member sits out directly after an infeasible answer and takes part again later")
    if not any(len({o["mode"] for o in rs if o is not None}) >= 3 and any(o is not None and o["rescue"] for o in rs) for rs in rows):
        miss.append("a call with three different modes and a rescue")
    return miss


def assert_schedule_covers_the_cases(name, steps, takes, named, rows):
    miss = schedule_gaps(takes, named, rows, inconsistent_index(steps[0]))
    assert not miss, (name, miss)


def masked_matrices(b, members, keep):
    b.set_matrix_values(nan_where([q.A_val for q in members], keep), nan_where([q.H_val for q in members], keep), members=keep)


@pytest.mark.parametrize("name,kernel", [("hs64", 0), ("hs64_small", 1), ("hbm12", 3)])
def test_masked_sequence_matches_the_oracle(capi, oracle, name, kernel):
    """participants: exit flag, nWSR_used, mode, rescue and working sets equal to the oracle-driven restatement, x and y within T.RTOL;
    members that sit out: nWSR_used 0, dispatch (-1, 0), results byte-identical to those before the call"""
    steps, budget, takes, named, ora = masked_oracle_run(oracle, name, SEEDS[name])
    assert_schedule_covers_the_cases(name, steps, takes, named, ora)
    b = capi.Batch(steps[0])
    b.set_options(qp_maxiter=budget)
    for k, (kind, members, rows) in enumerate(zip(T.STEP_KIND, steps, ora)):
        if k == 5:
            b.set_options(qp_maxiter=1000)
        b.set_members(takes[k])
        if kind == "newmats":
            masked_matrices(b, members, named[k])
        masked_vectors(b, members, takes[k])
        before = b.results()
        used = b.optimize_qp()
        assert b.last_kernel() == kernel
        mode, rescue = b.dispatch()
        res = b.results()
        wrong = []
        for q in range(b.nq):
            tag = (name, k + 1, q)
            try:
                if takes[k, q]:
                    T.assert_member(tag, res[q], rows[q], used[q], mode[q], rescue[q])
                else:
                    assert_sitter(tag, before[q], res[q], used[q], mode[q], rescue[q])
            except AssertionError as e:
                wrong.append(str(e).splitlines()[0])
        assert not wrong, wrong
    b.close()


@pytest.mark.parametrize("name", ["hs64", "hs64_small", "hbm12"])
def test_masked_sequence_matches_single_handles(capi, name):
    """the same schedules through nq single handles: handle q gets set_A_csc / set_H_csc only when named and optimize_qp only when it
    takes part. Flag, nWSR_used, last_mode (with the rescue rule of T.test_batch_members_match_single_handles) and raw working sets
    equal, x and y within T.RTOL"""
    steps, budget, sums = T.sequence(name)
    nq = len(steps[0])
    takes, named = schedule(SEEDS[name], T.STEP_KIND, nq, ("newmats",))
    b = capi.Batch(steps[0])
    b.set_options(qp_maxiter=budget)
    hs = []
    for q in steps[0]:
        s = capi.Solver(q.nV, q.nC)
        s.set_options(qp_maxiter=budget)
        s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        hs.append(s)
    for k, (kind, members) in enumerate(zip(T.STEP_KIND, steps)):
        if k == 5:
            b.set_options(qp_maxiter=1000)
        b.set_members(takes[k])
        if kind == "newmats":
            masked_matrices(b, members, named[k])
        masked_vectors(b, members, takes[k])
        used = b.optimize_qp()
        mode, rescue = b.dispatch()
        res = b.results()
        for q, (s, m) in enumerate(zip(hs, members)):
            if k == 5:
                s.set_options(qp_maxiter=1000)
            if named[k, q]:
                s.set_A_csc(m.A_jc, m.A_ir, m.A_val); s.set_H_csc(m.H_jc, m.H_ir, m.H_val)
            tag = (name, k + 1, q)
            if not takes[k, q]:
                assert int(used[q]) == 0 and (int(mode[q]), int(rescue[q])) == (-1, 0), tag
                continue
            for w, v in zip(range(5), (m.g, m.lb, m.ub, m.lbA, m.ubA)):
                s.set_vector(w, v)
            n = s.optimize_qp()
            r = res[q]
            assert r["status"] == s.status and int(used[q]) == n, (tag, r["status"], s.status, int(used[q]), n)
            if rescue[q] == 0:
                assert int(mode[q]) == s.last_mode(), (tag, int(mode[q]), s.last_mode())
            else:
                assert s.last_mode() == (capi.MODE_COLD if rescue[q] == 1 else capi.MODE_WARM_REINIT), tag
            wb, wc = s.working_set_raw()
            assert np.array_equal(r["ws_b"], wb) and np.array_equal(r["ws_c"], wc), tag
            xs, ys = max(1.0, np.abs(s.x).max()), max(1.0, np.abs(s.y).max())
            assert np.abs(s.x - r["x"]).max() <= T.RTOL * xs and np.abs(s.y - r["y"]).max() <= T.RTOL * ys, tag
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: the six-step LP sequence of R with a schedule
# ---------------------------------------------------------------------------------------------------------------------------------
_LP_RUNS = {}


def masked_lp_run(O, name, seed):
    """as masked_oracle_run, over R.LPRef"""
    if (name, seed) not in _LP_RUNS:
        steps, budget, sums = R.sequence(name)
        nq = len(steps[0])
        takes, named = schedule(seed, R.STEP_KIND, nq, ("newA",))
        refs = [R.LPRef(O, q, budget) for q in steps[0]]
        out = []
        for k, members in enumerate(steps):
            if k == R.FULL_BUDGET_FROM:
                for r in refs:
                    r.maxit = 1000
            rows = []
            for q, (r, m) in enumerate(zip(refs, members)):
                if named[k, q]:
                    r.set_mats(m)
                if not takes[k, q]:
                    rows.append(None)
                    continue
                rows.append(R.row_of(r, r.optimize(m), m))
            out.append(rows)
        _LP_RUNS[name, seed] = (steps, budget, takes, named, out)
    return _LP_RUNS[name, seed]


def lp_schedule_gaps(steps, takes, named, rows):
    nsteps, nq = takes.shape
    miss = []
    if not all(0 < takes[k].sum() < nq for k in range(nsteps)):
        miss.append("every step has a sitter and a participant")
    # an init at step i, sat out in between, a hot start at step k on the factors -- and the regVal -- of step i, while the gradients
    # of the steps between have another norm (the situation in which a regVal could be taken from a call the member sat out; regVal is
    # about 1e-13 |g|, so R.TOL would not show a wrong one: what is checked is that the member's later hot start matches its LPRef)
    found = False
    for q in range(nq):
        for i in range(nsteps):
            if rows[i][q] is None or rows[i][q]["mode"] not in (0, 3) or not rows[i][q]["solved"] or rows[i][q]["rescue"]:
                continue
            later = [p for p in range(i + 1, nsteps) if takes[p, q]]
            if later and later[0] > i + 1 and rows[later[0]][q]["mode"] in (1, 2):
                ng = [float(np.sqrt(np.sum(steps[j][q].g ** 2))) for j in range(i, later[0])]
                found = found or all(abs(n - ng[0]) > 1e-6 * ng[0] for n in ng[1:])
    if not found:
        miss.append("a member sits out between an init and a later hot start, the gradients between have another norm")
    return miss


@pytest.mark.parametrize("name", ["tiny", "hbm"])
def test_masked_lp_sequence_matches_the_oracle(capi, oracle, name):
    """rsqp_batch_optimize_lp with a schedule, on an LDS-resident and an HBM-resident batch: participants against R.LPRef within
    R.TOL -- a member that sat out between an init and a hot start included --, members that sit out untouched"""
    kernel = {"tiny": 0, "hbm": 3}[name]
    steps, budget, takes, named, ora = masked_lp_run(oracle, name, LP_SEEDS[name])
    miss = lp_schedule_gaps(steps, takes, named, ora)
    assert not miss, (name, miss)
    b = capi.Batch(steps[0])
    b.set_options(lp_maxiter=budget)
    for k, (kind, members, rows) in enumerate(zip(R.STEP_KIND, steps, ora)):
        if k == R.FULL_BUDGET_FROM:
            b.set_options(lp_maxiter=1000)
        b.set_members(takes[k])
        if kind == "newA":
            b.set_matrix_values(nan_where([q.A_val for q in members], named[k]), None, members=named[k])
        masked_vectors(b, members, takes[k])
        before = b.results()
        used = b.optimize_lp()
        assert b.last_kernel() == kernel
        mode, rescue = b.dispatch()
        res = b.results()
        wrong = []
        for q in range(b.nq):
            tag = (name, k + 1, q)
            try:
                if takes[k, q]:
                    R.assert_member(tag, res[q], rows[q], used[q], mode[q], rescue[q])
                else:
                    assert_sitter(tag, before[q], res[q], used[q], mode[q], rescue[q])
            except AssertionError as e:
                wrong.append(str(e).splitlines()[0])
        assert not wrong, wrong
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: a stored state of another kernel family is not hot-started
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_state_of_another_family_is_not_hot_started(capi):
    """hs64_small (at most 8 variables). a: everybody solves on the hs071-scale tableau kernel. b: member 0 is named with an H that
    is unsymmetric in one off-diagonal pair, which moves the batch to the LDS-resident null-space kernels; member 5 sits out and
    keeps a state in the tableau kernel's layout. c: everybody takes part, still on the null-space kernels: member 5 must start
    cold -- mode 0, and what a fresh handle finds from a cold start on the same data"""
    base = T.BATCHES["hs64_small"][0]()
    nq = len(base)
    rng = np.random.default_rng(9)
    b = capi.Batch(base)
    b.optimize_qp()
    assert b.last_kernel() == 1 and b.results()[5]["status"] == 20
    # b
    q0 = base[0]
    H = q0.dense_H()
    r, c = [(i, j) for j in range(q0.nV) for i in range(j + 1, q0.nV) if H[i, j] != 0.0][0]
    Hval = [q.H_val.copy() for q in base]
    for k in range(q0.H_jc[c], q0.H_jc[c + 1]):
        if q0.H_ir[k] == r:
            Hval[0][k] *= 1.0 + 1e-3
    only0 = np.arange(nq) == 0
    b.set_matrix_values(None, nan_where(Hval, only0), members=only0)
    b.set_members(np.arange(nq) != 5)
    stepb = [problems.perturb(rng, q, 0.05) for q in base]
    masked_vectors(b, stepb, np.arange(nq) != 5)
    before = b.results()[5]
    used = b.optimize_qp()
    mode, rescue = b.dispatch()
    assert b.last_kernel() == 0
    assert_sitter(("family", "b", 5), before, b.results()[5], used[5], mode[5], rescue[5])
    assert np.all(np.delete(mode, 5) == 0)            # (the others: hot starts on the tableau kernel's states run cold)
    # c
    stepc = [problems.perturb(rng, q, 0.05) for q in stepb]
    b.set_members(None)
    b.set_vectors_from(stepc)
    used = b.optimize_qp()
    mode, rescue = b.dispatch()
    assert b.last_kernel() == 0
    assert int(mode[5]) == 0 and int(mode[1]) == 1, (int(mode[5]), int(mode[1]))
    m = stepc[5]
    s = capi.Solver(m.nV, m.nC)
    s.set_A_csc(m.A_jc, m.A_ir, m.A_val); s.set_H_csc(m.H_jc, m.H_ir, m.H_val)
    for w, v in zip(range(5), (m.g, m.lb, m.ub, m.lbA, m.ubA)):
        s.set_vector(w, v)
    n = s.optimize_qp()
    r5 = b.results()[5]
    assert s.last_mode() == capi.MODE_COLD and rescue[5] == 0
    assert r5["status"] == s.status and int(used[5]) == n, (r5["status"], s.status, int(used[5]), n)
    wb, wc = s.working_set_raw()
    assert np.array_equal(r5["ws_b"], wb) and np.array_equal(r5["ws_c"], wc)
    xs, ys = max(1.0, np.abs(s.x).max()), max(1.0, np.abs(s.y).max())
    assert np.abs(s.x - r5["x"]).max() <= T.RTOL * xs and np.abs(s.y - r5["y"]).max() <= T.RTOL * ys
    ok, kkt = b.test_optimality()
    assert ok[5] == 1, float(kkt[5])
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: three SQP runs in lock step
# ---------------------------------------------------------------------------------------------------------------------------------
NLPS = {"hs071": problems.hs071_nlp, "hs035": problems.hs035_nlp, "hs065": problems.hs065_nlp}
LOCKSTEP = (("hs071", 0), ("hs035", 0), ("hs065", 0), ("hs071", 2), ("hs035", 1), ("hs065", 3))   # (trajectory, first batch step)


def full_pattern(q):
    """the QP with every entry of A and H stored, explicit zeros included: the Hessian's zero pattern moves with lam"""
    def full(M):
        nr, nc = M.shape
        return (np.arange(nc + 1, dtype=np.int32) * nr, np.tile(np.arange(nr, dtype=np.int32), nc),
                np.ascontiguousarray(M.flatten(order="F"), dtype=np.float64))
    return QPData(q.nV, q.nC, *full(q.dense_H()), *full(q.dense_A()), q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name)


def trajectory_qps(name):
    gold = json.load(open(os.path.join(GOLDEN, "sqp_traces.json")))[name]["qps"]
    return gold, [full_pattern(problems.handler_qp(NLPS[name](np.array(g["x"]), np.array(g["lam"])), g["delta"], g["rho"], name=name))
                  for g in gold]


def assert_oracle_replays_the_trajectories(oracle, runs):
    """conditions on the inputs of the lock-step test, from the oracle alone: T.Ref fed with problems.handler_qp of every trace
    entry -- new matrices iff the entry's flags say A or H -- runs the trace's modes and counts"""
    for name, (gold, qps) in runs.items():
        ref = T.Ref(oracle, qps[0], 1000)
        for g, q in zip(gold, qps):
            if g["flags"]["A"] or g["flags"]["H"]:
                ref.set_mats(q)
            n = ref.optimize(q)
            assert (ref.log[0], n, ref.qp.exitflag()) == (g["mode"], g["nWSR"], 20), (name, g["it"], ref.log, n)
            assert np.abs(ref.qp.x - np.array(g["x_qp"])).max() <= 1e-9 * max(1.0, np.abs(g["x_qp"]).max()), (name, g["it"])


def test_lockstep_replay_of_three_sqp_runs(capi, oracle):
    """six members: two copies each of the hs071, hs035 and hs065 trajectories of tests/golden/sqp_traces.json, the second copies 2,
    1 and 3 batch steps late. Per batch step a member is at its own trace entry, or sits out before its start and after its end; it
    is named for matrices iff its entry's flags say A or H and gets vectors iff it takes part. In most steps one copy hot-starts on
    vectors while another takes new matrices: a batch-wide update flag cannot give every member the trace's mode. The QPs are 8 x 2,
    5 x 1 and 11 x 4 (hs065: 3 variables, 4 constraints, two slacks each), so the batch runs the LDS-resident null-space kernels.
    Criteria per participant: those of test_sqp_trajectory.test_gpu_replays_the_trajectory."""
    runs = {name: trajectory_qps(name) for name in NLPS}
    assert_oracle_replays_the_trajectories(oracle, runs)
    nq = len(LOCKSTEP)
    b = capi.Batch([runs[name][1][0] for name, start in LOCKSTEP])
    nsteps = max(start + len(runs[name][0]) for name, start in LOCKSTEP)
    ties = [0] * nq
    mixed = 0
    for t in range(nsteps):
        entry = [t - start if 0 <= t - start < len(runs[name][0]) else None for name, start in LOCKSTEP]
        take = np.array([e is not None for e in entry])
        gold = [runs[name][0][e] if e is not None else None for (name, start), e in zip(LOCKSTEP, entry)]
        members = [runs[name][1][e if e is not None else 0] for (name, start), e in zip(LOCKSTEP, entry)]
        name_m = np.array([g is not None and bool(g["flags"]["A"] or g["flags"]["H"]) for g in gold])
        mixed += bool(name_m.any() and (take & ~name_m).any())
        b.set_members(take)
        if name_m.any():
            masked_matrices(b, members, name_m)
        masked_vectors(b, members, take)
        before = b.results()
        used = b.optimize_qp()
        assert b.last_kernel() == 0
        mode, rescue = b.dispatch()
        res = b.results()
        ok, kkt = b.test_optimality()
        for j, ((name, start), g) in enumerate(zip(LOCKSTEP, gold)):
            tag = (name, j, t)
            if g is None:
                assert_sitter(tag, before[j], res[j], used[j], mode[j], rescue[j])
                continue
            r = res[j]
            assert int(mode[j]) == T.MODES[g["mode"]] and int(rescue[j]) == 0, (tag, int(mode[j]), g["mode"], int(rescue[j]))
            assert r["status"] == g["status"] == 20, (tag, r["status"])
            assert ok[j] == 1, (tag, float(kkt[j]))
            gx, gy = np.array(g["x_qp"]), np.array(g["y_qp"])
            assert np.abs(r["x"] - gx).max() <= 1e-9 * max(1.0, np.abs(gx).max()), (tag, g["mode"])
            assert abs(r["obj"] - g["obj"]) <= 1e-9 * max(1.0, abs(g["obj"])), tag
            same_path = int(used[j]) == g["nWSR"] and np.array_equal(r["ws_b"], g["ws_b"]) and np.array_equal(r["ws_c"], g["ws_c"])
            if name == "hs065":
                ties[j] += not same_path
                continue
            assert same_path, (tag, g["mode"], int(used[j]), g["nWSR"])
            assert np.abs(r["y"] - gy).max() <= 1e-9 * max(1.0, np.abs(gy).max()), (tag, g["mode"])
    assert max(ties) <= 3, ties
    assert mixed >= nsteps // 2, (mixed, nsteps)          # (condition on the inputs: most steps mix the two kinds of member)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the named setters on every layout of the pools
# ---------------------------------------------------------------------------------------------------------------------------------
def _layout_members(layout):
    from test_matrix_forms import shuffle, split, with_matrices
    rng = np.random.default_rng(17)
    if layout == "one_pattern":                       # one shape, one pattern: the member of an entry is a division
        return problems.hs071_scale_batch(40)
    base = problems.hs_batch(24)                      # shapes of their own: the member of an entry is searched in the offsets
    if layout == "canonical":
        return base
    f = {"split": lambda jc, ir, v: split(rng, jc, ir, v), "shuffle": lambda jc, ir, v: shuffle(rng, jc, ir, v)}[layout]
    return [with_matrices(q, f(q.A_jc, q.A_ir, q.A_val), f(q.H_jc, q.H_ir, q.H_val)) for q in base]


@pytest.mark.parametrize("layout", ["one_pattern", "canonical", "split", "shuffle"])
def test_named_setters_write_the_named_members_only(capi, layout):
    """two batches of the same members. One gets whole pools: the new data of the named members, the old data of the others. The
    other gets the named setters, with NaN in every entry of a member that is not named -- as its FIRST refresh, so the values a
    non-canonical layout keeps in the caller's form are those of rsqp_batch_create. A cold rsqp_batch_solve reads nothing but the
    pools: the results are byte-identical iff the pools are. split / shuffle: layouts that are folded into the canonical pools."""
    probs = _layout_members(layout)
    nq = len(probs)
    rng = np.random.default_rng(23)
    named_m = rng.random(nq) < 0.5; named_v = rng.random(nq) < 0.5
    assert 0 < named_m.sum() < nq and 0 < named_v.sum() < nq and (named_m != named_v).any()
    new = [problems.perturb(rng, q, 0.05) for q in probs]
    A2 = [q.A_val * (1.0 + 0.01 * rng.normal(size=q.A_val.shape)) for q in probs]
    H2 = [q.H_val * 1.05 for q in probs]
    merged = lambda old, neu, keep: np.concatenate([n if k else o for o, n, k in zip(old, neu, keep)] + [np.zeros(0)])
    x, y = capi.Batch(probs), capi.Batch(probs)
    x.set_matrix_values(merged([q.A_val for q in probs], A2, named_m), merged([q.H_val for q in probs], H2, named_m))
    x.set_vectors(*[merged([getattr(q, n) for q in probs], [getattr(q, n) for q in new], named_v) for n in ("g", "lb", "ub", "lbA", "ubA")])
    y.set_matrix_values(nan_where(A2, named_m), nan_where(H2, named_m), members=named_m)
    masked_vectors(y, new, named_v)
    nobody = np.zeros(nq, bool)                        # naming nobody does nothing
    y.set_matrix_values(nan_where(A2, nobody), nan_where(H2, nobody), members=nobody)
    masked_vectors(y, new, nobody)
    x.solve(capi.MODE_COLD, 1000); y.solve(capi.MODE_COLD, 1000)
    assert x.last_kernel() == y.last_kernel()
    rx, ry = x.results(), y.results()
    assert all(same_bytes(a, c) for a, c in zip(rx, ry)), [q for q, (a, c) in enumerate(zip(rx, ry)) if not same_bytes(a, c)]
    # (the comparison is not between two failures: most members solve, and no NaN reached a pool)
    assert sum(r["status"] == 20 for r in ry) > nq // 2 and np.all(np.isfinite(np.concatenate([r["x"] for r in ry])))
    x.close(); y.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# calls in which nobody takes part
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["qp", "lp"])
def test_a_call_nobody_takes_part_in(capi, oracle, kind):
    """an empty mask is legal: the call does nothing, reports nWSR_used 0 and dispatch (-1, 0) for everybody and leaves the results
    alone -- as the FIRST call of a batch and after a full call. The full call behind the first empty one starts every member cold
    and says so (mode 0, not the -1 the empty call left), the one behind it hot-starts on new vectors; both against the reference."""
    if kind == "qp":
        members = problems.hs_batch(16)
        refs = [T.Ref(oracle, q, 1000) for q in members]
        row = lambda r, n, q: dict(used=n, mode=T.MODES[r.log[0]], rescue=T.RESCUES[([e for e in r.log if e.startswith("rescue")] + [None])[0]],
                                   flag=r.qp.exitflag(), x=r.qp.x.copy(), y=r.qp.y.copy(), ws_b=r.qp.ws_bounds.copy(),
                                   ws_c=r.qp.ws_constraints.copy())
        check = T.assert_member
    else:
        members = R.sequence("tiny")[0][0]
        refs = [R.LPRef(oracle, q, 1000) for q in members]
        row = lambda r, n, q: R.row_of(r, n, q)
        check = R.assert_member
    nq = len(members)
    rng = np.random.default_rng(4)
    second = [q if np.any(q.lbA > q.ubA) else problems.perturb(rng, q, 0.05) for q in members]      # (crossed bounds stay crossed)
    b = capi.Batch(members)
    b.set_options(qp_maxiter=1000, lp_maxiter=1000)
    run = b.optimize_qp if kind == "qp" else b.optimize_lp

    def empty_call(tag):
        b.set_members(np.zeros(nq))
        before = b.results()
        used = run()
        mode, rescue = b.dispatch()
        for q, (a, c) in enumerate(zip(before, b.results())):
            assert_sitter((kind, tag, q), a, c, used[q], mode[q], rescue[q])
        b.set_members(None)

    empty_call("first")
    for call, data in enumerate((members, second)):
        if call > 0:
            b.set_vectors_from(data)
        rows = [row(r, r.optimize(q), q) for r, q in zip(refs, data)]
        assert all(o["mode"] == 0 for o in rows) if call == 0 else any(o["mode"] == 1 for o in rows)
        used = run()
        mode, rescue = b.dispatch()
        res = b.results()
        for q in range(nq):
            check((kind, "full", call, q), res[q], rows[q], used[q], mode[q], rescue[q])
        empty_call("behind full call %d" % call)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: the default path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_all_ones_mask_is_the_default_path(capi):
    """a 70-member one-pattern batch: set_members(ones) followed by optimize_qp gives byte-identical results to the same call on a
    batch that never saw set_members, on the same kernel"""
    rng = np.random.default_rng(7)
    base = problems.hs071_first_qp()
    first = [base] + [problems.perturb(rng, base, 0.05) for _ in range(69)]
    second = [problems.perturb(rng, q, 0.05) for q in first]
    a, c = capi.Batch(first), capi.Batch(first)
    c.set_members(np.ones(c.nq))
    for call, members in enumerate((first, second)):
        if call > 0:
            a.set_vectors_from(members); c.set_vectors_from(members)
        ua, uc = a.optimize_qp(), c.optimize_qp()
        assert a.last_kernel() == c.last_kernel() == 1
        assert np.array_equal(ua, uc) and all(np.array_equal(m, n) for m, n in zip(a.dispatch(), c.dispatch()))
        assert all(same_bytes(x, y) for x, y in zip(a.results(), c.results()))
    a.close(); c.close()
