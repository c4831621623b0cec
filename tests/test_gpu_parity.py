"""Parity of the HIP path (through the C ABI of include/rsqp_hip.h) against the CPU oracle.

Bar: working sets, statuses and iteration counts bit-exact; x, y within 1e-9 relative
(fp64 everywhere; the GPU differs from the oracle only in summation order and FMA
contraction). Products: <= 4*nnz_row*eps relative ("Summation order")."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, clamp, dump_paths, oracle_certificate, oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc, read_qore_dump

pytestmark = pytest.mark.gpu

RTOL = 1e-9


def assert_same_solution(qp, r, n_oracle, check_nwsr=True):
    assert r["status"] == qp.exitflag()
    assert np.array_equal(qp.ws_bounds, r["ws_b"]) and np.array_equal(qp.ws_constraints, r["ws_c"])
    if check_nwsr:
        assert r["nWSR"] == n_oracle
    xs, ys = max(1.0, np.abs(qp.x).max()), max(1.0, np.abs(qp.y).max())
    assert np.abs(qp.x - r["x"]).max() <= RTOL * xs
    assert np.abs(qp.y - r["y"]).max() <= RTOL * ys


def test_library_on_gpu(capi):
    assert capi.device_count() >= 1


def test_hs071_single_qp_bit_exact_active_set(capi, oracle):
    """BASELINE config 1: hs071 first QP, one QP on one MI355X, through optimizeQP."""
    q = problems.hs071_first_qp()
    s = capi.Solver(q.nV, q.nC)
    s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
    for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
        s.set_vector(w, v)
    n = s.optimize_qp()
    qp, rc, n_or = oracle_cold(oracle, q)
    wb, wc = s.working_set_raw()
    assert s.is_solved() and s.status == 20 and n == n_or == 2
    assert wb.tolist() == qp.ws_bounds.tolist() == [-1, 0, -1, 0, -1, -1, -1, -1]
    assert wc.tolist() == qp.ws_constraints.tolist() == [-1, 1]
    assert np.abs(s.x - np.array([0, -0.25, -1, 0.25, 0, 0, 0, 0])).max() < 1e-14
    assert np.abs(s.y - qp.y).max() < 1e-12 and abs(s.objective - 0.1875) < 1e-14
    ok, st, Wc, Wb = s.test_optimality()
    ok_o, st_o, Wb_o, Wc_o = oracle_certificate(oracle, q, s.x, s.y, wb, wc)
    assert ok and ok_o and Wc.tolist() == Wc_o.tolist() and Wb.tolist() == Wb_o.tolist()
    assert abs(st.KKT_error - st_o.KKT_error) < 1e-12


def test_batch_random_convex(capi, oracle):
    rng = np.random.default_rng(5)
    probs = [problems.random_qp(rng, int(rng.integers(1, 45)), int(rng.integers(0, 50))) for _ in range(96)]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    ok, kkt = b.test_optimality()
    for q, r, o, k in zip(probs, b.results(), ok, kkt):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
        if rc == 0:
            assert o == 1 and k < 1e-9
            assert abs(r["obj"] - qp.objective) <= 1e-9 * max(1.0, abs(qp.objective))


def test_one_shape_batches_with_one_and_with_several_patterns(capi, oracle):
    """Batches of ONE shape (8 x 2 .. 6 x 5: the register-resident kernel): when every member also has the sparsity pattern of
    member 0 the kernel computes its offsets and reads member 0's pattern arrays (QPPools::uni_pat); one member with another
    pattern -- same sizes, same entry counts or not -- must switch that off. Cold solve, then a hot start on new vectors."""
    rng = np.random.default_rng(77)
    for nV, nC in ((8, 2), (6, 5), (3, 8)):
        base = problems.random_qp(rng, nV, nC, density=0.6)
        same = [problems.perturb(rng, base, 0.05) for _ in range(40)]
        # values differ per member as well (the pattern stays)
        for q in same:
            q.A_val = q.A_val * (1.0 + 0.05 * rng.normal(size=q.A_val.shape))
        other = [problems.random_qp(rng, nV, nC, density=0.6) for _ in range(8)]
        for probs in (same, same[:20] + other + same[20:], other):
            b = capi.Batch(probs)
            b.solve(capi.MODE_COLD, 1000)
            orcs = []
            for q, r in zip(probs, b.results()):
                qp, rc, n = oracle_cold(oracle, q)
                assert_same_solution(qp, r, n)
                orcs.append(qp)
            # hot start on new vectors (state I/O of every member: offState = q * uni_state on the one-pattern path) ...
            p2 = [problems.perturb(rng, q, 0.05) for q in probs]
            b.set_vectors_from(p2)
            b.solve(capi.MODE_HOT_VECTORS, 1000)
            for q, qp, r in zip(p2, orcs, b.results()):
                rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
                assert_same_solution(qp, r, n)
            # ... and on new matrix values as well (member 0's pattern arrays are read in this mode too)
            p3 = [problems.perturb(rng, q, 0.05) for q in p2]
            for q in p3:
                q.A_val = q.A_val * (1.0 + 0.02 * rng.normal(size=q.A_val.shape))
            b.set_vectors_from(p3)
            b.set_matrix_values(np.concatenate([q.A_val for q in p3]), np.concatenate([q.H_val for q in p3]))
            b.solve(capi.MODE_HOT_MATRICES, 1000)
            for q, qp, r in zip(p3, orcs, b.results()):
                qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
                rc, n = qp.hotstart_matrices(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
                assert_same_solution(qp, r, n)
            b.close()


def test_batch_edge_cases(capi, oracle):
    """No constraints, a single variable, infinite bounds, equalities, infeasible, iteration limit."""
    rng = np.random.default_rng(11)
    probs = [problems.random_qp(rng, 6, 0), problems.random_qp(rng, 1, 0), problems.random_qp(rng, 1, 3)]
    q = problems.random_qp(rng, 7, 4); q.lb[:] = -np.inf; q.ub[:] = 1e20; probs.append(q)      # free variables
    q = problems.random_qp(rng, 7, 4); q.lbA[:] = -np.inf; probs.append(q)
    q = problems.random_qp(rng, 9, 3); q.ubA[:] = q.lbA; probs.append(q)                       # equalities
    q = problems.random_qp(rng, 5, 2); q.ub[:] = q.lb; probs.append(q)                          # fixed variables
    A = np.array([[1.0, 1.0]])
    probs.append(QPData(2, 1, *dense_to_csc(np.eye(2)), *dense_to_csc(A), np.zeros(2), -np.ones(2), np.ones(2),
                        np.array([3.0]), np.array([np.inf])))                                   # infeasible
    H = np.diag([1.0, -1.0])
    probs.append(QPData(2, 0, *dense_to_csc(H), *dense_to_csc(np.zeros((0, 2))), np.array([0.0, -1.0]),
                        np.array([-1.0, 0.0]), np.array([1.0, np.inf]), np.zeros(0), np.zeros(0)))   # unbounded
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    res = b.results()
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
    assert res[-2]["status"] == 22 and res[-1]["status"] == 23
    # iteration limit: same count, same (unfinished) status as the oracle
    q = problems.random_qp(np.random.default_rng(3), 30, 40)
    b = capi.Batch([q]); b.solve(capi.MODE_COLD, 3)
    qp, rc, n = oracle_cold(oracle, q, nWSR=3)
    r = b.results()[0]
    assert r["nWSR"] == n == 3 and r["status"] == qp.exitflag() == 28


def test_reference_dumps(capi, oracle):
    """The 18 QPs of reference test/unsolved_QP_data plus hs071 against the committed oracle
    vectors. Every dump has an indefinite or singular Hessian, so the homotopy path (and with
    it nWSR) is not unique under rounding; the final working set, x and y are compared, nWSR
    only where no bound flip occurred."""
    gold = json.load(open(os.path.join(GOLDEN, "oracle_qp_solutions.json")))
    probs = [problems.hs071_first_qp()] + [read_qore_dump(p) for p in dump_paths()]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    ok, kkt = b.test_optimality()
    for q, r, o, k in zip(probs, b.results(), ok, kkt):
        e = gold[q.name]
        assert r["status"] == e["exitflag"] == 20
        xs, ys = max(1.0, np.abs(e["x"]).max()), max(1.0, np.abs(e["y"]).max())
        assert np.abs(np.array(e["x"]) - r["x"]).max() <= 1e-9 * xs
        if e["nflips"] == 0:
            assert r["ws_b"].tolist() == e["ws_b"] and r["ws_c"].tolist() == e["ws_c"]
            assert r["nWSR"] == e["nWSR"]
            assert np.abs(np.array(e["y"]) - r["y"]).max() <= 1e-9 * ys
        else:
            # bound flips on a non-convex QP: an equality held "at its lower side" by one run may be held
            # "at its upper side" by the other (the batch runs the explicit-inverse formulation for
            # nV > 8, the golden vectors come from the Givens / TQ oracle). Same point, same objective,
            # same set of active quantities, same sides wherever the two sides differ.
            wb, wc, eb, ec = r["ws_b"], r["ws_c"], np.array(e["ws_b"]), np.array(e["ws_c"])
            eq_b, eq_c = q.lb == q.ub, q.lbA == q.ubA
            assert np.array_equal(wb != 0, eb != 0) and np.array_equal(wc != 0, ec != 0)
            assert np.array_equal(wb[~eq_b], eb[~eq_b]) and np.array_equal(wc[~eq_c], ec[~eq_c])
            assert abs(r["obj"] - e["objective"]) <= 1e-9 * max(1.0, abs(e["objective"]))
        # certificate of the SAME (x, y): the residuals are cancellation noise of terms as large
        # as the data (up to 1e11 in these dumps), so the two summation orders agree to
        # eps * data scale, not to an absolute 1e-9
        ok_o, st_o, _, _ = oracle_certificate(oracle, q, r["x"], r["y"], r["ws_b"], r["ws_c"])
        scale = max(1.0, np.abs(q.g).max(), np.abs(q.H_val).max() * max(1.0, np.abs(r["x"]).max()), ys)
        tol = 1e-13 * scale
        assert abs(k - st_o.KKT_error) <= tol
        if abs(st_o.KKT_error - 1e-6) > tol:
            assert (o == 1) == ok_o


def test_unsolved_qp_headers(capi, oracle):
    """The reference's second set of real inputs (test/unsolved_QPs/*.hpp -> tests/golden/unsolved_qps.json):
    nine non-convex QPs, most with a non-symmetric H as recorded. LDS engine (batch) and HBM engine against
    the oracle: same verdict, and where a KKT point is found the same point and objective. The two
    `_unbounded` files record qpOASES' verdict 23; the QPs are bounded below (boxed variables, positive
    slack cost) and engine and oracle both return a KKT point instead -- recorded, not hidden."""
    qps = problems.unsolved_qps()
    probs = [q for q, _ in qps]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    res = b.results()
    verdicts = {}
    for (q, expected), r in zip(qps, res):
        qp, rc, n = oracle_cold(oracle, q)
        verdicts[q.name] = (r["status"], qp.exitflag(), expected)
        if q.name == "hs047":        # bound flips cycle on this one (999 flips in the oracle): only "not solved"
            assert r["status"] == qp.exitflag() == 28
            continue
        assert r["status"] == qp.exitflag(), verdicts
        if r["status"] == 20:
            xs = max(1.0, np.abs(qp.x).max())
            assert np.abs(qp.x - r["x"]).max() <= 1e-9 * xs, q.name
            assert abs(r["obj"] - qp.objective) <= 1e-9 * max(1.0, abs(qp.objective))
            s = capi.Solver(q.nV, q.nC)
            s.set_engine(2)
            s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
            for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
                s.set_vector(w, v)
            s.solve(capi.MODE_COLD, 1000)
            assert s.status == 20 and np.abs(s.x - qp.x).max() <= 1e-9 * xs, q.name
    assert verdicts["hs035_unbounded"][2] == verdicts["hs067_unbounded"][2] == 23


def test_hot_start_sequence(capi, oracle):
    """hotstart(g,lb,ub,lbA,ubA) and hotstart(H,...,A,...) keep pace with the oracle solve for solve."""
    rng = np.random.default_rng(21)
    probs = [problems.random_qp(rng, int(rng.integers(4, 40)), int(rng.integers(0, 35))) for _ in range(24)]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    orc = []
    for q in probs:
        qp, rc, n = oracle_cold(oracle, q)
        orc.append(qp)
    for step in range(4):
        probs = [problems.perturb(rng, q, 0.05) for q in probs]
        changed = step % 2 == 1
        if changed:
            for q in probs:
                q.A_val = q.A_val * (1.0 + 0.01 * rng.normal(size=q.A_val.shape))
                q.H_val = q.H_val * 1.05
            b.set_matrix_values(np.concatenate([q.A_val for q in probs]), np.concatenate([q.H_val for q in probs]))
        b.set_vectors_from(probs)
        b.solve(capi.MODE_HOT_MATRICES if changed else capi.MODE_HOT_VECTORS, 1000)
        for q, qp, r in zip(probs, orc, b.results()):
            if changed:
                qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
                rc, n = qp.hotstart_matrices(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            else:
                rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            assert_same_solution(qp, r, n)


def test_assembly_from_triplets(capi, oracle):
    """set_A / set_H: setStructure on first call, setMatVal afterwards -- device CSC, order_
    and refreshed values identical (exact) to the oracle's restatement of SpHbMat."""
    rng = np.random.default_rng(31)
    for _ in range(10):
        n, m = int(rng.integers(2, 12)), int(rng.integers(1, 8))
        dens = rng.random((m, n)) < 0.5
        r, c = np.nonzero(dens)
        perm = rng.permutation(len(r))
        irow, jcol = r[perm] + 1, c[perm] + 1
        val = rng.normal(size=len(r))
        ident = [(1, n + 1, m, 1.0), (1, n + m + 1, m, -1.0)]
        s = capi.Solver(n + 2 * m, m)
        s.set_A_triplet(irow, jcol, val, ident)
        jc, ir, v, order = s.get_A_csc()
        jo, io, vo, oo = oracle.sphb_set_structure(m, n + 2 * m, irow, jcol, val, ident)
        assert np.array_equal(jc, jo) and np.array_equal(ir, io) and np.array_equal(v, vo) and np.array_equal(order, oo)
        val2 = rng.normal(size=len(r))
        s.set_A_triplet(irow, jcol, val2, ident)
        v2 = s.get_A_csc()[2]
        assert np.array_equal(v2, oracle.sphb_set_matval(oo, val2, vo.copy(), 2 * m))
        # products use the refreshed values, also through the CSR copy
        x = rng.normal(size=n + 2 * m); y = rng.normal(size=m)
        A = np.zeros((m, n + 2 * m))
        for cc in range(n + 2 * m):
            for k in range(jc[cc], jc[cc + 1]):
                A[ir[k], cc] = v2[k]
        assert np.abs(s.A_times(x) - A @ x).max() < 1e-13 and np.abs(s.A_transposed_times(y) - A.T @ y).max() < 1e-13
        # symmetric H: lower triangle, mirrored, two writes per off-diagonal on refresh
        L = np.tril(rng.normal(size=(n, n))) * (rng.random((n, n)) < 0.6)
        hr, hc = np.nonzero(L)
        if len(hr) == 0:
            continue
        nV = n + 2 * m
        s.set_H_triplet(hr + 1, hc + 1, L[hr, hc], True)
        hj, hi, hv, ho = s.get_H_csc()
        oj, oi, ov, ooo = oracle.sphb_set_structure_sym(nV, nV, hr + 1, hc + 1, L[hr, hc], True)
        assert np.array_equal(hj, oj) and np.array_equal(hi, oi) and np.array_equal(hv, ov) and np.array_equal(ho, ooo)
        nv = rng.normal(size=len(hr))
        s.set_H_triplet(hr + 1, hc + 1, nv, True)
        assert np.array_equal(s.get_H_csc()[2], oracle.sphb_set_matval_sym(hr + 1, hc + 1, True, ooo, nv, ov.copy()))


@pytest.mark.parametrize("arena_mapped", ["0", "1"])
def test_structure_upload_of_small_handles_arena_and_fallback(capi, oracle, arena_mapped, monkeypatch):
    """LDS-scale handles take their pattern arrays from an arena allocated by rsqp_create (one copy per set_A / set_H, or none at
    all when the arena is host-mapped -- the default at hs071 scale). A triplet list with so many DUPLICATE entries that it exceeds
    the arena must fall back to the allocating path with the same result."""
    monkeypatch.setenv("RSQP_ARENA_MAPPED", arena_mapped)          # (read per handle, at rsqp_create)
    rng = np.random.default_rng(91)
    n, m = 4, 2
    for ndup in (1, 30):                                       # 8 entries / 240 entries (the arena holds a dense 2 x 4 + slack)
        r, c = np.nonzero(np.ones((m, n)))
        irow = np.tile(r + 1, ndup); jcol = np.tile(c + 1, ndup)
        val = rng.normal(size=len(irow))
        s = capi.Solver(n, m)
        s.set_A_triplet(irow, jcol, val, [])
        jc, ir, v, order = s.get_A_csc()
        jo, io, vo, oo = oracle.sphb_set_structure(m, n, irow, jcol, val, [])
        assert np.array_equal(jc, jo) and np.array_equal(ir, io) and np.array_equal(v, vo) and np.array_equal(order, oo)
        val2 = rng.normal(size=len(irow))
        s.set_A_triplet(irow, jcol, val2, [])
        assert np.array_equal(s.get_A_csc()[2], oracle.sphb_set_matval(oo, val2, vo.copy(), 0))
        A = np.zeros((m, n))
        np.add.at(A, (irow - 1, jcol - 1), val2)
        x = rng.normal(size=n); y = rng.normal(size=m)
        assert np.abs(s.A_times(x) - A @ x).max() < 1e-12 and np.abs(s.A_transposed_times(y) - A.T @ y).max() < 1e-12
        s.close()


@pytest.mark.parametrize("from_y0", [True, False])
def test_dispatch_state_machine(capi, oracle, from_y0):
    """optimizeQP's FIXED / VARIED dispatch (qpOASESInterface.cpp:137-224, 817-833) driven by
    the QPhandler call sequence of Algorithm::setupQP: cold init, hot start on vectors, status
    flip -> init(..., x_qp, y_qp, &bounds), hot start with matrices; the oracle is driven by a
    restatement of the same decisions. hs071 with c2 relaxed to an inequality (see the next
    test for why the reference's own equality handling cannot be replayed).
    from_y0: the status flip re-initialises without guessed constraints; the engine's default takes their sides
    from sign(y_qp), rsqp_set_reinit_guess(0) follows the reference (constraints from A x_qp only). Each rule
    against the oracle run with the same rule; both must reach the same point and working set."""
    from restartsqp_amd.handler import QPhandler
    from restartsqp_amd.sqptypes import Stats

    def nlp_at(x):
        d = problems.hs071_nlp(x, lam=np.zeros(2))
        d["c_u"] = np.array([np.inf, np.inf])
        return d

    nlp = nlp_at(None)
    h = QPhandler(nlp["info"])
    h.solverInterface_._s.set_reinit_guess(from_y0)
    stats = Stats()
    h.set_A(nlp["J"]); h.set_H(nlp["H"])
    h.set_bounds(1.0, nlp["x_l"], nlp["x_u"], nlp["x"], nlp["c_l"], nlp["c_u"], nlp["c"])
    h.set_g(nlp["grad"], 1.0)
    h.solveQP(stats)
    q = problems.handler_qp(nlp)
    qp, rc, n = oracle_cold(oracle, q)
    qp.set_guess_constraints_from_y0(from_y0)
    assert stats.qp_iter == n and h.get_status() == 20
    assert np.abs(h.get_optimal_solution() - qp.x).max() < 1e-12
    # iteration 2: rejected step, trust region shrinks (update_delta): FIXED -> hotstart(vectors)
    h.update_delta(0.5, nlp["x_l"], nlp["x_u"], nlp["x"])
    h.solveQP(stats)
    q2 = problems.handler_qp(nlp, delta=0.5)
    rc, n2 = qp.hotstart(q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA, 1000)
    assert np.abs(h.get_optimal_solution() - qp.x).max() < 1e-12 and stats.qp_iter == n + n2
    # iteration 3: accepted step -> new J, H, bounds, gradient: FIXED -> VARIED flips the
    # status, the adapter re-initialises from (x, y, bounds) (:201-208)
    nlp1 = nlp_at(nlp["x"] + h.get_optimal_solution()[:4])
    h.update_A(nlp1["J"]); h.update_H(nlp1["H"])
    h.update_bounds(0.5, nlp1["x_l"], nlp1["x_u"], nlp1["x"], nlp1["c_l"], nlp1["c_u"], nlp1["c"])
    h.update_grad(nlp1["grad"])
    before = stats.qp_iter
    h.solveQP(stats)
    q3 = problems.handler_qp(nlp1, delta=0.5)
    qp.set_A_csc(q3.A_jc, q3.A_ir, q3.A_val); qp.set_H_csc(q3.H_jc, q3.H_ir, q3.H_val)
    rc, n3 = qp.init(q3.g, q3.lb, q3.ub, q3.lbA, q3.ubA, 1000, x0=qp.x, y0=qp.y, guess_b=qp.ws_bounds)
    assert rc == 0 and stats.qp_iter - before == n3
    assert np.abs(h.get_optimal_solution() - qp.x).max() < 1e-10
    wb, wc = h.solverInterface_._s.working_set_raw()
    assert np.array_equal(wb, qp.ws_bounds) and np.array_equal(wc, qp.ws_constraints)
    # iteration 4: another accepted step: status UNDEFINED again after the re-init, so
    # old := VARIED, new stays UNDEFINED -> hotstart(H, g, A, ...) (:177-187)
    nlp2 = nlp_at(nlp1["x"] + h.get_optimal_solution()[:4])
    h.update_A(nlp2["J"]); h.update_H(nlp2["H"])
    h.update_bounds(0.5, nlp2["x_l"], nlp2["x_u"], nlp2["x"], nlp2["c_l"], nlp2["c_u"], nlp2["c"])
    h.update_grad(nlp2["grad"])
    before = stats.qp_iter
    h.solveQP(stats)
    q4 = problems.handler_qp(nlp2, delta=0.5)
    qp.set_A_csc(q4.A_jc, q4.A_ir, q4.A_val); qp.set_H_csc(q4.H_jc, q4.H_ir, q4.H_val)
    rc, n4 = qp.hotstart_matrices(q4.g, q4.lb, q4.ub, q4.lbA, q4.ubA, 1000)
    assert rc == 0 and stats.qp_iter - before == n4
    assert np.abs(h.get_optimal_solution() - qp.x).max() < 1e-10


def test_stale_ubA_quirk_reports_infeasible(capi, oracle):
    """QPhandler::update_bounds never refreshes ubA on the qpOASES branch
    (src/QPhandler.cpp:358-360). With the equality c2 of hs071 an accepted step therefore leaves
    lbA > ubA; qpOASES rejects such data as infeasible, handle_error re-inits and throws
    QP_NOT_OPTIMAL (src/qpOASESInterface.cpp:720-756). Engine and oracle do the same."""
    from restartsqp_amd.handler import QPhandler
    from restartsqp_amd.sqptypes import QP_NOT_OPTIMAL, Stats
    nlp = problems.hs071_nlp()
    h = QPhandler(nlp["info"])
    h.set_A(nlp["J"]); h.set_H(nlp["H"])
    h.set_bounds(1.0, nlp["x_l"], nlp["x_u"], nlp["x"], nlp["c_l"], nlp["c_u"], nlp["c"])
    h.set_g(nlp["grad"], 1.0)
    h.solveQP(Stats())
    nlp1 = problems.hs071_nlp(nlp["x"] + h.get_optimal_solution()[:4])
    h.update_A(nlp1["J"]); h.update_H(nlp1["H"])
    h.update_bounds(1.0, nlp1["x_l"], nlp1["x_u"], nlp1["x"], nlp1["c_l"], nlp1["c_u"], nlp1["c"])
    h.update_grad(nlp1["grad"])
    with pytest.raises(QP_NOT_OPTIMAL):
        h.solveQP(Stats())
    assert h.get_status() == 22
    q = problems.handler_qp(nlp1)
    q.ubA = problems.hs071_first_qp().ubA
    assert q.lbA[1] > q.ubA[1]
    qp, rc, n = oracle_cold(oracle, q)
    assert rc == 2 and n == 0 and qp.exitflag() == 22


@pytest.mark.parametrize("engine", [1, 2])
def test_handle_error_iteration_limit_then_cold_reinit(capi, oracle, engine):
    """handle_error, QP branch (reference src/qpOASESInterface.cpp:718-757): a hot start that exhausts qp_maxiter
    leaves the solver unsolved and NOT infeasible -> plain re-init (init from scratch, :737-749) with a fresh
    budget, which succeeds here: cold start of the first QP 31 changes; the second QP (same matrices, unrelated
    vectors) needs 65 changes as a hot start but 43 from scratch; budget 50. optimizeQP reports 50 + 43 to
    Stats::qp_iter and ends solved. (The other rescue -- infeasible -> re-init from the slack point x_0 -- cannot
    SUCCEED on consistent data: every QP along the homotopy between two feasible QPs is feasible, so "infeasible"
    means inconsistent bounds, which x_0 does not cure; its failing case is
    test_stale_ubA_quirk_reports_infeasible.)"""
    rng = np.random.default_rng(7024)
    nV, nC = int(rng.integers(8, 20)), int(rng.integers(6, 20))
    qa = problems.random_qp(rng, nV, nC)
    xh = rng.normal(size=nV) * 3
    A = qa.dense_A()
    lb = xh - np.abs(rng.normal(size=nV)); ub = xh + np.abs(rng.normal(size=nV))
    lbA = A @ xh - np.abs(rng.normal(size=nC)); ubA = A @ xh + np.abs(rng.normal(size=nC))
    g = 10 * rng.normal(size=nV)
    qb = QPData(nV, nC, qa.H_jc, qa.H_ir, qa.H_val, qa.A_jc, qa.A_ir, qa.A_val, g, lb, ub, lbA, ubA)
    qp, rc, na = oracle_cold(oracle, qa)
    rc, nh = qp.hotstart(qb.g, qb.lb, qb.ub, qb.lbA, qb.ubA, 1000)
    qc, rc2, ncold = oracle_cold(oracle, qb)
    assert (nV, nC, na, nh, ncold) == (18, 14, 31, 65, 43)          # the instance this test was built on
    s = capi.Solver(nV, nC)
    s.set_engine(engine)
    s.set_options(qp_maxiter=50)
    s.set_A_csc(qa.A_jc, qa.A_ir, qa.A_val); s.set_H_csc(qa.H_jc, qa.H_ir, qa.H_val)
    for w, v in zip(range(5), (qa.g, qa.lb, qa.ub, qa.lbA, qa.ubA)):
        s.set_vector(w, v)
    assert s.optimize_qp() == na and s.status == 20
    for w, v in zip(range(5), (qb.g, qb.lb, qb.ub, qb.lbA, qb.ubA)):
        s.set_vector(w, v)
    assert s.optimize_qp() == 50 + ncold        # the exhausted hot start + the re-init
    assert s.status == 20 and s.is_solved()
    wb, wc = s.working_set_raw()
    assert np.array_equal(wb, qc.ws_bounds) and np.array_equal(wc, qc.ws_constraints)
    assert np.abs(s.x - qc.x).max() <= 1e-9 * max(1.0, np.abs(qc.x).max())
    # budget too small for the re-init as well: still unsolved, status "performing homotopy" (28), the adapter throws
    s.set_options(qp_maxiter=20)
    for w, v in zip(range(5), (qa.g, qa.lb, qa.ub, qa.lbA, qa.ubA)):
        s.set_vector(w, v)
    assert s.optimize_qp() == 40 and not s.is_solved() and s.status == 28


def test_hot_start_after_the_hessian_lost_its_symmetry(capi, oracle):
    """an 8 x 2 handle solves on the register-resident tableau kernel while H is symmetric; a value refresh that makes H
    non-symmetric sends the next solve to the LDS-resident kernel, whose state layout differs -- the hot start must not restore
    the other kernel's bytes (it starts cold), and with symmetric values again the tableau kernel must not either."""
    rng = np.random.default_rng(99)
    q = problems.hs071_first_qp()
    H = q.dense_H() + np.eye(q.nV)                # (convex, so that the non-symmetric solve is well defined too)
    irow, jcol = np.nonzero(np.ones_like(H))
    vals = H[irow, jcol]
    s = capi.Solver(q.nV, q.nC)
    s.set_A_csc(q.A_jc, q.A_ir, q.A_val)
    s.set_H_triplet(irow + 1, jcol + 1, vals, is_symmetric=0)          # a general triplet matrix whose values happen to be symmetric
    for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
        s.set_vector(w, v)
    s.solve(capi.MODE_COLD, 1000)
    assert s.status == 20
    for trial, bump in enumerate((0.05, 0.0, 0.05)):                   # non-symmetric, symmetric again, non-symmetric
        H2 = H.copy(); H2[0, 1] += bump
        s.set_H_triplet(irow + 1, jcol + 1, H2[irow, jcol], is_symmetric=0)
        q2 = problems.perturb(rng, q, 0.02)
        for w, v in zip(range(5), (q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA)):
            s.set_vector(w, v)
        s.solve(capi.MODE_HOT_MATRICES, 1000)
        from restartsqp_amd.qpdump import QPData, dense_to_csc
        qq = QPData(q.nV, q.nC, *dense_to_csc(H2), q.A_jc, q.A_ir, q.A_val, q2.g, q2.lb, q2.ub, q2.lbA, q2.ubA)
        qp, rc, n_or = oracle_cold(oracle, qq)
        assert s.status == qp.exitflag() == 20, trial
        ok, st, _, _ = s.test_optimality()
        assert ok and np.abs(s.x - qp.x).max() <= 1e-9 * max(1.0, np.abs(qp.x).max()), trial


@pytest.mark.parametrize("engine", [1, 2])
def test_first_solve_and_its_rescue_both_fail(capi, oracle, engine):
    """optimizeQP when the FIRST init runs out of iterations and handle_error's re-init does too: the reference throws
    QP_NOT_OPTIMAL inside handle_error (src/qpOASESInterface.cpp:161-163, 754-756), so the rest of optimizeQP never runs -- one
    rescue, not two, and Stats::qp_iter receives the rescue's count only (:751-752; :211-212 are skipped). Then the same handle,
    larger budget: firstQPsolved_ is still false -> a cold init that succeeds."""
    rng = np.random.default_rng(7024)
    nV, nC = int(rng.integers(8, 20)), int(rng.integers(6, 20))
    qa = problems.random_qp(rng, nV, nC)
    qp, rc, na = oracle_cold(oracle, qa)
    assert na == 31
    s = capi.Solver(nV, nC)
    s.set_engine(engine)
    s.set_options(qp_maxiter=20)
    s.set_A_csc(qa.A_jc, qa.A_ir, qa.A_val); s.set_H_csc(qa.H_jc, qa.H_ir, qa.H_val)
    for w, v in zip(range(5), (qa.g, qa.lb, qa.ub, qa.lbA, qa.ubA)):
        s.set_vector(w, v)
    assert s.optimize_qp() == 20 and not s.is_solved() and s.status == 28
    s.set_options(qp_maxiter=100)
    assert s.optimize_qp() == na and s.is_solved() and s.status == 20
    assert s.last_mode() == capi.MODE_COLD
    wb, wc = s.working_set_raw()
    assert np.array_equal(wb, qp.ws_bounds) and np.array_equal(wc, qp.ws_constraints)


def test_spmv_batched_parity_and_properties(capi, oracle):
    """Stream SpMV: small case against the oracle's entry-order loops; BASELINE-size case
    (n=10k, m=20k, 200k non-zeros) through size-independent properties: linearity,
    <y, A x> == <A'y, x>, and agreement of the CSR-copy product with the CSC one."""
    jc, ir, rng = problems.sparse_pattern(300, 500, 4000, seed=7)
    nb = 3
    vals = rng.normal(size=(nb, 4000)); x = rng.normal(size=(nb, 300)); y = rng.normal(size=(nb, 500))
    p = capi.SpmvPlan(500, 300, jc, ir, nb)
    p.upload(vals, x, transposed=False); p.upload(None, y, transposed=True)
    p.run(False); p.run(True)
    Ax, ATy = p.download(False), p.download(True)
    for k in range(nb):
        ax = oracle.sphb_times(500, 300, jc, ir, vals[k], x[k])
        aty = oracle.sphb_transposed_times(500, 300, jc, ir, vals[k], y[k])
        assert np.abs(Ax[k] - ax).max() <= 4 * 30 * 2.3e-16 * np.abs(ax).max() + 1e-300
        assert np.array_equal(ATy[k], aty)   # same entry order as the reference loop: bit-exact
    # LDS-resident-vector kernel (chosen for batches >= 64): fixed-shape tree reduction, so the
    # bound is the summation-order tolerance, not bit equality
    jc, ir, rng = problems.sparse_pattern(700, 900, 9000, seed=9)
    nb = 64
    vals = rng.normal(size=(nb, 9000)); x = rng.normal(size=(nb, 700)); y = rng.normal(size=(nb, 900))
    p = capi.SpmvPlan(900, 700, jc, ir, nb)
    p.upload(vals, x, transposed=False); p.upload(None, y, transposed=True)
    p.run(False); p.run(True)
    Ax, ATy = p.download(False), p.download(True)
    for k in range(0, nb, 7):
        ax = oracle.sphb_times(900, 700, jc, ir, vals[k], x[k])
        aty = oracle.sphb_transposed_times(900, 700, jc, ir, vals[k], y[k])
        assert np.abs(Ax[k] - ax).max() <= 4 * 40 * 2.3e-16 * max(1.0, np.abs(ax).max())
        assert np.abs(ATy[k] - aty).max() <= 4 * 40 * 2.3e-16 * max(1.0, np.abs(aty).max())
    # full size
    n, m, nnz = 10000, 20000, 200000
    jc, ir, rng = problems.sparse_pattern(n, m, nnz)
    vals = rng.normal(size=(2, nnz)); x = rng.normal(size=(2, n)); y = rng.normal(size=(2, m))
    p = capi.SpmvPlan(m, n, jc, ir, 2)
    p.upload(vals, x, False); p.upload(None, y, True)
    p.run(False); p.run(True)
    Ax, ATy = p.download(False), p.download(True)
    for k in range(2):
        lhs, rhs = float(y[k] @ Ax[k]), float(ATy[k] @ x[k])
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))
    p.upload(None, 2.0 * x, False); p.run(False)
    assert np.array_equal(p.download(False), 2.0 * Ax)   # exact: scaling by 2 commutes with rounding


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["plain_10k_x_20k", "handler_J_I_mI", "plain_int_index", "plain_subwave_kernels"])
def test_roofline_spmv_kernels_match_the_oracle(capi, oracle, shape, monkeypatch):
    """The kernels behind `roofline_spmv` in bench.py (profiles/*kernel_stats*: csx_ldsvec_segscan for A'y and Ax;
    the sub-wave kernels csx_ldsvec_spmv_pipe2<4,3,.> / <2,4,.> for short majors and 32-bit indices) at the benchmarked
    shape -- n=10k columns, m=20k rows, 200 000 entries, nbatch >= 64 -- against the oracle's restatement of
    SpHbMat::times / transposed_times (reference src/SpHbMat.cpp:659-737). The chosen kernel variant is
    asserted so that a change of the selection rule cannot silently move the test to another kernel.
    Tolerance: the kernel sums a major in a fixed tree instead of entry order -> 4 * nnz_major * eps * |sum|abs."""
    eps = 2.3e-16
    if shape == "handler_J_I_mI":
        # QPhandler shape A = [J I -I] (reference src/QPhandler.cpp:39-40, SpHbMat.cpp:196-268):
        # 20 000 x 50 000, 240 000 entries, 3 640 004 algorithmic bytes per product
        n, m, nnzJ = 10000, 20000, 200000
        jcJ, irJ, rng = problems.sparse_pattern(n, m, nnzJ)
        ncol = n + 2 * m
        jc = np.concatenate([jcJ, nnzJ + np.arange(1, 2 * m + 1)]).astype(np.int32)
        ir = np.concatenate([irJ, np.arange(m), np.arange(m)]).astype(np.int32)
        ident = np.concatenate([np.ones(m), -np.ones(m)])
        nnz = nnzJ + 2 * m
        expect_t, expect_n = 38, 0          # 4.8 entries per column -> <2,4>; a 50 000-vector (400 KB) exceeds the LDS -> stream kernel
    else:
        n, m, nnz = 10000, 20000, 200000
        jc, ir, rng = problems.sparse_pattern(n, m, nnz)
        ncol, ident = n, None
        expect_t, expect_n = 40, 40         # 20 entries per column, 10 per row -> entry-parallel csx_ldsvec_segscan
    if shape == "plain_subwave_kernels":
        monkeypatch.setenv("RSQP_SPMV_VARIANT", "35")   # csx_ldsvec_spmv_pipe2<4,3,unsigned short> for both products
        expect_t, expect_n = 35, 35
    if shape == "plain_int_index":
        monkeypatch.setenv("RSQP_SPMV_IDX16", "0")     # the <.., int> instantiation (dimensions >= 65 536 take it by themselves)
        expect_t, expect_n = 35, 38                     # the entry-parallel kernel exists for 16-bit indices only
    nb = 64
    vals = rng.normal(size=(nb, nnz))
    if ident is not None:
        vals[:, nnz - 2 * m:] = ident
    x = rng.normal(size=(nb, ncol)); y = rng.normal(size=(nb, m))
    p = capi.SpmvPlan(m, ncol, jc, ir, nb)
    vt, i16t = p.variant(True); vn, i16n = p.variant(False)
    assert (vt, vn) == (expect_t, expect_n), (vt, vn)
    assert i16t == (shape != "plain_int_index") and i16n == i16t
    p.upload(vals, x, transposed=False); p.upload(None, y, transposed=True)
    p.run(False); p.run(True)
    Ax, ATy = p.download(False), p.download(True)
    per_col = int(np.diff(jc).max()); per_row = int(np.bincount(ir, minlength=m).max())
    for k in (0, 1, 9, 17, 31, 40, 55, 63):
        ax = oracle.sphb_times(m, ncol, jc, ir, vals[k], x[k])
        aty = oracle.sphb_transposed_times(m, ncol, jc, ir, vals[k], y[k])
        ax_abs = oracle.sphb_times(m, ncol, jc, ir, np.abs(vals[k]), np.abs(x[k]))
        aty_abs = oracle.sphb_transposed_times(m, ncol, jc, ir, np.abs(vals[k]), np.abs(y[k]))
        assert np.all(np.abs(Ax[k] - ax) <= 4 * per_row * eps * ax_abs + 1e-300)
        assert np.all(np.abs(ATy[k] - aty) <= 4 * per_col * eps * aty_abs + 1e-300)
    p.close()


def test_full_size_hs071_batch_properties(capi, oracle):
    """BASELINE config 5 size (512 hs0xx-scale QPs) and a larger hs071-shape batch: every
    answer carries the reference's KKT certificate; a sample is compared with the oracle;
    solving the batch twice gives bit-identical results (deterministic reductions)."""
    probs = problems.hs_batch(512)
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    res = b.results(); ok, kkt = b.test_optimality()
    assert all(r["status"] == 20 for r in res) and all(o == 1 for o in ok)
    for k in range(0, 512, 16):
        qp, rc, n = oracle_cold(oracle, probs[k])
        assert_same_solution(qp, res[k], n, check_nwsr=probs[k].name != "hs071_first_qp")
    b.solve(capi.MODE_COLD, 1000)
    res2 = b.results()
    assert all(np.array_equal(a["x"], c["x"]) and np.array_equal(a["y"], c["y"]) and a["nWSR"] == c["nWSR"]
               for a, c in zip(res, res2))


def test_optimize_lp(capi, oracle):
    """optimizeLP (qpOASESInterface.cpp:227-284): H = 0, solved like qpOASES does an all-zero
    Hessian (regVal*I + one regularisation step). Against the oracle driven the same way, and
    against an independent LP solver (scipy / HiGHS) for the optimal value."""
    from scipy.optimize import linprog
    rng = np.random.default_rng(61)
    for engine in (1, 2):
        for _ in range(8):
            nV, nC = int(rng.integers(2, 14)), int(rng.integers(1, 14))
            A = rng.normal(size=(nC, nV)); g = rng.normal(size=nV); xh = rng.normal(size=nV)
            lb = xh - np.abs(rng.normal(size=nV)) - 0.1; ub = xh + np.abs(rng.normal(size=nV)) + 0.1
            lbA = A @ xh - np.abs(rng.normal(size=nC)) - 0.1; ubA = A @ xh + np.abs(rng.normal(size=nC)) + 0.1
            Ac = dense_to_csc(A)
            s = capi.Solver(nV, nC)
            s.set_engine(engine)
            s.set_A_csc(*Ac)
            for w, v in zip(range(5), (g, lb, ub, lbA, ubA)):
                s.set_vector(w, v)
            n = s.optimize_lp()
            qp = oracle.OracleQP(nV, nC); qp.set_A_csc(*Ac); qp.set_H_csc(None, None, None)
            reg = np.linalg.norm(g) * 1e3 * 2.221e-16
            qp.set_regularisation(reg)
            rc, n1 = qp.init(g, lb, ub, lbA, ubA, 100)
            rc2, n2 = qp.hotstart(g - reg * qp.x, lb, ub, lbA, ubA, 100)
            assert rc == 0 and rc2 == 0 and s.is_solved() and n == n1 + n2
            wb, wc = s.working_set_raw()
            assert np.array_equal(wb, qp.ws_bounds) and np.array_equal(wc, qp.ws_constraints)
            assert np.abs(s.x - qp.x).max() <= 1e-8 * max(1.0, np.abs(qp.x).max())
            r = linprog(g, A_ub=np.vstack([A, -A]), b_ub=np.concatenate([ubA, -lbA]), bounds=list(zip(lb, ub)))
            assert abs(s.objective - r.fun) <= 1e-8 * max(1.0, abs(r.fun))


def test_degenerate_inputs_both_engines(capi, oracle):
    """Same degenerate inputs as tests/test_oracle_qp.py::test_degenerate_inputs: the kernels make
    the same tie-breaking decisions as the oracle (lowest candidate id)."""
    rng = np.random.default_rng(0)
    probs = [problems.degenerate_qp(rng, t % 5) for t in range(100)]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 500)
    res = b.results()
    for q, r in zip(probs, res):
        qp, rc, n = oracle_cold(oracle, q, 500)
        assert_same_solution(qp, r, n)
    for q in probs[:25]:
        s = capi.Solver(q.nV, q.nC)
        s.set_engine(2)
        s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
            s.set_vector(w, v)
        n = s.solve(capi.MODE_COLD, 500)
        qp, rc, n_or = oracle_cold(oracle, q, 500)
        wb, wc = s.working_set_raw()
        assert s.status == qp.exitflag() and n == n_or
        assert np.array_equal(wb, qp.ws_bounds) and np.array_equal(wc, qp.ws_constraints)
        assert np.abs(s.x - qp.x).max() <= 1e-9 * max(1.0, np.abs(qp.x).max())


@pytest.mark.parametrize("keep_state", [True, False])
def test_degenerate_sweep_mismatch_rate_is_bounded(capi, oracle, keep_state):
    """The bit-exact claim is for NON-degenerate QPs (unique optimal working set). On degenerate inputs -- duplicate / zero
    rows, constraints parallel to bounds, integer data, singular H: exact ties in the ratio tests -- a tie is broken by the
    last bits of differently ordered sums, and a few answers end in another (equally optimal) working set than the
    oracle's. This sweep (the former tools/random_parity_sweep.py --degenerate) pins the observed rate: at most 1 % of
    1 500 seeded degenerate inputs may differ, and every one of them must still be a certified KKT point whenever the
    oracle's answer is. keep_state False = the KKT-tableau kernel + null-space fallback, True = null-space only."""
    rng = np.random.default_rng(20260105)
    probs = [problems.degenerate_qp(rng, k % 5) for k in range(1500)]
    b = capi.Batch(probs)
    b.set_keep_state(keep_state)
    b.solve(capi.MODE_COLD, 2000)
    res = b.results()
    ok, kkt = b.test_optimality()
    differ = 0
    for q, r, o in zip(probs, res, ok):
        qp, rc, n = oracle_cold(oracle, q, 2000)
        same = (r["status"] == qp.exitflag() and r["nWSR"] == n and np.array_equal(r["ws_b"], qp.ws_bounds)
                and np.array_equal(r["ws_c"], qp.ws_constraints))
        if same and qp.is_solved():
            sc = max(1.0, float(np.abs(qp.x).max()), float(np.abs(qp.y).max()))
            same = np.abs(r["x"] - qp.x).max() <= 1e-9 * sc and np.abs(r["y"] - qp.y).max() <= 1e-9 * sc
        if not same:
            differ += 1
            if qp.is_solved() and r["status"] == 20:      # another vertex of a degenerate face: same objective, certified
                assert o == 1 and abs(r["obj"] - qp.objective) <= 1e-7 * max(1.0, abs(qp.objective)), (q.name, r["obj"], qp.objective)
    assert differ <= 15, differ
    b.close()


def test_single_qp_handles_on_degenerate_hs071_scale_inputs(capi, oracle):
    """the hs071-scale tableau kernel serves every single-QP handle of <= 8 x 8 and has no hand-over of its own; where it
    gives up on a rounding-band pivot (numerical failure), rsqp_solve lets the LDS-resident Givens / TQ kernel take the call over.
    400 seeded degenerate QPs of <= 8 variables / <= 8 constraints, one handle each: the status is the oracle's, every solved one
    is a certified KKT point with the oracle's objective, and at most 2 % end in another working set (exact ties)."""
    rng = np.random.default_rng(20260106)
    probs = []
    while len(probs) < 400:
        q = problems.degenerate_qp(rng, len(probs) % 5)
        if q.nV <= 8 and q.nC <= 8:
            probs.append(q)
    differ = 0
    for q in probs:
        s = capi.Solver(q.nV, q.nC)
        s.set_A_csc(q.A_jc, q.A_ir, q.A_val); s.set_H_csc(q.H_jc, q.H_ir, q.H_val)
        for w, v in zip(range(5), (q.g, q.lb, q.ub, q.lbA, q.ubA)):
            s.set_vector(w, v)
        n = s.solve(capi.MODE_COLD, 2000)
        qp, rc, n_or = oracle_cold(oracle, q, 2000)
        assert s.status == qp.exitflag(), (q.name, q.nV, q.nC, s.status, qp.exitflag())
        if s.status == 20:
            ok, st, _, _ = s.test_optimality()
            assert ok and abs(s.objective - qp.objective) <= 1e-7 * max(1.0, abs(qp.objective)), (q.name, s.objective, qp.objective)
            wb, wc = s.working_set_raw()
            differ += not (np.array_equal(wb, qp.ws_bounds) and np.array_equal(wc, qp.ws_constraints))
        s.close()
    assert differ <= 8, differ


@pytest.mark.gpu
def test_packed_waves_match_one_problem_per_wave():
    """64/L problems share a wave in the LDS engine (L = 16 / 32 lanes per problem). Every packing
    must return bit-identical x, y, working sets, nWSR and objective, cold and hot start, on
    heterogeneous batches (problems of one wave diverge). tools/small_pack_check.py runs each setting in a
    process of its own (the switches are read per handle, at rsqp_batch_create) and fails a setting whose
    launches did not run the build it asked for, or ran the reference setting's build."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "small_pack_check.py"), "--quick"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ALL IDENTICAL" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["0", "1"])
def test_both_formulations_pass_the_parity_suite(engine):
    """The LDS engine exists in two formulations -- Givens / TQ (qp_small.hip Engine, default for
    nV <= 8) and explicit inverses (qp_small_x.h EngineX, default above) -- chosen per batch from
    nVmax. Force each of them on every batch of this file (RSQP_SMALL_ENGINE is read per handle, when it is
    created; the subprocess gives every test of the file the setting): both must match the oracle's working
    sets, nWSR, x and y."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RSQP_SMALL_ENGINE=engine)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"), "-q", "-x",
                        "-k", "not packed and not both_formulations and not reference_dumps"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_blocking_waits_give_the_same_answers():
    """Single-QP solves, the certificate and the HBM-resident engine wait for their results by spinning on a host-mapped
    sequence word the kernels raise (INTEGRATION.md "Host waits"); RSQP_NO_SPIN / RSQP_LARGE_NO_SPIN select the blocking
    hipStreamSynchronize fallback instead. The single-QP tests of this file and the mid-size tests of the HBM engine must
    pass on that path as well (the switches are read once per process, hence the subprocess)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RSQP_NO_SPIN="1", RSQP_LARGE_NO_SPIN="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_parity.py"),
                        os.path.join(root, "tests", "test_gpu_large_engine.py"), "-q", "-x", "-k",
                        "hs071_single_qp or dispatch_state_machine or optimize_lp or random_convex_against_oracle or hot_start_modes"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


@pytest.mark.gpu
def test_fuzz_mixed_shapes_against_oracle():
    """Randomised shapes (nV = 1, nC = 0, nC > nV included) in four size classes, so that every packing
    of the LDS engines (8 / 16 / 32 lanes per problem, one and four waves) and both formulations see
    cold and hot starts: working sets, status, nWSR bit-exact, x / y to 1e-9 (tests/checks/fuzz_small_vs_oracle.py)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "checks", "fuzz_small_vs_oracle.py"), "7", "120"],
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0 and "FUZZ OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_device_side_result_records_match_host_packing(capi):
    """rsqp_batch_pack_records_dev (what a rank hands to the RCCL all-gather of a sharded batch) writes the
    same fixed-stride records as parallel.pack_records builds on the host from rsqp_batch_get_results: Exitflag, nWSR,
    objective, KKT error, x, y (bounds | constraints), working sets -- on a mixed-shape batch incl. an infeasible member."""
    from restartsqp_amd import parallel
    probs = problems.hs_batch(40)
    bad = problems.random_qp(np.random.default_rng(2), 5, 3)
    bad.lbA[:] = 5.0; bad.ubA[:] = 4.0              # inconsistent: status 22
    probs.append(bad)
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    ok, kkt = b.test_optimality()
    res = b.results()
    nVmax, nCmax = max(p.nV for p in probs), max(p.nC for p in probs)
    stride = b.record_stride
    assert stride == parallel.RECORD_HEAD + 3 * nVmax + 2 * nCmax
    got = b.pack_records()          # the device kernel of rsqp_batch_pack_records_dev, then a copy to the host
    want = parallel.pack_records(res, kkt, nVmax, nCmax)
    assert want.shape == got.shape and np.array_equal(got, want)
    assert got[-1, 0] == 22 and got[0, 0] == 20
    back = parallel.unpack_record(got[3], probs[3].nV, probs[3].nC, nVmax, nCmax)
    assert np.array_equal(back["x"], res[3]["x"]) and np.array_equal(back["ws_c"], res[3]["ws_c"])


def test_entry_parallel_spmv_edge_patterns(capi, oracle, monkeypatch):
    """csx_ldsvec_segscan (SpMV variant 40) on the patterns that stress its segmented scan: empty majors, majors of a
    single entry (eight starts in one lane), majors as long as a whole chunk (512 entries) and just below, starts on
    every position of a lane, a last chunk of one entry -- against the oracle's SpHbMat::times / transposed_times
    (reference src/SpHbMat.cpp:659-737). A major longer than a chunk makes the plan fall back to the sub-wave kernels."""
    monkeypatch.setenv("RSQP_SPMV_VARIANT", "40")
    rng = np.random.default_rng(77)
    eps = 2.3e-16

    def check(nrow, ncol, col_lengths, nb=64, expect40=True):
        jc = np.concatenate([[0], np.cumsum(col_lengths)]).astype(np.int32)
        ir = np.concatenate([np.sort(rng.choice(nrow, size=int(k), replace=False)) for k in col_lengths] + [np.zeros(0, int)]).astype(np.int32)
        nnz = int(jc[-1])
        vals = rng.normal(size=(nb, nnz)); x = rng.normal(size=(nb, ncol)); y = rng.normal(size=(nb, nrow))
        p = capi.SpmvPlan(nrow, ncol, jc, ir, nb)
        vt, _ = p.variant(True)
        assert (vt == 40) == expect40, (vt, expect40)
        p.upload(vals, x, transposed=False); p.upload(None, y, transposed=True)
        p.run(False); p.run(True)
        Ax, ATy = p.download(False), p.download(True)
        per_col = max(int(max(col_lengths)), 1); per_row = max(int(np.bincount(ir, minlength=nrow).max()), 1)
        for k in (0, 13, nb - 1):
            ax = oracle.sphb_times(nrow, ncol, jc, ir, vals[k], x[k])
            aty = oracle.sphb_transposed_times(nrow, ncol, jc, ir, vals[k], y[k])
            ax_abs = oracle.sphb_times(nrow, ncol, jc, ir, np.abs(vals[k]), np.abs(x[k]))
            aty_abs = oracle.sphb_transposed_times(nrow, ncol, jc, ir, np.abs(vals[k]), np.abs(y[k]))
            assert np.all(np.abs(ATy[k] - aty) <= 4 * per_col * eps * aty_abs + 1e-300), ("A'y", k)
            assert np.all(np.abs(Ax[k] - ax) <= 4 * per_row * eps * ax_abs + 1e-300), ("Ax", k)
        p.close()

    check(900, 700, rng.integers(0, 40, size=700))                       # mixed lengths incl. empty columns
    check(800, 800, np.ones(800, int))                                   # every major a single entry
    check(2000, 40, np.array([512, 511, 1, 0, 513 - 1, 7, 8, 9] * 5))    # whole-chunk majors, neighbours of every size
    check(600, 1025, np.concatenate([np.full(1024, 4), [1]]))            # 4 096 entries = 8 full chunks, then a chunk of one entry
    lens = np.zeros(300, int); lens[::3] = 23                            # two empty columns between the filled ones
    check(500, 300, lens)
    check(3000, 10, np.array([600] + [5] * 9), expect40=False)           # a major longer than a chunk: not this kernel
