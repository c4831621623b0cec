"""Batches whose members' images exceed the LDS of a CU (nV above about 90): every member runs on the HBM-resident
null-space kernel (qp_small_hbm.hip, rsqp_batch_get_last_kernel() == 3) and matches the CPU oracle by the rule of
test_gpu_parity.py: status, working sets and nWSR equal, x and y within RTOL."""
import os

import numpy as np
import pytest

from conftest import oracle_cold
from restartsqp_amd import batch_problems, problems

pytestmark = pytest.mark.gpu

RTOL = 1e-9
HBM_KERNEL = 3


def assert_same_solution(qp, r, n_oracle, check_nwsr=True):
    # (the rule of test_gpu_parity.assert_same_solution)
    assert r["status"] == qp.exitflag()
    assert np.array_equal(qp.ws_bounds, r["ws_b"]) and np.array_equal(qp.ws_constraints, r["ws_c"])
    if check_nwsr:
        assert r["nWSR"] == n_oracle
    xs, ys = max(1.0, np.abs(qp.x).max()), max(1.0, np.abs(qp.y).max())
    assert np.abs(qp.x - r["x"]).max() <= RTOL * xs
    assert np.abs(qp.y - r["y"]).max() <= RTOL * ys


def large_random_batch(seed, nq, vmin=96, vmax=200, cmax=120):
    rng = np.random.default_rng(seed)
    return [problems.random_qp(rng, int(rng.integers(vmin, vmax + 1)), int(rng.integers(0, cmax + 1)), name="big%d" % k)
            for k in range(nq)]


def test_cold_start_beyond_the_lds_image(capi, oracle):
    """24 random convex QPs of 96-200 variables and 0-120 constraints: refused (ERR_TOO_LARGE) before this kernel."""
    probs = large_random_batch(101, 24)
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == HBM_KERNEL
    ok, kkt = b.test_optimality()
    for q, r, o, k in zip(probs, b.results(), ok, kkt):
        qp, rc, n = oracle_cold(oracle, q)
        assert rc == 0, q.name
        assert_same_solution(qp, r, n)
        assert o == 1 and k < 1e-9, (q.name, o, k)
        assert abs(r["obj"] - qp.objective) <= 1e-9 * max(1.0, abs(qp.objective))
    b.close()


def test_handler_shaped_members(capi, oracle):
    """A = [J I -I], H = blkdiag(H_k, 0) as QPhandler builds them (n = 40-80, m = 20-40), H_k definite or indefinite."""
    rng = np.random.default_rng(202)
    probs = [batch_problems.handler_shaped_qp(rng, 80, 40, definite=True)]
    for k in range(15):
        n, m = int(rng.integers(40, 81)), int(rng.integers(20, 41))
        probs.append(batch_problems.handler_shaped_qp(rng, n, m, definite=k % 2 == 1))
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == HBM_KERNEL
    for q, r in zip(probs, b.results()):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
    b.close()


def test_hot_start_sequence_beyond_the_lds_image(capi, oracle):
    """Two hot starts on new vectors and two on new matrices keep pace with the oracle's hotstart / hotstart_matrices."""
    rng = np.random.default_rng(303)
    probs = [problems.random_qp(rng, int(rng.integers(96, 141)), int(rng.integers(0, 80))) for _ in range(12)]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    orc = []
    for q, r in zip(probs, b.results()):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
        orc.append(qp)
    for step in range(4):
        probs = [problems.perturb(rng, q, 0.05) for q in probs]
        changed = step >= 2
        if changed:
            for q in probs:
                q.A_val = q.A_val * (1.0 + 0.01 * rng.normal(size=q.A_val.shape))
                q.H_val = q.H_val * 1.05
            b.set_matrix_values(np.concatenate([q.A_val for q in probs]), np.concatenate([q.H_val for q in probs]))
        b.set_vectors_from(probs)
        b.solve(capi.MODE_HOT_MATRICES if changed else capi.MODE_HOT_VECTORS, 1000)
        assert b.last_kernel() == HBM_KERNEL
        for q, qp, r in zip(probs, orc, b.results()):
            if changed:
                qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)
                rc, n = qp.hotstart_matrices(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            else:
                rc, n = qp.hotstart(q.g, q.lb, q.ub, q.lbA, q.ubA, 1000)
            assert_same_solution(qp, r, n)
    b.close()


def test_mixed_batch_small_and_large_members(capi, oracle):
    """hs0xx-scale members and large ones in one batch: all of them run on the HBM-resident kernel."""
    probs = problems.hs_batch(24) + large_random_batch(404, 4, vmin=100, vmax=160, cmax=60)
    rng = np.random.default_rng(404)
    order = rng.permutation(len(probs))
    probs = [probs[i] for i in order]
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == HBM_KERNEL
    for q, r in zip(probs, b.results()):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, r, n)
    b.close()


def test_iteration_limit_beyond_the_lds_image(capi, oracle):
    probs = large_random_batch(505, 8, vmax=150, cmax=80)
    b = capi.Batch(probs)
    for lim in (3, 10):
        b.solve(capi.MODE_COLD, lim)
        for q, r in zip(probs, b.results()):
            qp, rc, n = oracle_cold(oracle, q, lim)
            assert r["status"] == qp.exitflag() and r["nWSR"] == n, (q.name, lim, r["status"], qp.exitflag(), r["nWSR"], n)
            assert_same_solution(qp, r, n)
    b.close()


def test_keep_state_off_makes_the_hot_start_cold(capi, oracle):
    rng = np.random.default_rng(606)
    probs = [problems.random_qp(rng, int(rng.integers(96, 131)), int(rng.integers(10, 60))) for _ in range(8)]
    b = capi.Batch(probs)
    b.set_keep_state(False)
    b.solve(capi.MODE_COLD, 1000)
    probs = [problems.perturb(rng, q, 0.05) for q in probs]
    b.set_vectors_from(probs)
    b.solve(capi.MODE_HOT_VECTORS, 1000)
    hot = b.results()
    b.solve(capi.MODE_COLD, 1000)
    cold = b.results()
    for q, h, c in zip(probs, hot, cold):
        qp, rc, n = oracle_cold(oracle, q)
        assert_same_solution(qp, h, n)
        for key in ("status", "nWSR"):
            assert h[key] == c[key]
        for key in ("x", "y", "ws_b", "ws_c"):
            assert np.array_equal(h[key], c[key]), key
    b.close()


def test_device_records_match_host_packing_beyond_the_lds_image(capi):
    from restartsqp_amd import parallel
    probs = problems.hs_batch(6) + large_random_batch(707, 3, vmax=130, cmax=50)
    bad = problems.random_qp(np.random.default_rng(7), 100, 3)
    bad.lbA[:] = 5.0; bad.ubA[:] = 4.0              # inconsistent: status 22
    probs.append(bad)
    b = capi.Batch(probs)
    b.solve(capi.MODE_COLD, 1000)
    assert b.last_kernel() == HBM_KERNEL
    ok, kkt = b.test_optimality()
    res = b.results()
    nVmax, nCmax = max(p.nV for p in probs), max(p.nC for p in probs)
    got = b.pack_records()
    want = parallel.pack_records(res, kkt, nVmax, nCmax)
    assert want.shape == got.shape and np.array_equal(got, want)
    assert got[-1, 0] == 22 and got[0, 0] == 20
    b.close()


@pytest.mark.parametrize("engine", ["0", "1"])
def test_both_formulations_beyond_the_lds_image(engine):
    """RSQP_SMALL_ENGINE=0 runs the Givens / TQ engine (one wave per problem), =1 the explicit-inverse engine (four waves);
    the switch is read when a batch is created, hence a fresh process per setting."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RSQP_SMALL_ENGINE=engine)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_batch_beyond_lds.py"), "-q", "-x",
                        "-k", "test_cold_start_beyond_the_lds_image"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_members_beyond_the_batch_limit_are_refused(capi):
    rng = np.random.default_rng(808)
    for nV, nC in ((513, 10), (120, 513)):
        probs = [problems.random_qp(rng, 100, 20), problems.random_qp(rng, nV, nC, density=0.02)]
        with pytest.raises(capi.RsqpError) as e:
            capi.Batch(probs)
        assert e.value.code == capi.ERR_TOO_LARGE and "512" in str(e.value)
