"""The QPhandler of every member of a batch on the device (rsqp_batch_handler_set_problem / _update / _get_step, rsqp_batch_get_vectors;
restartsqp_amd/csrc/rsqp_batch_handler.hip). Expected vectors come from handler.batch_handler_reference and problems.handler_qp (checked
against each other and against QPhandler's setters on the CPU, tests/test_batch_handler_args.py), never from the library; the
step data are compared with the results() of the same solve."""
import numpy as np
import pytest

from restartsqp_amd import problems
from restartsqp_amd.handler import BatchQPhandler, batch_handler_reference
from restartsqp_amd.sqptypes import NLPInfo, SpTripletMat

import test_gpu_batch_members as M

pytestmark = pytest.mark.gpu

RAGGED = [(4, 2), (3, 1), (3, 4), (5, 0), (1, 3), (4, 2), (3, 1)]   # the search route; no constraints; more slacks than variables
SENTINEL = (-7.25e3, -6.5e3, 5.75e3, -4.125e3, 3.0625e3)            # g, lb, ub, lbA, ubA
VEC = ("g", "lb", "ub", "lbA", "ubA")


def synthetic_nlp(rng, n, m):
    """an NLP iterate of n variables and m constraints: H_k = I, a full Jacobian with 0.01 <= |J_ij| <= 0.1, bounds with +-inf"""
    rows, cols = [r + 1 for r in range(m) for c in range(n)], [c + 1 for r in range(m) for c in range(n)]
    vals = list(rng.uniform(0.01, 0.1, m * n) * rng.choice([-1.0, 1.0], m * n))
    x_l, x_u = rng.uniform(-3.0, -1.0, n), rng.uniform(1.0, 3.0, n)
    x_l[rng.random(n) < 0.3] = -np.inf; x_u[rng.random(n) < 0.3] = np.inf
    c_l, c_u = rng.uniform(-2.0, 0.0, m), rng.uniform(0.0, 2.0, m)
    c_l[rng.random(m) < 0.3] = -np.inf; c_u[rng.random(m) < 0.3] = np.inf
    return dict(x=rng.normal(size=n), grad=rng.normal(size=n), c=rng.normal(size=m), x_l=x_l, x_u=x_u, c_l=c_l, c_u=c_u,
                J=SpTripletMat(m, n, rows, cols, vals, False),
                H=SpTripletMat(n, n, list(range(1, n + 1)), list(range(1, n + 1)), [1.0] * n, True),
                info=NLPInfo(nCon=m, nVar=n, nnz_jac_g=m * n, nnz_h_lag=n))


def cat(parts):
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts] + [np.zeros(0)])


class Fixture:
    """a batch of synthetic members with its NLP bounds set and its pools full of SENTINEL"""

    def __init__(self, capi, shapes, seed):
        self.rng = np.random.default_rng(seed)
        self.n, self.m = [s[0] for s in shapes], [s[1] for s in shapes]
        self.nlps = [synthetic_nlp(self.rng, n, m) for n, m in shapes]
        self.b = capi.Batch([problems.handler_qp(p, name="synthetic") for p in self.nlps])
        self.bounds = tuple(cat([p[k] for p in self.nlps]) for k in ("x_l", "x_u", "c_l", "c_u"))
        sV, sC = int(self.b.offV[-1]), int(self.b.offC[-1])
        self.state = tuple(np.full(sV if k < 3 else sC, s) for k, s in enumerate(SENTINEL))
        self.b.set_vectors(*self.state)

    def iterate(self, words):
        """a fresh iterate for every member; NaN in everything that belongs to a member with word 0 (a read of it would show)"""
        rng, nq = self.rng, len(self.n)
        hide = lambda parts: cat([a if w else np.full(a.shape, np.nan) for a, w in zip(parts, words)])
        delta, rho = hide(rng.uniform(0.5, 2.0, (nq, 1))), hide(rng.uniform(1.0, 10.0, (nq, 1)))
        return (delta, rho, hide([rng.normal(size=k) for k in self.n]), hide([rng.normal(size=k) for k in self.m]),
                hide([rng.normal(size=k) for k in self.n]))

    def expect(self, words, it, with_grad=True):
        delta, rho, x_k, c_k, grad = it
        self.state = batch_handler_reference(self.state, words, delta, rho, x_k, c_k, grad if with_grad else None, self.n, self.m,
                                             *self.bounds)
        return self.state


def assert_pools(tag, b, expected, words, before, offV, offC):
    got = b.get_vectors()
    for k, (name, g, e) in enumerate(zip(VEC, got, expected)):
        assert np.array_equal(g, e), (tag, name, np.flatnonzero(g != e)[:8])
        off = offV if k < 3 else offC
        for q, w in enumerate(words):
            if w == 0:                                # a sitter keeps every byte
                assert g[off[q]:off[q + 1]].tobytes() == before[k][off[q]:off[q + 1]].tobytes(), (tag, name, q)
    return got


def ragged_schedule(capi):
    S, B, D, P, G, U = capi.HU_SET, capi.HU_BOUNDS, capi.HU_DELTA, capi.HU_PENALTY, capi.HU_GRAD, capi.HU_UBA
    # (words of the 7 members, a gradient is given); U alone and S beside other bits: the precedence of the header
    return [([S, S, 0, S, S, 0, S], True),
            ([G, 0, S, P, 0, S, B], True),
            ([B | U, D, 0, 0, P | G, B, D | P], True),
            ([0, B | G | P, D | G, B | U, 0, U, 0], True),
            ([S, 0, G, 0, S, P | G, D], False),
            ([D | B, S | G | D, 0, D, B | U | P, 0, G], True),
            ([0, 0, S | B, G | D, D, B | U | G | P | D, 0], True)]


def test_update_ragged_batch(capi):
    """seven members of five shapes: the member of a pool entry is searched in the descriptors' offsets. After every one of seven
    calls the five pools equal the reference, and members with word 0 keep SENTINEL (or what an earlier call wrote) bit for bit"""
    f = Fixture(capi, RAGGED, 31)
    f.b.handler_set_problem(*f.bounds)
    sched = ragged_schedule(capi)
    seen = 0
    for k, (words, with_grad) in enumerate(sched):
        assert sum(w == 0 for w in words) >= 2
        seen |= int(np.bitwise_or.reduce(words))
        it = f.iterate(words)
        before = f.state
        f.b.handler_update(words, *it[:4], grad=it[4] if with_grad else None)
        assert_pools(("ragged", k), f.b, f.expect(words, it, with_grad), words, before, f.b.offV, f.b.offC)
    assert seen == 63 and len(sched) >= 6
    assert np.isinf(f.bounds[0]).any() and np.isinf(f.bounds[1]).any() and np.isinf(f.bounds[2]).any() and np.isinf(f.bounds[3]).any()
    assert np.isinf(f.state[3]).any() and np.isinf(f.state[4]).any()      # (an infinite c_l / c_u reached lbA / ubA)
    f.b.close()


def one_shape_words(capi, call, nq):
    S, B, D, P, G, U = capi.HU_SET, capi.HU_BOUNDS, capi.HU_DELTA, capi.HU_PENALTY, capi.HU_GRAD, capi.HU_UBA
    cycle = [S, 0, B | U, G, 0, D | P, B, P | G, S | D, 0, D, B | G | P | U]
    return [cycle[(q + 5 * call) % len(cycle)] if call else (S if q % 7 else 0) for q in range(nq)]


def run_one_shape(capi, on_device):
    """130 members of (4, 2): 1 040 entries in g, lb and ub, so the division route crosses four block boundaries of 256 in each of
    them. Five calls with alternating words; returns the fixture and the pools after every call"""
    f = Fixture(capi, [(4, 2)] * 130, 37)
    f.b.handler_set_problem(*f.bounds)
    if on_device:
        import torch
        dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device="cuda")
    pools = []
    for call in range(5):
        words = one_shape_words(capi, call, 130)
        assert sum(w == 0 for w in words) >= 2
        with_grad = call != 3
        it = f.iterate(words)
        before = f.state
        grad = it[4] if with_grad else None
        if on_device:
            args = [dev(words, np.int32)] + [dev(a, np.float64) for a in it[:4]] + [dev(grad, np.float64)]
            torch.cuda.synchronize()                  # (the inputs are complete before the call)
            f.b.handler_update(*args, on_device=True)
        else:
            f.b.handler_update(words, *it[:4], grad=grad)
        pools.append(assert_pools(("one shape", on_device, call), f.b, f.expect(words, it, with_grad), words, before, f.b.offV, f.b.offC))
    return f, pools


def solvable_iterate(f):
    """SET for everybody at an iterate whose QP is feasible without slack: x_k inside the box, c_k between the constraint bounds"""
    nq = len(f.n)
    x_k = cat([np.clip(np.zeros(n), p["x_l"], p["x_u"]) for n, p in zip(f.n, f.nlps)])
    c_k = cat([np.where(np.isfinite(p["c_l"]), p["c_l"] + 0.25, np.where(np.isfinite(p["c_u"]), p["c_u"] - 0.25, 0.0)) for p in f.nlps])
    return np.ones(nq), np.ones(nq), x_k, c_k, cat([f.rng.normal(size=n) for n in f.n])


def test_update_one_shape_batch(capi):
    f, _ = run_one_shape(capi, False)
    f.b.close()


def test_device_pointers():
    """the same calls with every argument a torch tensor on the device give the same pools, and handler_step(on_device=True) writes
    into torch tensors what the host-pointer call returns. In a child process that imports torch BEFORE the library is loaded
    (tests/checks/handler_device_pointers.py says why): this process loaded the library first"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "handler_device_pointers.py")], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "HANDLER DEVICE POINTERS OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_step_against_results(capi):
    """the seven ragged members and one of n = 5, m = 35 (75 QP variables, 70 slack entries: a wave-strided sum takes a second
    pass; still an LDS-resident batch). delta = rho = 1, c_l - c_k = 10 and |J_ij| <= 0.1: every u_i comes out near 10.
    infea_model: any summation order of k non-negative terms is within 2 k 2^-53 s of the index-order sum s (each of the k - 1
    additions of either order has a relative error of at most 2^-53 on a partial sum of at most s)"""
    f = Fixture(capi, RAGGED + [(5, 35)], 41)
    nq = len(f.n)
    x_l, x_u = np.full(sum(f.n), -np.inf), np.full(sum(f.n), np.inf)
    c_l, c_u = np.zeros(sum(f.m)), np.full(sum(f.m), np.inf)
    f.b.handler_set_problem(x_l, x_u, c_l, c_u)
    f.b.handler_update([capi.HU_SET] * nq, np.ones(nq), np.ones(nq), np.zeros(sum(f.n)), np.full(sum(f.m), -10.0),
                       grad=cat([f.rng.normal(size=n) for n in f.n]))
    g, lb, ub, lbA, ubA = f.b.get_vectors()
    assert np.all(lbA == 10.0) and np.all(np.isinf(ubA))
    f.b.optimize_qp()
    assert f.b.last_kernel() == 0
    res = f.b.results()
    st = f.b.handler_step()
    print("status", [r["status"] for r in res])
    big = res[-1]["x"][5:]
    print("nonzero slack entries of the big member:", int(np.count_nonzero(big)))
    assert np.count_nonzero(big) >= 30                # (condition on the input)
    oN = oC = 0
    for q, (r, n, m) in enumerate(zip(res, f.n, f.m)):
        x, y = r["x"], r["y"]
        assert st["p"][oN:oN + n].tobytes() == x[:n].tobytes(), q
        assert st["lam_x"][oN:oN + n].tobytes() == y[:n].tobytes(), q
        assert st["lam_c"][oC:oC + m].tobytes() == y[n + 2 * m:].tobytes(), q
        assert np.float64(st["norm_p"][q]).tobytes() == np.float64(np.abs(x[:n]).max()).tobytes(), q
        k = 2 * m
        s = float(np.cumsum(np.abs(x[n:]))[-1]) if k else 0.0
        err = abs(float(st["infea_model"][q]) - s)
        print("member %d: infea_model %.17g, index-order sum %.17g, |difference| %.3g, bound %.3g" % (q, st["infea_model"][q], s, err, 2 * k * 2.0 ** -53 * s))
        assert err <= 2 * k * 2.0 ** -53 * s, (q, err)
        oN += n; oC += m
    f.b.close()


def drive(h, nq, j, flags, nlp, delta, rho, offN, offC):
    """the calls Algorithm::setupQP makes for one trace entry (src/Algorithm.cpp:645-697), for member j alone"""
    one = np.arange(nq) == j
    pooled = lambda a, off: np.concatenate([np.full(off[j], np.nan), a, np.full(off[-1] - off[j] - a.size, np.nan)])
    x_k, grad, c_k = pooled(nlp["x"], offN), pooled(nlp["grad"], offN), pooled(nlp["c"], offC)
    if flags["first"]:
        h.set_bounds(one, delta, x_k, c_k)
        h.set_g(one, grad, rho)
        return
    if flags["bounds"]:
        h.update_bounds(one, delta, x_k, c_k, refresh_ubA=True)
    elif flags["delta"]:
        h.update_delta(one, delta, x_k)
    if flags["penalty"]:
        h.update_penalty(one, rho)
    if flags["g"]:
        h.update_grad(one, grad)


def test_lockstep_replay_through_the_handler(capi, oracle):
    """test_gpu_batch_members.test_lockstep_replay_of_three_sqp_runs with the vectors built on the device: per batch step the
    participants' trace flags become BatchQPhandler calls (sitters get word 0 and are masked out), one flush writes the pools --
    which must equal problems.handler_qp's bit for bit for every participant --, solveQP runs the masked optimize_qp and the
    certificate, and the existing test's criteria hold per participant; handler_step's p and infea_model agree with the trace"""
    T = M.T
    runs = {name: M.trajectory_qps(name) for name in M.NLPS}
    M.assert_oracle_replays_the_trajectories(oracle, runs)
    nq = len(M.LOCKSTEP)
    b = capi.Batch([runs[name][1][0] for name, start in M.LOCKSTEP])
    nlp0 = [M.NLPS[name]() for name, start in M.LOCKSTEP]
    ns, ms = [p["info"].nVar for p in nlp0], [p["info"].nCon for p in nlp0]
    offN, offC = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(ms)])
    h = BatchQPhandler(b, *[cat([p[k] for p in nlp0]) for k in ("x_l", "x_u", "c_l", "c_u")])
    nsteps = max(start + len(runs[name][0]) for name, start in M.LOCKSTEP)
    ties = [0] * nq
    for t in range(nsteps):
        entry = [t - start if 0 <= t - start < len(runs[name][0]) else None for name, start in M.LOCKSTEP]
        take = np.array([e is not None for e in entry])
        gold = [runs[name][0][e] if e is not None else None for (name, start), e in zip(M.LOCKSTEP, entry)]
        members = [runs[name][1][e if e is not None else 0] for (name, start), e in zip(M.LOCKSTEP, entry)]
        name_m = np.array([g is not None and bool(g["flags"]["A"] or g["flags"]["H"]) for g in gold])
        if name_m.any():
            M.masked_matrices(b, members, name_m)
        for j, ((name, start), g) in enumerate(zip(M.LOCKSTEP, gold)):
            if g is not None:
                drive(h, nq, j, g["flags"], M.NLPS[name](np.array(g["x"]), np.array(g["lam"])), g["delta"], g["rho"], offN, offC)
        pools_before = b.get_vectors()
        words = h.flush()
        assert np.array_equal(words != 0, take), (t, words)
        pools = b.get_vectors()
        for j, (q, g) in enumerate(zip(members, gold)):
            for k, name in enumerate(VEC):
                lo, hi = (b.offV[j], b.offV[j + 1]) if k < 3 else (b.offC[j], b.offC[j + 1])
                if g is None:
                    assert pools[k][lo:hi].tobytes() == pools_before[k][lo:hi].tobytes(), (t, j, name)
                else:
                    assert np.array_equal(pools[k][lo:hi], getattr(q, name)), (t, j, name)
        before = b.results()
        used, ok, kkt = h.solveQP(take)
        assert b.last_kernel() == 0
        mode, rescue = b.dispatch()
        res = b.results()
        st = h.step()
        for j, ((name, start), g) in enumerate(zip(M.LOCKSTEP, gold)):
            tag = (name, j, t)
            if g is None:
                M.assert_sitter(tag, before[j], res[j], used[j], mode[j], rescue[j])
                continue
            r = res[j]
            assert int(mode[j]) == T.MODES[g["mode"]] and int(rescue[j]) == 0, (tag, int(mode[j]), g["mode"], int(rescue[j]))
            assert r["status"] == g["status"] == 20, (tag, r["status"])
            assert ok[j] == 1, (tag, float(kkt[j]))
            gx, gy = np.array(g["x_qp"]), np.array(g["y_qp"])
            tol = 1e-9 * max(1.0, np.abs(gx).max())
            assert np.abs(r["x"] - gx).max() <= tol, (tag, g["mode"])
            assert abs(r["obj"] - g["obj"]) <= 1e-9 * max(1.0, abs(g["obj"])), tag
            assert np.abs(st["p"][offN[j]:offN[j + 1]] - gx[:ns[j]]).max() <= tol, tag
            assert abs(st["infea_model"][j] - np.abs(gx[ns[j]:]).sum()) <= tol, (tag, float(st["infea_model"][j]))
            same_path = int(used[j]) == g["nWSR"] and np.array_equal(r["ws_b"], g["ws_b"]) and np.array_equal(r["ws_c"], g["ws_c"])
            if name == "hs065":
                ties[j] += not same_path
                continue
            assert same_path, (tag, g["mode"], int(used[j]), g["nWSR"])
            assert np.abs(r["y"] - gy).max() <= 1e-9 * max(1.0, np.abs(gy).max()), (tag, g["mode"])
    assert max(ties) <= 3, ties
    b.close()


def test_call_order_and_shape_errors(capi):
    f = Fixture(capi, RAGGED, 43)
    nq = len(f.n)
    it = f.iterate([capi.HU_SET] * nq)
    with pytest.raises(capi.RsqpError) as e:
        f.b.handler_update([capi.HU_SET] * nq, *it[:4], grad=it[4])
    assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.RsqpError) as e:
        f.b.handler_step()
    assert e.value.code == capi.ERR_ARG
    assert all(np.array_equal(a, c) for a, c in zip(f.b.get_vectors(), f.state))      # (nothing was written)
    f.b.close()
    # a member that has no NLP variable beside its slacks: 4 variables, 2 constraints
    rng = np.random.default_rng(3)
    b = capi.Batch([problems.hs071_first_qp(), problems.random_qp(rng, 4, 2)])
    with pytest.raises(capi.RsqpError) as e:
        b.handler_set_problem(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4))
    assert e.value.code == capi.ERR_ARG
    b.close()
