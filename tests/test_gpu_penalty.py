"""update_penalty_parameter per member of a batch on the device (rsqp_batch_handler_update_penalty, include/rsqp_hip_penalty.h;
restartsqp_amd/csrc/rsqp_batch_penalty.hip). Two yardsticks, neither from the call itself: (a) the host-driven loop of
tests/penalty_cases.py, which does the same work on a second pair of batches with the entry points that existed before the call and
numpy decisions -- compared bit for bit --, and (b) handler.batch_update_penalty_reference over the C oracle, which
tests/test_penalty_args.py has shown to take every branch on these inputs."""
import numpy as np
import pytest

import penalty_cases as PC
from lp_batch_ref import TOL

pytestmark = pytest.mark.gpu

HS071_NQ = len(PC.HS071_GPU)       # 70: a wave of the 8-lane kernels holds eight members, of different branches in this batch
STATE = ("rho", "eps1", "trial", "succ", "fail")


def call(capi, qp, members, S, o, out, on_device):
    """the new call on host arrays, or on torch tensors of the batch's device; S and out are written in place either way"""
    opts = capi.PenaltyOptions(**{k: o[k] for k in o})
    if not on_device:
        qp.handler_update_penalty(**S, options=opts, out=out)
        return
    torch = capi.device_torch()
    dS = {k: torch.as_tensor(v, device="cuda") for k, v in S.items()}
    dout = {k: torch.as_tensor(v, device="cuda") for k, v in out.items()}
    torch.cuda.synchronize()
    qp.handler_update_penalty(**dS, options=opts, out=dout, on_device=True)
    for k in STATE:
        S[k][:] = dS[k].cpu().numpy()
    for k in out:
        out[k][:] = dout[k].cpu().numpy()


def prepared(capi, batch, option_set, what=None):
    """two pairs with the first QP solve done, the re-solves' budget set, a sticky mask on each batch of the first pair, and the inputs"""
    members = PC.members_of(batch)
    fields, eps1, budget = PC.OPTION_SETS[option_set]
    o = capi.PenaltyOptions(**fields).as_dict()
    pairs = [PC.make_pair(capi, members) for _ in range(2)]
    for qp, lp in pairs:
        qp.set_options(qp_maxiter=budget)
    qp, lp = pairs[0]
    sticky = np.array([q % 3 != 0 for q in range(len(members))], np.int32)
    qp.set_members(sticky); lp.set_members(sticky)
    qp.handler_pair_lp(lp)
    return members, o, pairs, PC.pooled(members, eps1, what)


def close(pairs):
    for qp, lp in pairs:
        qp.handler_pair_lp(None)
        qp.close(); lp.close()


HOST_DRIVEN_CASES = [("hs071_gpu", k) for k in PC.OPTION_SETS] + [("mixed", k) for k in PC.OPTION_SETS]


def check_against_the_host_driven_loop(capi, batch, option_set, on_device):
    """(a): every output and state array, the result pools, the g pools, the LP batch's A pool and the dispatch of the last inner
    calls are equal bit for bit; a member with word 0 keeps every byte; the sticky masks survive"""
    members, o, pairs, S = prepared(capi, batch, option_set)
    nq = len(members)
    (qp, lp), (hq, hl) = pairs
    before = PC.snapshot(capi, qp, lp)
    S1, S2 = {k: v.copy() for k, v in S.items()}, {k: v.copy() for k, v in S.items()}
    out1, out2 = PC.fresh_out(capi, nq), PC.fresh_out(capi, nq)
    call(capi, qp, members, S1, o, out1, on_device)
    x_exp, obj_exp = PC.host_driven(capi, hq, hl, members, S2, o, out2)
    for k in S:
        assert PC.same_bytes(S1[k], S2[k]), (k, np.flatnonzero(S1[k] != S2[k])[:5])
    for k in out1:
        assert PC.same_bytes(out1[k], out2[k]), (k, out1[k][:12], out2[k][:12])
    got, exp = PC.snapshot(capi, qp, lp), PC.snapshot(capi, hq, hl)
    exp["qp.x"], exp["qp.obj"] = x_exp, obj_exp
    assert set(got) == set(exp)
    for k in got:
        assert PC.same_bytes(got[k], exp[k]), (k, np.flatnonzero(got[k] != exp[k])[:5])
    # something happened, on every path the option set is meant for
    looped = out1["rounds"] > 0
    assert looped.any()
    if batch == "hs071_gpu":
        assert (out1["hu_word"] == capi.HU_PENALTY).any() == (option_set in ("eps2", "budget"))
    # a member with word 0: every byte of its outputs, its state and both batches' pools is what it was
    sat = S["what"] == 0
    assert sat.sum() >= 2
    for k in out1:
        assert PC.same_bytes(out1[k][sat], PC.fresh_out(capi, nq)[k][sat]), k
    offV = np.concatenate([[0], np.cumsum([d["n"] + 2 * d["m"] for d in members])])
    for q in np.flatnonzero(sat):
        for tag in ("qp.", "lp."):
            for k in ("x", "g", "lb", "ub"):
                assert PC.same_bytes(got[tag + k][offV[q]:offV[q + 1]], before[tag + k][offV[q]:offV[q + 1]]), (q, tag + k)
            assert PC.same_bytes(got[tag + "obj"][q:q + 1], before[tag + "obj"][q:q + 1]), (q, tag + "obj")
    # the sticky masks are what they were: an optimize call behind it leaves the members of the mask out
    used = qp.optimize_qp()
    assert np.all(used[::3] == 0) and np.array_equal(qp.dispatch()[0][::3], np.full(len(used[::3]), -1))
    used = lp.optimize_lp()
    assert np.all(used[::3] == 0) and np.array_equal(lp.dispatch()[0][::3], np.full(len(used[::3]), -1))
    close(pairs)


@pytest.mark.parametrize("batch,option_set", HOST_DRIVEN_CASES)
def test_against_the_host_driven_loop(capi, batch, option_set):
    check_against_the_host_driven_loop(capi, batch, option_set, False)


def test_device_pointers():
    """the same comparison with every array a device tensor (torch), for every case. In a child process that imports torch BEFORE
    the library is loaded (tests/checks/handler_device_pointers.py says why)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "penalty_device_pointers.py")], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "PENALTY DEVICE POINTERS OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("batch,option_set", [("hs071_gpu", k) for k in PC.OPTION_SETS] + [("mixed", "default"), ("mixed", "eps1")])
def test_against_the_oracle_driven_reference(capi, oracle, batch, option_set):
    """(b): branch, rounds, rho, eps1, the counters, hu_word and exitflag exactly; x and the objective within lp_batch_ref.TOL,
    relative to max(1, |.|_inf) -- for the members solved throughout on the oracle"""
    members, S, o, rows, first = PC.oracle_run(oracle, capi, batch, option_set)
    nq = len(members)
    members2, o2, pairs, S1 = prepared(capi, batch, option_set)
    qp, lp = pairs[0]
    out = PC.fresh_out(capi, nq)
    call(capi, qp, members2, S1, o2, out, False)
    res = qp.results()
    tol = o["penalty_update_tol"]
    compared = 0
    for q in range(nq):
        r = rows[q]
        if not PC.solved_throughout(r):
            continue
        compared += 1
        tag = (batch, option_set, q, PC.kind_of(r))
        branch = "none" if np.isnan(out["infea_infty"][q]) else ("A" if out["infea_infty"][q] <= tol else "B")
        assert branch == r["branch"], tag
        assert (out["rounds"][q], out["hu_word"][q], out["exitflag"][q]) == (r["rounds"], r["hu_word"], r["exitflag"]), tag
        assert (S1["rho"][q], S1["eps1"][q]) == (r["rho"], r["eps1"]), tag
        assert (S1["trial"][q], S1["succ"][q], S1["fail"][q]) == (r["trial"], r["succ"], r["fail"]), tag
        xs = max(1.0, np.abs(r["x"]).max())
        assert np.abs(res[q]["x"] - r["x"]).max() <= TOL * xs, tag
        assert abs(res[q]["obj"] - r["obj"]) <= TOL * max(1.0, abs(r["obj"])), tag
    assert compared >= nq // 2, compared
    close(pairs)


def test_two_calls_with_an_accepted_step_between(capi):
    """(c): the second LP solve of a member is a hot start with new matrices (mode 2) on the regVal of its first init. Between the
    calls: a new J through handler_set_matrices and the QP solved again, as an accepted step brings them"""
    members, o, pairs, S = prepared(capi, "hs071_gpu", "default", what=np.ones(HS071_NQ, np.int32))
    nq = len(members)
    (qp, lp), (hq, hl) = pairs
    twice = None
    for step in range(2):
        S1, S2 = {k: v.copy() for k, v in S.items()}, {k: v.copy() for k, v in S.items()}
        out1, out2 = PC.fresh_out(capi, nq), PC.fresh_out(capi, nq)
        call(capi, qp, members, S1, o, out1, False)
        x_exp, obj_exp = PC.host_driven(capi, hq, hl, members, S2, o, out2)
        ran_lp = out1["nwsr_lp"] > 0
        mode = lp.dispatch()[0]
        if step == 0:
            assert np.all(mode[ran_lp] == capi.MODE_COLD) and np.all(mode[~ran_lp] == -1)
            twice = ran_lp
        else:
            both = twice & ran_lp
            assert both.sum() >= 2 and np.all(mode[both] == capi.MODE_HOT_MATRICES)
        for k in out1:
            assert PC.same_bytes(out1[k], out2[k]), (step, k)
        got, exp = PC.snapshot(capi, qp, lp), PC.snapshot(capi, hq, hl)
        exp["qp.x"], exp["qp.obj"] = x_exp, obj_exp
        for k in got:
            assert PC.same_bytes(got[k], exp[k]), (step, k)
        if step == 0:
            # the accepted step: a new Jacobian (and the QP of the new iterate solved) on both pairs alike
            rng = np.random.default_rng(3)
            A = qp.get_matrix_values()[0]
            offA = np.concatenate([[0], np.cumsum(qp.annz)])
            jac = np.concatenate([A[offA[q]:offA[q] + qp.jnz[q]] for q in range(nq)]) * (1.0 + 0.01 * rng.normal(size=int(qp.jnz.sum())))
            for b in (qp, hq):
                b.handler_set_matrices(np.full(nq, capi.HM_JAC, np.int32), jac=jac)
                b.handler_update(np.full(nq, capi.HU_PENALTY, np.int32), S["delta"], S["rho"], S["x_k"], S["c_k"])
                b.set_members(None)
                b.optimize_qp()
    close(pairs)


def test_nobody_exceeds_the_tolerance(capi):
    """(d): with a tolerance nobody's model exceeds, both batches keep every byte and every member reports rounds == 0"""
    members, o, pairs, S = prepared(capi, "hs071_gpu", "default")
    nq = len(members)
    qp, lp = pairs[0]
    before = PC.snapshot(capi, qp, lp)
    out = PC.fresh_out(capi, nq)
    S1 = {k: v.copy() for k, v in S.items()}
    call(capi, qp, members, S1, dict(o, penalty_update_tol=1.0e30), out, False)
    after = PC.snapshot(capi, qp, lp)
    for k in before:
        assert PC.same_bytes(before[k], after[k]), k
    for k in STATE:
        assert PC.same_bytes(S1[k], S[k]), k
    took = (S["what"] != 0) & (before["qp.status"] == capi.QP_OPTIMAL)
    assert took.sum() >= 40 and np.all(out["rounds"][took] == 0) and np.all(out["rounds"][~took] == PC.INT_FILL)
    assert np.all(out["nwsr_lp"][took] == 0) and np.all(out["hu_word"][took] == 0) and np.all(out["exitflag"][took] == capi.EXIT_UNKNOWN)
    unsolved = (S["what"] != 0) & ~took
    assert np.array_equal(out["exitflag"][unsolved], before["qp.status"][unsolved])
    close(pairs)


def test_failure_path_member(capi):
    """(e): after a failure, handler_step returns the first solve's p and infea_model, results() the first solve's objective and
    the LAST solve's y"""
    members, o, pairs, S = prepared(capi, "hs071_gpu", "eps2")
    nq = len(members)
    qp, lp = pairs[0]
    r0, step0 = PC.raw_results(qp), qp.handler_step()
    out = PC.fresh_out(capi, nq)
    S1 = {k: v.copy() for k, v in S.items()}
    call(capi, qp, members, S1, o, out, False)
    r1, step1 = PC.raw_results(qp), qp.handler_step()
    failed = np.flatnonzero(out["hu_word"] == capi.HU_PENALTY)
    assert failed.size >= 2
    for q in failed:
        assert out["rounds"][q] >= 1 and S1["fail"][q] == S["fail"][q] + 1 and S1["rho"][q] == S["rho"][q]
        assert PC.same_bytes(step1["p"][4 * q:4 * q + 4], step0["p"][4 * q:4 * q + 4])
        assert step1["infea_model"][q] == step0["infea_model"][q] == out["infea_model"][q]
        assert r1["obj"][q] == r0["obj"][q]
        assert PC.same_bytes(r1["x"][8 * q:8 * q + 8], r0["x"][8 * q:8 * q + 8])
    # ... the multipliers are the last solve's: rho_trial changed the QP, so some member's y moved
    assert any(not PC.same_bytes(r1["y"][10 * q:10 * q + 10], r0["y"][10 * q:10 * q + 10]) for q in failed)
    close(pairs)


def test_pairing_is_checked(capi):
    """rsqp_batch_handler_pair_lp refuses what the call could not work on, and the call refuses a batch without a pair"""
    members = PC.hs071_members()[:6]
    qp, lp = PC.make_pair(capi, members)
    S = PC.pooled(members, PC.EPS1)
    with pytest.raises(capi.RsqpError) as e:
        qp.handler_update_penalty(**S)
    assert e.value.code == capi.ERR_ARG
    fewer = capi.Batch([d["qp"] for d in members[:5]])
    no_problem = capi.Batch([d["qp"] for d in members])
    other = PC.make_pair(capi, PC.mixed_members()[:6])
    for bad in (fewer, no_problem, other[1], qp):
        with pytest.raises(capi.RsqpError) as e:
            qp.handler_pair_lp(bad)
        assert e.value.code == capi.ERR_ARG
    lp.set_keep_state(False)
    with pytest.raises(capi.RsqpError):
        qp.handler_pair_lp(lp)
    lp.set_keep_state(True)
    qp.handler_pair_lp(lp)
    with pytest.raises(capi.RsqpError) as e:
        qp.handler_update_penalty(**S, options=capi.PenaltyOptions(increase_parm=1.0))
    assert e.value.code == capi.ERR_ARG
    qp.handler_pair_lp(None)
    with pytest.raises(capi.RsqpError):
        qp.handler_update_penalty(**S)
    for b in (qp, lp, fewer, no_problem) + other:
        b.close()
