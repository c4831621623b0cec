"""second_order_correction per member of a batch on the device (rsqp_batch_handler_soc_begin / _soc_end, rsqp_batch_set_objective;
include/rsqp_hip_soc.h, restartsqp_amd/csrc/rsqp_batch_soc.hip). Two yardsticks, neither from the calls themselves: (a) the
host-driven loop of tests/soc_cases.py, which does the same work on a second batch with the entry points that existed before the
calls (plus set_objective) and numpy decisions -- compared bit for bit --, and (b) handler.batch_soc_reference over the C oracle,
which tests/test_soc_args.py has shown to take every branch on these inputs."""
import ctypes as C

import numpy as np
import pytest

import soc_cases as SC
from lp_batch_ref import TOL

pytestmark = pytest.mark.gpu


def prepared(capi, batch, option_set, what=None):
    """two batches with the first QP solve done and the correction solve's budget set, a sticky mask on the first, and the inputs"""
    members = SC.members_of(batch)
    fields, soc_fields, budget, give_model = SC.OPTION_SETS[option_set]
    o, so = capi.NlpStepOptions(**fields).as_dict(), capi.SocOptions(**soc_fields).as_dict()
    b, hb = SC.make_batch(capi, members, budget), SC.make_batch(capi, members, budget)
    b.set_members(np.array([q % 3 != 0 for q in range(len(members))], np.int32))
    model = b.handler_step()["infea_model"] if give_model else None
    return members, o, so, b, hb, SC.pooled(members, what), model


HOST_DRIVEN_CASES = [(b, k) for b in ("hs071_gpu", "mixed") for k in SC.OPTION_SETS]
POOLS = ("x", "y", "ws_b", "ws_c", "status", "obj", "g", "lb", "ub", "lbA", "ubA", "A", "H", "mode", "rescue")


def check_against_the_host_driven_loop(capi, batch, option_set, on_device):
    """(a): every in/out and out array -- between the two calls and behind them --, the result pools, g / lb / ub / lbA / ubA, the
    matrix pools and the dispatch of the inner call are equal bit for bit; a member with word 0 keeps every byte; the sticky mask
    survives; a member with RSQP_SOC_TEST alone gets what rsqp_batch_handler_ratio_test writes"""
    members, o, so, b, hb, S, model = prepared(capi, batch, option_set)
    nq = len(members)
    n, m, offN, offC, offV = SC.offsets(members)
    bias = SC.biases_of(members)
    before = SC.snapshot(capi, b)
    S1, S2 = {k: v.copy() for k, v in S.items()}, {k: v.copy() for k, v in S.items()}
    out1, out2 = SC.fresh_out(capi, members), SC.fresh_out(capi, members)
    mid1 = SC.device_route(capi, b, members, S1, o, so, out1, bias, on_device, model)
    mid2 = SC.host_driven(capi, hb, members, S2, o, so, out2, bias, model)
    for k in mid1:
        assert SC.same_bytes(mid1[k], mid2[k]), ("between the calls", k, np.flatnonzero(mid1[k] != mid2[k])[:5])
    for k in S:
        assert SC.same_bytes(S1[k], S2[k]), (k, np.flatnonzero(S1[k] != S2[k])[:5])
    for k in out1:
        assert SC.same_bytes(out1[k], out2[k]), (k, np.flatnonzero(out1[k] != out2[k])[:5], out1[k][:12], out2[k][:12])
    got, exp = SC.snapshot(capi, b), SC.snapshot(capi, hb)
    assert set(got) == set(exp) == set(POOLS)
    for k in got:
        assert SC.same_bytes(got[k], exp[k]), (k, np.flatnonzero(got[k] != exp[k])[:5])
    # something happened, on every path the option set is meant for
    went = mid1["soc"] == 1
    assert went.sum() >= 2 and (out1["accept"][went] == 0).sum() >= 2
    corrected = (S["what"] & capi.SOC_CORRECT) != 0
    unsolved = corrected & (mid1["soc"] == 0) & (mid1["accept"] == SC.INT_FILL)     # (accepted at once writes accept = 1)
    if option_set == "budget":
        assert unsolved.sum() >= 2 and np.all(out1["exitflag"][unsolved] != capi.EXIT_UNKNOWN)
    if batch == "hs071_gpu" and option_set != "budget":
        assert (out1["accept"][went] == 1).sum() >= 1
    # a member with word 0: every byte of its outputs, its iterate and the batch's pools is what it was
    sat = S["what"] == 0
    assert sat.sum() >= 2
    fresh = SC.fresh_out(capi, members)
    for q in np.flatnonzero(sat):
        for k in out1:
            sl = slice(offN[q], offN[q + 1]) if k == "x_trial" else slice(q, q + 1)
            assert SC.same_bytes(out1[k][sl], fresh[k][sl]), (q, k)
        for k in ("x", "g", "lb", "ub", "ws_b"):
            assert SC.same_bytes(got[k][offV[q]:offV[q + 1]], before[k][offV[q]:offV[q + 1]]), (q, k)
        for k in ("lbA", "ubA", "ws_c"):
            assert SC.same_bytes(got[k][offC[q]:offC[q + 1]], before[k][offC[q]:offC[q + 1]]), (q, k)
        assert got["obj"][q] == before["obj"][q] and got["status"][q] == before["status"][q]
        assert SC.same_bytes(S1["x_k"][offN[q]:offN[q + 1]], S["x_k"][offN[q]:offN[q + 1]]) and S1["delta"][q] == S["delta"][q]
    # a member with RSQP_SOC_TEST alone: every byte is rsqp_batch_handler_ratio_test's (a third batch runs it for these members)
    only = S["what"] == capi.SOC_TEST
    assert only.sum() >= 2
    tb = SC.make_batch(capi, members)
    f_t, c_t, _ = SC.first_trial_values(tb, members, bias)
    S3 = {k: v.copy() for k, v in S.items()}
    out3 = {k: fresh[k].copy() for k in capi.NlpTrial.OUT}
    tb.handler_ratio_test(only.astype(np.int32), S3["rho"], f_t, c_t, *(S3[k] for k in SC.ITERATE), options=capi.NlpStepOptions(**o), out=out3)
    for q in np.flatnonzero(only):
        for k in out3:
            assert out1[k][q:q + 1].tobytes() == out3[k][q:q + 1].tobytes(), (q, k)
        for k in ("f_k", "infea_k", "delta"):
            assert S1[k][q:q + 1].tobytes() == S3[k][q:q + 1].tobytes(), (q, k)
        assert SC.same_bytes(S1["x_k"][offN[q]:offN[q + 1]], S3["x_k"][offN[q]:offN[q + 1]]), q
        assert SC.same_bytes(S1["c_k"][offC[q]:offC[q + 1]], S3["c_k"][offC[q]:offC[q + 1]]), q
        assert (out1["soc"][q], out1["nwsr_soc"][q]) == (0, 0) and out1["qp_obj"][q] == before["obj"][q]
        for k in ("x", "g", "lb", "ub"):
            assert SC.same_bytes(got[k][offV[q]:offV[q + 1]], before[k][offV[q]:offV[q + 1]]), (q, k)
    # the sticky mask is what it was: an optimize call behind it leaves the members of the mask out
    used = b.optimize_qp()
    assert np.all(used[::3] == 0) and np.array_equal(b.dispatch()[0][::3], np.full(len(used[::3]), -1))
    for x in (b, hb, tb):
        x.close()


@pytest.mark.parametrize("batch,option_set", HOST_DRIVEN_CASES)
def test_against_the_host_driven_loop(capi, batch, option_set):
    check_against_the_host_driven_loop(capi, batch, option_set, False)


def test_device_pointers():
    """(c): the same comparison with every array a device tensor (torch), for every case. In a child process that imports torch
    BEFORE the library is loaded (tests/checks/handler_device_pointers.py says why)"""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "checks", "soc_device_pointers.py")], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "SOC DEVICE POINTERS OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.parametrize("batch,option_set", [("hs071_gpu", k) for k in SC.OPTION_SETS] + [("mixed", "default"), ("mixed", "ubA")])
def test_against_the_oracle_driven_reference(capi, oracle, batch, option_set):
    """(b): branch, accept flags, words, exit flags and delta exactly; x, the objective and x_trial within lp_batch_ref.TOL,
    relative to max(1, |.|_inf) -- for the members solved throughout on the oracle"""
    members, S, o, so, rows = SC.oracle_run(oracle, capi, batch, option_set)
    nq = len(members)
    n, m, offN, offC, offV = SC.offsets(members)
    members2, o2, so2, b, hb, S1, model = prepared(capi, batch, option_set)
    hb.close()
    out = SC.fresh_out(capi, members)
    mid = SC.device_route(capi, b, members2, S1, o2, so2, out, SC.biases_of(members), False, model)
    res = b.results()
    compared = 0
    for q in range(nq):
        r = rows[q]
        if not SC.solved_throughout(r):
            continue
        compared += 1
        tag = (batch, option_set, q, SC.kind_of(r))
        went = mid["soc"][q] == 1
        branch = ("soc_accepted" if out["accept"][q] else "soc_rejected") if went else \
                 ("no_correct" if not S["what"][q] & capi.SOC_CORRECT else ("accepted" if out["accept"][q] else "soc_unsolved"))
        assert branch == r["branch"], tag
        assert (out["accept"][q], out["hu_word"][q], out["hm_word"][q], out["exitflag"][q]) == \
               (r["accept"], r["hu_word"], r["hm_word"], r["exitflag"]), tag
        assert S1["delta"][q] == r["delta"], tag
        assert mid["soc"][q] == r["soc"], tag
        scale = lambda v: max(1.0, float(np.abs(v).max()))
        assert np.abs(res[q]["x"] - r["x"]).max() <= TOL * scale(r["x"]), tag
        assert abs(res[q]["obj"] - r["obj"]) <= TOL * max(1.0, abs(r["obj"])), tag
        assert np.abs(S1["x_k"][offN[q]:offN[q + 1]] - r["x_k"]).max() <= TOL * scale(r["x_k"]), tag
        if went:
            assert np.abs(out["x_trial"][offN[q]:offN[q + 1]] - r["x_trial"]).max() <= TOL * scale(r["x_trial"]), tag
            assert abs(out["qp_obj"][q] - r["qp_obj"]) <= TOL * max(1.0, abs(r["qp_obj"])), tag
    assert compared >= nq // 2, compared
    b.close()


def test_rejected_correction_then_the_next_iteration(capi):
    """(d): two iterations back to back. Behind a rejected correction, handler_update with the returned words leaves the g and bound
    pools of the corrected members those of a batch that never ran the correction and takes the same update; then a new solve"""
    members, o, so, b, fresh, S, model = prepared(capi, "hs071_gpu", "ubA")
    nq = len(members)
    n, m, offN, offC, offV = SC.offsets(members)
    b.set_members(None)
    out = SC.fresh_out(capi, members)
    S1 = {k: v.copy() for k, v in S.items()}
    mid = SC.device_route(capi, b, members, S1, o, so, out, SC.biases_of(members))
    rejected = (mid["soc"] == 1) & (out["accept"] == 0)
    assert rejected.sum() >= 2
    dirty = SC.snapshot(capi, b)
    clean = SC.snapshot(capi, fresh)
    for q in np.flatnonzero(rejected):      # the correction's vectors are still there: the words are needed
        assert not SC.same_bytes(dirty["g"][offV[q]:offV[q + 1]], clean["g"][offV[q]:offV[q + 1]]), q
        assert out["hu_word"][q] == capi.HU_BOUNDS | capi.HU_GRAD | capi.HU_UBA and out["hm_word"][q] == 0
        assert SC.same_bytes(dirty["x"][offV[q]:offV[q + 1]], clean["x"][offV[q]:offV[q + 1]]) and dirty["obj"][q] == clean["obj"][q]
    words = np.where(rejected, out["hu_word"], 0).astype(np.int32)
    for x in (b, fresh):
        x.handler_update(words, S1["delta"], S1["rho"], S1["x_k"], S1["c_k"], grad=S1["grad"])
    got, exp = b.get_vectors(), fresh.get_vectors()
    for k, u, v in zip(("g", "lb", "ub", "lbA", "ubA"), got, exp):
        off = offV if k in ("g", "lb", "ub") else offC
        for q in np.flatnonzero(rejected):
            assert SC.same_bytes(u[off[q]:off[q + 1]], v[off[q]:off[q + 1]]), (k, q)
    b.set_members(rejected.astype(np.int32))
    used = b.optimize_qp()
    assert np.all(used[~rejected] == 0) and np.all(b.dispatch()[0][rejected] >= 0)
    for k, u, v in zip(("g", "lb", "ub", "lbA", "ubA"), b.get_vectors(), got):
        assert SC.same_bytes(u, v), k
    # a second soc_begin on the new solve runs, and soc_end ignores the members it did not set going
    out2 = SC.fresh_out(capi, members)
    S2 = {k: v.copy() for k, v in S1.items()}
    S2["what"] = np.where(rejected, capi.SOC_TEST, 0).astype(np.int32)
    SC.device_route(capi, b, members, S2, o, so, out2, SC.biases_of(members))
    assert np.all(out2["soc"][rejected] == 0) and np.all(out2["soc"][~rejected] == SC.INT_FILL)
    stale = {k: v.copy() for k, v in out2.items()}
    stale["soc"][:] = 1                     # nobody is pending: every byte is kept
    keep = {k: v.copy() for k, v in stale.items()}
    S3 = {k: v.copy() for k, v in S2.items()}
    pools = SC.snapshot(capi, b)
    b.handler_soc_end(S3["rho"], np.zeros(nq), np.zeros(int(m.sum())), *(S3[k] for k in SC.ITERATE), out=stale)
    for k in keep:
        assert SC.same_bytes(stale[k], keep[k]), k
    for k in SC.ITERATE:
        assert SC.same_bytes(S3[k], S2[k]), k
    after = SC.snapshot(capi, b)
    for k in pools:
        assert SC.same_bytes(pools[k], after[k]), k
    b.close(); fresh.close()


def test_set_objective(capi):
    """(e): the named members change; the others and every other pool keep every byte"""
    members = SC.members_of("mixed")
    b = SC.make_batch(capi, members)
    nq = len(members)
    before = SC.snapshot(capi, b)
    new = np.arange(nq, dtype=np.float64) * 0.5 - 3.0
    named = np.array([q % 4 == 1 for q in range(nq)], np.int32)
    b.set_objective(new, members=named)
    after = SC.snapshot(capi, b)
    assert SC.same_bytes(after["obj"], np.where(named != 0, new, before["obj"]))
    for k in before:
        if k != "obj":
            assert SC.same_bytes(before[k], after[k]), k
    b.set_objective(new)
    assert SC.same_bytes(SC.snapshot(capi, b)["obj"], new)
    b.set_objective(before["obj"], members=np.zeros(nq, np.int32))
    assert SC.same_bytes(SC.snapshot(capi, b)["obj"], new)
    b.close()


def test_argument_errors_of_a_batch(capi):
    """what the calls refuse on a batch, before any launch of theirs: soc_end before any soc_begin, grad missing beside a CORRECT
    word, a batch that keeps no state, a missing required pointer, null options, no handler_set_problem, no H"""
    import copy
    L = capi.lib()
    members = SC.members_of("hs071_gpu")[:3]
    cat = lambda k: np.concatenate([d[k] for d in members])
    S = SC.pooled(members)
    f_t, c_t = np.zeros(3), np.zeros(6)
    it = {k: S[k] for k in SC.ITERATE}
    out = SC.fresh_out(capi, members)

    def refused(call):
        with pytest.raises(capi.RsqpError) as e:
            call()
        assert e.value.code == capi.ERR_ARG

    b = capi.Batch([d["qp"] for d in members])
    b.handler_set_problem(cat("x_l"), cat("x_u"), cat("c_l"), cat("c_u"))
    refused(lambda: b.handler_soc_end(S["rho"], f_t, c_t, **it, out=out))                            # no soc_begin yet
    refused(lambda: b.handler_soc_begin(S["what"], S["rho"], f_t, c_t, **it, grad=None, out=out))    # CORRECT without grad
    b.set_keep_state(False)
    refused(lambda: b.handler_soc_begin(S["what"], S["rho"], f_t, c_t, **it, grad=S["grad"], out=out))
    b.set_keep_state(True)
    arrays = dict(out, **S, f_trial=f_t, c_trial=c_t)
    t = capi.SocTrial(**{k: arrays[k].ctypes.data for k, _ in capi.SocTrial._fields_ if k in arrays})
    o, so = capi.NlpStepOptions(), capi.SocOptions()
    for missing in ("what", "rho", "f_trial", "c_trial", "x_k", "c_k", "f_k", "infea_k", "delta", "x_trial", "soc"):
        keep = getattr(t, missing)
        setattr(t, missing, None)
        assert L.rsqp_batch_handler_soc_begin(b._h, C.addressof(t), C.addressof(o), C.addressof(so), 0) == capi.ERR_ARG, missing
        setattr(t, missing, keep)
    assert L.rsqp_batch_handler_soc_begin(b._h, C.addressof(t), None, C.addressof(so), 0) == capi.ERR_ARG
    assert L.rsqp_batch_handler_soc_begin(b._h, C.addressof(t), C.addressof(o), None, 0) == capi.ERR_ARG
    assert L.rsqp_batch_set_objective(b._h, None, None) == capi.ERR_ARG
    b.close()
    no_problem = capi.Batch([d["qp"] for d in members])
    qps = [copy.copy(d["qp"]) for d in members]
    for q in qps:
        q.H_jc = q.H_ir = q.H_val = None
    no_H = capi.Batch(qps)
    no_H.handler_set_problem(cat("x_l"), cat("x_u"), cat("c_l"), cat("c_u"))
    for bad in (no_problem, no_H):
        refused(lambda: bad.handler_soc_begin(S["what"], S["rho"], f_t, c_t, **it, grad=S["grad"], out=out))
        bad.close()
