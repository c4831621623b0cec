"""second_order_correction per member of a batch (include/rsqp_hip_soc.h: rsqp_soc_default_options, rsqp_batch_handler_soc_begin,
rsqp_batch_handler_soc_end, rsqp_batch_set_objective), the part that needs no GPU: the entry points are declared, exported and bound
through a table of their own, the structs of the binding are the header's, the defaults, the argument checks that need no batch answer before
any device call (those on a batch, soc_end before any soc_begin among them, need a device to create one and are in
tests/test_gpu_soc.py), and handler.batch_soc_reference over the C oracle takes every branch on the inputs of tests/soc_cases.py -- which is
asserted here, from that run alone, before tests/test_gpu_soc.py compares the kernels with it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soc_cases as SC
from abi_cases import assert_entry_points
from conftest import ROOT

NEW = ("rsqp_soc_default_options", "rsqp_batch_handler_soc_begin", "rsqp_batch_handler_soc_end", "rsqp_batch_set_objective")


def test_entry_points_are_declared_exported_and_bound(capi):
    # ... through a table of their own, and the struct layouts of the binding are the header's, field by field and in order
    header = assert_entry_points(capi, "rsqp_hip_soc.h", capi.SOC_SYMBOLS, NEW, structs=(
        ("rsqp_soc_options", capi.SocOptions), ("rsqp_soc_trial", capi.SocTrial)))
    for method in ("handler_soc_begin", "handler_soc_end", "set_objective"):
        assert callable(getattr(capi.Batch, method)), method
    # the header says which objective the second test reads, where H comes from, and what is saved and put back
    assert "THE CORRECTION QP'S OWN OBJECTIVE" in header and "composite_pred" in header and "READ IN PLACE" in header
    assert "ARE SAVED" in header and "ARE PUT BACK TO THE SAVED FIRST SOLVE'S" in header and "INSTEAD OF" in header
    assert (capi.SOC_TEST, capi.SOC_CORRECT) == (1, 2) and re.search(r"RSQP_SOC_TEST = 1, RSQP_SOC_CORRECT = 2", header)
    # the trial begins as rsqp_nlp_trial does
    nlp = [k for k, _ in capi.NlpTrial._fields_]
    assert [k for k, _ in capi.SocTrial._fields_][:len(nlp)] == nlp
    assert dict(capi.SocOptions._fields_)["composite_pred"] is C.c_int
    # the unit is built with the library, contraction off
    from restartsqp_amd import build
    assert "rsqp_batch_soc.hip" in build.SOURCES
    unit = open(os.path.join(ROOT, "restartsqp_amd", "csrc", "rsqp_batch_soc.hip")).read()
    assert "#pragma clang fp contract(off)" in unit


def test_default_options(capi):
    assert capi.SocOptions().as_dict() == dict(composite_pred=0)
    assert capi.SocOptions(composite_pred=1).composite_pred == 1
    with pytest.raises(TypeError):
        capi.SocOptions(refresh_ubA=1)            # a step option, not an SOC option
    assert capi.lib().rsqp_soc_default_options(None) == capi.ERR_ARG


def test_null_batch_and_null_pointers_are_argument_errors(capi):
    """RSQP_ERR_ARG before any device call: this machine may have no device at all"""
    L = capi.lib()
    v, w = np.zeros(4), np.ones(4, np.int32)
    o, so = capi.NlpStepOptions(), capi.SocOptions()
    t = capi.SocTrial(**{k: (w if k in capi.SocTrial.INTS else v).ctypes.data for k, _ in capi.SocTrial._fields_})
    for fn in (L.rsqp_batch_handler_soc_begin, L.rsqp_batch_handler_soc_end):
        for on_device in (0, 1):
            assert fn(None, C.addressof(t), C.addressof(o), C.addressof(so), on_device) == capi.ERR_ARG
        assert L.rsqp_last_error()
    assert L.rsqp_batch_set_objective(None, None, v.ctypes.data) == capi.ERR_ARG


def test_lengths_are_checked_by_the_binding(capi):
    """the binding refuses arrays of the wrong length, a missing required one and an iterate array it could not write in place,
    before they reach the library. Members (4, 2), (3, 1), (5, 0): 12 NLP entries, 3 constraint entries"""
    b = capi.Batch.__new__(capi.Batch)
    b.nq, b.nV, b.nC, b._h = 3, np.array([8, 5, 5], np.int32), np.array([2, 1, 0], np.int32), None
    nq, sN, sC = 3, 12, 3
    good = dict(what=np.ones(nq, np.int32), rho=np.ones(nq), f_trial=np.ones(nq), c_trial=np.ones(sC), x_k=np.ones(sN), c_k=np.ones(sC),
                f_k=np.ones(nq), infea_k=np.ones(nq), delta=np.ones(nq), grad=np.ones(sN))
    for k, bad in (("x_k", np.ones(sN + 1)), ("c_trial", np.ones(sC - 1)), ("rho", None), ("delta", [1.0, 1.0, 1.0]),
                   ("f_k", np.ones(nq, np.float32)), ("what", np.ones(nq + 1, np.int32)), ("grad", np.ones(sN - 1)),
                   ("infea_model", np.ones(nq + 2))):
        with pytest.raises(ValueError):
            b.handler_soc_begin(**dict(good, **{k: bad}))
    for bad_out in (dict(soc=np.zeros(nq)), dict(x_trial=np.zeros(nq)), dict(qp_obj=np.zeros(nq, np.float32))):
        with pytest.raises(ValueError):
            b.handler_soc_begin(**good, out=bad_out)
    end = {k: v for k, v in good.items() if k not in ("what", "grad")}
    with pytest.raises(ValueError):
        b.handler_soc_end(**end, out=None)                                            # soc is required
    with pytest.raises(ValueError):
        b.handler_soc_end(**dict(end, c_k=np.ones(sC + 1)), out=dict(soc=np.ones(nq, np.int32)))
    for bad in (np.ones(nq + 1), None):
        with pytest.raises(ValueError):
            b.set_objective(bad)
    with pytest.raises(ValueError):
        b.set_objective(np.ones(nq), members=[1, 0])


CASES = [(b, k) for b in ("hs071_gpu", "mixed") for k in SC.OPTION_SETS]


@pytest.mark.parametrize("batch,option_set", CASES)
def test_reference_over_the_oracle_takes_the_branches(capi, oracle, batch, option_set):
    """conditions on the INPUTS, from the oracle run alone: at least two members per branch the option set is meant for"""
    members, S, o, so, rows = SC.oracle_run(oracle, capi, batch, option_set)
    c = SC.census(rows)
    print(batch, option_set, dict(sorted(c.items())))
    SC.assert_margins(rows)
    nq = len(members)
    some = lambda *parts: sum(v for k, v in c.items() if all(p in k for p in parts))
    assert SC.lanes(members) == (8 if batch == "hs071_gpu" else 64) and nq == (70 if batch == "hs071_gpu" else 40)
    assert c["sits_out"] == int(np.sum(S["what"] == 0)) >= 2
    for r, w in zip(rows, S["what"]):
        if w == 0:
            assert r["exitflag"] is None and r["soc"] is None and r["x"] is None
        elif not w & capi.SOC_CORRECT:
            assert r["branch"] == "no_correct" and r["soc"] == 0 and r["nwsr_soc"] == 0
    # every option set: the word without CORRECT on both verdicts, accepted at once, corrected and rejected; the three radius branches
    assert some("no_correct_accepted") >= 2 and some("no_correct_rejected") >= 2
    assert sum(r["branch"] == "accepted" for r in rows) >= 2
    assert some("soc_rejected") >= 2
    assert some("_shrunk") >= 2 and some("_grown") >= 2 and some("_unchanged") >= 2
    # the members test (b) of tests/test_gpu_soc.py compares
    assert sum(SC.solved_throughout(r) for r in rows) >= nq // 2
    if option_set in ("default", "composite", "ubA") and (batch == "hs071_gpu" or option_set == "ubA"):
        assert some("soc_accepted") >= 2
    if option_set == "budget" or (batch == "hs071_gpu" and option_set == "default"):
        # (hs071, full budget: the reference leaves ubA stale, so the correction QP of an equality constraint is infeasible)
        assert c["soc_unsolved"] >= 2
        for r in rows:
            if r["branch"] == "soc_unsolved":
                assert r["exitflag"] not in (capi.EXIT_UNKNOWN, capi.QP_OPTIMAL, None) and r["soc"] == 0 and r["accept"] is None
    if option_set == "ubA":
        assert c["soc_unsolved"] <= 1
    if option_set == "delta_min":
        assert some("too_small") >= 2 and some("soc_rejected", "too_small") >= 2
        assert all((r["exitflag"] == capi.EXIT_TRUST_REGION_TOO_SMALL) == r["too_small"] for r in rows if r["radius"] is not None)
    else:
        assert some("too_small") == 0


def test_reference_rows_are_consistent(capi, oracle):
    """what a row must satisfy whatever the inputs"""
    for batch, option_set in CASES:
        members, S, o, so, rows = SC.oracle_run(oracle, capi, batch, option_set)
        n, m, offN, offC, offV = SC.offsets(members)
        accepted_hu = capi.HU_BOUNDS | capi.HU_GRAD | (capi.HU_UBA if o["refresh_ubA"] else 0)
        for q, (r, d) in enumerate(zip(rows, members)):
            tag = (batch, option_set, q)
            if r["branch"] in (None, "soc_unsolved"):
                # the iterate is untouched, delta included
                assert np.array_equal(r["x_k"], d["x_k"]) and r["delta"] == d["delta"] and r["f_k"] == S["f_k"][q], tag
                continue
            if r["accept"]:
                assert (r["hu_word"], r["hm_word"]) == (accepted_hu, capi.HM_JAC | capi.HM_HESS), tag
                assert np.array_equal(r["x_k"], d["x_k"] + r["x"][:d["n"]]), tag          # x_k moved by the step in the pool
            else:
                assert np.array_equal(r["x_k"], d["x_k"]) and r["hm_word"] == 0, tag
            if r["branch"] == "soc_rejected":
                assert r["hu_word"] == accepted_hu and r["qp_obj"] == r["obj"], tag       # update_grad + update_bounds, first objective
            if r["branch"] == "soc_accepted":
                assert r["soc"] == 1 and r["qp_obj"] != r["obj"], tag                     # the composite beside the correction's own
            assert {"shrunk": r["delta"] < d["delta"], "grown": r["delta"] > d["delta"], "unchanged": r["delta"] == d["delta"]}[r["radius"]], tag
