"""update_penalty_parameter per member of a batch (include/rsqp_hip_penalty.h: rsqp_penalty_default_options,
rsqp_batch_handler_pair_lp, rsqp_batch_handler_update_penalty), the part that needs no GPU: the entry points are declared, exported
and bound through a table of their own, the structs of the binding are the header's, the defaults are the reference's, the argument
checks answer before any device call, and handler.batch_update_penalty_reference over the C oracle takes every branch on the inputs
of tests/penalty_cases.py -- which is asserted here, from that run alone, before tests/test_gpu_penalty.py compares the kernels
with it."""
import ctypes as C
import os

import numpy as np
import pytest

import penalty_cases as PC
from abi_cases import assert_entry_points
from conftest import ROOT

NEW = ("rsqp_penalty_default_options", "rsqp_batch_handler_pair_lp", "rsqp_batch_handler_update_penalty")


def test_entry_points_are_declared_exported_and_bound(capi):
    # ... through a table of their own, and the struct layouts of the binding are the header's, field by field and in order
    header = assert_entry_points(capi, "rsqp_hip_penalty.h", capi.PENALTY_SYMBOLS, NEW, structs=(
        ("rsqp_penalty_options", capi.PenaltyOptions), ("rsqp_penalty_state", capi.PenaltyState)))
    for method in ("handler_pair_lp", "handler_update_penalty"):
        assert callable(getattr(capi.Batch, method)), method
    # the header says where J comes from, which layouts are refused, and what the failure path restores and what it leaves
    assert "READ IN PLACE" in header and "NON-CANONICAL LAYOUT" in header and "THE ASYMMETRY" in header
    assert "ARE PUT BACK TO THE FIRST SOLVE'S" in header
    types = dict(capi.PenaltyOptions._fields_)
    assert types["penalty_iter_max"] is C.c_int and all(t is C.c_double for k, t in types.items() if k != "penalty_iter_max")
    # the sentence of rsqp_hip_nlp_step.h about the penalty bit points at the call
    assert "rsqp_batch_handler_update_penalty" in open(os.path.join(ROOT, "include", "rsqp_hip_nlp_step.h")).read()


def test_default_options_are_the_reference_s(capi):
    """src/Options.cpp:43-52"""
    o = capi.PenaltyOptions()
    assert o.as_dict() == dict(penalty_update_tol=1.0e-8, increase_parm=10.0, rho_max=1.0e6, penalty_iter_max=200, eps1_change_parm=0.1,
                               eps2=1.0e-6)
    assert capi.PenaltyOptions(eps2=0.9, penalty_iter_max=0).as_dict()["penalty_iter_max"] == 0
    with pytest.raises(TypeError):
        capi.PenaltyOptions(eps1=0.1)          # per-member state, not an option
    assert capi.lib().rsqp_penalty_default_options(None) == capi.ERR_ARG


def test_null_batch_and_null_pointers_are_argument_errors(capi):
    """RSQP_ERR_ARG before any device call: this machine may have no device at all"""
    L = capi.lib()
    v, w = np.zeros(4), np.ones(4, np.int32)
    o = capi.PenaltyOptions()
    s = capi.PenaltyState(**{k: (w if k in capi.PenaltyState.INTS else v).ctypes.data for k, _ in capi.PenaltyState._fields_})
    for on_device in (0, 1):
        assert L.rsqp_batch_handler_update_penalty(None, C.addressof(s), C.addressof(o), on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_update_penalty(None, None, C.addressof(o), on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_update_penalty(None, C.addressof(s), None, on_device) == capi.ERR_ARG
    assert L.rsqp_batch_handler_pair_lp(None, None) == capi.ERR_ARG
    assert L.rsqp_last_error()


def test_lengths_are_checked_by_the_binding(capi):
    """the binding refuses arrays of the wrong length, a missing required one and a state array it could not write in place, before
    they reach the library. Members (4, 2), (3, 1), (5, 0): 12 NLP entries, 3 constraint entries"""
    b = capi.Batch.__new__(capi.Batch)
    b.nq, b.nV, b.nC, b._h = 3, np.array([8, 5, 5], np.int32), np.array([2, 1, 0], np.int32), None
    nq, sN, sC = 3, 12, 3
    good = dict(what=np.ones(nq, np.int32), infea_k=np.ones(nq), delta=np.ones(nq), x_k=np.ones(sN), c_k=np.ones(sC), rho=np.ones(nq),
                eps1=np.ones(nq), trial=np.zeros(nq, np.int32), succ=np.zeros(nq, np.int32), fail=np.zeros(nq, np.int32))
    for k, bad in (("x_k", np.ones(sN + 1)), ("c_k", np.ones(sC - 1)), ("infea_k", None), ("rho", [1.0, 1.0, 1.0]),
                   ("eps1", np.ones(nq, np.float32)), ("trial", np.zeros(nq, np.int64)), ("fail", None)):
        with pytest.raises(ValueError):
            b.handler_update_penalty(**dict(good, **{k: bad}))
    with pytest.raises(ValueError):
        b.handler_update_penalty(**good, out=dict(rounds=np.zeros(nq)))              # (not int32)


CASES = [(b, k) for b in ("hs071", "hs071_gpu", "mixed") for k in PC.OPTION_SETS]


@pytest.mark.parametrize("batch,option_set", CASES)
def test_reference_over_the_oracle_takes_the_branches(capi, oracle, batch, option_set):
    """conditions on the INPUTS, from the oracle run alone"""
    members, S, o, rows, first = PC.oracle_run(oracle, capi, batch, option_set)
    c = PC.census(rows)
    print(batch, option_set, dict(sorted(c.items())))
    PC.assert_margins(rows)
    nq = len(members)
    assert c["sits_out"] == int(np.sum(S["what"] == 0)) >= 2
    for r, st in zip(rows, S["what"]):
        if st == 0:
            assert r["exitflag"] is None and r["rounds"] == 0 and (r["trial"], r["succ"], r["fail"]) == (3, 2, 1)
    some = lambda prefix: sum(v for k, v in c.items() if k.startswith(prefix))
    if batch == "mixed":
        assert PC.lanes(members) == 64 and 35 <= nq <= 45
        assert c["nothing"] >= 2 and some("A_success") >= 2 and c["B_no_round"] >= 2
        if option_set not in ("rho_max", "budget"):
            assert max(r["rounds"] for r in rows) >= 3                 # several rounds in one call: the loop, not one step
        return
    assert PC.lanes(members) == 8 and nq == (400 if batch == "hs071" else 70)
    if option_set != "budget":
        # members with an unsolved QP, first solve or inside the loop: at most 1 in 6, so that the compared set stays large
        assert 2 <= c["qp_unsolved"] and 6 * (c["qp_unsolved"] + c["loop_qp_unsolved"]) <= nq
    assert c["lp_unsolved"] == 0                                        # (the LP of hs071 inside a box always solves)
    assert c["nothing"] >= 2 and c["B_no_round"] >= 2
    if option_set == "default":
        assert c["A_success_1"] >= 2 and c["A_success_2"] >= 2 and some("B_success") >= 2
        assert some("A_failure") + some("B_failure") == 0
    elif option_set == "eps2":
        assert some("A_failure") >= 2 and some("B_failure") >= 2
    elif option_set == "rho_max":
        assert sum(v for k, v in c.items() if k.endswith("_capped")) >= 2
        assert all(r["rho"] <= 10.0 or r["outcome"] is None for r in rows)
    elif option_set == "eps1":
        assert c["B_success_2"] >= 2
    elif option_set == "iter_max":
        assert some("B_success") + some("B_failure") == 0 and some("A_success") >= 2
    elif option_set == "budget":
        assert c["loop_qp_unsolved"] >= 2 and some("A_success") >= 2
        for r in rows:
            if r["broke"]:      # the stated deviation: the failure path, whatever :979 says
                assert (r["outcome"], r["hu_word"], r["exitflag"] != capi.EXIT_UNKNOWN) == ("failure", capi.HU_PENALTY, True)


def test_reference_rows_are_consistent(capi, oracle):
    """what a row must satisfy whatever the inputs: the counters move as the branches say, a success raises rho and eps1, a failure
    keeps both and puts the first solve back"""
    for option_set in PC.OPTION_SETS:
        members, S, o, rows, first = PC.oracle_run(oracle, capi, "hs071", option_set)
        for q, (r, d, f) in enumerate(zip(rows, members, first)):
            if r["branch"] in (None, "qp_unsolved"):
                assert (r["rho"], r["trial"], r["succ"], r["fail"], r["rounds"]) == (d["rho"], 3, 2, 1, 0)
                continue
            assert r["trial"] == 3 + r["rounds"] and r["succ"] + r["fail"] == 3 + (r["outcome"] is not None)
            if r["outcome"] == "success":
                assert r["rho"] > d["rho"] and r["eps1"] > S["eps1"][q] and r["hu_word"] == 0
            else:
                assert r["rho"] == d["rho"] and r["eps1"] == S["eps1"][q]
                assert np.array_equal(r["x"], f["x"]) and r["obj"] == f["obj"]
                assert r["hu_word"] == (capi.HU_PENALTY if r["outcome"] == "failure" else 0)
