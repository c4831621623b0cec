"""The decisions of a lock-step SQP loop per member of a batch (include/rsqp_hip_nlp_step.h: rsqp_batch_handler_infeasibility,
_ratio_test, _check_optimality, rsqp_nlp_step_default_options), the part that needs no GPU: the entry points are declared, exported
and bound through a table of their own, the argument checks answer before any device call, the default options are the reference's,
and the two numpy references of handler.py reproduce the decisions recorded in tests/golden/sqp_traces.json -- which pins them to
committed data before tests/test_gpu_nlp_step.py compares the kernels with them."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from abi_cases import assert_entry_points
from restartsqp_amd import handler, problems
from conftest import GOLDEN

NEW = ("rsqp_nlp_step_default_options", "rsqp_batch_handler_infeasibility", "rsqp_batch_handler_ratio_test",
       "rsqp_batch_handler_check_optimality")
NLPS = {"hs071": problems.hs071_nlp, "hs035": problems.hs035_nlp, "hs065": problems.hs065_nlp}


def test_entry_points_are_declared_exported_and_bound(capi):
    # ... through a table of their own, and the struct layouts of the binding are the header's, field by field and in order
    header = assert_entry_points(capi, "rsqp_hip_nlp_step.h", capi.NLP_STEP_SYMBOLS, NEW, structs=(
        ("rsqp_nlp_step_options", capi.NlpStepOptions), ("rsqp_nlp_trial", capi.NlpTrial), ("rsqp_nlp_point", capi.NlpPoint)))
    for method in ("handler_infeasibility", "handler_ratio_test", "handler_check_optimality"):
        assert callable(getattr(capi.Batch, method)), method
    # the header says where the Jacobian comes from and what is not built
    assert "READ IN PLACE" in header and "rsqp_batch_handler_set_matrices" in header and "W_constr_ / W_bounds_" in header
    assert (capi.EXIT_UNKNOWN, capi.EXIT_TRUST_REGION_TOO_SMALL) == (-99, 4)
    assert "#define RSQP_EXIT_UNKNOWN (-99)" in header and "#define RSQP_EXIT_TRUST_REGION_TOO_SMALL 4" in header
    assert "RSQP_KKT_PRIMAL = 1, RSQP_KKT_DUAL = 2, RSQP_KKT_COMPL = 4, RSQP_KKT_STAT = 8, RSQP_KKT_FIRST_ORDER_OPT = 16" in header


def test_default_options_are_the_reference_s(capi):
    """src/Options.cpp:28-42"""
    o = capi.NlpStepOptions()
    assert o.as_dict() == dict(active_set_tol=1.0e-5, opt_prim_fea_tol=1.0e-4, opt_dual_fea_tol=1.0e-4, opt_compl_tol=1.0e-4,
                               opt_stat_tol=1.0e-4, eta_s=1.0e-8, eta_c=0.25, eta_e=0.75, gamma_c=0.5, gamma_e=2.0, delta_min=1.0e-16,
                               delta_max=1.0e8, tol=1.0e-8, refresh_ubA=0)
    assert capi.NlpStepOptions(refresh_ubA=1, tol=1e-6).as_dict()["refresh_ubA"] == 1
    with pytest.raises(TypeError):
        capi.NlpStepOptions(eta=1.0)
    assert capi.lib().rsqp_nlp_step_default_options(None) == capi.ERR_ARG


def test_null_batch_and_null_pointers_are_argument_errors(capi):
    """RSQP_ERR_ARG before any device call: this machine may have no device at all"""
    L = capi.lib()
    v, w = np.zeros(4), np.ones(4, np.int32)
    o = capi.NlpStepOptions()
    t = capi.NlpTrial(*([w.ctypes.data] + [v.ctypes.data] * 11 + [w.ctypes.data] * 4))
    pt = capi.NlpPoint(w.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data, v.ctypes.data)
    for on_device in (0, 1):
        assert L.rsqp_batch_handler_infeasibility(None, v.ctypes.data, v.ctypes.data, on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_infeasibility(None, None, None, on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_ratio_test(None, C.addressof(t), C.addressof(o), on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_ratio_test(None, None, C.addressof(o), on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_ratio_test(None, C.addressof(t), None, on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_check_optimality(None, C.addressof(pt), C.addressof(o), v.ctypes.data, w.ctypes.data, on_device) == capi.ERR_ARG
        assert L.rsqp_batch_handler_check_optimality(None, None, None, None, None, on_device) == capi.ERR_ARG
    assert L.rsqp_last_error()


def test_lengths_are_checked_by_the_binding(capi):
    """the binding refuses arrays of the wrong length, a missing required one, and an in/out array it could not write in place,
    before they reach the library. Members (4, 2), (3, 1), (5, 0): 12 NLP entries, 3 constraint entries"""
    b = capi.Batch.__new__(capi.Batch)
    b.nq, b.nV, b.nC, b._h = 3, np.array([8, 5, 5], np.int32), np.array([2, 1, 0], np.int32), None
    nq, sN, sC = 3, 12, 3
    good = dict(what=np.ones(nq, np.int32), rho=np.ones(nq), f_trial=np.ones(nq), c_trial=np.ones(sC), x_k=np.ones(sN), c_k=np.ones(sC),
                f_k=np.ones(nq), infea_k=np.ones(nq), delta=np.ones(nq))
    for k, bad in (("x_k", np.ones(sN + 1)), ("c_trial", np.ones(sC - 1)), ("rho", None), ("delta", [1.0, 1.0, 1.0]),
                   ("f_k", np.ones(nq, np.float32)), ("c_k", np.ones(2 * sC)[::2])):
        with pytest.raises(ValueError):
            b.handler_ratio_test(**dict(good, **{k: bad}))
    with pytest.raises(ValueError):
        b.handler_ratio_test(**good, out=dict(accept=np.zeros(nq)))              # (not int32)
    pgood = dict(what=np.ones(nq, np.int32), x_k=np.ones(sN), grad=np.ones(sN), c_k=np.ones(sC), infea=np.ones(nq))
    for k, bad in (("grad", np.ones(sN - 1)), ("infea", None), ("c_k", np.ones(sC + 2))):
        with pytest.raises(ValueError):
            b.handler_check_optimality(**dict(pgood, **{k: bad}))
    with pytest.raises(ValueError):
        b.handler_check_optimality(**pgood, out=np.zeros((nq, 4)))
    with pytest.raises(ValueError):
        b.handler_infeasibility(np.ones(sC + 1))


def trace_entry(name, e):
    """the NLP at a trace entry's iterate, its step, and the NLP at the trial point"""
    nlp = NLPS[name](np.array(e["x"]), np.array(e["lam"]))
    n = nlp["info"].nVar
    p = np.array(e["x_qp"])[:n]
    return nlp, p, NLPS[name](nlp["x"] + p, np.array(e["lam"]))


def effective_flags(flags):
    """a trace entry's dirty flags as Algorithm::setupQP acts on them (src/Algorithm.cpp:672-695): update_bounds covers a changed
    radius, so `delta` counts only without `bounds`"""
    return dict(A=bool(flags["A"]), H=bool(flags["H"]), bounds=bool(flags["bounds"]), g=bool(flags["g"]),
                delta=bool(flags["delta"]) and not flags["bounds"])


def word_flags(capi, hu, hm):
    """the same flags read off the two words of a ratio test"""
    return dict(A=bool(hm & capi.HM_JAC), H=bool(hm & capi.HM_HESS), bounds=bool(hu & capi.HU_BOUNDS), g=bool(hu & capi.HU_GRAD),
                delta=bool(hu & capi.HU_DELTA))


@pytest.mark.parametrize("name,entries", [("hs071", 6), ("hs035", 3), ("hs065", 14)])
def test_ratio_test_reference_reproduces_the_traces(capi, name, entries):
    """every entry of a recorded run but the last: from its iterate, its delta and rho, the recorded step and QP objective, the
    reference gives the accept / reject, the delta and the dirty flags of the FOLLOWING entry, and on accept its iterate"""
    gold = json.load(open(os.path.join(GOLDEN, "sqp_traces.json")))[name]["qps"]
    assert len(gold) == entries
    o = capi.NlpStepOptions(refresh_ubA=1).as_dict()
    seen = set()
    for e, nxt in zip(gold[:-1], gold[1:]):
        assert nxt["rho"] == e["rho"] and not nxt["flags"]["penalty"]     # (no penalty update in these runs: every entry is a ratio test)
        nlp, p, trial = trace_entry(name, e)
        n, m = nlp["info"].nVar, nlp["info"].nCon
        infea = handler.cal_infea_reference(nlp["c"], nlp["c_l"], nlp["c_u"], handler.nlp_step_lanes([n], [m]))
        r = handler.batch_ratio_test_reference(o, [1], [e["rho"]], [trial["f"]], trial["c"], nlp["x"], nlp["c"], [nlp["f"]], [infea],
                                               [e["delta"]], p, [np.abs(p).max()], [e["obj"]], [n], [m], nlp["c_l"], nlp["c_u"])
        tag = (name, e["it"])
        assert bool(r["accept"][0]) == bool(nxt["flags"]["A"]), tag
        assert r["delta"][0] == nxt["delta"], tag
        assert word_flags(capi, int(r["hu_word"][0]), int(r["hm_word"][0])) == effective_flags(nxt["flags"]), tag
        assert bool(r["hu_word"][0] & capi.HU_UBA) == bool(r["accept"][0]), tag
        assert r["exitflag"][0] == capi.EXIT_UNKNOWN, tag
        x_next = r["x_k"] if r["accept"][0] else nlp["x"]
        assert np.array_equal(x_next, np.array(nxt["x"])), tag
        if r["accept"][0]:
            assert r["f_k"][0] == trial["f"] and np.array_equal(r["c_k"], trial["c"]) and r["infea_k"][0] == r["infea_trial"][0], tag
        seen.add((bool(r["accept"][0]), r["delta"][0] > e["delta"], r["delta"][0] < e["delta"]))
    if name == "hs065":
        assert seen == {(True, True, False), (True, False, False), (False, False, True)}      # accept + grow, accept, reject + shrink


def test_ratio_test_reference_branches_the_traces_do_not_take(capi):
    """an accepted step with pred < 0 (it cannot shrink the radius: eta_s * pred > eta_c * pred there), an accepted step that shrinks
    it (pred > 0, eta_s * pred <= actual < eta_c * pred), a rejected step that grows it, a rejected step with no radius change (two
    zero words), a radius below delta_min (exitflag 4), the cap at delta_max, and a member with word 0 -- one (2, 1) member each,
    c_l = 0, c_u = 1"""
    o = capi.NlpStepOptions().as_dict()
    nq = 7
    n, m = [2] * nq, [1] * nq
    c_l, c_u = np.zeros(nq), np.ones(nq)
    what = [1, 1, 1, 1, 0, 1, 1]
    # accept (pred < 0) | reject + shrink | too small | cap | sitter | reject + grow | accept + shrink
    f_k = np.array([0.0, 0.0, 0.0, 10.0, 0.0, 0.0, 1.0])
    f_t = np.array([0.0, 0.5, 5.0, 0.0, 0.0, 0.25, 0.875])
    obj = np.array([4.0, -1.0, -1.0, -10.0, 0.0, 2.0, -1.0])       # pred = -obj (infea_k = 0): -4, 1, 1, 10, ., -2, 1
    delta = np.array([1.0, 1.0, 1.5e-16, 9.0e7, 3.0, 1.0, 1.0])
    norm_p = np.array([1.0, 0.25, 1.5e-16, 9.0e7, 3.0, 1.0, 1.0])
    x_k, p = np.arange(2.0 * nq), np.full(2 * nq, 0.5)
    r = handler.batch_ratio_test_reference(o, what, np.ones(nq), f_t, np.full(nq, 0.5), x_k, np.full(nq, 0.25), f_k, np.zeros(nq), delta, p,
                                           norm_p, obj, n, m, c_l, c_u)
    assert r["accept"].tolist() == [1, 0, 0, 1, 0, 0, 1]
    # member 0: actual = 0 >= eta_s * (-4), 0 >= -tol: accepted; 0 < eta_c * (-4) is false, 0 > eta_e * (-4) and |delta - norm_p| = 0: grows
    assert r["delta"][0] == 2.0 and r["hu_word"][0] == capi.HU_BOUNDS | capi.HU_GRAD and r["hm_word"][0] == 3
    # member 1: actual = -0.5: rejected; -0.5 < 0.25 * 1: shrinks
    assert r["delta"][1] == 0.5 and (r["hu_word"][1], r["hm_word"][1]) == (capi.HU_DELTA, 0)
    assert r["delta"][2] == 0.75e-16 and r["exitflag"][2] == capi.EXIT_TRUST_REGION_TOO_SMALL and r["exitflag"][1] == capi.EXIT_UNKNOWN
    assert r["delta"][3] == 1.0e8 and r["accept"][3] == 1                   # min(gamma_e * delta, delta_max)
    assert r["delta"][4] == 3.0 and np.isnan(r["actual_reduction"][4]) and np.array_equal(r["x_k"][8:10], x_k[8:10])
    # member 5: pred = -2, actual = -0.25: rejected (< -tol), not below eta_c * pred = -0.5, above eta_e * pred, the step at the radius: grows
    assert r["accept"][5] == 0 and r["delta"][5] == 2.0 and (r["hu_word"][5], r["hm_word"][5]) == (capi.HU_DELTA, 0)
    # member 6: pred = 1, actual = 0.125: accepted, and below eta_c * pred: the radius shrinks under an accepted step
    assert r["accept"][6] == 1 and r["delta"][6] == 0.5 and (r["hu_word"][6], r["hm_word"][6]) == (capi.HU_BOUNDS | capi.HU_GRAD, 3)
    assert np.array_equal(r["x_k"][:2], x_k[:2] + 0.5) and np.array_equal(r["x_k"][2:4], x_k[2:4])
    # "QP is not changed": rejected, |delta - norm_p| >= tol keeps the radius -- pred < 0, actual between eta_c * pred and -tol
    r = handler.batch_ratio_test_reference(o, [1], [1.0], [1.0], [0.5], [0.0, 0.0], [0.5], [0.0], [0.0], [1.0], [0.1, 0.1], [0.1], [8.0],
                                           [2], [1], [0.0], [1.0])
    assert (r["accept"][0], r["hu_word"][0], r["hm_word"][0], r["delta"][0]) == (0, 0, 0, 1.0)


def test_classification_is_the_reference_s_as_written():
    """src/Utils.cpp:29-45, the quirk included"""
    c = handler.classify_single_constraint
    inf = np.inf
    assert c(0.0, 1.0) == handler.BOUNDED and c(1.0, 1.0 + 0.9e-8) == handler.EQUAL and c(1.0, 1.0) == handler.EQUAL
    assert c(-inf, inf) == handler.UNBOUNDED and c(-2e19, 2e19) == handler.UNBOUNDED and c(-1e18, 1e18) == handler.UNBOUNDED
    assert c(0.0, inf) == handler.BOUNDED_BELOW and c(0.0, 2e19) == handler.BOUNDED_BELOW
    assert c(-inf, 0.0) == handler.BOUNDED_ABOVE and c(-2e19, 0.0) == handler.BOUNDED_ABOVE
    assert c(0.0, 1e18) == handler.UNBOUNDED and c(-1e18, 0.0) == handler.UNBOUNDED        # the second and third branch test > INF, < -INF


@pytest.mark.parametrize("name,entries", [("hs071", 6), ("hs065", 14)])
def test_check_optimality_reference_on_the_traces(capi, name, entries):
    """the point the recorded run ends on, with the multipliers of the QP solved there, is first-order optimal (bit 16); the
    starting point with the multipliers of its QP is not"""
    gold = json.load(open(os.path.join(GOLDEN, "sqp_traces.json")))[name]["qps"]
    assert len(gold) == entries
    o = capi.NlpStepOptions().as_dict()
    verdicts = []
    for e in (gold[0], gold[-1]):
        nlp = NLPS[name](np.array(e["x"]), np.array(e["lam"]))
        n, m = nlp["info"].nVar, nlp["info"].nCon
        y = np.array(e["y_qp"])
        J = np.zeros((m, n))
        for r_, c_, v in zip(nlp["J"].RowIndex, nlp["J"].ColIndex, nlp["J"].MatVal):
            J[r_ - 1, c_ - 1] += v
        infea = handler.cal_infea_reference(nlp["c"], nlp["c_l"], nlp["c_u"], handler.nlp_step_lanes([n], [m]))
        st, v, scale = handler.batch_check_optimality_reference(o, [1], nlp["x"], nlp["grad"], nlp["c"], [infea], y[:n], y[n + 2 * m:], [J],
                                                                [n], [m], nlp["x_l"], nlp["x_u"], nlp["c_l"], nlp["c_u"])
        assert st[0, 4] == st[0, 1] + st[0, 0] + st[0, 2] + st[0, 3]
        verdicts.append(int(v[0]))
    assert not verdicts[0] & capi.KKT_FIRST_ORDER_OPT and verdicts[1] == 31, verdicts


def test_tree_sum_is_the_order_the_header_states():
    rng = np.random.default_rng(5)
    t = rng.normal(size=19) * 10.0 ** rng.integers(-8, 8, 19)
    lanes = [np.float64(0.0)] * 8
    for i, v in enumerate(t):
        lanes[i % 8] = lanes[i % 8] + v
    a = [lanes[l] + lanes[l ^ 4] for l in range(8)]
    a = [a[l] + a[l ^ 2] for l in range(8)]
    assert handler.tree_sum(t, 8) == a[0] + a[1]
    assert handler.tree_sum([], 64) == 0.0 and handler.tree_sum([3.0], 64) == 3.0
    assert handler.nlp_step_lanes([4, 3], [2, 1]) == 8 and handler.nlp_step_lanes([4, 5], [2, 35]) == 64 and handler.nlp_step_lanes([11], [2]) == 64
