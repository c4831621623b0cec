"""CPU-side checks of the matrix half of the QPhandler layer of a batch (include/rsqp_hip.h: rsqp_batch_handler_set_matrices,
rsqp_batch_get_matrix_values): declared, exported, bound, their argument checks answer before any device call, and
handler.batch_matrices_reference -- the expected value of tests/test_gpu_batch_handler_matrices.py -- is the rule QPhandler states:
fed with the J and H values of the next recorded SQP iterate it turns the pools of problems.handler_qp at one iterate into those at
the next, byte for byte, in the layout that stores every entry of A and H."""
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from restartsqp_amd import problems
from restartsqp_amd.handler import batch_matrices_reference
from restartsqp_amd.qpdump import QPData

NEW = ("rsqp_batch_handler_set_matrices", "rsqp_batch_get_matrix_values")
NLPS = {"hs071": problems.hs071_nlp, "hs035": problems.hs035_nlp, "hs065": problems.hs065_nlp}


def test_entry_points_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "rsqp_hip.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    for bit, value in (("JAC", 1), ("HESS", 2)):
        assert re.search(r"\bRSQP_HM_%s\s*=\s*%d\b" % (bit, value), header), bit
        assert getattr(capi, "HM_" + bit) == value
    for method in ("handler_set_matrices", "get_matrix_values"):
        assert callable(getattr(capi.Batch, method)), method


def test_null_batch_is_an_argument_error(capi):
    L = capi.lib()
    v = np.zeros(4)
    w = np.ones(4, np.int32)
    for on_device in (0, 1):
        assert L.rsqp_batch_handler_set_matrices(None, w.ctypes.data, v.ctypes.data, v.ctypes.data, on_device) == capi.ERR_ARG
        assert L.rsqp_last_error()
        assert L.rsqp_batch_handler_set_matrices(None, None, None, None, on_device) == capi.ERR_ARG
    assert L.rsqp_batch_get_matrix_values(None, v.ctypes.data_as(capi.dp), v.ctypes.data_as(capi.dp)) == capi.ERR_ARG
    assert L.rsqp_batch_get_matrix_values(None, None, None) == capi.ERR_ARG
    assert L.rsqp_last_error()


def test_lengths_are_checked_by_the_binding(capi):
    """Batch.handler_set_matrices refuses arrays of the wrong length, and a missing one that a word names, before it reaches the
    library (which would read past them). Members (4,2), (3,1), (5,0) with 6, 2 and 0 entries in J and 4, 3 and 5 in H"""
    b = capi.Batch.__new__(capi.Batch)
    b._h = None
    b.nq = 3
    b.nV = np.array([8, 5, 5], np.int32); b.nC = np.array([2, 1, 0], np.int32)
    b.jnz = np.array([6, 2, 0]); b.annz = np.array([10, 4, 0]); b.hnnz = np.array([4, 3, 5])
    J, H = capi.HM_JAC, capi.HM_HESS
    w, jac, hess = np.array([J | H, J, H], np.int32), np.zeros(8), np.zeros(12)
    for bad in (np.zeros(7), np.zeros(9), np.zeros((8, 1))):
        with pytest.raises(ValueError):
            b.handler_set_matrices(w, bad, hess)
    for bad in (np.zeros(11), np.zeros(13)):
        with pytest.raises(ValueError):
            b.handler_set_matrices(w, jac, bad)
    for bad in (np.zeros(2, np.int32), np.zeros(4, np.int32)):
        with pytest.raises(ValueError):
            b.handler_set_matrices(bad, jac, hess)
    with pytest.raises(ValueError):
        b.handler_set_matrices(None, jac, hess)
    with pytest.raises(ValueError):
        b.handler_set_matrices(w, None, hess)           # a word has JAC
    with pytest.raises(ValueError):
        b.handler_set_matrices(w, jac, None)            # a word has HESS and the batch has an H
    with pytest.raises(ValueError):
        b.handler_set_matrices([0, 0, H], jac, None)


def full_pattern(q):
    """tests/test_gpu_batch_members.py::full_pattern (a GPU test module: restated): every entry of A and H stored"""
    def full(M):
        nr, nc = M.shape
        return (np.arange(nc + 1, dtype=np.int32) * nr, np.tile(np.arange(nr, dtype=np.int32), nc),
                np.ascontiguousarray(M.flatten(order="F"), dtype=np.float64))
    return QPData(q.nV, q.nC, *full(q.dense_H()), *full(q.dense_A()), q.g, q.lb, q.ub, q.lbA, q.ubA, name=q.name)


def nlp_entries(q, n, m):
    """the J and the H_k entries of a full-pattern QP: columns [0, n) of A; H has the layout of the QP's H"""
    return q.A_val[:n * m].copy(), q.H_val.copy()


@pytest.mark.parametrize("name,entries", [("hs071", 6), ("hs035", 3), ("hs065", 14)])
def test_reference_reproduces_handler_qp_along_the_traces(capi, name, entries):
    """the pools of trace entry k, the J / H values of entry k + 1 and the word JAC | HESS give the A_val / H_val of entry k + 1 byte
    for byte; with JAC or HESS alone the other pool keeps the bytes of entry k; with 0 both do. The slack columns are stored densely
    here, zeros included, and are never among the entries the reference takes: they come out as problems.handler_qp builds them"""
    gold = json.load(open(os.path.join(GOLDEN, "sqp_traces.json")))[name]["qps"]
    assert len(gold) == entries
    qps = [full_pattern(problems.handler_qp(NLPS[name](np.array(g["x"]), np.array(g["lam"])), g["delta"], g["rho"], name=name)) for g in gold]
    n, m = NLPS[name]()["info"].nVar, NLPS[name]()["info"].nCon
    J, H = capi.HM_JAC, capi.HM_HESS
    moved = 0
    for a, c in zip(qps[:-1], qps[1:]):
        jac, hess = nlp_entries(c, n, m)
        arg = ([a.nV], [a.nC], [a.A_jc], [a.H_jc])
        A2, H2 = batch_matrices_reference(a.A_val, a.H_val, [J | H], jac, hess, *arg)
        assert A2.tobytes() == c.A_val.tobytes() and H2.tobytes() == c.H_val.tobytes(), name
        moved += A2.tobytes() != a.A_val.tobytes() or H2.tobytes() != a.H_val.tobytes()
        A2, H2 = batch_matrices_reference(a.A_val, a.H_val, [J], jac, np.full(hess.shape, np.nan), *arg)
        assert A2.tobytes() == c.A_val.tobytes() and H2.tobytes() == a.H_val.tobytes(), name
        A2, H2 = batch_matrices_reference(a.A_val, a.H_val, [H], np.full(jac.shape, np.nan), hess, *arg)
        assert A2.tobytes() == a.A_val.tobytes() and H2.tobytes() == c.H_val.tobytes(), name
        A2, H2 = batch_matrices_reference(a.A_val, a.H_val, [0], np.full(jac.shape, np.nan), np.full(hess.shape, np.nan), *arg)
        assert A2.tobytes() == a.A_val.tobytes() and H2.tobytes() == a.H_val.tobytes(), name
        A2, H2 = batch_matrices_reference(a.A_val, None, [J | H], jac, None, [a.nV], [a.nC], [a.A_jc])
        assert A2.tobytes() == c.A_val.tobytes() and H2 is None, name      # a batch without H ignores HESS
    # (condition on the input: the trajectory has steps that change a matrix -- hs035 is a QP itself, its J and H are constant)
    assert moved >= 1 or name == "hs035"


def test_reference_on_two_members_with_sparse_patterns(capi):
    """two members with patterns of their own, (3, 1) with an empty first column of J and (2, 2) with one slack column stored with
    an explicit zero: every member owns its share of jac and hess whatever its word says"""
    J, H = capi.HM_JAC, capi.HM_HESS
    Ajc = [np.array([0, 0, 1, 2, 3, 4]), np.array([0, 2, 3, 5, 6, 7, 8])]
    Hjc = [np.array([0, 1, 2, 3, 3, 3]), np.array([0, 2, 4, 4, 4, 4, 4])]
    A, Hv = np.arange(1.0, 13.0), np.arange(21.0, 28.0)
    jac, hess = -np.arange(1.0, 6.0), -np.arange(21.0, 28.0)
    A2, H2 = batch_matrices_reference(A, Hv, [H, J], jac, hess, [5, 6], [1, 2], Ajc, Hjc)
    assert np.array_equal(A2, [1, 2, 3, 4, -3, -4, -5, 8, 9, 10, 11, 12])
    assert np.array_equal(H2, [-21, -22, -23, 24, 25, 26, 27])
    A2, H2 = batch_matrices_reference(A, Hv, [J, H], jac, hess, [5, 6], [1, 2], Ajc, Hjc)
    assert np.array_equal(A2, [-1, -2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12])
    assert np.array_equal(H2, [21, 22, 23, -24, -25, -26, -27])
