"""CPU-side checks of the hand-over switch of a batch (include/rsqp_hip_handover.h, which include/rsqp_hip.h includes:
rsqp_batch_set_handover, rsqp_batch_get_handover): declared, exported, bound, their argument checks answer before any device
call; and the generator of the members the register-resident tableau kernels give up on (problems.stiff_free_batch), against the
CPU oracle. The behaviour itself needs a GPU:
tests/test_gpu_batch_handover.py."""
import copy
import inspect

import numpy as np
import pytest

from abi_cases import assert_entry_points
from conftest import oracle_cold
from restartsqp_amd import problems

NEW = ("rsqp_batch_set_handover", "rsqp_batch_get_handover")
# the shapes and seeds of the GPU tests: (8, 2) / (7, 4) / (8, 8) are the three MC builds of the 8-lane tableau kernel, (8, 2) / (4, 1)
# / (2, 0) what the lane-per-problem kernel takes
SHAPES = [(8, 2), (4, 1), (2, 0), (8, 8), (7, 4)]


def stiff_batch(nV, nC, n=100, every=3):
    return problems.stiff_free_batch(np.random.default_rng(5000 + 10 * nV + nC), nV, nC, n, every=every)


def test_entry_points_are_declared_exported_and_bound(capi):
    # the two entry points are declared in an extension header of their own, which rsqp_hip.h includes (one include declares the
    # whole C ABI), and bound through a table of their own: header and table name the same entry points, as rsqp_hip.h and
    # capi.SYMBOLS do
    assert_entry_points(capi, "rsqp_hip_handover.h", capi.HANDOVER_SYMBOLS, NEW)
    assert callable(capi.Batch.set_handover) and callable(capi.Batch.handover)
    from restartsqp_amd import handler
    par = inspect.signature(handler.BatchQPhandler.__init__).parameters
    assert "handover" in par and par["handover"].default is False


def test_null_batch_is_an_argument_error(capi):
    L = capi.lib()
    h = np.zeros(4, np.int32)
    import ctypes as C
    n = C.c_int(7)
    assert L.rsqp_batch_set_handover(None, 1) == capi.ERR_ARG
    assert L.rsqp_batch_set_handover(None, 0) == capi.ERR_ARG
    assert L.rsqp_batch_get_handover(None, h.ctypes.data_as(capi.ip), C.byref(n)) == capi.ERR_ARG
    assert L.rsqp_batch_get_handover(None, None, None) == capi.ERR_ARG
    assert L.rsqp_last_error()
    assert n.value == 7 and not h.any()


def test_a_handed_array_of_the_wrong_length_is_refused_by_the_binding(capi):
    """Batch.handover(handed=...) refuses an array the library would write past (or one it would fill with another type's bytes)
    before it reaches the library"""
    b = capi.Batch.__new__(capi.Batch)
    b._h = None
    b.nq = 3
    for bad in (np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros((3, 1), np.int32), np.zeros(3, np.int64), np.zeros(3), [0, 0, 0],
                np.zeros(6, np.int32)[::2]):
        with pytest.raises(ValueError):
            b.handover(bad)


@pytest.mark.parametrize("shape", SHAPES)
def test_generator_members_are_well_conditioned_for_the_oracle(oracle, shape):
    """Every member solved (status 20). A stiff member has H[0, 0] <= 1e-9 max diag(H) -- below the 1e-8 hscale the tableau kernels
    ask of a free variable -- and the oracle solves it exactly as it solves the same member with H[j, j] = 1: x, both working sets
    and nWSR identical, bit for bit (variable j never enters a factorisation)."""
    nV, nC = shape
    j = nV - 1
    probs = stiff_batch(nV, nC)
    assert len(probs) == 100
    base = probs[0]
    stiff = 0
    for t, q in enumerate(probs):
        assert np.array_equal(q.H_jc, base.H_jc) and np.array_equal(q.H_ir, base.H_ir)           # one pattern
        assert np.array_equal(q.A_jc, base.A_jc) and np.array_equal(q.A_ir, base.A_ir)
        assert q.lb[j] == 0.0 and q.ub[j] == 1.0 and q.g[j] == 100.0
        H = q.dense_H()
        assert np.array_equal(H, H.T) and not H[j, :j].any()
        qp, rc, n = oracle_cold(oracle, q)
        assert rc == 0 and qp.exitflag() == 20, (shape, t, qp.exitflag())
        if t % 3:
            assert H[j, j] == 1.0 and np.isfinite(q.lb[0]) and np.isfinite(q.ub[0])
            continue
        stiff += 1
        assert q.lb[0] == -np.inf and q.ub[0] == np.inf
        assert H[j, j] == 1.0e10 and H[0, 0] <= 1e-9 * np.diag(H).max()
        assert qp.ws_bounds[0] == 0 and qp.ws_bounds[j] == -1                                   # variable 0 free, j on its lower bound
        mild = copy.deepcopy(q)
        mild.H_val[-1] = 1.0
        assert mild.dense_H()[j, j] == 1.0
        qm, rcm, nm = oracle_cold(oracle, mild)
        assert rcm == 0 and nm == n
        assert np.array_equal(qm.x, qp.x)
        assert np.array_equal(qm.ws_bounds, qp.ws_bounds) and np.array_equal(qm.ws_constraints, qp.ws_constraints)
    assert stiff == 34
