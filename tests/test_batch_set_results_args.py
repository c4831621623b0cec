"""CPU-side checks of the verification entries of the batch certificate (include/rsqp_hip.h: rsqp_batch_set_results and the getter of
the mapped working sets, rsqp_batch_get_working_set): declared, exported, bound, and their argument checks answer before any device call. The behaviour itself needs a GPU:
tests/test_gpu_certificate.py."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_entry_point_is_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "rsqp_hip.h")).read()
    L = capi.lib()
    for name in ("rsqp_batch_set_results", "rsqp_batch_get_working_set"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert callable(capi.Batch.mapped_working_sets)
    assert list(inspect.signature(capi.Batch.set_results).parameters) == ["self", "x", "y", "ws_b", "ws_c"]
    assert callable(capi.Batch.certificates)
    # test_optimality keeps its signature
    assert list(inspect.signature(capi.Batch.test_optimality).parameters) == ["self"]
    assert capi.Batch.CERTIFICATE_FIELDS == tuple(name for name, _ in capi.OptimalityStatus._fields_)


def test_null_batch_is_an_argument_error(capi):
    L = capi.lib()
    v = np.zeros(4)
    w = np.zeros(4, np.int32)
    vp, wp = v.ctypes.data_as(capi.dp), w.ctypes.data_as(capi.ip)
    assert L.rsqp_batch_set_results(None, vp, vp, wp, wp) == capi.ERR_ARG
    assert L.rsqp_batch_set_results(None, None, None, None, None) == capi.ERR_ARG
    assert L.rsqp_batch_get_working_set(None, wp, wp) == capi.ERR_ARG
    assert L.rsqp_last_error()


def test_lengths_are_checked_by_the_binding(capi):
    """Batch.set_results refuses arrays of the wrong length before they reach the library (which would read past them)"""
    b = capi.Batch.__new__(capi.Batch)
    b._h = None
    b.nq = 2
    b.offV, b.offC = np.array([0, 3, 5]), np.array([0, 1, 1])
    good = dict(x=np.zeros(5), y=np.zeros(6), ws_b=np.zeros(5, np.int32), ws_c=np.zeros(1, np.int32))
    for name, bad in (("x", np.zeros(4)), ("y", np.zeros(5)), ("ws_b", np.zeros(6, np.int32)), ("ws_c", np.zeros(2, np.int32)),
                      ("x", np.zeros((5, 1)))):
        with pytest.raises(ValueError):
            b.set_results(**dict(good, **{name: bad}))
