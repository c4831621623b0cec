"""CPU-side checks of the per-member entry points of a batch (include/rsqp_hip.h: rsqp_batch_set_members,
rsqp_batch_set_matrix_values_of, rsqp_batch_set_vectors_of): declared, exported, bound, and their argument checks answer before any
device call. The behaviour itself needs a GPU: tests/test_gpu_batch_members.py."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rsqp_batch_set_members", "rsqp_batch_set_matrix_values_of", "rsqp_batch_set_vectors_of")


def test_entry_points_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "rsqp_hip.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert callable(capi.Batch.set_members)
    import inspect
    for method in ("set_matrix_values", "set_vectors", "set_vectors_from"):
        assert "members" in inspect.signature(getattr(capi.Batch, method)).parameters, method


def test_null_batch_is_an_argument_error(capi):
    L = capi.lib()
    m = np.ones(4, np.int32)
    v = np.zeros(4)
    mp, vp = m.ctypes.data_as(capi.ip), v.ctypes.data_as(capi.dp)
    assert L.rsqp_batch_set_members(None, mp) == capi.ERR_ARG
    assert L.rsqp_batch_set_members(None, None) == capi.ERR_ARG
    assert L.rsqp_batch_set_matrix_values_of(None, mp, vp, vp) == capi.ERR_ARG
    assert L.rsqp_batch_set_matrix_values_of(None, None, None, None) == capi.ERR_ARG
    assert L.rsqp_batch_set_vectors_of(None, mp, vp, vp, vp, vp, vp) == capi.ERR_ARG
    assert L.rsqp_batch_set_vectors_of(None, None, vp, vp, vp, vp, vp) == capi.ERR_ARG
    assert L.rsqp_last_error()


def test_mask_lengths_are_checked_by_the_binding(capi):
    """Batch.set_members and the `members` arguments refuse masks of the wrong length before they reach the library (which would
    read past them)"""
    b = capi.Batch.__new__(capi.Batch)
    b._h = None
    b.nq = 3
    v = np.zeros(6)
    for bad in (np.ones(2, np.int32), np.ones(4, np.int32), np.ones((3, 1), np.int32)):
        with pytest.raises(ValueError):
            b.set_members(bad)
        with pytest.raises(ValueError):
            b.set_matrix_values(v, v, members=bad)
        with pytest.raises(ValueError):
            b.set_vectors(v, v, v, v, v, members=bad)
