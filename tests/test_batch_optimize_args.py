"""CPU-side checks of the batch optimizeQP entry points (include/rsqp_hip.h: rsqp_batch_set_warm_start, rsqp_batch_set_options,
rsqp_batch_optimize_qp, rsqp_batch_get_dispatch): declared, exported, bound, and their argument checks answer before any device
call. The behaviour itself needs a GPU: tests/test_gpu_batch_optimize.py."""
import os
import re

import numpy as np

from conftest import ROOT

NEW = ("rsqp_batch_set_warm_start", "rsqp_batch_set_options", "rsqp_batch_optimize_qp", "rsqp_batch_get_dispatch")


def test_entry_points_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "rsqp_hip.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    for method in ("set_warm_start", "set_options", "optimize_qp", "dispatch"):
        assert callable(getattr(capi.Batch, method))
    # the header no longer excludes the re-initialisation from batches
    assert "WARM_REINIT not available" not in header


def test_null_batch_is_an_argument_error(capi):
    L = capi.lib()
    used = np.zeros(4, np.int32)
    assert L.rsqp_batch_set_warm_start(None, None, None, None) == capi.ERR_ARG
    assert L.rsqp_batch_set_options(None, 1000) == capi.ERR_ARG
    assert L.rsqp_batch_optimize_qp(None, used.ctypes.data_as(capi.ip)) == capi.ERR_ARG
    assert L.rsqp_batch_get_dispatch(None, None, None) == capi.ERR_ARG
    assert L.rsqp_last_error()
    # rsqp_batch_solve takes the fourth call shape now, and still refuses what is none
    assert L.rsqp_batch_solve(None, capi.MODE_WARM_REINIT, 10) == capi.ERR_ARG


def test_warm_start_sizes_are_checked_by_the_binding(capi):
    """Batch.set_warm_start refuses pooled arrays of the wrong length before they reach the library (which would read past them)"""
    import pytest
    b = capi.Batch.__new__(capi.Batch)
    b._h = None
    b.offV = np.array([0, 4, 9]); b.offC = np.array([0, 2, 3])
    for kw in (dict(x0=np.zeros(8)), dict(y0=np.zeros(9)), dict(guess_b=np.zeros(10, np.int32))):
        with pytest.raises(ValueError):
            b.set_warm_start(**kw)
