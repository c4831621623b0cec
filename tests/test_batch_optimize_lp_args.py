"""CPU-side checks of optimizeLP per member of a batch (include/rsqp_hip.h: rsqp_batch_optimize_lp, rsqp_batch_set_lp_options):
declared, exported, bound, their argument checks answer before any device call -- and the conditions on the INPUTS of
tests/test_gpu_batch_optimize_lp.py, checked on the CPU oracle alone so that they hold wherever the CPU suite runs."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import lp_batch_ref as R

NEW = ("rsqp_batch_optimize_lp", "rsqp_batch_set_lp_options")


def test_entry_points_are_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "rsqp_hip.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert callable(getattr(capi.Batch, "optimize_lp"))
    # the header says which kernels an LP call runs on
    doc = header[header.index("int rsqp_batch_set_lp_options"):header.index("int rsqp_batch_optimize_lp")]
    assert "null-space kernels" in doc and "never" in doc and "tableau" in doc


def test_null_batch_and_negative_budget_are_argument_errors(capi):
    L = capi.lib()
    used = np.zeros(4, np.int32)
    assert L.rsqp_batch_optimize_lp(None, used.ctypes.data_as(capi.ip)) == capi.ERR_ARG
    assert L.rsqp_batch_optimize_lp(None, None) == capi.ERR_ARG
    assert L.rsqp_batch_set_lp_options(None, 100) == capi.ERR_ARG
    assert L.rsqp_last_error()
    # (a negative budget is refused whatever the batch is: the check needs no device)
    assert L.rsqp_batch_set_lp_options(None, -1) == capi.ERR_ARG
    # lp_maxiter has a setter of its own: rsqp_batch_set_options keeps its two arguments
    assert L.rsqp_batch_set_options(None, 1000) == capi.ERR_ARG
    assert capi.SYMBOLS["rsqp_batch_set_options"][1] == [capi.C.c_void_p, capi.C.c_int]


def test_set_options_forwards_lp_maxiter_only_when_given(capi, monkeypatch):
    """Batch.set_options(qp_maxiter) is unchanged; the keyword lp_maxiter calls rsqp_batch_set_lp_options"""
    calls = []

    class Lib:
        def rsqp_batch_set_options(self, h, n):
            calls.append(("qp", n)); return 0

        def rsqp_batch_set_lp_options(self, h, n):
            calls.append(("lp", n)); return 0

    monkeypatch.setattr(capi, "lib", lambda: Lib())
    b = capi.Batch.__new__(capi.Batch)
    b._h = None
    b.set_options(500)
    b.set_options(qp_maxiter=20, lp_maxiter=16)
    b.set_options(lp_maxiter=70)
    assert calls == [("qp", 500), ("qp", 20), ("lp", 16), ("qp", 1000), ("lp", 70)]


@pytest.mark.parametrize("name", sorted(R.BATCHES))
def test_inputs_cover_the_branches_on_the_oracle(oracle, name):
    """LPRef over the CPU oracle on the three six-step sequences: within single calls cold, hot-vectors, hot-matrices and
    flip-to-plain-init members side by side, rescues from scratch after a cold start and after a flip, the slack-point rescue, members
    that stay unsolved; every solved member sits on a vertex; the per-step sums of nWSR_used are the pinned ones"""
    steps, budget, sums, ora = R.oracle_run(oracle, name)
    assert len(ora) == len(R.STEP_KIND) == 6 and all(len(rows) == len(steps[0]) for rows in ora)
    R.assert_inputs_cover_the_branches(name, sums, ora)


def test_one_pattern_members_share_one_pattern():
    first, second = R.one_pattern_members()
    assert len(first) == 70 and all((q.nV, q.nC) == (8, 2) for q in first + second)
    assert all(np.array_equal(q.A_jc, first[0].A_jc) and np.array_equal(q.A_ir, first[0].A_ir) for q in first + second)
