"""Every instantiation of the small-QP kernels against the CPU oracle, asserted by name: the cases of tests/small_builds.py, at least one
per build, 31 builds.

A batch reports the plan of its last launch (Batch.last_plan, rsqp_batch_get_last_plan); each case states its switches, its batch and
the build it must reach, and FAILS when the launch reached another one -- a case that silently runs a neighbouring build is the gap
this file closes. The bar is the one of test_gpu_parity.py, on every member: status, nWSR and both working sets equal to the
oracle's, x and y within 1e-9 of max(1, |.|max) -- cold, after a hot start on new vectors and after one on new matrix values, with
the same build and the asked mode reported after each (a silent fall to cold would hide the build's state I/O). Members that turn
infeasible under the perturbation stay in. That the batches do work is asserted from the oracle's counts alone (no GPU needed).
Builds that differ only in their waves per SIMD must give the same bits."""
import json
import os

import numpy as np
import pytest

import small_builds as SB
from conftest import GOLDEN

RTOL = 1e-9
STAGES = ("cold", "hot_vectors", "hot_matrices")
FIELDS = ("x", "y", "obj", "nWSR", "status", "ws_b", "ws_c")
IDS = [c.name for c in SB.CASES]


def set_switches(monkeypatch, case):
    for k in SB.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------
def test_the_cases_and_the_golden_table_name_the_same_31_builds(capi):
    golden = json.load(open(os.path.join(GOLDEN, "small_launch_plans.json")))
    from_golden = {b for c in golden for b in capi.plan_builds(c["out"])}
    assert len(SB.BUILDS) == 31 and len({c.name for c in SB.CASES}) == len(SB.CASES)
    assert from_golden == set(SB.BUILDS)
    assert {k for c in golden for k in c["kernels"]} == {SB.kernel_name(b) for b in SB.BUILDS}


@pytest.mark.parametrize("case", SB.CASES, ids=IDS)
def test_the_plan_of_each_batch_is_its_build_and_the_oracle_works_on_it(capi, oracle, case):
    """the plan rsqp_batch_create's facts give (restated from the members, describe_small_launch) starts the build; at least 80 %
    of the members take two or more working-set changes cold, at least 40 % one or more in each hot start (oracle's counts)"""
    ref = SB.reference(oracle, case)
    probs = ref["cold"][0]
    assert case.build in capi.plan_builds(SB.predicted_plan(capi, case, probs))
    n = case.tile or len(probs)
    per_wave = {"qp": 64 // min(case.build[2], 64) if case.build[0] == "qp" else 1, "tiny": 32, "lane": 64}.get(case.build[0], 1)
    assert per_wave == 1 or n % per_wave != 0
    act = SB.activity(ref)
    print(case.name, {k: round(v, 2) for k, v in act.items()})
    assert act["cold"] >= SB.COLD_SHARE, act
    assert set(act) == set(STAGES if case.hot else STAGES[:1])
    for k in STAGES[1:]:
        assert not case.hot or act[k] >= SB.HOT_SHARE, act


# ------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------
def same_as_oracle(rec, r, tag):
    assert r["status"] == rec["status"], tag
    assert r["nWSR"] == rec["nWSR"], tag
    assert np.array_equal(r["ws_b"], rec["ws_b"]) and np.array_equal(r["ws_c"], rec["ws_c"]), tag
    assert np.abs(r["x"] - rec["x"]).max() <= RTOL * max(1.0, np.abs(rec["x"]).max()), tag
    assert np.abs(r["y"] - rec["y"]).max() <= RTOL * max(1.0, np.abs(rec["y"]).max()), tag


def same_bits(a, c, tag):
    for f in FIELDS:
        assert np.array_equal(np.asarray(a[f]), np.asarray(c[f])), tag + (f,)


def run_case(capi, oracle, monkeypatch, case, compare=True):
    """the case's batch through its stages -> {stage: results}; every stage's plan is the build and the asked mode"""
    ref = SB.reference(oracle, case)
    set_switches(monkeypatch, case)
    b = capi.Batch(case.members(ref["cold"][0]))
    if case.keep is not None:
        b.set_keep_state(case.keep)
    out = {}
    for stage, mode in zip(STAGES, (capi.MODE_COLD, capi.MODE_HOT_VECTORS, capi.MODE_HOT_MATRICES)):
        if stage not in ref:
            continue
        distinct, recs = ref[stage]
        probs = case.members(distinct)
        if stage != "cold":
            b.set_vectors_from(probs)
        if stage == "hot_matrices":
            b.set_matrix_values(np.concatenate([q.A_val for q in probs]), np.concatenate([q.H_val for q in probs]))
        b.solve(mode, 1000)
        plan = b.last_plan()
        builds = capi.plan_builds(plan)
        print(case.name, stage, "ran", builds, "mode", plan["mode"])
        if case.build[0] == "qpg" and stage == "hot_matrices":
            # (the plan's rule: the mid-size tableau kernel carries cold starts and hot starts on new vectors only)
            assert plan["first"] == 0 and len(builds) == 1 and builds[0][0] == "qp", (case.name, stage, builds)
        else:
            assert case.build in builds, (case.name, stage, builds)
        assert plan["mode"] == mode and b.last_kernel() == plan["family"], (case.name, stage, plan)
        res = b.results()
        assert len(res) == len(probs)
        if compare:
            nd = len(distinct)
            for k, r in enumerate(res):
                if k < nd:
                    same_as_oracle(recs[k], r, (case.name, stage, k, distinct[k].name))
                else:
                    same_bits(res[k % nd], r, (case.name, stage, k))       # a tiled copy: the bits of its first copy
        out[stage] = res
    b.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", SB.CASES, ids=IDS)
def test_build_matches_the_oracle(capi, oracle, monkeypatch, case):
    run_case(capi, oracle, monkeypatch, case)


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted({c.group for c in SB.CASES if c.group}))
def test_builds_that_differ_only_in_waves_give_the_same_bits(capi, oracle, monkeypatch, group):
    """the arithmetic order does not depend on the register budget: the same batch on the W builds of an engine, cold and
    hot -- x, y, objective, nWSR, status and working sets bit for bit"""
    cases = [c for c in SB.CASES if c.group == group]
    assert len(cases) >= 2 and len({c.build for c in cases}) == len(cases) and len({c.build[:4] + c.build[5:] for c in cases}) == 1
    runs = [run_case(capi, oracle, monkeypatch, c, compare=False) for c in cases]
    for c, run in zip(cases[1:], runs[1:]):
        for stage in STAGES:
            assert len(run[stage]) == len(runs[0][stage])
            for k, (a, r) in enumerate(zip(runs[0][stage], run[stage])):
                same_bits(a, r, (c.name, stage, k))


@pytest.mark.gpu
def test_last_plan_before_the_first_launch_and_with_wrong_arguments(capi):
    L = capi.lib()
    b = capi.Batch(SB.one_shape(1, 3))
    out = np.zeros(len(capi.SMALL_LAUNCH_OUT), np.int32)
    op = out.ctypes.data_as(capi.ip)
    assert L.rsqp_batch_get_last_plan(b._h, op, len(out)) == capi.ERR_ARG and b.last_kernel() == -1
    b.solve(capi.MODE_COLD, 1000)
    assert L.rsqp_batch_get_last_plan(b._h, None, len(out)) == capi.ERR_ARG
    assert L.rsqp_batch_get_last_plan(b._h, op, len(out) - 1) == capi.ERR_ARG
    assert L.rsqp_batch_get_last_plan(None, op, len(out)) == capi.ERR_ARG
    assert b.last_plan()["family"] == b.last_kernel() == 1
    b.close()
