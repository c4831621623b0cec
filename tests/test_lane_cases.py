"""tests/lane_cases.py's assert helpers, which the test files of the lane-per-problem kernel lean on, must not be vacuous: each one
raises on the smallest difference it is there to catch and passes on what it should let through. Hand-made results of one 3 x 1
member; no GPU. The unambiguity check runs the oracle on QPs of three variables."""
import copy

import numpy as np
import pytest

import lane_cases as LC
from conftest import oracle_cold
from restartsqp_amd import problems
from restartsqp_amd.qpdump import QPData, dense_to_csc


def result():
    return dict(x=np.array([1.0, -2.0, 0.5]), y=np.array([0.0, 3.0, 0.0, -1.5]), ws_b=np.array([0, -1, 0], np.int32),
                ws_c=np.array([1], np.int32), status=20, nWSR=3, obj=-7.25)


class Answer:
    """what assert_same_solution and the objective bar read of an OracleQP"""

    def __init__(self, r):
        self.x, self.y, self.ws_bounds, self.ws_constraints, self.objective, self.status = r["x"], r["y"], r["ws_b"], r["ws_c"], r["obj"], r["status"]

    def exitflag(self):
        return self.status


def changed(**how):
    """result() with fields replaced, or (field, index) entries moved by a relative amount / set to a value"""
    r = copy.deepcopy(result())
    for f, v in how.items():
        if isinstance(v, tuple):
            i, rel = v
            r[f][i] = r[f][i] * (1.0 + rel) if r[f].dtype.kind == "f" else rel
        else:
            r[f] = v
    return r


def last_bit(v):
    return float(np.nextafter(v, np.inf))


def test_same_bits_raises_on_a_last_bit_and_passes_on_copies():
    r = result()
    LC.assert_same_bits(r, copy.deepcopy(r))
    LC.assert_same_bits([r, r], [copy.deepcopy(r), copy.deepcopy(r)])
    x = r["x"].copy(); x[1] = last_bit(x[1])
    for other in (changed(x=x), changed(ws_c=np.array([2], np.int32)), changed(nWSR=4), changed(obj=last_bit(r["obj"]))):
        with pytest.raises(AssertionError):
            LC.assert_same_bits(r, other)
        with pytest.raises(AssertionError):
            LC.assert_same_bits([r, r], [copy.deepcopy(r), other])            # (the second of a list is looked at too)
    with pytest.raises(AssertionError):
        LC.assert_same_bits([r, r], [r])


def test_the_oracle_bar_is_1e_9_relative_on_x_and_the_objective_and_exact_on_the_working_sets():
    r = result()
    qp = Answer(r)
    LC.assert_oracle_answer(qp, copy.deepcopy(r), 3)
    LC.assert_oracle_answer(qp, changed(x=(1, 1e-10), obj=r["obj"] * (1.0 + 1e-10)), 3)
    for other in (changed(x=(1, 1e-8)), changed(y=(1, 1e-8)), changed(obj=r["obj"] * (1.0 + 1e-8)), changed(ws_b=(0, 1)), changed(ws_c=(0, -1)),
                  changed(nWSR=2), changed(status=0)):
        with pytest.raises(AssertionError):
            LC.assert_oracle_answer(qp, other, 3)
    unsolved = changed(status=-2)
    with pytest.raises(AssertionError):                     # (the bar is for members the oracle solves)
        LC.assert_oracle_answer(Answer(unsolved), unsolved, 3)


def test_the_eight_lane_agreement_is_exact_on_the_path_and_1e_9_on_x_and_y():
    r = result()
    LC.assert_eight_lane_agreement(r, copy.deepcopy(r))
    LC.assert_eight_lane_agreement(r, changed(x=(0, 1e-10), y=(3, 1e-10)))
    for other in (changed(status=0), changed(y=(1, 1e-8)), changed(x=(1, 1e-8)), changed(nWSR=4), changed(ws_b=(2, -1)), changed(ws_c=(0, 0))):
        with pytest.raises(AssertionError):
            LC.assert_eight_lane_agreement(r, other)


def qp3(g, lb, ub, A, lbA, ubA):
    """min x'x / 2 + g'x over three variables"""
    A = np.atleast_2d(np.array(A, float))
    return QPData(3, A.shape[0], *dense_to_csc(np.eye(3)), *dense_to_csc(A), *(np.array(v, float) for v in (g, lb, ub, lbA, ubA)), name="qp3")


def unambiguous(oracle, q):
    LC.assert_unambiguous(oracle, q, *oracle_cold(oracle, q), np.random.default_rng(1), q.name)


def test_the_unambiguity_check_raises_on_a_tie_and_on_a_zero_multiplier(oracle):
    inf, row = np.inf, [1.0, 1.0, 1.0]
    unambiguous(oracle, problems.hs071_first_qp())
    unambiguous(oracle, qp3([-1, -2, -3], [-5] * 3, [5] * 3, [row], [-9], [3]))
    # free variables, the constraint x_0 + x_1 + x_2 <= 3 twice: the first ratio test of the homotopy is a tie between the two
    tie = qp3([-1, -2, -3], [-inf] * 3, [inf] * 3, [row, row], [-9, -9], [3, 3])
    qp, rc, n = oracle_cold(oracle, tie)
    assert rc == 0 and n == 1 and qp.ws_constraints.tolist() == [1, 0]                      # (the lower id entered)
    with pytest.raises(AssertionError):
        unambiguous(oracle, tie)
    # the unconstrained minimum x = -g lies ON the lower bound of x_0: the bound is active with a zero multiplier
    flat = qp3([-1, -2, -3], [1, -5, -5], [5] * 3, [row], [-9], [30])
    qp, rc, n = oracle_cold(oracle, flat)
    assert rc == 0 and qp.ws_bounds[0] == -1 and qp.y[0] == 0.0
    with pytest.raises(AssertionError):
        unambiguous(oracle, flat)
    # a tie that leaves no trace at the solution: x_0 <= 1.5 and x_1 <= 1.5 enter at the same step length, both end active with
    # multiplier -1.5 (strictly complementary). Only the path tells: it moves with the vectors
    pair = qp3([-3, -3, 0.5], [-inf] * 3, [inf] * 3, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], [-9, -9], [1.5, 1.5])
    qp, rc, n = oracle_cold(oracle, pair)
    assert rc == 0 and n == 2 and qp.ws_constraints.tolist() == [1, 1] and np.all(np.abs(qp.y[3:]) > 1.0)
    d = [np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(2), 1e-10 * np.array([1.0, -1.0])]
    assert LC.path(oracle, pair, n, d, 1.0) != LC.path(oracle, pair, n, d, -1.0)
    with pytest.raises(AssertionError):
        unambiguous(oracle, pair)
