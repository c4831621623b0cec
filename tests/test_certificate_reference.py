"""The oracle's KKT certificate (oracle/kkt_oracle.c) against an independent long-double restatement (tests/kkt_ref.py) on points that
are NOT optimal, where the four terms are far from zero. Discrete outputs (W_b, W_c, verdict, invalid flag) are equal; the fields lie
within the derived bound 2^-52 (n_terms + k_max + 4) M_field of kkt_ref. Also the CPU half of the GPU certificate tests
(test_gpu_certificate.py): the threshold guards of every generated input the GPU is given, and the branch tallies of the exact cases."""
import numpy as np
import pytest

import kkt_cases as K
import kkt_ref as R
from conftest import clamp


def oracle_certificate(O, q, x, y, ws_b, ws_c, lp=False):
    """(invalid, ok, values, W_b, W_c) by the oracle, with the bounds clamped as every caller of it does"""
    A = (q.A_jc, q.A_ir, q.A_val)
    H = None if lp or q.H_jc is None else (q.H_jc, q.H_ir, q.H_val)
    lb, ub, lbA, ubA = clamp(q.lb), clamp(q.ub), clamp(q.lbA), clamp(q.ubA)
    try:
        Wb, Wc = O.kkt_get_working_set(q.nV, q.nC, A, x, lb, ub, lbA, ubA, ws_b, ws_c)
    except ValueError:
        return True, None, None, None, None
    ok, st = O.kkt_test_optimality(q.nV, q.nC, A, H, q.g, lb, ub, lbA, ubA, x, y, Wb, Wc)
    return False, int(ok), np.array([getattr(st, f) for f in R.FIELDS]), Wb, Wc


def compare(O, case, lp=False, exact=False):
    """the worst observed error / bound over the five fields"""
    q = case.q
    ref = R.of_problem(q, case.x, case.y, case.ws_b, case.ws_c, lp=lp)
    invalid, ok, val, Wb, Wc = oracle_certificate(O, q, case.x, case.y, case.ws_b, case.ws_c, lp=lp)
    assert invalid == ref.invalid, q.name
    if invalid:
        assert ref.ok == R.ERR_WORKING_SET
        return 0.0
    assert np.array_equal(Wb, ref.W_b) and np.array_equal(Wc, ref.W_c), q.name
    assert ok == ref.ok, (q.name, ok, ref.ok)
    worst = 0.0
    for k, f in enumerate(R.FIELDS):
        err, bnd = abs(float(R.LD(val[k]) - ref.fields[f])), R.bound(ref, f)
        if exact:
            assert val[k] == ref.values[k], (q.name, f, val[k], ref.values[k])
        assert err <= bnd, (q.name, f, val[k], ref.values[k], err, bnd)
        worst = max(worst, err / bnd if bnd > 0 else 0.0)
    return worst


def test_random_points_that_are_not_optimal(oracle):
    cases = K.real_cases(K.REF_SHAPES, seed=20261021)
    worst = 0.0
    for c in cases:
        ref = R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c)
        assert ref.ok == 0 and float(ref.fields["KKT_error"]) > 1.0e-5, c.q.name
        assert R.guard_of_problem(c.q, ref, c.x, c.ws_b, c.ws_c) > 1.0, c.q.name
        worst = max(worst, compare(oracle, c))
    print("oracle vs reference, random points: worst error / bound = %.3f" % worst)
    # the generated set takes every value of W on bounds and on constraints, and has infinite and +-1e20 sides, equalities and fixed
    # variables among its rows
    Wb = np.concatenate([R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c).W_b for c in cases])
    Wc = np.concatenate([R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c).W_c for c in cases])
    for W in (Wb, Wc):
        assert set(W.tolist()) == {R.ABOVE, R.BELOW, R.BOTH, R.INACTIVE}
    for name in ("lb", "ub", "lbA", "ubA"):
        v = np.concatenate([getattr(c.q, name) for c in cases])
        assert np.isinf(v).any() and (np.abs(v) == 1.0e20).any(), name
    assert any((c.q.lb == c.q.ub).any() for c in cases) and any((c.q.lbA == c.q.ubA).any() for c in cases)


def test_exact_cases_are_bit_equal_and_reach_every_branch(oracle):
    cases = K.exact_cases()
    tally = {}
    for c in cases:
        compare(oracle, c, exact=True)
        for k, v in R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c).tally.items():
            tally[k] = tally.get(k, 0.0) + float(v)
    assert_every_branch(tally)


def assert_every_branch(tally):
    """summed over a case set, every branch of map_bound, map_constr and kkt_terms contributed a nonzero amount"""
    assert len(tally) == 20, sorted(tally)
    for name, v in tally.items():
        assert v > 0.0, (name, v)


def test_active_side_at_an_infinite_bound(oracle):
    """ACTIVE_BELOW with lb = -inf and a multiplier: the complementarity term is |y| (x + 1e20), in both"""
    rng = np.random.default_rng(5)
    c = K.make_case(rng, 8, 8)
    c.q.lb[:] = -np.inf
    c.q.ub[:] = c.x + 1.0
    c.ws_b[:] = -1
    c.y[:8] = -1.0
    ref = R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c)
    assert np.all(ref.W_b == R.BELOW) and float(ref.fields["compl_violation"]) > 7.9e20
    compare(oracle, c)


@pytest.mark.parametrize("where", ["bound", "constraint"])
@pytest.mark.parametrize("entry", [2, -7])
def test_invalid_working_set_entries(oracle, where, entry):
    rng = np.random.default_rng(7)
    for nV, nC, at in ((8, 8, 0), (300, 511, 280)):
        c = K.make_case(rng, nV, nC)
        (c.ws_b if where == "bound" else c.ws_c)[at] = entry
        ref = R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c)
        assert ref.invalid and ref.ok == R.ERR_WORKING_SET
        compare(oracle, c)


def test_absent_H(oracle):
    rng = np.random.default_rng(11)
    for nV, nC in K.REF_SHAPES:
        c = K.make_case(rng, nV, nC, haveH=False)
        compare(oracle, c)
        # and a present H that the caller asks to leave out (the LP certificate)
        c2 = K.make_case(rng, nV, nC)
        with_h = R.of_problem(c2.q, c2.x, c2.y, c2.ws_b, c2.ws_c).values
        without = R.of_problem(c2.q, c2.x, c2.y, c2.ws_b, c2.ws_c, lp=True).values
        assert with_h[3] != without[3] and np.array_equal(with_h[:3], without[:3])
        compare(oracle, c2, lp=True)


def test_non_canonical_csc(oracle):
    rng = np.random.default_rng(13)
    for nV, nC in K.REF_SHAPES[1:]:
        c = K.make_case(rng, nV, nC)
        q2 = K.noncanonical(rng, c.q)
        assert nV < 8 or (len(q2.A_val) > len(c.q.A_val) and len(q2.H_val) > len(c.q.H_val))     # repeated positions exist
        c2 = K.Case(q2, c.x, c.y, c.ws_b, c.ws_c)
        compare(oracle, c2)
        # the scrambled arrays describe the same matrix: the reference agrees with itself up to the rounding of the split entries
        a, b = R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c), R.of_problem(q2, c.x, c.y, c.ws_b, c.ws_c)
        assert np.array_equal(a.W_b, b.W_b) and np.array_equal(a.W_c, b.W_c)
        for f in R.FIELDS:
            assert abs(float(a.fields[f] - b.fields[f])) <= R.bound(b, f)


def test_exact_non_canonical_is_bit_equal(oracle):
    """the split entries of an exact case are quarters: still exact"""
    rng = np.random.default_rng(17)
    for c in K.exact_cases()[2:6]:
        compare(oracle, K.Case(K.noncanonical(rng, c.q), c.x, c.y, c.ws_b, c.ws_c), exact=True)


def test_reference_by_hand():
    """the reference itself on a 2 x 1 problem worked out by hand"""
    jc, ir, val = np.array([0, 1, 2], np.int32), np.array([0, 0], np.int32), np.array([1.0, 2.0])     # A = [1 2]
    H = (np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([2.0, 4.0]))               # H = diag(2, 4)
    x, y = [1.0, 0.5], [0.25, -1.0, 3.0]        # Ax = 2
    # bounds: x0 = 1 in [1.5, 3] with ws +1 (ABOVE, below its lower side by 0.5); x1 = 0.5 in [0, 0.5] with ws -1 (at ub: BOTH)
    # constraint: Ax = 2 in [-1, 1] with ws -1: Ax - ubA = 1 >= 1e-8, BELOW
    c = R.certificate(2, 1, (jc, ir, val), H, [1.0, -2.0], [1.5, 0.0], [3.0, 0.5], [-1.0], [1.0], x, y, [1, -1], [-1])
    assert c.W_b.tolist() == [R.ABOVE, R.BOTH] and c.W_c.tolist() == [R.BELOW]
    # primal 0.5 + (2 - 1); dual max(0, .25) + 0 + -min(0, 3); compl |.25 (3 - 1)| + |3 (2 + 1)|
    # stat |3*1 + .25 - 1 - 2| + |3*2 - 1 + 2 - 2| = .25 + 5
    assert c.values.tolist() == [1.5, 0.25, 9.5, 5.25, 16.5] and c.ok == 0
    assert c.n["primal_violation"] == 6 and c.k_max == 2
    assert float(c.M["stationarity_violation"]) == (3 + .25 + 1 + 2) + (6 + 1 + 2 + 2)
    # without H the stationarity alone changes
    c = R.certificate(2, 1, (jc, ir, val), None, [1.0, -2.0], [1.5, 0.0], [3.0, 0.5], [-1.0], [1.0], x, y, [1, -1], [-1])
    assert c.values.tolist() == [1.5, 0.25, 9.5, 2.25 + 7.0, 20.5]
    # an optimal point says yes
    c = R.certificate(1, 0, (np.zeros(2, np.int32), [], []), None, [0.0], [-1.0], [1.0], [], [], [0.0], [0.0], [0], [])
    assert c.ok == 1 and c.values.tolist() == [0.0] * 5


def test_guards_of_the_inputs_the_gpu_tests_inject():
    """every generated non-exact input of test_gpu_certificate.py whose x does not come from the GPU keeps away from the thresholds of
    the working-set mapping: the GPU's Ax, rounded otherwise, cannot decide a row differently. No row is excluded"""
    sets = {"A3/A5": K.real_cases(), "A5 unscaled": K.real_cases(spread=False, seed=20261022),
            "A6": [K.refreshed(c) for c in K.real_cases()]}
    for name, cases in sets.items():
        for c in cases:
            ref = R.of_problem(c.q, c.x, c.y, c.ws_b, c.ws_c)
            m = R.guard_of_problem(c.q, ref, c.x, c.ws_b, c.ws_c)
            assert m > 1.0, (name, c.q.name, m)
            assert ref.ok == 0 and float(ref.fields["KKT_error"]) > 1.0e-5, (name, c.q.name)
