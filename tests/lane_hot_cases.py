"""The inputs of tests/test_gpu_lane_hot.py (hot starts on new vectors on the lane-per-problem kernel, rsqp_batch_set_lane_hot) and
the oracle's answers for them, each computed once per session: the steady-state sequence cold -> new vectors -> new vectors -> new
matrices -> new vectors of a one-pattern batch, and the same per member on the CPU oracle. tests/test_lane_hot_inputs.py asserts
without a GPU that the sequences hold what the GPU tests are about."""
import numpy as np

from lane_cases import one_pattern_batch, own_pattern_batch
from restartsqp_amd import problems

SHAPES = ((8, 2), (6, 1), (4, 2), (8, 0), (1, 2))
RELS = (0.3, 0.02)
KINDS = ("cold", "vectors", "vectors", "matrices", "vectors")
NMEMBERS = 150


def vecs(q):
    return q.g, q.lb, q.ub, q.lbA, q.ubA


def oracle_mats(qp, q):
    qp.set_A_csc(q.A_jc, q.A_ir, q.A_val); qp.set_H_csc(q.H_jc, q.H_ir, q.H_val)


def new_vectors(rng, members, rel):
    return [problems.perturb(rng, q, rel) for q in members]


def new_matrices(rng, members, rel=0.3):
    out = new_vectors(rng, members, rel)
    for q in out:
        q.A_val = q.A_val * (1.0 + 0.02 * rng.normal(size=q.A_val.shape))
    return out


def sequence(rng, first, rel, kinds=KINDS):
    """[step][member]: `first`, then new vectors (every vector perturbed by rel) or new matrices (vectors by 0.3, A rescaled)"""
    steps = [first]
    for kind in kinds[1:]:
        steps.append(new_matrices(rng, steps[-1]) if kind == "matrices" else new_vectors(rng, steps[-1], rel))
    return steps


_STEPS = {}


def steady_steps(shape, rel):
    """the steady-state sequence of a one-pattern batch of `shape`; (6, 1): with free variables"""
    key = (shape, rel)
    if key not in _STEPS:
        nV, nC = shape
        rng = np.random.default_rng(9000 + 10 * nV + nC)
        _STEPS[key] = sequence(rng, one_pattern_batch(rng, nV, nC, NMEMBERS, free=(nV == 6)), rel)
    return _STEPS[key]


def own_pattern_steps():
    """the same sequence for members whose sparsity patterns differ (the build without the one pattern)"""
    if "own" not in _STEPS:
        rng = np.random.default_rng(9300)
        _STEPS["own"] = sequence(rng, own_pattern_batch(rng, 8, 2, 197), 0.3)
    return _STEPS["own"]


def modes_of(capi, kinds=KINDS):
    return [{"cold": capi.MODE_COLD, "vectors": capi.MODE_HOT_VECTORS, "matrices": capi.MODE_HOT_MATRICES}[k] for k in kinds]


class Answer:
    """what a test reads of an OracleQP after one call, frozen (the object itself moves on with the next call); quacks like it for
    assert_same_solution"""

    def __init__(self, qp, n):
        self.flag, self.n, self.solved, self.infeasible = qp.exitflag(), n, bool(qp.is_solved()), bool(qp.is_infeasible())
        self.x, self.y = qp.x.copy(), qp.y.copy()
        self.ws_bounds, self.ws_constraints = qp.ws_bounds.copy(), qp.ws_constraints.copy()
        self.objective = qp.objective if self.solved else None

    def exitflag(self):
        return self.flag

    def is_solved(self):
        return self.solved


def oracle_sequence(oracle, steps, kinds=KINDS, limits=None):
    """[step][member] = Answer: init / hotstart / hotstart_matrices, one OracleQP per member"""
    qps = []
    for q in steps[0]:
        qp = oracle.OracleQP(q.nV, q.nC)
        oracle_mats(qp, q)
        qps.append(qp)
    out = []
    for k, (members, kind) in enumerate(zip(steps, kinds)):
        lim = limits[k] if limits else 1000
        row = []
        for qp, q in zip(qps, members):
            if kind == "cold":
                rc, n = qp.init(*vecs(q), lim)
            elif kind == "vectors":
                rc, n = qp.hotstart(*vecs(q), lim)
            else:
                oracle_mats(qp, q)
                rc, n = qp.hotstart_matrices(*vecs(q), lim)
            row.append(Answer(qp, n))
        out.append(row)
    return out


_ORACLE = {}


def steady_oracle(oracle, shape, rel):
    key = (shape, rel)
    if key not in _ORACLE:
        _ORACLE[key] = oracle_sequence(oracle, steady_steps(shape, rel))
    return _ORACLE[key]


def own_pattern_oracle(oracle):
    if "own" not in _ORACLE:
        _ORACLE["own"] = oracle_sequence(oracle, own_pattern_steps())
    return _ORACLE["own"]


def changes(row):
    """(members without, members with) a working-set change in one step"""
    return sum(a.n == 0 for a in row), sum(a.n > 0 for a in row)
