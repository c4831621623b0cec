"""QPs shaped like the ones QPhandler builds from an NLP iterate (problems.handler_qp: variables (p, u, v),
A = [J I -I], H = blkdiag(H_k, 0), g = (grad f, rho e)), from random data instead of an NLP: the members of batches
whose images exceed the LDS of a CU (n + 2 m above about 90)."""
import numpy as np

from .qpdump import QPData, dense_to_csc
from .sqptypes import INF


def handler_shaped_qp(rng, n, m, definite=True, density=0.3, delta=1.0, rho=10.0, n_eq=None, name=""):
    """n NLP variables, m constraints -> an (n + 2 m) x m QP. definite=False gives H_k one negative eigenvalue
    (an indefinite Hessian of the Lagrangian); the trust-region box |p| <= delta keeps the QP bounded either way.
    The first n_eq constraints (default m // 3) are equalities c(x) = 0, the others one- or two-sided inequalities."""
    nV = n + 2 * m
    J = rng.normal(size=(m, n)) * (rng.random((m, n)) < density)
    J[np.arange(m), rng.integers(0, n, size=m)] += 1.0          # no empty row
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = rng.uniform(0.5, 5.0, size=n)
    if not definite:        # one direction of negative curvature (stronger ones mostly end in cycles of bound flips)
        ev[rng.integers(0, n)] = -rng.uniform(0.1, 0.2)
    Hk = (Q * ev) @ Q.T
    Hk = 0.5 * (Hk + Hk.T)
    H = np.zeros((nV, nV))
    H[:n, :n] = Hk
    A = np.hstack([J, np.eye(m), -np.eye(m)])
    lb = np.zeros(nV); ub = np.full(nV, INF)
    lb[:n] = -delta * rng.uniform(0.5, 1.0, size=n)
    ub[:n] = delta * rng.uniform(0.5, 1.0, size=n)
    g = np.concatenate([3.0 * rng.normal(size=n), rho * np.ones(2 * m)])
    c = rng.normal(size=m)
    n_eq = m // 3 if n_eq is None else n_eq
    lbA = -c.copy(); ubA = -c.copy()
    kind = rng.integers(0, 3, size=m)
    for i in range(n_eq, m):
        if kind[i] == 0:
            lbA[i] = -INF
        elif kind[i] == 1:
            ubA[i] = INF
        else:
            ubA[i] = lbA[i] + rng.uniform(0.5, 2.0)
    return QPData(nV, m, *dense_to_csc(H), *dense_to_csc(A), g, lb, ub, lbA, ubA,
                  name=name or "handler-%dx%d-%s" % (nV, m, "pd" if definite else "indef"))


def handler_batch(nq, n, m, seed=20261016, indefinite_every=3):
    """nq members of one shape, (n + 2 m) x m; every indefinite_every-th member has an indefinite H_k (0: none)"""
    rng = np.random.default_rng(seed)
    return [handler_shaped_qp(rng, n, m, definite=not (indefinite_every and k % indefinite_every == indefinite_every - 1))
            for k in range(nq)]
