"""rsqp_batch_handler_set_matrices with DEVICE pointers: what, jac and hess as torch tensors on the batch's device. The one-pattern
batch and the twins of tests/test_gpu_batch_handler_matrices.py, once with host arrays and once with tensors: the value pools must be
the same bytes after every call (and equal the reference; the twins' solves must agree with the host setter's in both runs). Then a
BatchQPhandler(on_device=True) with matrices and vectors pending: one flush must leave the pools a host-pointer handler leaves.

A process of its own that imports torch FIRST (tests/checks/handler_device_pointers.py says why).
Usage (GPU box): python tests/checks/handler_matrices_device_pointers.py"""
import os
import sys

import torch  # noqa: F401  (before anything loads librsqp_hip.so)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from restartsqp_amd import build, capi  # noqa: E402

build.build_lib()
import test_gpu_batch_handler_matrices as X  # noqa: E402

same = lambda a, c: all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, c))
host, dev = X.run_one_pattern(capi, False), X.run_one_pattern(capi, True)
assert len(host) == len(dev) == 4 and all(same(a, c) for a, c in zip(host, dev))
assert same(X.run_twins(capi, False), X.run_twins(capi, True))

# the handler object: matrices and vectors pending on 130 members of (4, 2), one flush each
rng = np.random.default_rng(67)
members = [X.handler_member(rng, 4, 2) for _ in range(130)]
nq, J, H = len(members), capi.HM_JAC, capi.HM_HESS
bounds = (np.full(4 * nq, -2.0), np.full(4 * nq, 2.0), np.full(2 * nq, -1.0), np.full(2 * nq, 1.0))
bh, bd = capi.Batch(members), capi.Batch(members)
hh, hd = X.BatchQPhandler(bh, *bounds), X.BatchQPhandler(bd, *bounds, on_device=True)
t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")
new = [X.new_entries(rng, q) for q in members]
third, even = np.arange(nq) % 3 == 0, np.arange(nq) % 2 == 0
jac, hess = X.pooled([e[0] for e in new], third), X.pooled([e[1] for e in new], even)
x_k, c_k, grad = rng.normal(size=4 * nq) * 0.1, rng.normal(size=2 * nq) * 0.1, rng.normal(size=4 * nq)
for h, conv in ((hh, lambda a: a), (hd, t)):
    h.update_A(third, conv(jac))
    h.update_H(even, conv(hess))
    h.set_bounds(None, 1.0, conv(x_k), conv(c_k))
    h.set_g(None, conv(grad), 2.0)
    words = h.flush()
    assert np.all(words == capi.HU_SET)
    assert np.array_equal(h.matrix_words, third * J + even * H)
    assert not h.flush().any() and not h.matrix_words.any()      # nothing is pending behind a flush
A2, H2 = X.batch_matrices_reference(np.concatenate([q.A_val for q in members]), np.concatenate([q.H_val for q in members]),
                                    third * J + even * H, jac, hess, bh.nV, bh.nC, [q.A_jc for q in members], [q.H_jc for q in members])
for b in (bh, bd):
    gA, gH = b.get_matrix_values()
    assert gA.tobytes() == A2.tobytes() and gH.tobytes() == H2.tobytes()
assert all(x.tobytes() == y.tobytes() for x, y in zip(bh.get_vectors(), bd.get_vectors()))
uh, ud = bh.optimize_qp(), bd.optimize_qp()
assert np.array_equal(uh, ud) and all(X.M.same_bytes(a, c) for a, c in zip(bh.results(), bd.results()))
assert all(r["status"] == 20 for r in bd.results())
bh.close(); bd.close()
print("HANDLER MATRICES DEVICE POINTERS OK")
