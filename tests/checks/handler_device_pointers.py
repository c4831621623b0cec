"""rsqp_batch_handler_update and rsqp_batch_handler_get_step with DEVICE pointers: every argument a torch tensor on the batch's device.
The 130-member one-shape batch and the five calls of tests/test_gpu_batch_handler.py::test_update_one_shape_batch, once with host
arrays and once with tensors: the pools must be the same bytes after every call (and equal the reference), and after a solve the
step data written into torch tensors must be the bytes the host-pointer call returns.

A process of its own that imports torch FIRST: torch ships its own copy of the HIP runtime, with the soname librsqp_hip.so asks
for. Loaded before the library, that copy serves both, and a tensor's data_ptr() is memory of the runtime the batch runs on. The
other order -- the library first, as in the test session -- leaves two runtimes in the process, and torch finds no GPU.
Usage (GPU box): python tests/checks/handler_device_pointers.py"""
import os
import sys

import torch  # noqa: F401  (before anything loads librsqp_hip.so)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from restartsqp_amd import build, capi  # noqa: E402

build.build_lib()
import test_gpu_batch_handler as G  # noqa: E402

fh, host = G.run_one_shape(capi, False)
fd, devp = G.run_one_shape(capi, True)
for a, c in zip(host, devp):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
it = G.solvable_iterate(fh)
for f in (fh, fd):
    f.b.handler_update([capi.HU_SET] * 130, *it[:4], grad=it[4])
    f.b.optimize_qp()
assert all(r["status"] == 20 for r in fd.b.results())
h = fh.b.handler_step()
d = fd.b.handler_step(on_device=True)
out = {k: torch.full_like(v, float("nan")) for k, v in d.items()}
torch.cuda.synchronize()
assert fd.b.handler_step(on_device=True, out=out) is out
h2 = fd.b.handler_step()
for k in ("p", "lam_c", "lam_x", "infea_model", "norm_p"):
    assert d[k].is_cuda and d[k].dtype == torch.float64
    assert h[k].tobytes() == d[k].cpu().numpy().tobytes() == out[k].cpu().numpy().tobytes() == h2[k].tobytes(), k
assert np.abs(h["p"]).max() > 0.0
# the handler object with its iterate on the device: one flush, the same pools as the host-pointer batch
S = capi.HU_SET
hd = G.BatchQPhandler(fd.b, *fd.bounds, on_device=True)
t = lambda a: torch.as_tensor(a, device="cuda")
even = np.arange(130) % 2 == 0
hd.update_delta(even, 0.5, t(it[2]))
hd.update_penalty(~even, 3.0)
hd.update_grad(None, t(it[4] * 2.0))
words = hd.flush()
fh.b.handler_update(words, np.full(130, 0.5), np.full(130, 3.0), it[2], it[3], grad=it[4] * 2.0)
assert all(x.tobytes() == y.tobytes() for x, y in zip(fh.b.get_vectors(), fd.b.get_vectors()))
assert set(words.tolist()) == {capi.HU_DELTA | capi.HU_GRAD, capi.HU_PENALTY | capi.HU_GRAD}
fh.b.close(); fd.b.close()
print("HANDLER DEVICE POINTERS OK")
