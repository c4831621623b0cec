"""rsqp_batch_handler_ratio_test, _check_optimality and _infeasibility with DEVICE pointers: every array a torch tensor on the batch's
device. The ragged batch and the one-shape batch of tests/test_gpu_nlp_step.py, the same calls once with host arrays and once with
tensors: every in/out array and every output must be the same bytes (and the host-pointer answers are the references', which the
test session checks).

A process of its own that imports torch FIRST, as tests/checks/handler_device_pointers.py explains.
Usage (GPU box): python tests/checks/nlp_step_device_pointers.py"""
import os
import sys

import torch  # noqa: F401  (before anything loads librsqp_hip.so)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from restartsqp_amd import build, capi  # noqa: E402

build.build_lib()
import test_gpu_nlp_step as N  # noqa: E402

for key in ("ragged", "one_shape"):
    f = N.make_fixture(capi, key)
    o, c, ref, branch, st = N.ratio_case(capi, f)
    host = N.run_ratio(capi, f, o, c, on_device=False)
    dev = N.run_ratio(capi, f, o, c, on_device=True)
    exp = N.expected_ratio(capi, c, ref)
    for k in exp:
        assert host[k].tobytes() == dev[k].tobytes() == exp[k].tobytes(), (key, k)
    assert dev["accept"].dtype == np.int32 and set(dev["accept"].tolist()) == {0, 1, N.INT_FILL}
    kc = N.kkt_case(f)
    hs, hv = N.run_kkt(capi, f, kc, on_device=False)
    ds, dv = N.run_kkt(capi, f, kc, on_device=True)
    assert hs.tobytes() == ds.tobytes() and hv.tobytes() == dv.tobytes(), key
    assert np.isnan(ds).any() and not np.isnan(ds).all() and (dv == N.INT_FILL).any()
    cc = N.cat([f.rng.normal(size=m) * 3.0 for m in f.m])
    hi = f.b.handler_infeasibility(cc)
    t = torch.as_tensor(cc, device="cuda")
    torch.cuda.synchronize()
    di = f.b.handler_infeasibility(t, on_device=True)
    assert di.is_cuda and di.dtype == torch.float64 and hi.tobytes() == di.cpu().numpy().tobytes(), key
    f.b.close()
print("NLP STEP DEVICE POINTERS OK")
