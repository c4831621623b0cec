"""rsqp_batch_handler_soc_begin / _soc_end with DEVICE pointers: every array a torch tensor on the batch's device. Comparison (a) of
tests/test_gpu_soc.py -- the two calls against the host-driven loop on a second batch, bit for bit -- for every batch and option
set, with tensors where the test session passes host arrays.

A process of its own that imports torch FIRST, as tests/checks/handler_device_pointers.py explains.
Usage (GPU box): python tests/checks/soc_device_pointers.py"""
import os
import sys

import torch  # noqa: F401  (before anything loads librsqp_hip.so)

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from restartsqp_amd import build, capi  # noqa: E402

build.build_lib()
import test_gpu_soc as T  # noqa: E402

for batch, option_set in T.HOST_DRIVEN_CASES:
    T.check_against_the_host_driven_loop(capi, batch, option_set, True)
print("SOC DEVICE POINTERS OK")
