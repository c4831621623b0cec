"""The certificate of a single handle on the synchronous path: started by tests/test_gpu_certificate.py::test_b4_synchronous_path with
RSQP_NO_SPIN=1, which the library reads once per process. Runs the checks of that file (limits_and_staleness) on one problem of the
tableau kernel's size and one of the LDS-resident kernels' and prints the worst observed error / bound."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

if __name__ == "__main__":
    if os.environ.get("RSQP_NO_SPIN") != "1":
        raise SystemExit("certificate_no_spin.py: set RSQP_NO_SPIN=1")
    from restartsqp_amd import build, capi
    build.build_lib()
    capi.lib()
    import test_gpu_certificate as T
    worst, n = T.synchronous_path_body(capi)
    print("B4 synchronous path: %d cases, worst error / bound = %.3f" % (n, worst))
