"""The host's small eigenproblem and small SVD (csrc/smm_jacobi.h: jacobiEigen, jacobiSvd) on their own, under AddressSanitizer + UBSan
(tests/cpp/jacobi_case.cpp, built by tests/cpp/Makefile).  The drivers reach them only through whole GPU solves."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_small_eigen_and_svd_under_address_and_ub_sanitizers():
    """orthogonality, residual and order of the factors for the shapes the drivers build, the rank-deficient matrices, the values that
    are not finite -- run directly, nothing preloaded"""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "jacobi_case"], check=True)
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "jacobi_case")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAILED" not in r.stdout, r.stdout[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
