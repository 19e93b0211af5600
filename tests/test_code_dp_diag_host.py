"""The diagonal form of the code-filter sieve's window DP (apm_code_dp_diag in csrc/apm_core.h, k <= 3) against the
oracle's literal window DP, on the host (g++, no GPU): it passes exactly the centres from which the verify launch can
find a matching window, never more than the column form, and fewer random regions than the column form."""
import os
import subprocess

import helpers as H


def test_code_dp_diag_predicate_on_host(tmp_path):
    src = os.path.join(H.ROOT, "tests", "host_code_dp_diag_test.cpp")
    exe = str(tmp_path / "host_code_dp_diag_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(H.PKG_DIR, "csrc"), "-I", os.path.join(H.ROOT, "oracle"),
                    src, os.path.join(H.ROOT, "oracle", "apm_oracle.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
