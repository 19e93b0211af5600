"""The code-filter sieve's window DP on codes (apm_code_dp_pass in csrc/apm_core.h) against the oracle's literal
window DP, on the host (g++, no GPU): it must pass every region that holds a matching window, for every shift a
unit can nominate that window from."""
import os
import subprocess

import helpers as H


def test_code_dp_predicate_on_host(tmp_path):
    src = os.path.join(H.ROOT, "tests", "host_code_dp_test.cpp")
    exe = str(tmp_path / "host_code_dp_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(H.PKG_DIR, "csrc"), "-I", os.path.join(H.ROOT, "oracle"),
                    src, os.path.join(H.ROOT, "oracle", "apm_oracle.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
