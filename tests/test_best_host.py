"""The best-hit pass's arithmetic (csrc/apm_best.h) on the host (g++, no GPU): apm_best_decide -- the lane form at
k = 0..7, the wave form's emulated lanes at k = 0..9 -- against a brute force of the rule over the oracle's literal window
DP, at every pos of random DNA, poly-A and ACG tandem texts with patterns of 1..24 bytes (m > n and k >= m included) and
r in {0, 1, 2, 5, 64}; and the coverage predicate at every shard cut of one small text.  The program is a stand-alone one
with its own main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_best_core_on_host(tmp_path):
    exe = str(tmp_path / "host_best_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), "-I", os.path.join(H.ROOT, "oracle"),
                    os.path.join(H.ROOT, "tests", "host_best_test.cpp"), os.path.join(H.ROOT, "oracle", "apm_oracle.c"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
