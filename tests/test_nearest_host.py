"""The nearest-occurrence search's arithmetic (csrc/apm_nearest.h) on the host (g++, no GPU): the occurrence search's segment
walk at the bound m - 1 with the nearest sink -- started exactly 2 m - 1 bytes in front of its first end, with poison outside
the bytes the warm-up lemma lets it read -- its keys merged in shuffled order, against a literal DP written in the test
program, at W = 1..4, m = 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, segments of 1 and of 16 bytes, the bytes 0x00, 0xFF
and '\\n'; and the key at end = 2^56 - 1.  The program is a stand-alone one with its own main, built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_nearest_core_on_host(tmp_path):
    exe = str(tmp_path / "host_nearest_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_nearest_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
