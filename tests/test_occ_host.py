"""The occurrence search's arithmetic (csrc/apm_occ.h) on the host (g++, no GPU): the segment walk -- started exactly
m + k bytes in front of its first end, with poison outside the bytes the warm-up lemma lets it read -- and the span walk
against a literal DP written in the test program, at W = 1..4, m = 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, k from 0 up
to m - 1 for the small m, segments of one byte, and the bytes 0x00, 0xFF and '\\n'; and the segment chooser.  The program
is a stand-alone one with its own main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_occ_core_on_host(tmp_path):
    exe = str(tmp_path / "host_occ_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_occ_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
