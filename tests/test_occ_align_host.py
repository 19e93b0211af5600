"""The occurrence-script pass's arithmetic (csrc/apm_occ_align.h) on the host (g++, no GPU): the forward walk that keeps
every column, and the walk back that counts cells out of the kept columns, against a literal full-matrix DP and the pinned
rule written in the test program, at W = 1..4, m = 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, k from 0 up to m - 1 for the
small m, every text length from m - k to m + k there, the bytes 0x00, 0xFF and '\\n', pairs farther than k and tie-rich pairs.
The program is a stand-alone one with its own main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_occ_align_core_on_host(tmp_path):
    exe = str(tmp_path / "host_occ_align_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_occ_align_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " checked, 0 wrong" in r.stdout, r.stdout
