"""The per-sequence occurrence search's arithmetic (csrc/apm_seqocc.h) on the host (g++, no GPU): the boundary-aware walk cut
into segments of 1, 16 and 61 bytes and the whole text, the union of what the segments report against the literal recurrence
run on every sequence as a text of its own -- exactly, so no duplicate at a seam and no lost end.  Both flags, k in
{0, 1, 3, m - 1}, m = 1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, boundaries at b, b +- 1, e, e +- 1, b - (m + k) and
b - (m + k) +- 1, runs of empty sequences, 1-byte sequences, random tables, poison outside the bytes a walk may read, and a
table that breaks its promise.  The program is a stand-alone one with its own main, built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_seqocc_core_on_host(tmp_path):
    exe = str(tmp_path / "host_seqocc_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_seqocc_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
