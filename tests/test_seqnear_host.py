"""The per-sequence nearest search's arithmetic (csrc/apm_seqnear.h) on the host (g++, no GPU): the walk cut into segments of
1, 16 and 61 bytes and the whole text, every segment flushing into one key per sequence, against a literal DP run on every
sequence as a text of its own -- boundaries at a segment's first end b, at b +- 1, b - m and b - (2 m - 1) +- 1, runs of empty
sequences, 1-byte sequences, random tables, m = 1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128, poison outside the bytes a walk
may read, and the bounded table search on tables that break their promise.  The program is a stand-alone one with its own
main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_seqnear_core_on_host(tmp_path):
    exe = str(tmp_path / "host_seqnear_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_seqnear_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
