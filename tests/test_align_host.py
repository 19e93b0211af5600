"""The align pass's arithmetic core (csrc/apm_align.h) on the host (g++, no GPU) over the 3000 pairs of
helpers.window_distance_pairs(), whole and truncated to size < m: the lane form at k = 0..7 and the wave form -- as its
plain loop over 64 emulated lanes -- at k = 0..9, 16, 40, 130, 300 must report no script exactly when dist > k and
otherwise, bit for bit, the canonical script of a literal full-matrix DP and walk back written out in the test program
(its distance cross-checked against the oracle's).  The program is a stand-alone one with its own main, built with the
address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import helpers as H


def test_align_core_on_host(tmp_path):
    pairs = H.window_distance_pairs()
    assert len(pairs) == 3000 and max(len(p) for p, _ in pairs) == 140
    data = tmp_path / "pairs.txt"
    data.write_text("".join("%s %s\n" % (p.hex(), t.hex()) for p, t in pairs))
    exe = str(tmp_path / "host_align_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), "-I", os.path.join(H.ROOT, "oracle"),
                    os.path.join(H.ROOT, "tests", "host_align_test.cpp"), os.path.join(H.ROOT, "oracle", "apm_oracle.c"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"\b[1-9]\d* checked, 0 wrong", r.stdout), r.stdout
