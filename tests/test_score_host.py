"""The scoring pass's arithmetic core (csrc/apm_score.h) on the host (g++, no GPU), against the oracle's literal window
DP over the 3000 pairs of helpers.window_distance_pairs(): the lane form at k = 0..7 and the wave form -- as its plain
loop over 64 emulated lanes, the chunks and the carry of the kernel -- at k = 0..9, 16, 40, 130, 300 must return
min(dist, k + 1), on whole pairs and on pairs truncated to size < m.  The program is a stand-alone one with its own
main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_score_core_on_host(tmp_path):
    pairs = H.window_distance_pairs()
    assert len(pairs) == 3000 and max(len(p) for p, _ in pairs) == 140
    data = tmp_path / "pairs.txt"
    data.write_text("".join("%s %s\n" % (p.hex(), t.hex()) for p, t in pairs))
    exe = str(tmp_path / "host_score_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), "-I", os.path.join(H.ROOT, "oracle"),
                    os.path.join(H.ROOT, "tests", "host_score_test.cpp"), os.path.join(H.ROOT, "oracle", "apm_oracle.c"),
                    "-o", exe], check=True)
    r = subprocess.run([exe, str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
