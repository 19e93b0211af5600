"""The prefix form of the nomination predicate (csrc/apm_core.h, apm_unit_pred16) on the host (g++, no GPU): for units
split as the plan builder splits them (k = 0..7, m = 17..512; random patterns, patterns over one and two letters, tandem
repeats) and texts built from the pattern with 0..k+2 edits in front of and behind the 16th byte of exact parts and
partners, the full byte-loop predicate implies the prefix form, and the prefix form implies what the sieve tests at the
position: the 16-bit and 18-bit code words are among the unit's enumerated words and apm_cf_pass holds on the codes.
The program is a stand-alone one with its own main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H


def test_prefix_predicate_on_host(tmp_path):
    exe = str(tmp_path / "host_prefix_pred_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_prefix_pred_test.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
