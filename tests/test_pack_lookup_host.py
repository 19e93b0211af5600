"""The sieve's streaming arithmetic (apm_pack16_join, apm_lookup2_mid and apm_lookup2_word in csrc/apm_core.h) against the
forms it replaced and against its definitions, on the host (g++, no GPU): 10^6 random dword quadruples at code shifts
0..6, the eight lookup words of a chunk for 10^6 random (slo, shi)."""
import os
import subprocess

import helpers as H


def test_pack16_combine_and_lookup_words_on_host(tmp_path):
    src = os.path.join(H.ROOT, "tests", "host_pack_lookup_test.cpp")
    exe = str(tmp_path / "host_pack_lookup_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(H.PKG_DIR, "csrc"), src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
