"""CPU: host-side logic of the engine (partition arithmetic, synthetic generator,
workload definitions, the bit-vector DP core compiled for the host)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H


def test_shard_range_partitions_exactly():
    apm = H.pkg()
    for n, k, g in [(0, 0, 1), (5, 7, 3), (1000, 3, 3), (1 << 20, 0, 8), (12345677, 5, 7), (1 << 33, 2, 8), (17, 0, 8)]:
        prev = 0
        for s in range(g):
            b, e = apm.shard_range(n, k, s, g)
            assert b == prev and e >= b
            if 0 < s:
                assert b % 16 == 0 or b == max(0, n - k)
            prev = e
        assert prev == max(0, n - k)


def test_shard_range_rejects_bad_arguments():
    apm = H.pkg()
    for args in [(10, 0, 3, 3), (10, 0, -1, 3), (10, -1, 0, 1), (10, 0, 0, 0)]:
        with pytest.raises(apm.ApmError):
            apm.shard_range(*args)


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    return x ^ (x >> 31)


def test_synth_generator_matches_spec():
    """byte i = "ACGT"[(splitmix64(seed ^ (i>>5)) >> (2*(i&31))) & 3]  """
    apm = H.pkg()
    seed = 0x5EED0002
    for off, ln in [(0, 100), (31, 70), (123456789, 65), ((1 << 33) - 40, 40)]:
        got = apm.synth_fill_host(off, ln, seed)
        want = bytes(b"ACGT"[(_splitmix64(seed ^ (i >> 5)) >> (2 * (i & 31))) & 3] for i in range(off, off + ln))
        assert got == want
    big = np.frombuffer(apm.synth_fill_host(0, 1 << 16, seed), dtype=np.uint8)
    freq = np.bincount(big, minlength=256)[[65, 67, 71, 84]] / big.size
    assert freq.sum() == 1.0 and abs(freq - 0.25).max() < 0.02


def test_workload_definitions_match_baseline():
    wl = H.workloads()
    c = wl.CONFIGS
    assert c["cfg2"]["n"] == 1 << 28 and c["cfg2"]["lens"] == [32] * 8 and c["cfg2"]["k"] == 0
    assert c["cfg3"]["n"] == 1 << 30 and len(c["cfg3"]["lens"]) == 32 and c["cfg3"]["k"] == 3
    assert min(c["cfg3"]["lens"]) == 16 and max(c["cfg3"]["lens"]) == 128
    assert sum(m * m for m in c["cfg3"]["lens"]) == 201456
    assert c["cfg4"]["lens"] == [64] * 16 and c["cfg4"]["k"] == 2 and c["cfg4"]["n"] == 1 << 33
    assert c["cfg5"]["lens"] == [50] * 256 and c["cfg5"]["k"] == 5
    assert abs(wl.algorithmic_cells(1 << 28, [32] * 8, 0) - 2.199e12) / 2.199e12 < 1e-3


def test_planted_patterns_are_found_by_the_oracle():
    wl = H.workloads()
    apm = H.pkg()
    n, k = 1 << 14, 3
    lens = [16, 32, 50, 64, 100, 128, 20, 40]
    seed = wl.seed_of(3)
    pats, planted = wl.make_patterns(n, lens, k, seed)
    text = apm.synth_fill_host(0, n, seed)
    counts = H.oracle_counts(text, pats, k, banded=True)
    for (o, d), cnt, p in zip(planted, counts, pats):
        assert H.window_distance(p, text[o:o + len(p)]) == d
        if d <= k:
            assert cnt >= 1


def test_bitvector_core_on_host(tmp_path):
    """apm_core.h's Myers/Hyyro column == the oracle's window distance (compiled with g++)."""
    src = os.path.join(H.ROOT, "tests", "host_core_test.cpp")
    exe = str(tmp_path / "host_core_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(H.PKG_DIR, "csrc"), "-I", os.path.join(H.ROOT, "oracle"),
                    src, os.path.join(H.ROOT, "oracle", "apm_oracle.c"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_plan_builder_matches_golden_digests(tmp_path):
    """csrc/apm_plan.cpp, compiled with g++ alone, plans the sets of helpers.plan_sets() exactly as recorded in
    tests/golden/plan_digests.json: status and error text, every pattern's resolved kernel, the launch structure, and
    a digest over everything of the plan that reaches a device buffer or a launch argument (tests/plan_digest.h).
    A later change that alters the plan on purpose regenerates the file with this harness and says so in its message."""
    import json
    csrc = os.path.join(H.PKG_DIR, "csrc")
    exe = str(tmp_path / "host_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", csrc,
                    os.path.join(H.ROOT, "tests", "host_plan_test.cpp"), os.path.join(csrc, "apm_plan.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("APM_")}  # (the plan's switches at their defaults)
    r = subprocess.run([exe], input=H.plan_sets_input(), capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("set "):
            cur = got.setdefault(line[4:], [])
        else:
            cur.append(line.rstrip())
    want = json.load(open(os.path.join(H.GOLDEN_DIR, "plan_digests.json")))
    assert sorted(got) == sorted(want) and len(want) == 16
    for name in want:
        assert got[name] == want[name], name
    assert want["unsupported"][0].startswith("status -6 pattern 1 (length 300): WAVEFRONT")
    assert "code_shift=4" in " ".join(want["alphabet_k2"])


def test_no_kernel_spills_to_scratch():
    """csrc/<object>.resources.txt, one per kernel object (written by the Makefile from the compiler's resource-usage
    remarks): a spill reload inside a streaming loop is a vector-memory op that drains every prefetch
    queued behind it (vmcnt counts in order) -- it cost 10 % on the headline kernel once."""
    import glob
    paths = sorted(glob.glob(os.path.join(H.PKG_DIR, "csrc", "*.resources.txt")))
    if len(paths) < 2:
        pytest.skip("library was not built by the Makefile in this checkout")
    name, seen = None, 0
    for line in (l for p in paths for l in open(p)):
        if line.startswith("Function Name:"):
            name = line.split(":", 1)[1].strip()
        elif line.startswith("ScratchSize"):
            seen += 1
            spilled = int(line.rsplit(":", 1)[1])
            # No kernel may spill (round 3: the two LDS-tile instantiations that kept 8 bytes per lane gave up a wave of
            # occupancy instead -- they are the fallback for unaligned text only).
            assert spilled == 0, "%s spills %d bytes to scratch" % (name, spilled)
        elif line.startswith("LDS Size") and any(t in name for t in ("apm_filter_kernel", "apm_stream_kernel", "apm_sieve2_kernel", "apm_sieve2cf_kernel",
                                                                      "apm_sieve8_kernel", "apm_fused_kernel")):
            # their key bitmap is addressed as a compile-time LDS constant: dynamic LDS must start at 0
            assert int(line.rsplit(":", 1)[1]) == 0, "%s owns static LDS" % name
    assert seen >= 40


def test_counting_and_record_objects_share_no_symbol():
    """Every unit of the Makefile's KERNEL_FILES is compiled twice, into csrc/<unit>.o and with -DAPM_REC into
    csrc/<unit>_rec.o, and csrc/apm_rec.h renames what the record build defines.  An external apm_ symbol defined in both
    builds missed its rename: two strong definitions fail the link, but of two weak ones (a template, an inline function,
    a kernel) the linker keeps one without a word, and the record calls would then run counting code."""
    import re
    import shutil
    units = re.search(r"^KERNEL_FILES *= *(.+)$", open(os.path.join(H.PKG_DIR, "Makefile")).read(), re.M).group(1).split()
    assert "apm_banded_tile_b0" in units and "apm_verify" in units
    objs = [[os.path.join(H.PKG_DIR, "csrc", u + suffix + ".o") for u in units] for suffix in ("", "_rec")]
    if not shutil.which("nm") or not all(os.path.exists(o) for o in objs[0] + objs[1]):
        pytest.skip("library was not built by the Makefile in this checkout, or there is no nm")

    def defined(paths):
        syms = set()
        for p in paths:
            for line in subprocess.run(["nm", "-C", "--defined-only", p], capture_output=True, text=True, check=True).stdout.splitlines():
                f = line.split(None, 2)
                if len(f) == 3 and f[1] in "TWVDBR" and "apm_" in f[2]:
                    syms.add(f[2])
        return syms

    counting, record = defined(objs[0]), defined(objs[1])
    assert len(counting) >= len(units) and len(record) >= len(units)  # (every unit defines a launcher or a getter at least)
    assert not counting & record, sorted(counting & record)
