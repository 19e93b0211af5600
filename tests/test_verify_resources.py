"""Registers, scratch and occupancy of the verify and fused kernels against the commit recorded in
tests/golden/verify_resources.json (the kernel resource digests the Makefile writes beside the objects of
csrc/apm_verify.hip and csrc/apm_sieve.hip, counting build and record build).  The dedup of matches (ApmVerifyCore::count_matches) is shared by
every instantiation of apm_verify_kernel and apm_fused_kernel; a form of it that suits the list-driven kernel may cost
another one a wave of occupancy or a spill -- such an instantiation keeps the earlier form (APM_DEDUP_WIDE,
APM_DEDUP_PREFETCH).  No instantiation may spill or fall below the recorded occupancy, and the sieve kernels, which share
the wave idioms of csrc/apm_wave.h but none of that code, must come out exactly as recorded."""
import json
import os

import pytest

import helpers as H

KEYS = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch",
        "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds"}


def _digest(unit):
    path = os.path.join(H.PKG_DIR, "csrc", unit + ".resources.txt")
    assert os.path.exists(path), "%s missing: the Makefile writes it beside the objects of csrc/%s.hip" % (path, unit.replace("_rec", ""))
    out, name = {}, None
    for line in open(path):
        key, value = line.strip().split(":", 1)
        if key == "Function Name":
            name = value.strip()
            out[name] = {}
        else:
            out[name][KEYS[key]] = int(value)
    return out


@pytest.mark.parametrize("unit", ["apm_sieve", "apm_sieve_rec"])  # the build: the sieve unit's name stands for its verify twin too
def test_verify_and_fused_kernels_keep_their_occupancy_and_the_sieve_kernels_their_digest(unit):
    golden = json.load(open(os.path.join(H.GOLDEN_DIR, "verify_resources.json")))
    assert len(golden["commit"]) == 40
    want, got = {}, {}
    for u in (unit, unit.replace("apm_sieve", "apm_verify")):
        assert sorted(_digest(u)) == sorted(golden[u]), u  # (every kernel in the unit it is recorded for)
        want.update(golden[u])
        got.update(_digest(u))
    assert sorted(got) == sorted(want) and len(want) == 28
    n_verify = n_sieve = 0
    for name, w in want.items():
        g = got[name]
        if "apm_verify_kernel" in name or "apm_fused_kernel" in name:
            n_verify += 1
            assert g["scratch"] == 0, "%s spills %d bytes to scratch" % (name, g["scratch"])
            assert g["occupancy"] >= w["occupancy"], "%s: %d waves per SIMD, %d recorded (%d registers, %d recorded)" % (
                name, g["occupancy"], w["occupancy"], g["vgprs"], w["vgprs"])
        else:
            n_sieve += 1
            assert "apm_sieve" in name and g == w, "%s: %r, recorded %r" % (name, g, w)
    assert n_verify == 24 and n_sieve == 4
