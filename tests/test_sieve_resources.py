"""Register budget of the code-filter sieve's window-DP form (csrc/apm_sieve.resources.txt, the digest the Makefile
writes from the compiler's resource-usage remarks).  The kernel is launched as two workgroups of 1024 threads per CU --
8 waves per SIMD -- and its LDS is sized for that: at 65 VGPRs the occupancy halves, and a spill reload in the
streaming loop drains the prefetches queued behind it."""
import os

import helpers as H


def _digest(path):
    """{mangled kernel name: {field: value}}"""
    assert os.path.exists(path), "%s is missing: the library was not built by the Makefile" % path
    out, cur = {}, None
    for line in open(path):
        key, _, val = line.partition(":")
        if key == "Function Name":
            cur = out.setdefault(val.strip(), {})
        elif cur is not None and val.strip():
            cur[key.strip()] = int(val)
    return out


def test_window_dp_sieve_keeps_8_waves_per_simd():
    for suffix, name in (("", "apm_sieve2cfdp_kernel"), ("_rec", "apm_sieve2cfdp_kernel_rec")):
        d = _digest(os.path.join(H.PKG_DIR, "csrc", "apm_sieve%s.resources.txt" % suffix))
        hits = [v for k, v in d.items() if ("%d%s13ApmSieve2Args" % (len(name), name)) in k]
        assert len(hits) == 1, (name, sorted(d))
        r = hits[0]
        assert r["VGPRs"] <= 64, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] == 8, (name, r)
