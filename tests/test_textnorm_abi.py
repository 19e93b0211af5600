"""CPU: the text-mode calls (apm_set_text_mode, apm_normalize_device, apm_map_positions_device) are declared in
include/apm.h, exported by the library and bound in Python; a NULL context is APM_ERR_INVALID; the ABI version, the record
layout and apm_timing did not move; the pass's kernels have a resource digest without scratch."""
import ctypes
import os
import re

import helpers as H

NAMES = ("apm_set_text_mode", "apm_normalize_device", "apm_map_positions_device")
INVALID = -1


def test_text_mode_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert getattr(apm.load_library(), name).argtypes, name
    for method in ("set_text_mode", "normalize_device", "map_positions_device"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    assert "#define APM_TEXT_FASTA 1u" in hdr and "#define APM_TEXT_UPPER 2u" in hdr
    assert (apm.APM_TEXT_FASTA, apm.APM_TEXT_UPPER) == (1, 2)
    assert ctypes.sizeof(apm.ApmTiming) == 80 and ctypes.sizeof(apm.ApmMatch) == 16


def test_null_context_is_invalid():
    lib = H.pkg().load_library()
    out = ctypes.c_uint64(7)
    assert lib.apm_set_text_mode(None, 1) == INVALID
    assert lib.apm_normalize_device(None, None, 0, 1, None, 0, ctypes.byref(out)) == INVALID
    assert lib.apm_map_positions_device(None, None, 0, None) == INVALID
    assert out.value == 7


def test_textnorm_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_textnorm.resources.txt")
    assert os.path.exists(path), "csrc/apm_textnorm.resources.txt missing: the Makefile writes it with apm_textnorm.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    for kernel in ("apm_tn_summary_kernel", "apm_tn_scan_kernel", "apm_tn_scatter_kernel", "apm_tn_map_kernel"):
        assert sum(kernel in n for n in names) == 1, kernel
    assert len(scratch) == len(names) == 4 and not any(scratch)
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_textnorm_rec.resources.txt"))   # compiled once
