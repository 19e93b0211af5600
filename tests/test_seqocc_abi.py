"""CPU: the per-sequence occurrence calls (apm_occ_seq_shard_device, apm_occ_seq_spans_device, apm_find_occ_seq_buffer) are
declared in include/apm.h, exported by the library, bound in Python and given argtypes; a NULL context is APM_ERR_INVALID;
the unit's two kernels have a resource digest of their own, compiled once, without scratch; the header names the launch
labels and the statistics."""
import ctypes
import os
import re

import helpers as H

ERR_INVALID = -1  # APM_ERR_INVALID of include/apm.h
NAMES = {"apm_occ_seq_shard_device": 14, "apm_occ_seq_spans_device": 12, "apm_find_occ_seq_buffer": 12}


def test_seqocc_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name, n_args in NAMES.items():
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert len(getattr(apm.load_library(), name).argtypes) == n_args, name
    for method in ("occ_seq_shard_device", "occ_seq_spans_device", "find_occ_seq_buffer"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    for label in ('"socc"', '"sspan"', '"seqocc_segment"', '"seqocc_lanes"', "occurrence search per sequence"):
        assert label in hdr, label


def test_seqocc_calls_refuse_a_null_context():
    lib = H.pkg().load_library()
    found = ctypes.c_uint64(7)
    assert lib.apm_find_occ_seq_buffer(None, None, 0, 0, None, None, None, 0, ctypes.byref(found), None, None, 0) == ERR_INVALID
    assert found.value == 7
    assert lib.apm_occ_seq_shard_device(None, None, 0, 0, 0, 0, 0, None, 1, 0, None, 0, None, None) == ERR_INVALID
    assert lib.apm_occ_seq_spans_device(None, None, 0, 0, 0, None, 1, None, 0, None, None, None) == ERR_INVALID


def test_seqocc_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_seqocc.resources.txt")
    assert os.path.exists(path), "csrc/apm_seqocc.resources.txt missing: the Makefile writes it with apm_seqocc.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    assert sum("apm_seqocc_scan_kernel" in n for n in names) == 1 and sum("apm_seqocc_span_kernel" in n for n in names) == 1
    assert len(scratch) == len(names) == 2 and not any(scratch)
    # compiled once: there is no record build of the per-sequence occurrence search
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_seqocc_rec.resources.txt"))
    mk = open(os.path.join(H.PKG_DIR, "Makefile")).read()
    once = re.search(r"^ONCE_FILES = (.*)$", mk, flags=re.M).group(1).split()
    kernel = re.search(r"^KERNEL_FILES = (.*)$", mk, flags=re.M).group(1).split()
    assert "apm_seqocc" in once and "apm_seqocc" not in kernel
