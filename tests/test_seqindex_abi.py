"""CPU: the sequence calls (apm_index_sequences_device, apm_locate_records_device, apm_locate_buffer, apm_get_sequences) are
declared in include/apm.h, exported by the library and bound in Python; apm_seq and apm_loc are 16 bytes; a NULL context
is APM_ERR_INVALID with the outputs untouched; the constants have their values; the ABI version and the record layout did
not move; the unit's kernels have a resource digest of their own without scratch."""
import ctypes
import os
import re

import helpers as H

NAMES = ("apm_index_sequences_device", "apm_locate_records_device", "apm_locate_buffer", "apm_get_sequences")
KERNELS = ("apm_sq_count_kernel", "apm_sq_scan_kernel", "apm_sq_emit_kernel", "apm_sq_locate_kernel")
INVALID = -1


def test_sequence_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert getattr(apm.load_library(), name).argtypes, name
    for method in ("index_sequences_device", "locate_records_device", "locate", "sequences"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    assert ctypes.sizeof(apm.ApmSeq) == ctypes.sizeof(apm.ApmLoc) == 16
    assert ctypes.sizeof(apm.ApmTiming) == 80 and ctypes.sizeof(apm.ApmMatch) == 16
    assert [f[0] for f in apm.ApmSeq._fields_] == ["hdr_off", "t_begin"]
    assert [f[0] for f in apm.ApmLoc._fields_] == ["off", "seq", "flags"] and apm.ApmLoc.seq.offset == 8 and apm.ApmLoc.flags.offset == 12


def test_constants():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    for line in ("#define APM_SEQ_NO_HEADER UINT64_MAX", "#define APM_SEQ_INVALID 0xFFFFFFFFu", "#define APM_LOC_SPANS 1u",
                 "#define APM_LOC_TRUNCATED 2u"):
        assert line in hdr, line
    assert apm.APM_SEQ_NO_HEADER == 2 ** 64 - 1 and apm.APM_SEQ_INVALID == 0xFFFFFFFF
    assert (apm.APM_LOC_SPANS, apm.APM_LOC_TRUNCATED) == (1, 2)


def test_null_context_is_invalid_and_touches_nothing():
    apm = H.pkg()
    lib = apm.load_library()
    n_seq = ctypes.c_uint64(7)
    table = (apm.ApmSeq * 2)()
    loc = (apm.ApmLoc * 1)()
    rec = (apm.ApmMatch * 1)()
    ctypes.memset(table, 0x5A, ctypes.sizeof(table))
    ctypes.memset(loc, 0x5A, ctypes.sizeof(loc))
    assert lib.apm_index_sequences_device(None, None, 0, ctypes.byref(n_seq)) == INVALID
    assert lib.apm_locate_records_device(None, None, 0, None, None, 1, None) == INVALID
    assert lib.apm_locate_buffer(None, rec, 1, loc) == INVALID
    assert lib.apm_get_sequences(None, table, 2, ctypes.byref(n_seq)) == INVALID
    assert n_seq.value == 7
    assert bytes(table) == b"\x5a" * 32 and bytes(loc) == b"\x5a" * 16


def test_seqindex_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_seqindex.resources.txt")
    assert os.path.exists(path), "csrc/apm_seqindex.resources.txt missing: the Makefile writes it with apm_seqindex.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    for kernel in KERNELS:
        assert sum(kernel in n for n in names) == 1, kernel
    assert len(scratch) == len(names) == len(KERNELS) and not any(scratch)
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_seqindex_rec.resources.txt"))   # compiled once
