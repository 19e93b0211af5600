"""CPU: the occurrence-script calls (apm_occ_align_row_words, apm_occ_align_device, apm_find_occ_align_buffer) are declared
in include/apm.h, exported by the library, bound in Python and given argtypes; the pass's kernel has a resource digest of its
own -- one kernel, compiled once, without scratch -- and the occurrence search's unit keeps its two."""
import ctypes
import os
import re

import helpers as H

NAMES = {"apm_occ_align_row_words": 1, "apm_occ_align_device": 11, "apm_find_occ_align_buffer": 11}


def test_occ_align_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name, n_args in NAMES.items():
        assert re.search(r"\bint %s\((const )?apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert len(getattr(apm.load_library(), name).argtypes) == n_args, name
    for method in ("occ_align_row_words", "occ_align_device", "find_occ_align_buffer"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    # the header's own words: the section exists, the launch is named, and the occurrence search no longer rules scripts out
    assert "occurrence scripts" in hdr and '"oalign"' in hdr
    assert "edit scripts for occurrences" not in hdr


def test_occ_align_kernel_has_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_occ_align.resources.txt")
    assert os.path.exists(path), "csrc/apm_occ_align.resources.txt missing: the Makefile writes it with apm_occ_align.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    lds = [int(v) for v in re.findall(r"^LDS Size[^:]*: *(\d+)", text, flags=re.M)]
    assert len(names) == 1 and "apm_occ_align_kernel" in names[0]
    assert scratch == [0]
    # the Eq table (4 KiB), the trace (256 columns of 8 words) and the span's bytes: everything the pass keeps
    assert lds == [4096 + 8192 + 256]
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_occ_align_rec.resources.txt"))
    mk = open(os.path.join(H.PKG_DIR, "Makefile")).read()
    once = re.search(r"^ONCE_FILES = (.*)$", mk, flags=re.M).group(1).split()
    kernel = re.search(r"^KERNEL_FILES = (.*)$", mk, flags=re.M).group(1).split()
    assert "apm_occ_align" in once and "apm_occ_align" not in kernel


def test_occ_unit_keeps_its_two_kernels():
    text = open(os.path.join(H.PKG_DIR, "csrc", "apm_occ.resources.txt")).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    assert len(names) == 2
    assert sum("apm_occ_scan_kernel" in n for n in names) == 1 and sum("apm_occ_span_kernel" in n for n in names) == 1
