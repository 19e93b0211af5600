"""CPU: the occurrence calls (apm_occ_shard_device, apm_occ_spans_device, apm_find_occ_buffer) are declared in
include/apm.h, exported by the library, bound in Python and given argtypes; the APM_OCC_* constants compiled from C are the
ones Python and csrc/apm_occ.h use; the unit's kernels have a resource digest of their own, compiled once, without scratch."""
import ctypes
import os
import re
import subprocess

import helpers as H

NAMES = {"apm_occ_shard_device": 12, "apm_occ_spans_device": 9, "apm_find_occ_buffer": 9}


def test_occ_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name, n_args in NAMES.items():
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert len(getattr(apm.load_library(), name).argtypes) == n_args, name
    for method in ("occ_shard_device", "occ_spans_device", "find_occ_buffer"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    assert apm.load_library().apm_abi_version() == 1


def test_occ_constants(tmp_path):
    src = tmp_path / "occ.c"
    src.write_text('#include <stdio.h>\n#include "apm.h"\n'
                   'int main(void) { printf("%u %u %d %d\\n", APM_OCC_ALL, APM_OCC_LOCAL_MIN, APM_OCC_MAX_PATTERN_LEN, '
                   'APM_OCC_NO_START == UINT64_MAX); return 0; }\n')
    exe = str(tmp_path / "occ")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["0", "1", "128", "1"]
    apm = H.pkg()
    assert (apm.APM_OCC_ALL, apm.APM_OCC_LOCAL_MIN, apm.APM_OCC_MAX_PATTERN_LEN) == (0, 1, 128)
    assert apm.APM_OCC_NO_START == (1 << 64) - 1
    core = open(os.path.join(H.PKG_DIR, "csrc", "apm_occ.h")).read()
    assert re.search(r"#define APM_OCC_ALL 0u\b", core) and re.search(r"#define APM_OCC_LOCAL_MIN 1u\b", core)
    assert re.search(r"#define APM_OCC_MAX_PATTERN_LEN 128\b", core)


def test_occ_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_occ.resources.txt")
    assert os.path.exists(path), "csrc/apm_occ.resources.txt missing: the Makefile writes it with apm_occ.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    assert sum("apm_occ_scan_kernel" in n for n in names) == 1 and sum("apm_occ_span_kernel" in n for n in names) == 1
    assert len(scratch) == len(names) == 2 and not any(scratch)
    # compiled once: there is no record build of the occurrence search
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_occ_rec.resources.txt"))
    mk = open(os.path.join(H.PKG_DIR, "Makefile")).read()
    once = re.search(r"^ONCE_FILES = (.*)$", mk, flags=re.M).group(1).split()
    kernel = re.search(r"^KERNEL_FILES = (.*)$", mk, flags=re.M).group(1).split()
    assert "apm_occ" in once and "apm_occ" not in kernel
