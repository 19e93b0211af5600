"""CPU: the nearest-occurrence calls (apm_nearest_shard_device, apm_nearest_records_device, apm_find_nearest_buffer) are
declared in include/apm.h, exported by the library, bound in Python and given argtypes; the APM_NEAREST_* constants compiled
from C are the ones Python, tests/nearest_ref.py and csrc/apm_nearest.h use; a NULL context is APM_ERR_INVALID; the unit's
kernels have a resource digest of their own, compiled once, without scratch."""
import ctypes
import os
import re
import subprocess

import helpers as H
import nearest_ref

ERR_INVALID = -1  # APM_ERR_INVALID of include/apm.h
NAMES = {"apm_nearest_shard_device": 8, "apm_nearest_records_device": 8, "apm_find_nearest_buffer": 5}


def test_nearest_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name, n_args in NAMES.items():
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert len(getattr(apm.load_library(), name).argtypes) == n_args, name
    for method in ("nearest_shard_device", "nearest_records_device", "find_nearest_buffer"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    assert apm.load_library().apm_abi_version() == 1
    for label in ('"nearest"', '"nspan"', '"nearest_segment"', '"nearest_lanes"'):
        assert label in hdr, label


def test_nearest_constants(tmp_path):
    src = tmp_path / "nearest.c"
    src.write_text('#include <stdio.h>\n#include "apm.h"\n'
                   'int main(void) { uint64_t k = ((uint64_t)127 << 56) | (((uint64_t)1 << 56) - 1);\n'
                   'printf("%d %u %llu %u %d\\n", APM_NEAREST_NONE == UINT64_MAX, APM_NEAREST_DIST(k), (unsigned long long)APM_NEAREST_END(k), '
                   'APM_NEAREST_DIST(APM_NEAREST_NONE), k < APM_NEAREST_NONE); return 0; }\n')
    exe = str(tmp_path / "nearest")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), str(src), "-o", exe], check=True)
    top = (1 << 56) - 1
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["1", "127", str(top), "255", "1"]
    apm = H.pkg()
    assert apm.APM_NEAREST_NONE == nearest_ref.NONE == (1 << 64) - 1
    k = apm.nearest_key(127, top)
    assert k == nearest_ref.key(127, top) and k < apm.APM_NEAREST_NONE
    assert (apm.nearest_dist(k), apm.nearest_end(k)) == (nearest_ref.key_dist(k), nearest_ref.key_end(k)) == (127, top)
    core = open(os.path.join(H.PKG_DIR, "csrc", "apm_nearest.h")).read()
    assert re.search(r"#define APM_NEAREST_NONE 0xffffffffffffffffull\b", core)
    assert re.search(r"#define APM_NEAREST_DIST\(key\) .*>> 56\)", core) and re.search(r"#define APM_NEAREST_END\(key\) .*0x00ffffffffffffffull\)", core)


def test_nearest_calls_refuse_a_null_context():
    lib = H.pkg().load_library()
    assert lib.apm_find_nearest_buffer(None, None, 0, None, None) == ERR_INVALID
    assert lib.apm_nearest_shard_device(None, None, 0, 0, 0, 0, 0, None) == ERR_INVALID
    assert lib.apm_nearest_records_device(None, None, 0, 0, 0, None, None, None) == ERR_INVALID


def test_nearest_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_nearest.resources.txt")
    assert os.path.exists(path), "csrc/apm_nearest.resources.txt missing: the Makefile writes it with apm_nearest.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    assert sum("apm_nearest_scan_kernel" in n for n in names) == 1 and sum("apm_nearest_span_kernel" in n for n in names) == 1
    assert len(scratch) == len(names) == 2 and not any(scratch)
    # compiled once: there is no record build of the nearest-occurrence search
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_nearest_rec.resources.txt"))
    mk = open(os.path.join(H.PKG_DIR, "Makefile")).read()
    once = re.search(r"^ONCE_FILES = (.*)$", mk, flags=re.M).group(1).split()
    kernel = re.search(r"^KERNEL_FILES = (.*)$", mk, flags=re.M).group(1).split()
    assert "apm_nearest" in once and "apm_nearest" not in kernel
