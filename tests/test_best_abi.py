"""CPU: the best-hit calls (apm_best_shard_device, apm_find_best_buffer) are declared in include/apm.h, exported by the
library and bound in Python; APM_BEST_MAX_RADIUS is 64; the pass's kernels have a resource digest of their own, compiled
once, that shows no scratch."""
import ctypes
import os
import re
import subprocess

import helpers as H

NAMES = ("apm_best_shard_device", "apm_find_best_buffer")


def test_best_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert getattr(apm.load_library(), name).argtypes, name
    assert len(apm.load_library().apm_best_shard_device.argtypes) == 12
    assert len(apm.load_library().apm_find_best_buffer.argtypes) == 10
    assert hasattr(apm.ApmContext, "find_best_buffer") and hasattr(apm.ApmContext, "best_shard_device")
    assert "#define APM_ABI_VERSION 1" in hdr
    assert apm.load_library().apm_abi_version() == 1


def test_max_radius_is_64(tmp_path):
    src = tmp_path / "radius.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "apm.h"\n'
                   'int main(void) { printf("%d %zu %zu\\n", APM_BEST_MAX_RADIUS, sizeof(apm_match), offsetof(apm_match, reserved)); return 0; }\n')
    exe = str(tmp_path / "radius")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["64", "16", "12"]
    assert H.pkg().APM_BEST_MAX_RADIUS == 64
    core = open(os.path.join(H.PKG_DIR, "csrc", "apm_best.h")).read()
    assert re.search(r"#define APM_BEST_MAX_RADIUS 64\b", core)


def test_best_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_best.resources.txt")
    assert os.path.exists(path), "csrc/apm_best.resources.txt missing: the Makefile writes it with apm_best.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    assert sum("apm_best_lane_kernel" in n for n in names) == 4 and sum("apm_best_wave_kernel" in n for n in names) == 1
    assert len(scratch) == len(names) == 5 and not any(scratch)
    # compiled once: there is no record build of the best-hit pass
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_best_rec.resources.txt"))
