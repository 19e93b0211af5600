"""CPU: the scoring calls (apm_score_shard_device, apm_find_all_dist_buffer) are declared in include/apm.h, exported by
the library and bound in Python; the record layout did not move; the scoring kernels' resource digest exists and shows
no scratch."""
import ctypes
import os
import re
import subprocess

import helpers as H

NAMES = ("apm_score_shard_device", "apm_find_all_dist_buffer")


def test_scoring_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert getattr(apm.load_library(), name).argtypes, name
    assert hasattr(apm.ApmContext, "find_all_dist_buffer") and hasattr(apm.ApmContext, "score_shard_device")
    assert "#define APM_ABI_VERSION 1" in hdr and "#define APM_DIST_INVALID 0xFFFFFFFFu" in hdr
    assert "0 from the find calls; the capped distance after a scoring call" in hdr


def test_record_layout_unchanged(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "apm.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u\\n", sizeof(apm_match), offsetof(apm_match, pos), '
                   'offsetof(apm_match, pattern), offsetof(apm_match, reserved), APM_DIST_INVALID); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["16", "0", "8", "12", "4294967295"]
    M = H.pkg().ApmMatch
    assert ctypes.sizeof(M) == 16 and (M.pos.offset, M.pattern.offset, M.reserved.offset) == (0, 8, 12)


def test_score_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_score.resources.txt")
    assert os.path.exists(path), "csrc/apm_score.resources.txt missing: the Makefile writes it with apm_score.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    assert sum("apm_score_lane_kernel" in n for n in names) == 4 and sum("apm_score_wave_kernel" in n for n in names) == 1
    assert len(scratch) == len(names) == 5 and not any(scratch)
    # compiled once: there is no record build of the scoring pass
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_score_rec.resources.txt"))
