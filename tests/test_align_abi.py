"""CPU: the align calls (apm_align_row_words, apm_align_shard_device, apm_find_all_align_buffer) are declared in
include/apm.h, exported by the library and bound in Python; the record layout and the ABI version did not move; the
align kernels' resource digest exists, lists four lane kernels and one wave kernel, and shows no scratch."""
import ctypes
import os
import re
import subprocess

import helpers as H

NAMES = ("apm_align_row_words", "apm_align_shard_device", "apm_find_all_align_buffer")


def test_align_calls_are_declared_exported_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    lib = ctypes.CDLL(apm.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\((const )?apm_ctx \*ctx" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in apm.ABI_SYMBOLS
        assert getattr(apm.load_library(), name).argtypes, name
    for method in ("align_row_words", "align_shard_device", "find_all_align_buffer"):
        assert hasattr(apm.ApmContext, method), method
    assert "#define APM_ABI_VERSION 1" in hdr
    # the convention, in the header's words
    for line in ("code 0, letter '=': bytes equal; consumes one byte of each", "code 1, letter 'X': substitution; consumes one byte of each",
                 "code 2, letter 'I': the text has a byte the pattern has not; consumes text only",
                 "code 3, letter 'D': the pattern has a byte the text has not; consumes pattern only",
                 "It is the pattern-to-text edit, not SAM's query/reference roles."):
        assert line in hdr, line


def test_ops_to_script():
    apm = H.pkg()
    assert apm.ops_to_script(bytes([0] * 11 + [1] + [0] * 4 + [3] + [0] * 7 + [2])) == "11=1X4=1D7=1I"
    assert apm.ops_to_script(b"") == "" and apm.ops_to_script(bytes([1, 1])) == "2X"
    row = [18, sum(op << (2 * j) for j, op in enumerate([0, 1, 2, 3] * 4)), 3 | (1 << 2), 0xdeadbeef]
    assert apm.unpack_ops(row) == bytes([0, 1, 2, 3] * 4 + [3, 1])


def test_record_layout_and_op_codes(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "apm.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u %d %d %d %d %d\\n", sizeof(apm_match), offsetof(apm_match, pos), '
                   'offsetof(apm_match, pattern), offsetof(apm_match, reserved), APM_DIST_INVALID, APM_ABI_VERSION, '
                   'APM_OP_EQ, APM_OP_SUB, APM_OP_INS, APM_OP_DEL); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == \
        ["16", "0", "8", "12", "4294967295", "1", "0", "1", "2", "3"]
    M = H.pkg().ApmMatch
    assert ctypes.sizeof(M) == 16 and (M.pos.offset, M.pattern.offset, M.reserved.offset) == (0, 8, 12)


def test_align_kernels_have_a_digest_without_scratch():
    path = os.path.join(H.PKG_DIR, "csrc", "apm_align.resources.txt")
    assert os.path.exists(path), "csrc/apm_align.resources.txt missing: the Makefile writes it with apm_align.o"
    text = open(path).read()
    names = re.findall(r"^Function Name: *(\S+)", text, flags=re.M)
    scratch = [int(v) for v in re.findall(r"^ScratchSize[^:]*: *(\d+)", text, flags=re.M)]
    assert sum("apm_align_lane_kernel" in n for n in names) == 4 and sum("apm_align_wave_kernel" in n for n in names) == 1
    assert len(scratch) == len(names) == 5 and not any(scratch)
    # compiled once: there is no record build of the align pass
    assert not os.path.exists(os.path.join(H.PKG_DIR, "csrc", "apm_align_rec.resources.txt"))
