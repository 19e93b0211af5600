"""The sequence index's shared core (csrc/apm_seqindex.h) on the host (g++, no GPU): the count, scan, emit and locate
kernels as plain loops over 64 emulated lanes, against a byte-serial state machine -- every layout of
seqindex_ref.layouts() (textnorm_ref.layouts() and the index's own) under every flag combination with the Python
reference's table alongside, then random texts over {A,C,G,T,a,c,\\n,\\r,>} of 0..20000 bytes; the table is compared entry
for entry and every source offset is located for pattern lengths 1, 5 and 5000.  The program is a stand-alone one with its
own main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H
import seqindex_ref as S
import textnorm_ref as R


def test_reference_on_the_worked_example():
    S.self_test()


def test_reference_layouts_cover_what_they_name():
    L = S.layouts()
    assert set(R.layouts()) < set(L)
    n_seq = lambda name: len(S.sequences(L[name], R.FASTA)) - 1
    assert S.sequences(L["sq_gt_at_0"], R.FASTA)[1] == (0, 0)
    assert n_seq("sq_no_header") == 1 and n_seq("sq_a_then_gt_at_block_start") == 1
    assert S.sequences(L["sq_nl_ends_block_gt_starts_next"], R.FASTA)[1][0] == R.BLOCK
    assert n_seq("sq_nl_gt_x3000") == n_seq("sq_gt_nl_x3000") == 3001          # 8 opens in a lane of 16 bytes
    t = S.sequences(L["sq_three_headers_in_a_row"], R.FASTA)
    assert t[1][1] == t[2][1] == t[3][1] == 0                                  # empty sequences
    assert S.sequences(L["sq_unterminated_header_at_end"], R.FASTA)[-2][1] == S.sequences(L["sq_unterminated_header_at_end"], R.FASTA)[-1][1]
    assert b"\r\n" in L["sq_crlf"] and n_seq("sq_crlf") == 4
    assert all(len(S.sequences(src, R.UPPER)) == 2 for src in L.values())       # no FASTA: no header opens


def test_seqindex_core_on_host(tmp_path):
    lines = []
    layouts = S.layouts()
    for name, src in sorted(layouts.items()):
        for flags in (R.FASTA, R.UPPER, R.FASTA | R.UPPER):
            table = ",".join("%s:%d" % ("-" if h == S.NO_HEADER else h, t) for h, t in S.sequences(src, flags))
            lines.append("%s %d %s %s\n" % (name, flags, src.hex() or "-", table))
    lines.append("empty 1 - -:0,0:0\n")
    data = tmp_path / "cases.txt"
    data.write_text("".join(lines))
    exe = str(tmp_path / "host_seqindex_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_seqindex_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
    assert int(r.stdout.split()[-4]) == 160 + 3 * (3 * len(layouts) + 1)
