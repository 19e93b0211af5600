"""The text-normalisation pass's shared core (csrc/apm_textnorm.h) on the host (g++, no GPU): the summary, scan, scatter
and map kernels as plain loops over 64 emulated lanes, against a byte-serial state machine -- the layouts of
textnorm_ref.layouts() under every flag combination with the Python reference's output alongside, then random texts over
{A,C,G,T,a,c,\\n,\\r,>} of 0..20000 bytes; the map inverse is checked for every kept byte.  The program is a stand-alone
one with its own main, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import helpers as H
import textnorm_ref as R


def test_reference_state_machine():
    assert R.normalize(b">h\nAC\nGT\n", R.FASTA) == (b"ACGT", [3, 4, 6, 7])
    assert R.normalize(b"AC>G\r\n>x", R.FASTA) == (b"AC>G", [0, 1, 2, 3])          # '>' inside a line is a byte; open header at the end
    assert R.normalize(b"a`{z\x80\n", R.UPPER) == (b"A`{Z\x80\n", list(range(6)))
    assert R.normalize(b"\n>a\n>b\nac", R.FASTA | R.UPPER) == (b"AC", [7, 8])
    assert R.normalize(b"", R.FASTA) == (b"", [])


def test_textnorm_core_on_host(tmp_path):
    lines = []
    for name, src in sorted(R.layouts().items()):
        for flags in (R.FASTA, R.UPPER, R.FASTA | R.UPPER):
            want = R.normalize(src, flags)[0]
            lines.append("%s %d %s %s\n" % (name, flags, src.hex() or "-", want.hex() or "-"))
    lines.append("empty 1 - -\n")
    data = tmp_path / "cases.txt"
    data.write_text("".join(lines))
    exe = str(tmp_path / "host_textnorm_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(H.PKG_DIR, "csrc"), os.path.join(H.ROOT, "tests", "host_textnorm_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
    assert int(r.stdout.split()[-4]) > 240 + 8 * 3 * len(R.layouts())
