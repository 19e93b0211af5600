"""The sequence table and the location of a record (include/apm.h: "sequences") as byte-serial Python on top of
textnorm_ref.normalize: the reference the index and locate passes are pinned to, and the layouts their tests add to
textnorm_ref.layouts()."""
import bisect
import random

import textnorm_ref as R

NO_HEADER = (1 << 64) - 1
SEQ_INVALID = 0xFFFFFFFF
SPANS, TRUNCATED = 1, 2
INVALID = (0, SEQ_INVALID, 0)


def sequences(src, flags):
    """[(hdr_off, t_begin)]: entry 0, one entry per '>' at a line start, the sentinel (src_len, |T|)"""
    T, src_of = R.normalize(src, flags)
    table = [(NO_HEADER, 0)]
    if flags & R.FASTA:
        kept = set(src_of)
        before, line_start = 0, True
        for i, b in enumerate(src):
            if line_start and b == 0x3E:
                table.append((i, before))
            if i in kept:
                before += 1
            line_start = b == 0x0A
    table.append((len(src), len(T)))
    return table


_index_of = {}


def _kept_index(src, flags):
    """(|T|, {source offset: index in T}) of the last few sources asked for"""
    key = (src, flags)
    if key not in _index_of:
        if len(_index_of) >= 8:
            _index_of.clear()
        T, src_of = R.normalize(src, flags)
        _index_of[key] = (len(T), {s: c for c, s in enumerate(src_of)})
    return _index_of[key]


def locate(src, flags, table, lens, pos, pattern):
    """(off, seq, flags) of the record (pattern, pos), pos a source offset; INVALID if it names no window"""
    n_T, index_of = _kept_index(src, flags)
    if pattern >= len(lens) or pos >= len(src) or pos not in index_of:
        return INVALID
    c = index_of[pos]
    n_seq = len(table) - 1
    seq = bisect.bisect_left(table, pos, 1, n_seq, key=lambda e: e[0]) - 1      # the largest i with hdr_off[i] < pos, else 0
    size = min(lens[pattern], n_T - c)
    fl = (SPANS if c + size - 1 >= table[seq + 1][1] else 0) | (TRUNCATED if size < lens[pattern] else 0)
    return (c - table[seq][1], seq, fl)


EXAMPLE = b"AC\n>one x\nACGT\nAC\n>two\n>three\r\nGGTT"
EXAMPLE_TABLE = [(NO_HEADER, 0), (3, 2), (18, 8), (23, 8), (35, 12)]
EXAMPLE_LOCATIONS = {0: (0, 0, 1), 1: (1, 0, 1), 10: (0, 1, 0), 15: (4, 1, 1), 32: (1, 3, 2),
                     3: INVALID, 17: INVALID, 35: INVALID, 40: INVALID}


def self_test():
    assert len(EXAMPLE) == 35 and len(R.normalize(EXAMPLE, R.FASTA)[0]) == 12
    assert sequences(EXAMPLE, R.FASTA) == EXAMPLE_TABLE
    for pos, want in EXAMPLE_LOCATIONS.items():
        assert locate(EXAMPLE, R.FASTA, EXAMPLE_TABLE, [4], pos, 0) == want, pos
    assert locate(EXAMPLE, R.FASTA, EXAMPLE_TABLE, [4], 10, 1) == INVALID
    assert sequences(EXAMPLE, R.UPPER) == [(NO_HEADER, 0), (35, 35)]
    assert sequences(b"", R.FASTA) == [(NO_HEADER, 0), (0, 0)]


def layouts(seed=12):
    """name -> source: textnorm_ref.layouts() and the layouts where the index can go wrong on its own"""
    rng = random.Random(seed)
    B = R.BLOCK
    n = 2 * B + 5
    out = dict(R.layouts())
    out.update({
        "sq_gt_at_0": b">first\n" + R.dna(rng, 300) + b"\n>second\n" + R.dna(rng, 200),
        "sq_no_header": R.fasta(rng, 2 * B, header=b""),
        "sq_nl_ends_block_gt_starts_next": R._at(rng, n, {B - 1: b"\n", B: b">x y\n"}),
        "sq_a_then_gt_at_block_start": R._at(rng, n, {B - 1: b"A", B: b">"}),
        "sq_nl_gt_x3000": b"\n>" * 3000,
        "sq_gt_nl_x3000": b">\n" * 3000,
        "sq_two_headers_in_a_row": R.dna(rng, 70) + b"\n>a\n>b\n" + R.dna(rng, 4100) + b"\n",
        "sq_three_headers_in_a_row": b">a\n>b\r\n>c\n" + R.dna(rng, 100) + b"\n>d\n",
        "sq_header_over_two_blocks": R.dna(rng, 100) + b"\n>" + b"h" * (2 * B + 300) + b"\n" + R.dna(rng, 500) + b"\n>t\nAC",
        "sq_unterminated_header_at_end": R.fasta(rng, 500) + b">no end of line",
        "sq_crlf": b"".join(R.fasta(rng, 1500 + 700 * i, cols=60, header=b">s%d crlf\r\n" % i, eol=b"\r\n") for i in range(3)),
        "sq_example": EXAMPLE,
    })
    return out
