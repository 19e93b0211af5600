"""Occurrence scripts on the GPU: apm_occ_align_device and apm_find_occ_align_buffer write, for every (end, span) pair, the
edit script include/apm.h pins ("occurrence scripts"), bit for bit.  The truth is the full matrix cell(x, y) of the pattern
against the span's bytes with the pinned rule walked back over it, both written here, over the records of tests/occ_ref.py;
the tests without the `gpu` mark pin that reference itself.  Rows carry preset sentinel words, and the tests compare those."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import helpers as H
import occ_ref as R
import test_occ_gpu as O
from test_occ_gpu import Dev, counts_of, run_cli, setup

gpu = pytest.mark.gpu
INVALID = -1
ALL, LOCAL_MIN = R.ALL, R.LOCAL_MIN
NO_START, DIST_INVALID = R.NO_START, 0xFFFFFFFF
SENT = 0xA5C3F00D
EQ, SUB, INS, DEL = 0, 1, 2, 3
LINE = 1 << 32


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


# ---------------------------------------------------------------- the reference
def matrix(p, t):
    """cell[x][y] = the distance of the first x bytes of t and the first y bytes of p: the literal recurrence, column by
    column as occ_ref.global_dist runs it, every column kept"""
    a = np.frombuffer(bytes(p), dtype=np.uint8)
    m = len(a)
    y = np.arange(m + 1, dtype=np.int64)
    c = np.empty((len(t) + 1, m + 1), dtype=np.int64)
    c[0] = y
    new = np.empty(m + 1, dtype=np.int64)
    for x, ch in enumerate(bytes(t), 1):
        new[0] = x
        np.minimum(c[x - 1][:-1] + (a != ch), c[x - 1][1:] + 1, out=new[1:])
        c[x] = y + np.minimum.accumulate(new - y)
    return c


def matrix_plain(p, t):
    """the same matrix, cell by cell"""
    c = [[0] * (len(p) + 1) for _ in range(len(t) + 1)]
    for x in range(len(t) + 1):
        for y in range(len(p) + 1):
            if x == 0 or y == 0:
                c[x][y] = x + y
            else:
                c[x][y] = min(c[x - 1][y - 1] + (p[y - 1] != t[x - 1]), c[x][y - 1] + 1, c[x - 1][y] + 1)
    return c


def script(p, t, c=None):
    """(distance, ops first to last) by the pinned rule, walked back from (L, m)"""
    c = matrix(p, t) if c is None else c
    x, y, ops = len(t), len(p), []
    while x or y:
        if y == 0:
            op = INS
        elif x == 0:
            op = DEL
        elif c[x - 1][y - 1] + (p[y - 1] != t[x - 1]) == c[x][y]:
            op = SUB if p[y - 1] != t[x - 1] else EQ
        elif c[x][y - 1] + 1 == c[x][y]:
            op = DEL
        else:
            op = INS
        ops.append(op)
        x -= op != DEL
        y -= op != INS
    return int(c[len(t)][len(p)]), ops[::-1]


def row_of(ops):
    """the words the row format defines: n_ops, then 16 ops per dword, the last one's unused high bits zero"""
    words = [len(ops)] + [0] * (-(-len(ops) // 16))
    for j, op in enumerate(ops):
        words[1 + j // 16] |= op << (2 * (j % 16))
    return words


def pair_row(text, pats, k, i, e, s):
    """the row of the pair (i, e) / s over `text`: [0] where the pair is farther than k"""
    d, ops = script(pats[i], text[s:e + 1])
    return row_of(ops) if d <= k else [0]


CASES = ((99, [24, 40], 2, 3000), (5, [33, 64, 65, 128], 7, 6000), (7, [8, 31, 97], 3, 4000), (11, [12], 11, 800))
_ref = {}


def case_ref(c, flags):
    """[(pattern, end, dist, start, ops)] sorted, of case c under `flags`; computed once"""
    if (c, flags) not in _ref:
        seed, lens, k, n = CASES[c]
        pats, text = R.planted(seed, lens, k, n)
        out = []
        for i, e, d, s in R.records_with_starts(text, pats, k, flags):
            assert s is not None
            dd, ops = script(pats[i], text[s:e + 1])
            assert dd == d
            out.append((i, e, d, s, ops))
        _ref[(c, flags)] = out
    return _ref[(c, flags)]


def test_reference_matrix_is_the_plain_one():
    rs = np.random.RandomState(3)
    for m, L, alphabet in ((1, 1, b"AC"), (5, 9, b"AC"), (12, 7, b"ACGT"), (40, 47, b"ab"), (33, 30, b"\x00\xff\n")):
        a = np.frombuffer(alphabet, dtype=np.uint8)
        p, t = a[rs.randint(0, len(a), size=m)].tobytes(), a[rs.randint(0, len(a), size=L)].tobytes()
        assert matrix(p, t).tolist() == matrix_plain(p, t)
    assert script(b"ACGTACGT", b"ACGACGT") == (1, [EQ, EQ, EQ, DEL, EQ, EQ, EQ, EQ])
    assert script(b"AAAA", b"AAAAA") == (1, [INS, EQ, EQ, EQ, EQ])           # the diagonal first, from the end
    assert row_of([EQ] * 16 + [DEL]) == [17, 0, 3] and row_of([SUB, INS]) == [2, 1 | 2 << 2]


@pytest.mark.parametrize("c", range(len(CASES)))
def test_reference_scripts_have_the_pinned_consequences(c):
    """#D - #I = m - L, n_ops = m + #I <= m + k, the ops that are not '=' are the distance, a span's first op is never I; and
    the cases hold what the GPU tests rely on: lengths on both sides of m, every W"""
    seed, lens, k, n = CASES[c]
    for flags in (ALL, LOCAL_MIN):
        recs = case_ref(c, flags)
        assert len(recs) >= 3 * len(lens)
        for i, e, d, s, ops in recs:
            m, L = lens[i], e + 1 - s
            assert ops.count(DEL) - ops.count(INS) == m - L and len(ops) == m + ops.count(INS) <= m + k
            assert len(ops) - ops.count(EQ) == d and ops[0] != INS
        assert {i for i, *_ in recs} == set(range(len(lens)))
        if k:
            assert any(e + 1 - s < lens[i] for i, e, _, s, _ in recs) and any(e + 1 - s > lens[i] for i, e, _, s, _ in recs)


# ---------------------------------------------------------------- 1. the host-level call
def find_raw(ctx, apm, text, flags, cap, stride):
    """apm_find_occ_align_buffer into sentinel rows: (status, ends, starts, rows as lists of `stride` words, total, counts)"""
    ends, starts = (apm.ApmMatch * max(cap, 1))(), (apm.ApmMatch * max(cap, 1))()
    ops = (ctypes.c_uint32 * max(cap * stride, 1))(*([SENT] * max(cap * stride, 1)))
    found, counts = ctypes.c_uint64(), (ctypes.c_uint64 * ctx.n_patterns)()
    rc = ctx._lib.apm_find_occ_align_buffer(ctx._ctx, bytes(text), len(text), flags, ends, starts, cap, ctypes.byref(found), counts, ops, stride)
    have = min(found.value, cap)
    return (rc, [(ends[q].pattern, ends[q].pos, ends[q].reserved) for q in range(have)],
            [(starts[q].pattern, starts[q].pos, starts[q].reserved) for q in range(have)],
            [list(ops[q * stride:(q + 1) * stride]) for q in range(cap)], found.value, list(counts))


@gpu
@pytest.mark.parametrize("c", range(len(CASES)))
def test_host_level_call(ctx, apm, c):
    seed, lens, k, n = CASES[c]
    pats, text = R.planted(seed, lens, k, n)
    setup(ctx, pats, k)
    words = ctx.occ_align_row_words()
    assert words == 1 + -(-(max(lens) + k) // 16)
    for flags in (ALL, LOCAL_MIN):
        want = case_ref(c, flags)
        cap = len(want) + 3
        for stride in ((words, words + 3) if flags == LOCAL_MIN else (words,)):
            rc, ends, starts, rows, total, counts = find_raw(ctx, apm, text, flags, cap, stride)
            assert rc == 0
            assert ends == [(i, e, d) for i, e, d, _, _ in want], (c, flags)
            assert starts == [(i, s, d) for i, _, d, s, _ in want], (c, flags)
            assert total == len(want) and counts == counts_of(want, len(lens))
            for q, (i, e, d, s, ops) in enumerate(want):
                row = row_of(ops)
                assert rows[q] == row + [SENT] * (stride - len(row)), (c, flags, stride, i, e)
            assert all(r == [SENT] * stride for r in rows[len(want):]), "rows without a record were written"
        assert [l for l, _ in ctx.launch_times()][-3:] == ["occ", "span", "oalign"]
        assert ctx.timing()["n_launches"] == 3
        rec, total, cnt = ctx.find_occ_align_buffer(text, flags, capacity=cap)
        assert rec == [(i, e, d, s, apm.ops_to_script(bytes(ops))) for i, e, d, s, ops in want]
        assert total == len(want) and cnt == counts_of(want, len(lens))
    # one word short of a row is refused, and nothing is written
    rc, _, _, rows, _, _ = find_raw(ctx, apm, text, LOCAL_MIN, 8, words - 1)
    assert rc == INVALID and all(r == [SENT] * (words - 1) for r in rows)
    # capacity 0: a count only -- neither spans nor scripts are launched
    rc, ends, _, _, total, counts = find_raw(ctx, apm, text, ALL, 0, words)
    assert rc == 0 and ends == [] and total == len(case_ref(c, ALL)) and counts == counts_of(case_ref(c, ALL), len(lens))
    assert [l for l, _ in ctx.launch_times()] == ["occ"]


@gpu
def test_capacity_below_the_records(ctx, apm):
    seed, lens, k, n = CASES[0]
    pats, text = R.planted(seed, lens, k, n)
    setup(ctx, pats, k)
    want = {(i, e): (d, s, ops) for i, e, d, s, ops in case_ref(0, ALL)}
    cap, stride = len(want) // 3, ctx.occ_align_row_words()
    rc, ends, starts, rows, total, _ = find_raw(ctx, apm, text, ALL, cap, stride)
    assert rc == 0 and total == len(want) and len(ends) == cap and ends == sorted(ends)
    for q, (i, e, d) in enumerate(ends):                        # an arbitrary subset, every row still its record's
        wd, ws, ops = want[(i, e)]
        assert (d, starts[q]) == (wd, (i, ws, wd))
        assert rows[q] == row_of(ops) + [SENT] * (stride - len(row_of(ops)))


# ---------------------------------------------------------------- 2. the text's edges
@gpu
def test_text_edges(ctx, apm):
    rs = np.random.RandomState(41)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    p = a[rs.randint(0, 4, size=37)].tobytes()
    filler = a[rs.randint(0, 4, size=300)].tobytes()
    k = 3
    setup(ctx, [p], k)
    # cut by the text's start: the pattern's first two bytes are missing, the script opens with D
    text = p[2:] + filler + p
    rec, total, _ = ctx.find_occ_align_buffer(text, LOCAL_MIN)
    want = [(i, e, d, s, apm.ops_to_script(bytes(script(p, text[s:e + 1])[1]))) for i, e, d, s in R.records_with_starts(text, [p], k, LOCAL_MIN)]
    assert rec == want and total == len(want)
    assert rec[0][:4] == (0, len(p) - 3, 2, 0) and rec[0][4] == "2D35="
    # ... and the text's last byte ends an exact occurrence
    assert rec[-1] == (0, len(text) - 1, 0, len(text) - 37, "37=")
    # n shorter than m: the whole text is the occurrence
    for text in (p[1:-1], p[:-3], p[3:]):
        rec, total, _ = ctx.find_occ_align_buffer(text, ALL)
        want = [(i, e, d, s, apm.ops_to_script(bytes(script(p, text[s:e + 1])[1]))) for i, e, d, s in R.records_with_starts(text, [p], k, ALL)]
        assert rec == want and total == len(want) and want
        assert (0, len(text) - 1) in [(r[3], r[1]) for r in rec]


# ---------------------------------------------------------------- 3. the device-level call on hand-made pairs
def pack_pairs(pairs):
    """(end records, span records), garbage in every fourth dword: the pass ignores both"""
    ends = b"".join(struct.pack("<QII", e, i, 0xDEAD0000 + q) for q, ((i, e), _) in enumerate(pairs))
    spans = b"".join(struct.pack("<QII", s, j, 0xBEEF0000 + q) for q, (_, (j, s)) in enumerate(pairs))
    return ends, spans


def run_pairs(ctx, dev, d_text, text_off, text_len, n_total, pairs, stride, extra_rows=2, count_beyond=5):
    """the device call over hand-made pairs into sentinel rows: the rows as lists, those behind the capacity included"""
    ends, spans = pack_pairs(pairs)
    n_rows = len(pairs) + extra_rows
    d_end, d_span = dev.alloc(len(ends), ends), dev.alloc(len(spans), spans)
    d_n = dev.counter(len(pairs) + count_beyond)                 # (*d_n_rec may exceed the capacity)
    d_ops = dev.alloc(4 * stride * n_rows, struct.pack("<I", SENT) * (stride * n_rows))
    ctx.occ_align_device(d_text, text_off, text_len, n_total, d_end, d_span, len(pairs), d_n, d_ops, stride)
    ctx.synchronize()
    raw = struct.unpack("<%dI" % (stride * n_rows), ctx.device_download(d_ops, 4 * stride * n_rows))
    assert ctx.device_download(d_end, len(ends)) == ends and ctx.device_download(d_span, len(spans)) == spans   # only read
    return [list(raw[q * stride:(q + 1) * stride]) for q in range(n_rows)]


def triage_case():
    return R.planted(4242, [33, 97], 3, 8192, copies=4)


@gpu
def test_device_call_triage(ctx, apm):
    pats, text = triage_case()
    k, n, m = 3, len(text), (33, 97)
    setup(ctx, pats, k)
    lo, hi = 1000, 6000                                         # the shard text handed to the pass
    real = [(i, e, s) for i, e, _, s in R.records_with_starts(text, pats, k, LOCAL_MIN)]
    inside = [r for r in real if lo < r[2] and r[1] < hi]
    outside = [r for r in real if r[1] < lo or r[2] >= hi]
    assert len(inside) >= 6 and len(outside) >= 4 and {i for i, _, _ in inside} == {0, 1}
    e0 = 3001                                                   # an end of nothing in particular
    assert R.global_dist(pats[0], text[e0 - 32:e0 + 1]) > k and R.global_dist(pats[1], text[e0 - 99:e0 + 1]) > k
    cases = {                                                   # name -> ((pattern, e), (pattern, s)), what its row must be
        "invalid pattern": (((2, 3000), (2, 2990)), [DIST_INVALID]),
        "pattern 0xffffffff": (((0xFFFFFFFF, 3000), (0xFFFFFFFF, 2990)), [DIST_INVALID]),
        "e == n_total": (((0, n), (0, n - 32)), [DIST_INVALID]),
        "e far beyond n_total": (((1, 1 << 40), (1, (1 << 40) - 96)), [DIST_INVALID]),
        "mismatched patterns": (((0, inside[0][1]), (1, inside[0][2])), [DIST_INVALID]),
        "no start": (((0, e0), (0, NO_START)), [0]),
        "no start outside the shard": (((1, 7000), (1, NO_START)), [0]),
        "s > e": (((0, e0), (0, e0 + 1)), [DIST_INVALID]),
        "L = m + k + 1": (((0, e0), (0, e0 - (m[0] + k))), [0]),
        "L = m - k - 1": (((1, e0), (1, e0 + 2 - (m[1] - k))), [0]),
        "L = m + k + 1 outside the shard": (((0, 7000), (0, 7000 - (m[0] + k))), [0]),   # decided with no look at the text
        "L = m + k, farther than k": (((0, e0), (0, e0 + 1 - (m[0] + k))), [0]),
        "L = m - k, farther than k": (((1, e0), (1, e0 + 1 - (m[1] - k))), [0]),
        "L = m, farther than k": (((0, e0), (0, e0 - 32)), [0]),
        "straddles the shard's start": (((0, lo + 10), (0, lo + 10 - 32)), None),
        "straddles the shard's end": (((1, hi + 20), (1, hi + 20 - 96)), None),
        "ends at the shard's last byte": (((0, hi - 1), (0, hi - 33)), "ref"),
        "begins at the shard's first byte": (((1, lo + 96), (1, lo)), "ref"),
    }
    for q, (i, e, s) in enumerate(outside[:4]):
        cases["another shard's %d" % q] = (((i, e), (i, s)), None)
    for q, (i, e, s) in enumerate(inside):
        cases["real %d" % q] = (((i, e), (i, s)), "ref")
        if q < 4:                                               # made-up spans around a real one: a byte more, a byte less
            cases["real %d, a byte earlier" % q] = (((i, e), (i, s - 1)), "ref")
            cases["real %d, a byte later" % q] = (((i, e), (i, s + 1)), "ref")
    names = sorted(cases, key=lambda nm: zlib.crc32(nm.encode()))   # the kinds interleaved, in an order of no meaning
    pairs = [cases[nm][0] for nm in names]
    stride = ctx.occ_align_row_words() + 1
    assert stride == 1 + 7 + 1
    with Dev(ctx) as dev:
        d_text = dev.text(text, lo, hi, mis=7)
        rows = run_pairs(ctx, dev, d_text, lo, hi - lo, n, pairs, stride)
        assert [l for l, _ in ctx.launch_times()] == ["oalign"]
        # the refusals: a short stride, a d_ops that is not 4-byte aligned, records that are not 16-byte aligned, NULL pointers
        ends, spans = pack_pairs(pairs)
        d_end, d_span, d_n = dev.alloc(len(ends), ends), dev.alloc(len(spans), spans), dev.counter(len(pairs))
        d_ops = dev.alloc(4 * stride * len(pairs) + 16, struct.pack("<I", SENT) * (stride * len(pairs) + 4))
        good = dict(d_end=d_end, d_span=d_span, d_n=d_n, d_ops=d_ops, stride=stride, cap=len(pairs))
        for change in (dict(stride=stride - 2), dict(d_ops=d_ops + 2), dict(d_ops=d_ops + 1), dict(d_span=d_span + 8), dict(d_end=d_end + 4),
                       dict(d_ops=None), dict(d_span=None), dict(d_end=None), dict(d_n=None)):
            a = dict(good, **change)
            with pytest.raises(apm.ApmError) as err:
                ctx.occ_align_device(d_text, lo, hi - lo, n, a["d_end"], a["d_span"], a["cap"], a["d_n"], a["d_ops"], a["stride"])
            assert err.value.status == INVALID, change
        ctx.synchronize()
        assert ctx.device_download(d_ops, 4 * stride * len(pairs)) == struct.pack("<I", SENT) * (stride * len(pairs)), "a refused call wrote"
    assert rows[len(pairs):] == [[SENT] * stride] * 2, "rows at or beyond capacity were written"
    scripts = 0
    for nm, row in zip(names, rows):
        ((i, e), (_, s)), want = cases[nm]
        if want is None:
            assert row == [SENT] * stride, nm
            continue
        if want == "ref":
            want = pair_row(text, pats, k, i, e, s)
            scripts += want != [0]
        assert row == want + [SENT] * (stride - len(want)), nm
    assert scripts >= len(inside)
    assert pair_row(text, pats, k, 0, hi - 1, hi - 33) == [0]    # (the two pairs at the shard's edges are covered, and decided)


def line_case():
    """(patterns, T, L): 4 KiB of DNA, L odd; an occurrence with a byte taken out begins 20 bytes in front of T[L], one with a
    byte put in 300 behind it, exact copies elsewhere"""
    rs = np.random.RandomState(2032)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = bytearray(a[rs.randint(0, 4, size=4096)].tobytes())
    pats = [a[rs.randint(0, 4, size=m)].tobytes() for m in (40, 100)]
    L = 2049
    short, longer = bytearray(pats[0]), bytearray(pats[1])
    del short[11]
    longer.insert(50, ord("A") if longer[50] != ord("A") else ord("C"))
    text[L - 20:L - 20 + len(short)] = short
    text[L + 300:L + 300 + len(longer)] = longer
    text[100:140], text[3500:3600] = pats[0], pats[1]
    return pats, bytes(text), L


@gpu
@pytest.mark.parametrize("base", [LINE - 2049, (1 << 33) + 5])
def test_shard_beyond_4gib(ctx, base):
    """a shard of 4 KiB at a global offset: a pair on each side of position 2^32 and one across it, and one beyond 2^33"""
    pats, text, L = line_case()
    k, n = 3, len(text)
    setup(ctx, pats, k)
    local = R.records_with_starts(text, pats, k, LOCAL_MIN)
    assert (0, L + 18, 1, L - 20) in local and (1, L + 400, 1, L + 300) in local and len(local) >= 4
    pairs = [((i, e + base), (i, s + base)) for i, e, _, s in local]
    pairs += [((0, base - 1), (0, base - 40)), ((1, base + n + 99), (1, base + n)), ((0, base + 10), (0, base - 29))]
    if base + L == LINE:
        assert any(s < LINE <= e for (_, e), (_, s) in pairs) and min(e for (_, e), _ in pairs) < LINE - 1000
    stride = ctx.occ_align_row_words()
    with Dev(ctx) as dev:
        rows = run_pairs(ctx, dev, dev.text(text, mis=3), base, n, base + n, pairs, stride)
    for q, (i, e, d, s) in enumerate(local):
        want = pair_row(text, pats, k, i, e, s)
        assert want[0] >= len(pats[i]) and rows[q] == want + [SENT] * (stride - len(want)), (i, e)
    # in front of the shard: another shard's; behind n_total: invalid; begins in front of the shard: another shard's
    assert rows[len(local):] == [[SENT] * stride, [DIST_INVALID] + [SENT] * (stride - 1), [SENT] * stride] + [[SENT] * stride] * 2


# ---------------------------------------------------------------- 4. a text mode
@gpu
def test_fasta_upper_rows_are_the_normalised_texts(ctx, apm):
    rs = np.random.RandomState(31)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = [a[rs.randint(0, 4, size=s)].tobytes() for s in (700, 900)]
    pats = [seq[0][290:330], seq[1][100:133]]
    occ = bytearray(pats[0])
    del occ[7]                                                  # one more copy, a byte short, in the second sequence
    seq[1] = seq[1][:520] + bytes(occ) + seq[1][520 + len(occ):]
    src = b""
    for name, s in zip((b">one first\n", b">two\n"), seq):
        body = b"\n".join(s[i:i + 60] for i in range(0, len(s), 60))   # a line break inside every occurrence
        src += name + body.lower() + b"\n"
    keep, hdr = [], False
    for off, c in enumerate(src):
        if c == ord(">") and (off == 0 or src[off - 1] == 10):
            hdr = True
        if hdr:
            hdr = c != 10
        elif c not in (10, 13):
            keep.append(off)
    T = bytes(src[o] for o in keep).upper()
    assert T == seq[0] + seq[1]
    k = 2
    setup(ctx, pats, k)
    ctx.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
    try:
        for flags in (ALL, LOCAL_MIN):
            want = R.records_with_starts(T, pats, k, flags)
            rec, total, cnt = ctx.find_occ_align_buffer(src, flags)
            # positions are source offsets, the scripts those of the normalised text
            assert rec == [(i, keep[e], d, keep[s], apm.ops_to_script(bytes(script(pats[i], T[s:e + 1])[1]))) for i, e, d, s in want], flags
            assert total == len(want) and cnt == counts_of(want, 2)
            assert [l for l, _ in ctx.launch_times()][-3:] == ["occ", "span", "oalign"]
        assert (0, keep[329], 0, keep[290], "40=") in rec and any(r[0] == 0 and r[2] == 1 and r[4].count("D") == 1 for r in rec)
    finally:
        ctx.set_text_mode(0)


# ---------------------------------------------------------------- 5. what the call leaves alone
@gpu
def test_counting_calls_are_untouched(ctx):
    pats, text = triage_case()
    setup(ctx, pats, 3)
    before = (ctx.count_buffer(text), [ctx.pattern_kernel(i) for i in range(2)])
    ctx.find_occ_align_buffer(text, LOCAL_MIN)
    assert [l for l, _ in ctx.launch_times()] == ["occ", "span", "oalign"]
    ctx.find_occ_align_buffer(text, ALL)
    assert (ctx.count_buffer(text), [ctx.pattern_kernel(i) for i in range(2)]) == before
    assert before[0] == H.oracle_counts(text, pats, 3)
    rec, _, _ = ctx.find_occ_buffer(text, LOCAL_MIN)            # the plain occurrence call still runs its two launches
    assert [l for l, _ in ctx.launch_times()] == ["occ", "span"] and rec


@gpu
def test_unsupported_sets(ctx, apm):
    for pats, k in (([b"ACGT" * 32 + b"A", b"ACGTAC"], 2), ([b"ACGTACGT", b"ACG"], 3)):     # m = 129; k >= m
        setup(ctx, pats, k)
        for call in (ctx.occ_align_row_words, lambda: ctx.find_occ_align_buffer(b"ACGT" * 64, ALL)):
            with pytest.raises(apm.ApmError) as e:
                call()
            assert e.value.status == O.UNSUPPORTED


# ---------------------------------------------------------------- 6. the command-line host
def render(text, pats, k, flags):
    recs = R.records_with_starts(text, pats, k, flags)
    lines = ["Number of matches for pattern <%s>: %d" % (p.decode(), sum(r[0] == i for r in recs)) for i, p in enumerate(pats)]
    for i, p in enumerate(pats):
        lines.append("Occurrences for pattern <%s>:" % p.decode() + "".join(
            " %d-%d:%d:%s" % (s, e, d, H.pkg().ops_to_script(bytes(script(p, text[s:e + 1])[1]))) for j, e, d, s in recs if j == i))
    return lines


@gpu
def test_cli_occurrence_scripts(tmp_path):
    pats, text = R.planted(99, [24, 40], 2, 3000, copies=2)
    path = tmp_path / "text.txt"
    path.write_bytes(text)
    base = ["2", str(path)] + [p.decode() for p in pats]
    for flag, flags in (("--occurrence-scripts", LOCAL_MIN), ("--occurrence-scripts=best", LOCAL_MIN), ("--occurrence-scripts=all", ALL)):
        r = run_cli(base + [flag])
        assert r.returncode == 0, r.stderr
        lines = [l for l in r.stdout.splitlines() if l.startswith(("Number of matches", "Occurrences for"))]
        assert lines == render(text, pats, 2, flags), flag
        assert any("D" in l.split(":", 1)[1] for l in lines[2:]) and any("I" in l.split(":", 1)[1] for l in lines[2:])
    for other in ("--positions", "--distances", "--alignments", "--best", "--best=2"):
        r = run_cli(base + ["--occurrence-scripts", other])
        assert r.returncode == 1 and "--occurrence-scripts" in r.stderr, other
    assert run_cli(base + ["--occurrence-scripts=worst"]).returncode == 1
    assert run_cli(base + ["--occurrences", "--alignments"]).returncode == 1


@gpu
def test_cli_occurrence_scripts_fasta_sequences(tmp_path):
    pats, body = R.planted(98, [30], 2, 600, copies=1)
    src = b">chr1 test\n" + b"\n".join(body[i:i + 50] for i in range(0, 300, 50)).lower() + b"\n>chr2\n" + \
          b"\n".join(body[i:i + 50] for i in range(300, 600, 50)) + b"\n"
    path = tmp_path / "text.fa"
    path.write_bytes(src)
    recs = R.records_with_starts(body, pats, 2, LOCAL_MIN)
    assert recs
    r = run_cli(["2", str(path), pats[0].decode(), "--fasta", "--upper", "--sequences", "--occurrence-scripts"])
    assert r.returncode == 0, r.stderr
    want = []
    for _, e, d, s in recs:
        if (s < 300) == (e < 300):                              # inside one sequence
            want.append("%s:%d-%d:%d:%s" % ("chr1" if s < 300 else "chr2", s % 300, e - s + 1, d,
                                            H.pkg().ops_to_script(bytes(script(pats[0], body[s:e + 1])[1]))))
    line = [l for l in r.stdout.splitlines() if l.startswith("Occurrences for")]
    assert line == ["Occurrences for pattern <%s>:" % pats[0].decode() + "".join(" " + w for w in want)]
    assert "Number of matches for pattern <%s>: %d" % (pats[0].decode(), len(recs)) in r.stdout
