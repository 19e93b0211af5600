"""The align pass on the GPU: apm_find_all_align_buffer and apm_align_shard_device write every record's edit script --
the canonical one of include/apm.h: walk back from (size, size), the diagonal first, else D, else I -- into its row of
ops.  Every comparison is over the complete record set and checks both (a) bit equality with the Python reference (the
literal full matrix and the walk for windows of up to 64 bytes, the same walk on a band of half-width k/2 beyond; the
two are asserted to agree on the short windows) and (b), independently of that reference, that applying the script to p
yields t, that '=' sits only on equal bytes and 'X' only on different ones, and that the number of ops that are not '='
equals the record's `reserved` and helpers.window_distance."""
import ctypes
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
PRESET = 0x5A5A5A5A
UNSUPPORTED = -6
BAD_ARGUMENT = -1
DNA = b"ACGT"
EQ, SUB, INS, DEL = 0, 1, 2, 3
INF = 1 << 20


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


# ---------------------------------------------------------------- the reference scripts
def _walk(size, D):
    """the walk back from (size, size) over D[x][y] = the op the rule takes at cell (x, y), x, y >= 1; ops first to last"""
    ops, x, y = [], size, size
    while x > 0 or y > 0:
        op = INS if y == 0 else (DEL if x == 0 else int(D[x][y]))
        ops.append(op)
        x -= op != DEL
        y -= op != INS
    return bytes(reversed(ops))


def literal_script(p, t):
    """the literal full matrix, cell(x, y): x text bytes against y pattern bytes, the rule at every cell -- the diagonal
    if cell(x-1, y-1) + (p[y-1] != t[x-1]) == cell(x, y), else D if cell(x, y-1) + 1 == cell(x, y), else I -- and the
    walk; (dist, ops)"""
    size = len(p)
    c = [[0] * (size + 1) for _ in range(size + 1)]
    D = [[0] * (size + 1) for _ in range(size + 1)]
    for x in range(size + 1):
        c[x][0] = x
    for y in range(size + 1):
        c[0][y] = y
    for x in range(1, size + 1):
        row, above, drow, tc = c[x], c[x - 1], D[x], t[x - 1]
        for y in range(1, size + 1):
            neq = p[y - 1] != tc
            diag = above[y - 1] + neq
            v = min(diag, above[y] + 1, row[y - 1] + 1)
            row[y] = v
            drow[y] = (SUB if neq else EQ) if diag == v else (DEL if row[y - 1] + 1 == v else INS)
    return c[size][size], _walk(size, D)


def band_scripts(p, ts, h):
    """the same recurrence and walk on the band |x - y| <= h, for all windows `ts` (each len(p) bytes) of one pattern
    side by side: column by column, the vertical dependency as a running minimum; [(band distance, ops)], ops None
    where the band's corner is INF-like (no path inside the band)"""
    size, W = len(p), len(ts)
    P = np.frombuffer(p, np.uint8).astype(np.int32)
    T = np.frombuffer(b"".join(ts), np.uint8).reshape(W, size).astype(np.int32)
    idx = np.arange(size + 1, dtype=np.int32)
    prev = np.broadcast_to(np.where(idx <= h, idx, INF).astype(np.int32), (W, size + 1)).copy()
    dirs = np.zeros((W, size + 1, size + 1), np.uint8)        # [w, x, y]: the op the rule takes at cell (x, y)
    for x in range(1, size + 1):
        neq = (P[None, :] != T[:, x - 1, None]).astype(np.int32)
        diag = prev[:, :-1] + neq
        c = np.empty((W, size + 1), np.int32)
        c[:, 0] = x
        c[:, 1:] = np.minimum(diag, prev[:, 1:] + 1)
        outside = np.abs(idx - x) > h
        c[:, outside] = INF
        nv = np.minimum.accumulate(c - idx, axis=1) + idx     # cell(x, y) = min over j <= y of c[j] + (y - j)
        nv[:, outside] = INF
        dirs[:, x, 1:] = np.where(diag == nv[:, 1:], neq, np.where(nv[:, :-1] + 1 == nv[:, 1:], DEL, INS))
        prev = nv
    out = []
    for w in range(W):
        d = int(prev[w, size])
        if d >= INF // 2:
            out.append((d, None))
            continue
        out.append((d, _walk(size, dirs[w])))
    return out


_script_cache = {}


def ref_scripts(pairs, k):
    """{(p, t): ops} for the (p, t) pairs, every one within k"""
    todo = {}
    for p, t in set(pairs):
        if (p, t, k) not in _script_cache:
            todo.setdefault(p, []).append(t)
    for p, ts in todo.items():
        for lo in range(0, len(ts), 128):                     # (the direction cube of a batch: 128 (size + 1)^2 bytes)
            part = ts[lo:lo + 128]
            for t, (d, ops) in zip(part, band_scripts(p, part, k // 2)):
                if len(p) <= 64:                              # the reference proper; the band must agree with it
                    dl, lit = literal_script(p, t)
                    assert (d, ops) == (dl, lit), (p, t, k)
                assert d <= k and ops is not None
                _script_cache[(p, t, k)] = ops
    return {(p, t): _script_cache[(p, t, k)] for p, t in pairs}


def check_script(p, t, ops, dist):
    """(b): the script alone, against the two strings"""
    out, x, y = bytearray(), 0, 0
    for op in ops:
        if op == EQ:
            assert p[y] == t[x]
            out.append(p[y])
        elif op == SUB:
            assert p[y] != t[x]
            out.append(t[x])
        elif op == INS:
            out.append(t[x])
        else:
            assert op == DEL
        x += op != DEL
        y += op != INS
    assert y == len(p) and x == len(t) and bytes(out) == t
    assert sum(1 for op in ops if op != EQ) == dist == H.window_distance(p, t)


# ---------------------------------------------------------------- the reference records (as test_score_gpu.py has them)
def _positions(text, pat, k):
    """matching window starts: short patterns window by window, long ones by bisection over the oracle's range counts"""
    if len(pat) <= 64:
        return [j for j in range(max(0, len(text) - k)) if H.window_distance(*window(text, pat, j)) <= k]
    banded = 8 * k <= len(pat)
    out = []

    def count(a, b):
        return H.oracle_counts(text, [pat], k, banded=banded, j_begin=a, j_end=b)[0]

    def descend(a, b, cnt):
        if cnt == 0:
            return
        if cnt == b - a:
            out.extend(range(a, b))
            return
        mid = (a + b) // 2
        left = count(a, mid)
        descend(a, mid, left)
        descend(mid, b, cnt - left)

    end = max(0, len(text) - k)
    if end:
        descend(0, end, count(0, end))
    return out


def window(text, pat, pos):
    size = min(len(pat), len(text) - pos)
    return pat[:size], text[pos:pos + size]


_ref_cache = {}


def ref_records(text, pats, k):
    """[(pattern, pos, dist, ops)] sorted: what apm_find_all_align_buffer returns"""
    key = (text, tuple(pats), k)
    if key not in _ref_cache:
        where = [(i, j) for i, p in enumerate(pats) for j in _positions(text, p, k)]
        scripts = ref_scripts([window(text, pats[i], j) for i, j in where], k)
        rec = []
        for i, j in where:
            p, t = window(text, pats[i], j)
            ops = scripts[(p, t)]
            rec.append((i, j, sum(1 for op in ops if op != EQ), ops))
        _ref_cache[key] = rec
    return _ref_cache[key]


def rand(rng, n, alphabet=DNA):
    return bytes(rng.choice(alphabet) for _ in range(n))


def edited(rng, p, e):
    """p under e edits that keep its length: substitutions at distinct places, now and then a deletion + an insertion"""
    w = bytearray(p)
    e = min(e, len(w))
    if e >= 2 and len(w) > 8 and rng.random() < 0.5:
        i, j = sorted(rng.sample(range(1, len(w) - 1), 2))
        del w[i]
        w.insert(j, rng.choice(DNA))
        e -= 2
    for at in rng.sample(range(len(w)), e):
        w[at] = rng.choice([c for c in DNA if c != w[at]])
    return bytes(w)


def planted(k, lens, seed, edits=None, gaps=8192):
    """`gaps` bytes of random DNA cut into pieces, between them a copy of every pattern at e edits for every e of `edits`
    (default 0..k); the copies' start offsets run through all 16 residues mod 16"""
    rng = random.Random(seed)
    pats = [rand(rng, m) for m in lens]
    plants = [(i, e) for e in (range(k + 1) if edits is None else edits) for i in range(len(pats))]
    while len(plants) < 16:
        plants = plants + plants
    gap = gaps // (len(plants) + 1)
    text, starts = bytearray(), []
    for q, (i, e) in enumerate(plants):
        text += rand(rng, gap)
        while len(text) % 16 != q % 16:
            text += rand(rng, 1)
        starts.append(len(text))
        text += edited(rng, pats[i], e)
    text += rand(rng, gap)
    assert {s % 16 for s in starts} == set(range(16)) and len(text) <= 65536
    return pats, bytes(text)


def same_records(got, want, text, pats):
    """(a) and (b) over the complete record set"""
    assert [(i, j, d) for i, j, d, _ in got] == [(i, j, d) for i, j, d, _ in want]
    for (i, j, d, ops), (_, _, _, ref) in zip(got, want):
        assert ops == ref, (i, j, d)
        check_script(*window(text, pats[i], j), ops, d)


def align_call(ctx, text, pats, k, want=None):
    """find_all_align_buffer == the reference, record for record, and every script stands on its own"""
    want = ref_records(text, pats, k) if want is None else want
    got, total = ctx.find_all_align_buffer(text, len(want) + 64)
    assert total == len(want)
    same_records(got, want, text, pats)
    return want


# ---------------------------------------------------------------- 1. planted edits
LENS = (1, 4, 15, 16, 17, 31, 33, 64, 129, 513)


@pytest.mark.parametrize("k", (0, 1, 2, 3, 6, 7, 8, 9, 16))
def test_planted_edits(ctx, k):
    # (from k = 6 on the short patterns match most windows: fewer plants and less filler keep the record set small)
    pats, text = planted(k, LENS, 2000 + k) if k < 6 else planted(k, LENS, 2000 + k, edits=sorted({0, 1, 2, k // 2, k - 1, k}), gaps=1024)
    want = ref_records(text, pats, k)
    if k >= 2:                                                  # (on the reference alone: not a test of substitutions only)
        assert any(INS in ops and DEL in ops for _, _, _, ops in want)
    assert any(SUB in ops for _, _, _, ops in want) or k == 0
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert ctx.align_row_words() == 1 + (513 + min(k // 2, 512) + 15) // 16
    align_call(ctx, text, pats, k, want)


# ---------------------------------------------------------------- 2. ties
def test_tie_takes_the_diagonal(ctx):
    """AB against BA at k = 2: two substitutions, not D = I"""
    text = b"CCCCCCCCBACCCCCCCCCC"
    ctx.set_kernel("auto")
    ctx.set_patterns([b"AB"], 2)
    want = align_call(ctx, text, [b"AB"], 2)
    assert (0, 8, 2, bytes([SUB, SUB])) in want


def test_low_entropy_every_lane_busy(ctx):
    k = 3
    text = b"A" * 4096
    pats = [b"A" * 20, b"A" * 19 + b"C"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    want = align_call(ctx, text, pats, k)
    assert len(want) == 2 * (len(text) - k)
    assert all(ops == bytes(min(20, len(text) - j)) for i, j, _, ops in want if i == 0)
    # the C is a substitution at the window's end; the tail windows lose it
    assert all(ops == (bytes(19) + bytes([SUB]) if j + 20 <= len(text) else bytes(len(text) - j)) for i, j, _, ops in want if i == 1)


# ---------------------------------------------------------------- 3. the wave form beyond 64 diagonals
def test_wave_form_with_more_than_64_cells(ctx):
    """m = 200, k = 130: 131 diagonals, three chunks of the wave form"""
    k = 130
    pats, text = planted(k, (200,), 77, edits=(0, 1, 2, 63, 64, 65, 66, 129, 130), gaps=2048)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    want = align_call(ctx, text, pats, k)
    ds = [d for _, _, d, _ in want]
    assert min(ds) == 0 and max(ds) > 64 and len(want) > len(text) // 2
    assert max(ops.count(INS) for _, _, _, ops in want) > 32    # paths that leave the first chunk of diagonals


# ---------------------------------------------------------------- 4. k >= m
def test_k_at_least_m_every_window_has_a_script(ctx):
    rng = random.Random(5)
    text = rand(rng, 3000)
    for k, lens in ((3, (1, 2, 3)), (9, (3, 5, 8, 9)), (16, (16, 7))):     # lane form and wave form
        pats = [rand(rng, m) for m in lens]
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        want = align_call(ctx, text, pats, k)
        assert len(want) == len(pats) * (len(text) - k)
        assert all(d <= min(len(pats[i]), len(text) - j) for i, j, d, _ in want)


# ---------------------------------------------------------------- 5. truncated tails, texts shorter than the patterns
@pytest.mark.parametrize("k", [0, 2, 3, 7, 9, 16])
def test_truncated_tails(ctx, k):
    """windows with size < m at the end of the text: the last bytes are a truncated copy of every pattern in turn"""
    rng = random.Random(40 + k)
    pats = [rand(rng, m) for m in (12, 20, 33, 70, 129, 300)]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    for p in pats:
        cut = len(p) * 2 // 3
        text = rand(rng, 2000) + p[:cut]
        want = align_call(ctx, text, pats, k)
        if cut > k:                                                    # (window starts end at n - k)
            assert (pats.index(p), 2000, 0, bytes(cut)) in want


@pytest.mark.parametrize("k", [0, 1, 3, 9])
def test_text_shorter_than_the_patterns(ctx, k):
    rng = random.Random(50 + k)
    pats = [rand(rng, m) for m in (20, 31, 64, 200)] + [b"A", b"AC"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    for text in (pats[0][:15], pats[2][:18] + b"T", b"A", b"C", rand(rng, 19)):   # n < m, and a one-byte text
        want = align_call(ctx, text, pats, k)
        if text == pats[0][:15]:
            assert (0, 0, 0, bytes(15)) in want                         # the whole text is a truncated copy
        if text == b"A" and k == 0:
            assert (4, 0, 0, bytes(1)) in want and (5, 0, 0, bytes(1)) in want


# ---------------------------------------------------------------- 6. a lane reuses its trace row
def test_trace_rows_are_reused(ctx):
    """the 4096-byte pattern makes a trace row 8 KiB: the budget then holds fewer rows than the full grid has lanes, and
    more records than rows means a lane aligns a second record over the trace of its first"""
    k = 3
    rng = random.Random(6)
    pats = [b"A" * 20, bytes(rng.choice(b"CGT") for _ in range(4096))]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert ctx.stat("align_rows") == 0                                   # no align launch since the patterns were set
    align_call(ctx, b"A" * 64, pats, k)
    rows = int(ctx.stat("align_rows"))
    text = b"A" * (rows + 700)
    assert len(text) <= 65536
    want = align_call(ctx, text, pats, k)
    assert len(want) > int(ctx.stat("align_rows")) == rows > 0
    assert all(i == 0 for i, _, _, _ in want)


# ---------------------------------------------------------------- 7. foreign records
def _records(rows):
    return b"".join(struct.pack("<QII", pos, pat, PRESET) for pat, pos in rows)


def _dwords(raw):
    return list(struct.unpack("<%dI" % (len(raw) // 4), raw))


def _row(stride, ops):
    """a preset row after the align pass: ops = bytes (a script), 0 (farther than k), INVALID or None (untouched)"""
    row = [PRESET] * stride
    if ops is None:
        return row
    if isinstance(ops, int):
        row[0] = ops
        return row
    row[0] = len(ops)
    for w in range((len(ops) + 15) // 16):
        row[1 + w] = sum(op << (2 * q) for q, op in enumerate(ops[16 * w:16 * w + 16]))
    return row


@pytest.mark.parametrize("k", [3, 9])
def test_foreign_records_through_align_shard_device(ctx, k):
    """hand-made records, every row preset: scripts for the windows inside the shard and within k, word 0 = 0 for those
    farther, untouched rows for windows that cross the shard's ends, APM_DIST_INVALID for records that name no window;
    every word the row format leaves alone keeps the preset, the records keep every bit"""
    rng = random.Random(60 + k)
    pats = [rand(rng, m) for m in (24, 40, 90)]
    n = 4096
    text = bytearray(rand(rng, n))
    text[1500:1524] = pats[0]
    text[1700:1740] = edited(rng, pats[1], 2)
    text[2200:2290] = edited(rng, pats[2], k)
    text[n - 10:] = pats[0][:10]
    text = bytes(text)
    off, length = 1000, 2000                                            # the shard: [1000, 3000) of [0, 4096)
    rows = [(0, 1500), (1, 1700), (2, 2200),                            # inside, within k
            (0, 1000), (1, 2960), (2, 2910), (0, 2976),                  # inside, the first and the last window that fit
            (2, 1100), (1, 1234), (0, 2001),                             # inside, random windows: farther than k
            (0, 2977), (1, 2961), (2, 2999), (0, 999), (2, 0), (1, 3000), (0, n - 10),   # cross an end of the shard: untouched
            (3, 1500), (0xFFFFFFFF, 1500), (0, n), (1, 1 << 40)]         # pattern == n_patterns, pos == n_total: invalid
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    stride = ctx.align_row_words() + 3
    inside = [(pat, pos) for pat, pos in rows if pat < len(pats) and pos < n and pos >= off and pos + min(len(pats[pat]), n - pos) <= off + length]
    near = [w for w in (window(text, pats[pat], pos) for pat, pos in inside) if H.window_distance(*w) <= k]
    scripts = ref_scripts(near, k)
    want = []
    for pat, pos in rows:
        if pat >= len(pats) or pos >= n:
            want.append(_row(stride, INVALID))
        elif (pat, pos) not in inside:
            want.append(_row(stride, None))
        else:
            want.append(_row(stride, scripts.get(window(text, pats[pat], pos), 0)))
    assert len(near) >= 3 and sum(r[0] == 0 for r in want) >= 3 and sum(r[0] == PRESET for r in want) == 7 and sum(r[0] == INVALID for r in want) == 4
    for w in near:
        check_script(*w, scripts[w], H.window_distance(*w))
    d_text, d_rec, d_n = ctx.device_alloc(length + 16), ctx.device_alloc(16 * (len(rows) + 8)), ctx.device_alloc(16)
    d_ops = ctx.device_alloc(4 * stride * (len(rows) + 8))
    try:
        ctx.device_upload(d_text, text[off:off + length])
        ctx.device_upload(d_rec, _records(rows))
        ctx.device_upload(d_n, struct.pack("<Q", len(rows)))
        ctx.device_memset(d_ops, 0x5A, 4 * stride * (len(rows) + 8))
        ctx.align_shard_device(d_text, off, length, n, d_rec, len(rows), d_n, d_ops, stride)
        ctx.synchronize()
        assert ctx.device_download(d_rec, 16 * len(rows)) == _records(rows)               # bit-identical
        got = _dwords(ctx.device_download(d_ops, 4 * stride * (len(rows) + 8)))
        assert [got[r * stride:(r + 1) * stride] for r in range(len(rows) + 8)] == want + [_row(stride, None)] * 8
        # *d_n_rec beyond capacity: `capacity` records are aligned, the rows behind them keep every bit
        cap = 6
        ctx.device_upload(d_n, struct.pack("<Q", cap + 4))
        ctx.device_memset(d_ops, 0x5A, 4 * stride * (len(rows) + 8))
        ctx.align_shard_device(d_text, off, length, n, d_rec, cap, d_n, d_ops, stride)
        ctx.synchronize()
        got = _dwords(ctx.device_download(d_ops, 4 * stride * (cap + 4)))
        assert [got[r * stride:(r + 1) * stride] for r in range(cap + 4)] == want[:cap] + [_row(stride, None)] * 4
    finally:
        for d in (d_text, d_rec, d_n, d_ops):
            ctx.device_free(d)


# ---------------------------------------------------------------- 8. two shards, one buffer
def _shard_text(ctx, text, lo, hi, mis):
    d = ctx.device_alloc(hi - lo + 32)
    ctx.device_upload(d + mis, text[lo:hi])
    return d


def _device_records(apm, ctx, d_rec, d_ops, total, stride):
    """the records and their rows off the device, sorted by (pattern, pos): [(pattern, pos, dist, ops)]"""
    rec = [struct.unpack_from("<QII", ctx.device_download(d_rec, 16 * total), 16 * i) for i in range(total)]
    rows = _dwords(ctx.device_download(d_ops, 4 * stride * total))
    return sorted((pat, pos, d, apm.unpack_ops(rows[r * stride:(r + 1) * stride])) for r, (pos, pat, d) in enumerate(rec))


@pytest.mark.parametrize("k,mis", [(3, 0), (3, 1), (3, 15), (9, 4), (9, 15)])
def test_two_shards_one_buffer(apm, ctx, k, mis):
    """find on both shards, score on both, align on both, all on one stream with one synchronisation at the end: every
    record ends with its distance and its script, whichever shard holds its window"""
    pats, text = planted(k, (16, 33, 64, 129), 70 + k)
    n = len(text)
    want = ref_records(text, pats, k)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    halo = max(len(p) for p in pats) - 1
    cut = (n // 2) | 5
    shards = [(0, cut, 0, min(n, cut + halo)), (cut, n, cut, n)]         # (own begin, own end, text begin, text end)
    cap = len(want) + 16
    stride = ctx.align_row_words()
    d_rec, d_n, d_ops = ctx.device_alloc(16 * cap), ctx.device_alloc(16), ctx.device_alloc(4 * stride * cap)
    bufs = [_shard_text(ctx, text, lo, hi, mis) for _, _, lo, hi in shards]
    try:
        ctx.device_memset(d_n, 0, 16)
        ctx.device_memset(d_ops, 0x5A, 4 * stride * cap)
        ctx.synchronize()
        for (ob, oe, lo, hi), d in zip(shards, bufs):
            ctx.find_shard_device(d + mis, lo, hi - lo, n, ob, oe, d_rec, cap, d_n, None)
        for (ob, oe, lo, hi), d in zip(shards, bufs):
            ctx.score_shard_device(d + mis, lo, hi - lo, n, d_rec, cap, d_n)
        for (ob, oe, lo, hi), d in zip(shards, bufs):
            ctx.align_shard_device(d + mis, lo, hi - lo, n, d_rec, cap, d_n, d_ops, stride)
        ctx.synchronize()
        total = struct.unpack("<Q", ctx.device_download(d_n, 8))[0]
        assert total == len(want)
        same_records(_device_records(apm, ctx, d_rec, d_ops, total, stride), want, text, pats)
        assert any(j < cut for _, j, _, _ in want) and any(j >= cut for _, j, _, _ in want)
    finally:
        for d in bufs + [d_rec, d_n, d_ops]:
            ctx.device_free(d)


# ---------------------------------------------------------------- 9. 64-bit positions
@pytest.mark.parametrize("k", [3, 9])
def test_shard_beyond_8gib_has_64_bit_positions(apm, ctx, k):
    pats, text = planted(k, (17, 64, 31), 80 + k, gaps=2048)
    n = len(text)
    base = (1 << 33) + 5
    ref = ref_records(text, pats, k)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    cap = len(ref) + 8
    stride = ctx.align_row_words()
    d_text, d_rec, d_n, d_ops = _shard_text(ctx, text, 0, n, 0), ctx.device_alloc(16 * cap), ctx.device_alloc(16), ctx.device_alloc(4 * stride * cap)
    try:
        ctx.device_memset(d_n, 0, 16)
        ctx.find_shard_device(d_text, base, n, base + n, base, base + n, d_rec, cap, d_n, None)
        ctx.score_shard_device(d_text, base, n, base + n, d_rec, cap, d_n)
        ctx.align_shard_device(d_text, base, n, base + n, d_rec, cap, d_n, d_ops, stride)
        ctx.synchronize()
        total = struct.unpack("<Q", ctx.device_download(d_n, 8))[0]
        assert total == len(ref)
        got = _device_records(apm, ctx, d_rec, d_ops, total, stride)
        assert all(pos > 1 << 33 for _, pos, _, _ in got)
        same_records([(i, pos - base, d, ops) for i, pos, d, ops in got], ref, text, pats)
    finally:
        for d in (d_text, d_rec, d_n, d_ops):
            ctx.device_free(d)


# ---------------------------------------------------------------- 10. multi-device contexts, rehearsed on one GPU
def _mixed(k, lens, n, seed):
    """the mixed set of test_score_gpu.py's test_multi_device_distances_equal_single_device"""
    rng = random.Random(seed)
    pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in lens]
    text = bytearray(rng.choice(b"ACGT") for _ in range(n))
    at = 500
    for p in pats:
        w = bytearray(p)
        if len(w) > 8 and k >= 1:
            w[len(w) // 2] = ord("A") if w[len(w) // 2] != ord("A") else ord("C")
        text[at:at + len(w)] = w
        at += len(w) + 211
    assert at < n - 5000
    cut = min(1200, len(pats[-1]) * 2 // 3)
    text[n - cut:] = pats[-1][:cut]
    return pats, bytes(text)


_single = {}


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
@pytest.mark.parametrize("partition", ["text", "patterns"])
def test_multi_device_scripts_equal_single_device(apm, ctx, devices, partition):
    k = 3
    pats, text = _mixed(k, (20, 300, 13, 700, 1500), 50000, 8)
    pats.append(pats[0])
    if not _single:
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        _single["rec"] = align_call(ctx, text, pats, k)
    single = _single["rec"]
    assert {d for _, _, d, _ in single} >= {0, 1}
    os.environ["APM_DEVICES"] = devices
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    with m:
        m.set_partition(partition)
        m.set_patterns(pats, k)
        got, total = m.find_all_align_buffer(text, 4096)
        assert total == len(single) and got == single
        assert m.find_all_dist_buffer(text, 4096)[0] == [(i, j, d) for i, j, d, _ in single]


# ---------------------------------------------------------------- 11. nothing else moved
def _raw_find_all(apm, ctx, text, capacity, dist):
    out = (apm.ApmMatch * capacity)()
    found = ctypes.c_uint64()
    fn = ctx._lib.apm_find_all_dist_buffer if dist else ctx._lib.apm_find_all_buffer
    ctx._check(fn(ctx._ctx, text, len(text), out, capacity, ctypes.byref(found)))
    return [(r.pattern, r.pos, r.reserved) for r in out[:min(found.value, capacity)]], found.value


def test_nothing_else_moved(apm, ctx):
    c = next(c for c in H.golden()["cases"] if c["name"] == "chrY_k3")
    text, pats, k = H.case_text(c), c["patterns"], c["k"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)

    def state():
        counts = ctx.count_buffer(text)
        return counts, ctx.stat("sieve_candidates"), [ctx.pattern_kernel(i) for i in range(len(pats))], ctx.stat("sieve_on")

    before = state()
    assert before[0] == c["counts"]
    cap = sum(before[0]) + 8
    plain, total = _raw_find_all(apm, ctx, text, cap, False)
    t_find, l_find = ctx.timing(), [l for l, _ in ctx.launch_times()]
    scored, _ = _raw_find_all(apm, ctx, text, cap, True)
    t_dist, l_dist = ctx.timing(), [l for l, _ in ctx.launch_times()]
    aligned, total_a = ctx.find_all_align_buffer(text, cap)
    t_align, l_align = ctx.timing(), [l for l, _ in ctx.launch_times()]
    assert total_a == total == sum(before[0])
    assert [(i, j, d) for i, j, d, _ in aligned] == scored
    same_records(aligned, ref_records(text, pats, k), text, pats)
    assert l_align == l_dist + ["align"] and l_dist == l_find + ["score"]
    assert t_align["n_launches"] == t_dist["n_launches"] + 1 == t_find["n_launches"] + 2 and t_align["kernel_ms"] > 0
    assert state() == before
    # the calls behind an align call return what they returned before it
    assert _raw_find_all(apm, ctx, text, cap, True)[0] == scored
    again, _ = _raw_find_all(apm, ctx, text, cap, False)
    assert again == plain and all(r == 0 for _, _, r in again)


# ---------------------------------------------------------------- 12. limits
def test_stride_below_the_row_is_refused(apm, ctx):
    pats, text = planted(3, (16, 33), 90, gaps=1024)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, 3)
    words = ctx.align_row_words()
    assert words == 1 + (33 + 1 + 15) // 16
    out, ops, found = (apm.ApmMatch * 64)(), (ctypes.c_uint32 * (64 * words))(*([PRESET] * (64 * words))), ctypes.c_uint64(7)
    rc = ctx._lib.apm_find_all_align_buffer(ctx._ctx, text, len(text), out, 64, ctypes.byref(found), ops, words - 1)
    assert rc == BAD_ARGUMENT and list(ops) == [PRESET] * (64 * words) and found.value == 7
    d_text, d_rec, d_n, d_ops = _shard_text(ctx, text, 0, len(text), 0), ctx.device_alloc(64), ctx.device_alloc(16), ctx.device_alloc(4 * words + 16)
    try:
        ctx.device_upload(d_rec, _records([(0, 0)]))
        ctx.device_upload(d_n, struct.pack("<Q", 1))
        ctx.device_memset(d_ops, 0x5A, 4 * words + 16)
        for bad_ops, bad_stride in ((d_ops, words - 1), (d_ops + 2, words)):      # too narrow; not 4-byte aligned
            with pytest.raises(apm.ApmError) as e:
                ctx.align_shard_device(d_text, 0, len(text), len(text), d_rec, 1, d_n, bad_ops, bad_stride)
            assert e.value.status == BAD_ARGUMENT
        ctx.synchronize()
        assert _dwords(ctx.device_download(d_ops, 4 * words)) == [PRESET] * words
    finally:
        for d in (d_text, d_rec, d_n, d_ops):
            ctx.device_free(d)


def test_band_limit(apm, ctx):
    """the align pass refuses exactly what the scoring pass refuses: half-band 2048 is served, 2049 is refused by both
    align calls with nothing written, and the plain find goes on"""
    rng = random.Random(9)
    m, k = 2049, 4096
    text = rand(rng, k + 24)
    pats = [rand(rng, m)]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert ctx.align_row_words() == 1 + (2049 + 2048 + 15) // 16
    want = align_call(ctx, text, pats, k)
    assert len(want) == 24 and all(k // 8 < d <= m for _, _, d, _ in want)
    assert ctx.stat("align_rows") >= 1
    m, k = 2050, 4098
    text = rand(rng, k + 24)
    ctx.set_patterns([rand(rng, m)], k)
    words = ctx.align_row_words()
    out, ops, found = (apm.ApmMatch * 64)(), (ctypes.c_uint32 * (64 * words))(*([PRESET] * (64 * words))), ctypes.c_uint64(7)
    rc = ctx._lib.apm_find_all_align_buffer(ctx._ctx, text, len(text), out, 64, ctypes.byref(found), ops, words)
    assert rc == UNSUPPORTED and all(w == PRESET for w in ops)
    d_text, d_rec, d_n, d_ops = _shard_text(ctx, text, 0, len(text), 0), ctx.device_alloc(64), ctx.device_alloc(16), ctx.device_alloc(4 * words)
    try:
        ctx.device_upload(d_rec, _records([(0, 0)]))
        ctx.device_upload(d_n, struct.pack("<Q", 1))
        ctx.device_memset(d_ops, 0x5A, 4 * words)
        with pytest.raises(apm.ApmError) as e:
            ctx.align_shard_device(d_text, 0, len(text), len(text), d_rec, 1, d_n, d_ops, words)
        assert e.value.status == UNSUPPORTED
        ctx.synchronize()
        assert _dwords(ctx.device_download(d_ops, 4 * words)) == [PRESET] * words
    finally:
        for d in (d_text, d_rec, d_n, d_ops):
            ctx.device_free(d)
    got, total = ctx.find_all_buffer(text, 64)
    assert total == 24 and got == [(0, j) for j in range(24)]


# ---------------------------------------------------------------- 13. the command line
CLI = os.path.join(H.PKG_DIR, "host", "apm_parallel")
LETTERS = {"=": EQ, "X": SUB, "I": INS, "D": DEL}


def _cli(args):
    r = subprocess.run([CLI] + args, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return [l for l in r.stdout.decode().splitlines() if not l.startswith("APM done in")]


def test_cli_alignments(apm, ctx):
    assert os.path.exists(CLI), "host/apm_parallel is not built"
    c = next(c for c in H.golden()["cases"] if c["name"] == "chrY_k3")
    text, pats, k = H.case_text(c), c["patterns"], c["k"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    lib, _ = ctx.find_all_align_buffer(text, sum(c["counts"]) + 8)
    args = [str(k), c["path"]] + [p.decode() for p in pats]
    plain, dist, ali = _cli(args + ["--positions"]), _cli(args + ["--distances"]), _cli(args + ["--alignments"])
    # without the flag: the lines of today -- banner, one count per pattern, the bare or pos:dist offsets
    head = ["Approximate Pattern Mathing: looking for %d pattern(s) in file %s w/ distance of %d" % (len(pats), c["path"], k)] + \
           ["Number of matches for pattern <%s>: %d" % (p.decode(), n) for p, n in zip(pats, c["counts"])]
    assert _cli(args) == head
    for i, p in enumerate(pats):
        mine = [(j, d) for q, j, d, _ in lib if q == i]
        assert plain[len(head) + i] == "Positions for pattern <%s>:" % p.decode() + "".join(" %d" % j for j, _ in mine)
        assert dist[len(head) + i] == "Positions for pattern <%s>:" % p.decode() + "".join(" %d:%d" % jd for jd in mine)
    assert plain[:len(head)] == dist[:len(head)] == ali[:len(head)] == head and len(ali) == len(head) + len(pats)
    # with it: every pos:dist:SCRIPT parses back to the library's record
    got = []
    for i, p in enumerate(pats):
        label, _, rest = ali[len(head) + i].partition(">:")
        assert label == "Positions for pattern <%s" % p.decode()
        for item in rest.split():
            pos, d, script = item.split(":")
            runs = re.findall(r"(\d+)([=XID])", script)
            assert "".join(n + l for n, l in runs) == script and all(int(n) >= 1 for n, _ in runs)
            assert all(a[1] != b[1] for a, b in zip(runs, runs[1:]))        # maximal runs
            ops = bytes(LETTERS[l] for n, l in runs for _ in range(int(n)))
            assert apm.ops_to_script(ops) == script
            got.append((i, int(pos), int(d), ops))
    assert got == lib and len(got) == sum(c["counts"])
