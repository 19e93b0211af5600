"""The occurrence search and the best-hit pass on the GPU in the parts of include/apm.h's promise the other modules leave
out: k up to m - 1 (a warm-up of 255 columns, a span walk that fills all of its text buffer, every lane reporting in every
column), positions at and beyond 2^32 (a few KiB of text handed over as a shard at a global offset: a record on each side
of the line in one launch), and the segment length of a large range, S = 16 (m_max + k), under hundreds of pattern rows.

The truth everywhere is tests/occ_ref.py and tests/best_ref.py, the literal recurrences; every comparison is over the
COMPLETE record set, sorted, with n_found and the per-pattern counts.  The tests without the `gpu` mark pin what the GPU
tests rely on: the reference over a cut text against the whole one, the many-pattern and many-span forms of the
reference (the same recurrences, one array column per pattern or per record: thousands of spans of 255 columns are
checked) against the plain ones, and that the wide-k texts are as dense, and their spans as long, as the GPU tests say."""
import random
import struct

import numpy as np
import pytest

import best_ref as B
import helpers as H
import occ_ref as R
import test_best_gpu as G
import test_occ_gpu as O
from test_occ_gpu import Dev, Out, counts_of, setup, unpack

gpu = pytest.mark.gpu
ALL, LOCAL_MIN = R.ALL, R.LOCAL_MIN
NO_START, DIST_INVALID = R.NO_START, 0xFFFFFFFF
LINE = 1 << 32
DNA = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


def up16(x):
    return (x + 15) & ~15


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def ref_both(key, text, pats, k):
    """{flags: records} of a case, one pass of the recurrence per pattern, computed once"""
    def make():
        out = {ALL: [], LOCAL_MIN: []}
        for i, p in enumerate(pats):
            E = R.ends_scores(text, p)
            for f in out:
                out[f] += [(i, int(e), int(E[e])) for e in R.reported(E, len(p), k, f)]
        return out
    return cached(("ref", key), make)


def scan_and_spans(ctx, text, n_patterns, flags, cap):
    """a whole-text scan and the span pass over its records, behind each other on the stream:
    ([(pattern, end, dist, start)] sorted, n_found, counts)"""
    n = len(text)
    with Dev(ctx) as dev:
        out = Out(ctx, dev, cap, n_patterns)
        d_text = dev.text(text)
        d_span = dev.alloc(16 * (cap + 4), O.GUARD * (cap + 4))
        ctx.occ_shard_device(d_text, 0, n, n, 0, n, flags, out.d_out, cap, out.d_n, out.d_counts)
        ctx.occ_spans_device(d_text, 0, n, n, out.d_out, cap, out.d_n, d_span)
        got, n_found, counts = out.read()
        have = min(n_found, cap)
        ends = unpack(ctx.device_download(out.d_out, 16 * have))
        raw = ctx.device_download(d_span, 16 * (cap + 4))
        assert raw[16 * have:] == O.GUARD * (cap + 4 - have), "span entries without a record were written"
        spans = unpack(raw[:16 * have])
        assert [(i, d) for i, _, d in spans] == [(i, d) for i, _, d in ends]      # an end's span has the end's distance
        rec = sorted((i, e, d, None if s == NO_START else s) for (i, e, d), (_, s, _) in zip(ends, spans))
        assert [r[:3] for r in rec] == got
        return rec, n_found, counts


def check_spans_many(text, pats, k, got):
    """test_occ_gpu's check_spans -- starts are the reference's, and the span has the distance reported -- with the
    reference run over all records of a pattern at once"""
    for i, p in enumerate(pats):
        every = [r for r in got if r[0] == i]
        for at in range(0, len(every), 1024):                                     # (arrays that stay in the cache)
            mine = every[at:at + 1024]
            starts, dists = R.span_many(text, p, k, [e for _, e, _, _ in mine])
            assert [(s, d) for _, _, d, s in mine] == list(zip(starts, dists)), i
            assert None not in starts
            assert R.global_dist_many(p, text, [(s, e) for _, e, _, s in mine]) == dists, i


# ================================================================ A. wide k
WIDE = [(8, 7), (33, 32), (64, 20), (64, 63), (97, 40), (128, 64), (128, 127)]
DENSE = [(64, 63), (128, 127)]          # k = m - 1 on DNA: every end is an occurrence
FAR = 192                               # a span longer than this reads the fourth stride of the span kernel's text fill


def wide_len(m_max, k):
    """two workgroups' segments and half a segment at the chooser's lower clamp S = m_max + k rounded up to 16 (what a
    range this small gets on any device: the GPU tests assert it), and a tail that is no multiple of anything"""
    S = up16(m_max + k)
    return 2 * 64 * S + S // 2 + 37


def wide_case(m, k):
    """(patterns, text, ends whose span is longer than FAR): occ_ref.planted, and at (128, 127) two copies followed by 70 and
    by 127 bytes outside the alphabet -- the shortest substring within k that ends there is the copy AND the run"""
    def make():
        n = wide_len(m, k)
        pats, text = R.planted(1000 * m + k, [m], k, n, copies=8)
        far = []
        if (m, k) == (128, 127):
            text = bytearray(text)
            for at, run in ((20011, 70), (26006, 127)):
                text[at:at + m + run] = pats[0] + b"N" * run
                far.append(at + m + run - 1)
            text = bytes(text)
        return pats, text, far
    return cached(("wide", m, k), make)


def test_wide_k_texts_are_as_dense_and_their_spans_as_long_as_claimed():
    for m, k in DENSE:
        pats, text, _ = wide_case(m, k)
        want = ref_both(("wide", m, k), text, pats, k)
        assert [e for _, e, _ in want[ALL]] == list(range(len(text))), (m, k)        # all 64 lanes report in every column
        assert 64 < len(want[LOCAL_MIN]) < len(text) // 2
    pats, text, far = wide_case(128, 127)
    want = ref_both(("wide", 128, 127), text, pats, 127)[ALL]
    lengths = []
    for e in far:
        s, d = R.span(text, pats[0], 127, e)
        assert (0, e, d) in want
        lengths.append(e + 1 - s)
    assert lengths == [128 + 70, 255] and min(lengths) > FAR                      # 255 = m + k: every column of the walk


def test_many_span_reference_is_the_plain_one():
    """dense and sparse, ends nearer the text's start than m + k, ends without an occurrence, the two long spans"""
    for (m, k), step in (((128, 127), 331), ((64, 20), 97)):
        pats, text, far = wide_case(m, k)
        ends = sorted(set(range(0, len(text), step)) | set(range(0, 9)) | {m + k - 2, m + k - 1, m + k, len(text) - 1} | set(far))
        want = [R.span(text, pats[0], k, e) for e in ends]
        starts, dists = R.span_many(text, pats[0], k, ends)
        assert list(zip(starts, dists)) == want
        assert (None in starts) == (k == 20) and len({d for d in dists}) > 4
        found = [(s, e) for s, e in zip(starts, ends) if s is not None]
        assert R.global_dist_many(pats[0], text, found) == [R.global_dist(pats[0], text[s:e + 1]) for s, e in found]
        assert len({e - s for s, e in found}) > 4


@gpu
@pytest.mark.parametrize("m,k", WIDE)
def test_wide_k(ctx, m, k):
    """a warm-up of m + k up to 255 columns, cap = k + 1 up to 128, S up to 256; scan, span pass and host-level call"""
    pats, text, far = wide_case(m, k)
    n = len(text)
    setup(ctx, pats, k)
    both = ref_both(("wide", m, k), text, pats, k)
    for flags in (ALL, LOCAL_MIN):
        want = both[flags]
        assert len(want) >= 16
        rec_dev, n_found, counts = scan_and_spans(ctx, text, 1, flags, len(want) + 8)
        assert [r[:3] for r in rec_dev] == want, (m, k, flags)
        assert n_found == len(want) and counts == [len(want)]
        S = int(ctx.stat("occ_segment"))
        assert S == up16(m + k) and n >= 2 * 64 * S + S // 2                      # at least two workgroups of segments
        assert ctx.stat("occ_lanes") == -(-n // S)
        rec, total, cnt = ctx.find_occ_buffer(text, flags, capacity=len(want) + 8)
        assert [r[:3] for r in rec] == want and total == len(want) and cnt == [len(want)]
        assert rec == rec_dev                                                     # (the same spans from both calls)
        some = rec if flags == LOCAL_MIN else rec[:: min(64, max(1, len(rec) // 64))]
        if flags == ALL:
            some = some + [r for r in rec if r[1] in far]
        check_spans_many(text, pats, k, some)
        if flags == ALL and far:
            assert sorted(r[1] + 1 - r[3] for r in rec if r[1] in far) == [128 + 70, 255]
            assert max(r[1] + 1 - r[3] for r in some) > FAR
    assert [l for l, _ in ctx.launch_times()] == ["occ", "span"]


MIXED_LENS, MIXED_K = (9, 33, 64, 97, 128), 8      # W = 1, 2, 2, 4, 4: two rows of pattern groups, three idle waves in the second


def mixed_case():
    return cached("mixed", lambda: R.planted(4711, list(MIXED_LENS), MIXED_K, wide_len(128, MIXED_K), copies=8))


@gpu
def test_wide_mixed_set_whole_and_in_three_shards(ctx):
    """the short pattern's warm-up is 17 bytes of a 136-byte halo; unaligned cuts, the minimal left halo, misaligned d_text"""
    pats, text = mixed_case()
    k, n, m_max, P = MIXED_K, len(mixed_case()[1]), 128, 5
    setup(ctx, pats, k)
    both = ref_both("mixed", text, pats, k)
    cuts = [0, n // 3 | 1, (2 * n // 3 | 1) + 6, n]
    assert cuts[1] % 16 and cuts[2] % 16
    for flags in (ALL, LOCAL_MIN):
        want = sorted(both[flags])
        assert all(counts_of(want, P))
        rec, n_found, counts = scan_and_spans(ctx, text, P, flags, len(want) + 8)
        assert [r[:3] for r in rec] == want, flags
        assert n_found == len(want) and counts == counts_of(want, P)
        S = int(ctx.stat("occ_segment"))
        assert S == up16(m_max + k) and n >= 2 * 64 * S + S // 2
        assert ctx.stat("occ_lanes") == -(-n // S) * P
        some = rec
        if flags == ALL:                                                          # (a stride per pattern: the short one has every end)
            per = [[r for r in rec if r[0] == i] for i in range(P)]
            some = [r for mine in per for r in mine[:: min(64, max(1, len(mine) // 64))]]
        check_spans_many(text, pats, k, some)
        host, total, cnt = ctx.find_occ_buffer(text, flags, capacity=len(want) + 8)
        assert host == rec and total == len(want) and cnt == counts_of(want, P)
        with Dev(ctx) as dev:
            out = Out(ctx, dev, len(want) + 8, P)
            for s in range(3):
                ob, oe = cuts[s], cuts[s + 1]
                lo, hi = max(0, ob - m_max - k), min(n, oe + 1)
                d_text = dev.text(text, lo, hi, mis=(5, 9, 3)[s])
                assert d_text % 16
                ctx.occ_shard_device(d_text, lo, hi - lo, n, ob, oe, flags, out.d_out, out.cap, out.d_n, out.d_counts)
            got, n_found, counts = out.read()
            assert got == want and n_found == len(want) and counts == counts_of(want, P)


@gpu
def test_wide_k_capacity_a_third_of_the_records(ctx):
    """k = m - 1: every lane of every wave appends in every column, and two thirds of it lies beyond the capacity"""
    m, k = 64, 63
    pats, text, _ = wide_case(m, k)
    setup(ctx, pats, k)
    want = ref_both(("wide", m, k), text, pats, k)[ALL]
    cap = len(want) // 3
    assert cap > 4096
    got, n_found, counts = O.scan(ctx, text, 1, ALL, cap)                         # (read() compares the guard words)
    assert n_found == len(want) and counts == [len(want)]
    assert len(got) == cap == len(set(got)) and set(got) <= set(want)


# ================================================================ B. positions beyond 2^32
def edited(rs, p, edits, kind):
    """p under `edits` substitutions (kind 0), deletions (1) or insertions (2)"""
    s = bytearray(p)
    for _ in range(edits):
        if kind == 0:
            at = rs.randint(0, len(s))
            s[at] = int(DNA[(list(DNA).index(s[at]) + 1) % 4])
        elif kind == 1:
            del s[rs.randint(0, len(s))]
        else:
            s.insert(rs.randint(0, len(s) + 1), int(DNA[rs.randint(0, 4)]))
    return bytes(s)


def line_case(seed, n, k, anchors, tail):
    """(patterns, T, L): T is n bytes of random DNA and L, odd, its byte that a shard base of 2^32 - L puts at position 2^32.
    Pattern i is T's own bytes at anchors[i] = (m, 'end' | 'start', offset from L) -- the one exact copy of it, wherever
    the line falls; six edited copies of each lie away from L, a copy of the first pattern begins at byte 1, and
    `tail(patterns)` ends the text."""
    rs = np.random.RandomState(seed)
    text = bytearray(DNA[rs.randint(0, 4, size=n)].tobytes())
    L = (n // 2) | 1
    pats = []
    for m, how, o in anchors:
        lo = L + o + 1 - m if how == "end" else L + o
        pats.append(bytes(text[lo:lo + m]))
    slots = [s for s in range(160, n - 600, 250) if abs(s - L) > 400]
    assert len(slots) >= 6 * len(pats)
    for c in range(6 * len(pats)):
        copy = edited(rs, pats[c % len(pats)], min(k, (0, 1, 2, 3, 5, 9)[c // len(pats)]), c % 3)
        text[slots[c] + c % 16:slots[c] + c % 16 + len(copy)] = copy
    text[1:1 + len(pats[0])] = pats[0]
    end = tail(pats)
    text[n - len(end):] = end
    for (m, how, o), p in zip(anchors, pats):
        lo = L + o + 1 - m if how == "end" else L + o
        assert bytes(text[lo:lo + m]) == p
    return pats, bytes(text), L


BASES = ("straddle", "far")


def base_of(name, L):
    base = LINE - L if name == "straddle" else (1 << 33) + 5
    assert base % 2 == 1
    return base


# exact copies that end at 2^32 - 1 and 2^32 + 1 (k = 3), at 2^32 and 2^32 + 1 (k = 20); W = 2 and 4
OCC_LINE = {3: ((64, "end", -1), (100, "end", 1)), 20: ((64, "end", 0), (100, "end", 1))}
OCC_N = 6144


def occ_line_case(k):
    # the text ends two bytes short of a copy: E falls to 2 at the last byte, reported under LOCAL_MIN only because
    # no byte follows
    return cached(("occ_line", k), lambda: line_case(900 + k, OCC_N, k, OCC_LINE[k], lambda pats: pats[0][:-2]))


@pytest.mark.parametrize("k", [3, 20])
def test_reference_over_a_cut_text_is_the_whole_texts(k):
    """the warm-up lemma as the GPU tests use it: the reference over T[off:] alone, ends at least h = m_max + k in, is the
    reference over T from off + h on"""
    pats, text, L = occ_line_case(k)
    h = 100 + k
    whole = ref_both(("occ_line", k), text, pats, k)
    assert (0, len(text) - 1, 2) in whole[LOCAL_MIN] and (0, len(text) - 2, 3) in whole[ALL]   # (the last byte's E is not a minimum of its own)
    for off in (1, 777, L - h - 1):
        for flags in (ALL, LOCAL_MIN):
            cut = R.records(text[off:], pats, k, flags, lo=h)
            assert [(i, e + off, d) for i, e, d in cut] == sorted(r for r in whole[flags] if r[1] >= off + h), (off, flags)
            assert cut


@gpu
@pytest.mark.parametrize("name", BASES)
@pytest.mark.parametrize("k", [3, 20])
def test_occ_positions_beyond_4gib(ctx, k, name):
    """scan and span pass over a shard whose text lies across position 2^32, and one beyond 2^33"""
    pats, text, L = occ_line_case(k)
    n, h = len(text), 100 + k
    base = base_of(name, L)
    setup(ctx, pats, k)
    both = ref_both(("occ_line", k), text, pats, k)
    exact = [(i, L + o, 0) for i, (_, _, o) in enumerate(OCC_LINE[k])]
    for flags in (ALL, LOCAL_MIN):
        local = sorted(r for r in both[flags] if r[1] >= h)                       # T alone; the global truth by the warm-up lemma
        want = [(i, e + base, d) for i, e, d in local]
        assert all(r in local for r in exact)
        if flags == LOCAL_MIN:
            assert (0, n - 1, 2) in local                                         # "true by definition at the last byte"
        if name == "straddle":
            ends = {e for _, e, _ in want}
            assert min(ends) < LINE - 1000 and max(ends) > LINE + 1000
            assert [(i, L + o + base) for i, (_, _, o) in enumerate(OCC_LINE[k])] == [(0, LINE - 1 if k == 3 else LINE), (1, LINE + 1)]
            if flags == ALL:
                assert {LINE - 1, LINE, LINE + 1, LINE + 2, LINE + 3} <= ends       # (the copies' next ends, at one edit each)
        else:
            assert all(e > 1 << 33 for _, e, _ in want)
        cap = len(want) + 8
        with Dev(ctx) as dev:
            out = Out(ctx, dev, cap, 2)
            d_text = dev.text(text, mis=3)
            ctx.occ_shard_device(d_text, base, n, base + n, base + h, base + n, flags, out.d_out, cap, out.d_n, out.d_counts)
            d_span = dev.alloc(16 * cap, O.GUARD * cap)
            ctx.occ_spans_device(d_text, base, n, base + n, out.d_out, cap, out.d_n, d_span)
            got, n_found, counts = out.read()
            assert got == want, (k, name, flags)
            assert n_found == len(want) and counts == counts_of(want, 2)
            ends = unpack(ctx.device_download(out.d_out, 16 * n_found))
            spans = unpack(ctx.device_download(d_span, 16 * cap))
            assert spans[n_found:] == unpack(O.GUARD * (cap - n_found))
            for (i, e, d), got_span in zip(ends, spans):
                ws, wd = R.span(text, pats[i], k, e - base)
                assert wd == d and got_span == (i, ws + base, d), (i, e)
            if name == "straddle":                                                # a span that begins in front of the line and ends behind it
                assert any(s < LINE <= e for (_, e, _), (_, s, _) in zip(ends, spans))


@gpu
@pytest.mark.parametrize("name", BASES)
def test_span_triage_beyond_4gib(ctx, name):
    """made-up records around a shard beyond 2^32: each is left alone or marked as test_spans_triage_made_up_records pins"""
    k = 3
    pats, text, L = occ_line_case(k)
    n, h = len(text), 100 + k
    base = base_of(name, L)
    setup(ctx, pats, k)
    real = [(i, e + base) for i, e, _ in ref_both(("occ_line", k), text, pats, k)[LOCAL_MIN] if e >= h]
    # in front of the text; the end inside, but the first of its m + k columns one byte in front
    left_alone = [(0, base - 1), (1, base - 1), (0, base + 10), (0, base + 64 + k - 2), (1, base + 100 + k - 2)]
    invalid = [(0, base + n), (1, base + n + 99), (0, 1 << 40), (2, base + 500), (0xFFFFFFFF, LINE)]
    none = [(0, base + L + 300), (1, base + L - 333)]
    assert all(R.span(text, pats[i], k, e - base)[0] is None for i, e in none)
    first = [(0, base + 64 + k - 1), (1, base + 100 + k - 1)]                     # the first column is the text's first byte: decided
    assert len(real) > 8 and not set(real) & set(left_alone + invalid + none + first)
    seeds = real[:5] + left_alone[:2] + invalid[:3] + real[5:] + none + first + left_alone[2:] + invalid[3:]
    preset = b"".join(struct.pack("<QII", 0x1111111111111111, 0x22222222, 0x33333333 + q) for q in range(len(seeds) + 2))
    with Dev(ctx) as dev:
        d_text = dev.text(text, mis=7)
        d_rec, d_n = dev.alloc(16 * len(seeds), O.pack(seeds)), dev.counter(len(seeds) + 5)
        d_span = dev.alloc(len(preset), preset)
        ctx.occ_spans_device(d_text, base, n, base + n, d_rec, len(seeds), d_n, d_span)
        ctx.synchronize()
        raw = ctx.device_download(d_span, len(preset))
        assert ctx.device_download(d_rec, 16 * len(seeds)) == O.pack(seeds)
    assert raw[16 * len(seeds):] == preset[16 * len(seeds):], "entries at or beyond capacity were written"
    for q, (i, e) in enumerate(seeds):
        pos, pat, d = struct.unpack_from("<QII", raw, 16 * q)
        if (i, e) in invalid:
            assert (pos, pat, d) == (NO_START, i, DIST_INVALID), (i, e)
        elif (i, e) in left_alone:
            assert raw[16 * q:16 * q + 16] == preset[16 * q:16 * q + 16], (i, e)
        else:
            ws, wd = R.span(text, pats[i], k, e - base)
            assert ((i, e) in none) <= (ws is None)
            assert (pos, pat, d) == (NO_START if ws is None else ws + base, i, wd), (i, e)


# the kept starts: 2^32 + 1 (its left neighbour is the record at exactly 2^32), exactly 2^32 (every left neighbour has
# another high word), 2^32 - 1 (every right neighbour has): each occurrence's run of records crosses or touches the line
BEST_LINE = ((16, "start", 1), (23, "start", 0), (40, "start", -1))
BEST_N = 6144


def best_line_case(k):
    # an edited copy of the longest pattern and the first k + 2 bytes of the shortest end the text: records within the
    # radius of the end of W = n_total - k, the last of them with a truncated window
    return cached(("best_line", k), lambda: line_case(
        700 + k, BEST_N, k, BEST_LINE, lambda pats: B.edited(random.Random(k), pats[2], 2) + pats[0][:k + 2]))


@gpu
@pytest.mark.parametrize("name", BASES)
@pytest.mark.parametrize("k", [3, 8])
def test_best_hits_beyond_4gib(ctx, k, name):
    """find, then the best-hit pass (k = 3: lane form, k = 8: wave form) on a shard across 2^32 and one beyond 2^33"""
    pats, text, L = best_line_case(k)
    n = len(text)
    base = base_of(name, L)
    full = B.ref_records(text, pats, k)
    cap = len(full) + 8
    setup(ctx, pats, k)
    with Dev(ctx) as dev:
        d_text, d_rec, d_n = dev.text(text, mis=5), dev.alloc(16 * cap), dev.counter()
        ctx.find_shard_device(d_text, base, n, base + n, base, base + n, d_rec, cap, d_n, None)
        for r in (3, 64):
            local = [h for h in B.best_hits(text, pats, k, r) if h[1] >= r]       # nearer the shard's start: not covered
            want = [(i, j + base, d) for i, j, d in local]
            assert (0, 1, 0) in B.best_hits(text, pats, k, r) and (0, 1 + base, 0) not in want
            got, n_out, _ = G.best_call(ctx, dev, d_text, base, n, base + n, d_rec, cap, d_n, r, cap)
            assert got == want, (k, r, name)
            assert n_out == len(want)
            kept = [(i, L + o + base, 0) for i, (_, _, o) in enumerate(BEST_LINE)]
            assert all(h in want for h in kept)
            assert any(n - k - r <= j < n - k for _, j, _ in full)                # decided against the end of W = n_total - k
            if name == "straddle":
                assert kept == [(0, LINE + 1, 0), (1, LINE, 0), (2, LINE - 1, 0)]
                assert min(j for _, j, _ in want) < LINE - 1000 and max(j for _, j, _ in want) > LINE + 1000
        ctx.synchronize()
        assert struct.unpack("<Q", ctx.device_download(d_n, 8))[0] == len(full)
        found = sorted((i, j - base) for i, j, _ in unpack(ctx.device_download(d_rec, 16 * len(full))))
        assert found == [(i, j) for i, j, _ in full]
    # every occurrence at the line leaves a run of records, its neighbour starts, which the pass thinned to the start above
    for i, (_, _, o) in enumerate(BEST_LINE):
        assert {j for q, j, _ in full if q == i and abs(j - (L + o)) <= 1} == {L + o - 1, L + o, L + o + 1}, i


# ================================================================ C. the upper clamp of the segment chooser
MANY_P, MANY_M, MANY_K = 1024, 12, 1
SEAMS = (1, 2, 63, 64, 65)             # ends at q S - 1, q S, q S + 1: lane seams, and 64, 65: the first workgroup's last and the second's first lanes


def _many(n, S):
    """(MANY_P distinct patterns, a text of n bytes, {pattern: (end, distance)}): fifteen of the patterns are the text's own
    bytes in front of a seam -- as they stand, with one byte taken out, or with one put in: an end within MANY_K there"""
    rs = np.random.RandomState(1212)
    text = DNA[rs.randint(0, 4, size=n)].tobytes()
    ends = [q * S + o for q in SEAMS for o in (-1, 0, 1)]
    own = []
    for c, e in enumerate(ends):
        if c % 4 == 1:                                                            # the text has a byte the pattern lacks
            p = bytearray(text[e - MANY_M:e + 1])
            del p[5]
        elif c % 4 == 3:                                                          # the pattern has a byte the text lacks
            p = bytearray(text[e - MANY_M + 2:e + 1])
            p.insert(6, ord("A") if p[6] != ord("A") else ord("C"))
        else:
            p = bytearray(text[e - MANY_M + 1:e + 1])
        assert len(p) == MANY_M
        own.append(bytes(p))
    pats = [DNA[rs.randint(0, 4, size=MANY_M)].tobytes() for _ in range(MANY_P)]
    at = {}
    for c, p in enumerate(own):
        pats[c * 67 + 3] = p                                                      # spread over the rows of pattern groups
        at[c * 67 + 3] = (ends[c], 0 if c % 2 == 0 else 1)
    assert len(set(pats)) == MANY_P
    return pats, text, at


def test_many_pattern_reference_is_the_plain_one():
    S = 208
    pats, text, at = _many(66 * S + 50, S)
    own = sorted(i for i, (e, _) in at.items() if e < 3 * S)                       # the six at the first two seams
    pats, text = [pats[i] for i in own] + [p for i, p in enumerate(pats[:90]) if i not in at][:74], text[:3 * S]
    many = R.records_many(text, pats, MANY_K)
    for flags in (ALL, LOCAL_MIN):
        want = R.records(text, pats, MANY_K, flags)
        assert many[flags] == want and len(want) >= 6
    assert len(own) == 6 and all((q, at[i][0], at[i][1]) in many[ALL] for q, i in enumerate(own))


@gpu
def test_segment_at_the_upper_clamp_with_256_pattern_rows(ctx):
    """S = 16 (m_max + k), what a large range runs at: a lane walks 16 warm-ups' worth of ends, the launch has P / 4 rows"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    lo = MANY_M + MANY_K
    S = 16 * lo
    groups = -(-MANY_P // 4)
    n = max(64 * -(-4 * n_cu // groups) * S, 66 * S) + S // 2 + 5               # apm_occ_segment: range / segments >= 16 (m_max + k)
    assert n <= 1 << 20, "a device of %d compute units needs %d bytes of text to reach the upper clamp: beyond this test's 1 MiB" % (n_cu, n)
    pats, text, at = _many(n, S)
    setup(ctx, pats, MANY_K)
    want = R.records_many(text, pats, MANY_K)
    assert all((i, e, d) in want[ALL] for i, (e, d) in at.items())                 # the ends at the seams
    for flags in (ALL, LOCAL_MIN):
        w = want[flags]
        got, n_found, counts = O.scan(ctx, text, MANY_P, flags, len(w) + 8)
        assert int(ctx.stat("occ_segment")) == S
        assert ctx.stat("occ_lanes") == -(-n // S) * MANY_P
        assert got == w, flags
        assert n_found == len(w) and counts == counts_of(w, MANY_P)
