"""The nearest-occurrence search per sequence on the GPU: apm_nearest_seq_shard_device, apm_nearest_seq_records_device and
apm_find_nearest_seq_buffer give exactly the keys and records include/apm.h pins ("nearest occurrences per sequence").  The
truth everywhere is tests/seqnear_ref.py -- nearest_ref on every sequence as a text of its own; every comparison is exact and
of the COMPLETE result.  Device buffers carry preset guard words around the keys and both record arrays, and the tests compare
those.  Texts are 4 .. 24 KiB, so the segment S shrinks to about 2 m_max: lane seams every S bytes, workgroup seams at 64
and 128 segments."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import nearest_ref as N
import occ_ref as R
import seqnear_ref as SR
import test_nearest_gpu as NG

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = -1, -8, -6
GUARD = b"\xa5" * 16
MS = NG.MS
NO_START, NONE, DIST_INVALID = N.NO_START, N.NONE, N.INVALID
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


def setup(ctx, pats, k=0):
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)


def dna(rs, n):
    return DNA[rs.randint(0, 4, size=n)].tobytes()


class Dev:
    """device buffers of one test, freed at its end: the shard texts, the tables, the guarded keys and the guarded record
    arrays of `rows` = n_seq * n_patterns pairs"""

    def __init__(self, ctx, rows):
        self.ctx, self.rows, self.ptrs = ctx, rows, []
        self.base_keys = self.alloc(32 + 8 * rows)
        self.base_end = self.alloc(64 + 16 * rows)
        self.base_start = self.alloc(64 + 16 * rows)
        self.d_keys, self.d_end, self.d_start = self.base_keys + 16, self.base_end + 32, self.base_start + 32
        self.reset()

    def alloc(self, nbytes):
        p = self.ctx.device_alloc(max(nbytes, 16))
        self.ptrs.append(p)
        return p

    def reset(self, keys=None):
        """guards everywhere, the keys preset to NONE (or to `keys`)"""
        keys = [NONE] * self.rows if keys is None else keys
        self.ctx.device_upload(self.base_keys, GUARD + struct.pack("<%dQ" % self.rows, *keys) + GUARD)
        for base in (self.base_end, self.base_start):
            self.ctx.device_upload(base, GUARD * (self.rows + 4))

    def text(self, text, lo=0, hi=None, mis=0):
        """the bytes [lo, hi) of the text at byte `mis` of an allocation with 16 readable bytes around them"""
        hi = len(text) if hi is None else hi
        d = self.alloc(hi - lo + 48)
        self.ctx.device_upload(d, b"\x5a" * (hi - lo + 48))
        if hi > lo:
            self.ctx.device_upload(d + mis, text[lo:hi])
        return d + mis

    def table(self, begins):
        """the apm_seq entries of t_begin[0 .. n_seq]; hdr_off holds a value nothing may depend on"""
        flat = []
        for s, b in enumerate(begins):
            flat += [0xDEAD000000000000 + s, b]
        d = self.alloc(16 * len(begins))
        self.ctx.device_upload(d, struct.pack("<%dQ" % len(flat), *flat))
        return d

    def keys(self):
        self.ctx.synchronize()
        raw = self.ctx.device_download(self.base_keys, 32 + 8 * self.rows)
        assert raw[:16] == GUARD and raw[-16:] == GUARD, "the guards around d_keys were written"
        return list(struct.unpack("<%dQ" % self.rows, raw[16:-16]))

    def records(self, base):
        """[(pos, pattern, dist)], None for an entry that still holds its guard"""
        self.ctx.synchronize()
        raw = self.ctx.device_download(base, 64 + 16 * self.rows)
        assert raw[:32] == GUARD * 2 and raw[-32:] == GUARD * 2, "the guards around a record array were written"
        body = raw[32:-32]
        return [None if body[16 * i:16 * i + 16] == GUARD else struct.unpack_from("<QII", body, 16 * i) for i in range(self.rows)]

    def ends(self):
        return self.records(self.base_end)

    def starts(self):
        return self.records(self.base_start)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.device_free(p)


def device_result(ctx, text, n_patterns, begins, mis=0):
    """both device calls over the whole text: (keys, end records, start records)"""
    n, n_seq = len(text), len(begins) - 1
    with Dev(ctx, n_seq * n_patterns) as dev:
        d_text, d_table = dev.text(text, mis=mis), dev.table(begins)
        ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, n, d_table, n_seq, dev.d_keys)
        ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, n_seq, dev.d_keys, dev.d_end, dev.d_start)
        return dev.keys(), dev.ends(), dev.starts()


def reference(text, pats, begins):
    ends, starts = SR.records(text, pats, begins)
    return [NONE if e == NO_START else N.key(d, e) for e, _, d in ends], ends, starts


def check_whole(ctx, text, pats, begins, mis=(0,)):
    """the whole text through both device calls (at every misalignment); -> the reference"""
    want = reference(text, pats, begins)
    assert want[0] == SR.keys(text, pats, begins)
    for a in mis:
        got = device_result(ctx, text, len(pats), begins, a)
        assert got[0] == want[0], a
        assert got == want, a
    return want


# ---------------------------------------------------------------- 1. random DNA with random boundaries, every width
def test_random_boundaries_every_width(ctx):
    n = 24 * 1024
    pats, text = R.planted(71, list(MS), 3, n, copies=2)
    rs = np.random.RandomState(1071)
    pats = pats + [dna(rs, m) for m in (16, 64, 128)]            # unplanted: large distances
    cuts = [int(c) for c in rs.randint(0, n + 1, size=34)]
    cuts += cuts[:3] + [0, n, n]                                 # empties: inside, at the first byte, behind the last
    begins = SR.begins_of(cuts, n)
    assert len(begins) - 1 == 41 and sum(a == b for a, b in zip(begins, begins[1:])) >= 6
    setup(ctx, pats, 3)
    keys, ends, _ = check_whole(ctx, text, pats, begins, mis=(0, 7))
    assert [l for l, _ in ctx.launch_times()] == ["snspan"]      # (the last device call)
    S = int(ctx.stat("seqnear_segment"))
    assert S % 16 == 0 and 2 * 128 - 1 <= S and n // S >= 65, "the launch has a workgroup seam at 64 segments"
    assert int(ctx.stat("seqnear_lanes")) == -(-n // S) * len(pats)
    assert sum(k != NONE for k in keys) > 30 * len(pats) and any(k == NONE for k in keys)
    assert max(d for e, _, d in ends if e != NO_START) >= 40


# ---------------------------------------------------------------- 2. one boundary against lane and workgroup seams
@pytest.mark.parametrize("q", (1, 63, 64, 65, 128))
def test_boundary_against_seams(ctx, q):
    rs = np.random.RandomState(200 + q)
    m = 20
    p = dna(rs, m)
    setup(ctx, [p])
    n = 6400
    with Dev(ctx, 1) as dev:                                     # S of this shape
        ctx.nearest_seq_shard_device(dev.text(b"A" * n), 0, n, n, 0, n, dev.table([0, n]), 1, dev.d_keys)
    S = int(ctx.stat("seqnear_segment"))
    assert S >= 2 * m - 1 and 129 * S + 2 * S < n, S
    # near copies everywhere: what a walk wrongly keeps from the far side of a boundary changes a distance
    t = bytearray(dna(rs, n))
    for at in range(5, n - m, m + 7):
        t[at:at + m] = p
        t[at + at % m] = ord("N")
    text = bytes(t)
    for delta in (-(2 * m - 1) - 1, -(2 * m - 1), -m, -1, 0, 1):
        c = q * S + delta
        check_whole(ctx, text, [p], [0, c, n])
        assert int(ctx.stat("seqnear_segment")) == S
    check_whole(ctx, text, [p], [0, q * S, q * S, q * S, q * S + 1, n])     # empties and a 1-byte sequence at the seam


# ---------------------------------------------------------------- 3. the defining case
def test_an_occurrence_across_a_boundary_is_none_of_either_sequence(ctx):
    rs = np.random.RandomState(31)
    n, c = 4096, 2000
    p = dna(rs, 24)
    t = bytearray(dna(rs, n))
    t[c - 12:c + 12] = p                                         # half in the tail of sequence 1, half in the head of sequence 2
    text = bytes(t)
    begins = [0, 700, c, 3100, n]
    setup(ctx, [p])
    ends, _ = SR.records(text, [p], begins)
    assert ends[1][2] > 0 and ends[2][2] > 0 and all(e[0] != NO_START for e in ends)   # (the case cannot degenerate)
    whole = NG.device_result(ctx, text, 1)
    assert whole[0] == [N.key(0, c + 11)] and whole[1] == [(c + 11, 0, 0)]            # the nearest search: d = 0 across the boundary
    keys, ends_got, starts_got = check_whole(ctx, text, [p], begins)
    assert whole[0][0] not in keys and min(keys) > whole[0][0]
    for s in range(4):                                           # every span stays inside its sequence
        assert begins[s] <= starts_got[s][0] <= ends_got[s][0] < begins[s + 1]


# ---------------------------------------------------------------- 4. many tiny sequences
def test_many_tiny_sequences(ctx):
    rs = np.random.RandomState(41)
    lens = rs.randint(0, 6, size=3000)
    begins = [0] + [int(x) for x in np.cumsum(lens)]
    n = begins[-1]
    text = dna(rs, n)
    pats = [dna(rs, m) for m in (1, 2, 3, 4, 5, 6, 7, 8)]
    setup(ctx, pats)
    keys, _, _ = check_whole(ctx, text, pats, begins)
    S = int(ctx.stat("seqnear_segment"))
    assert S // 6 >= 2 and (lens == 0).sum() > 300, "a lane crosses boundaries, runs of empty sequences among them"
    assert any(k == NONE for k in keys) and any(k != NONE for k in keys)


# ---------------------------------------------------------------- 5. one sequence: the nearest search
def test_one_sequence_equals_the_nearest_search(ctx):
    pats, text = R.planted(51, [9, 33, 70, 128], 3, 9000, copies=2)
    pats = pats + [b"NNNN"]
    setup(ctx, pats, 3)
    n = len(text)
    got = check_whole(ctx, text, pats, [0, n], mis=(0, 5))
    assert got == NG.device_result(ctx, text, len(pats))
    assert got[1:] == N.records(text, pats)
    assert int(ctx.stat("seqnear_segment")) == int(ctx.stat("nearest_segment"))


# ---------------------------------------------------------------- 6. ties: the first end of a sequence wins
def test_first_end_wins_inside_a_sequence(ctx):
    rs = np.random.RandomState(61)
    p = dna(rs, 20)
    n = 6400
    setup(ctx, [p])
    with Dev(ctx, 1) as dev:
        ctx.nearest_seq_shard_device(dev.text(b"A" * n), 0, n, n, 0, n, dev.table([0, n]), 1, dev.d_keys)
    S = int(ctx.stat("seqnear_segment"))
    assert 100 * S < n
    begins = [0, 10 * S + 5, n]
    # the same distance at two ends of sequence 1: in neighbouring lanes, then in different workgroups (lanes 20 and 90)
    for first, second in ((20 * S + 3, 21 * S + 9), (20 * S + 3, 90 * S + 1)):
        text = NG.tie_text(rs, n, p, (first, second), 9)
        assert N.n_attaining(text[begins[1]:], p) >= 2
        _, ends, _ = check_whole(ctx, text, [p], begins)
        assert ends[1] == (first, 0, 1)
    # the tie split by a boundary: each sequence keeps its own
    text = NG.tie_text(rs, n, p, (20 * S + 3, 90 * S + 1), 9)
    _, ends, _ = check_whole(ctx, text, [p], [0, 10 * S + 5, 50 * S, n])
    assert ends[1] == (20 * S + 3, 0, 1) and ends[2] == (90 * S + 1, 0, 1)


# ---------------------------------------------------------------- 7. pattern counts: slots not filled, m = 1 beside m = 128
@pytest.mark.parametrize("lens", ([11], [1, 128, 7, 64, 1], list(range(1, 34))))
def test_pattern_counts(ctx, lens):
    n = 5000
    pats, text = R.planted(70 + len(lens), lens, 2, n, copies=1)
    rs = np.random.RandomState(len(lens))
    begins = SR.begins_of([int(c) for c in rs.randint(0, n, size=9)] + [1234, 1234], n)
    setup(ctx, pats, 1)
    check_whole(ctx, text, pats, begins)


# ---------------------------------------------------------------- 8. shards
def shard_case():
    pats, text = R.planted(41, [9, 33, 70], 3, 9000, copies=2)
    begins = [0, 450, 450, 2500, 5200, 5203, 8000, len(text)]
    return pats, text, begins


@pytest.mark.parametrize("cuts", ([(0, 4001), (4001, 9000)], [(0, 2999), (2999, 6001), (6001, 9000)]))
def test_shards_share_the_keys(ctx, cuts):
    pats, text, begins = shard_case()
    n, halo, n_seq = len(text), 2 * 70 - 1, len(begins) - 1
    setup(ctx, pats)
    want = reference(text, pats, begins)
    for order in (cuts, cuts[::-1]):
        with Dev(ctx, n_seq * len(pats)) as dev:
            d_table = dev.table(begins)
            for ob, oe in order:
                lo, hi = max(0, ob - halo), min(n, oe + 1)         # exactly the bytes the call asks for
                ctx.nearest_seq_shard_device(dev.text(text, lo, hi, mis=3), lo, hi - lo, n, ob, oe, d_table, n_seq, dev.d_keys)
            assert dev.keys() == want[0]
            ctx.nearest_seq_records_device(dev.text(text), 0, n, n, d_table, n_seq, dev.d_keys, dev.d_end, dev.d_start)
            assert (dev.ends(), dev.starts()) == want[1:]
    # one shard's keys alone are the reference's of its ends
    with Dev(ctx, n_seq * len(pats)) as dev:
        ob, oe = cuts[1]
        lo, hi = ob - halo, min(n, oe + 1)
        ctx.nearest_seq_shard_device(dev.text(text, lo, hi), lo, hi - lo, n, ob, oe, dev.table(begins), n_seq, dev.d_keys)
        assert dev.keys() == SR.keys(text, pats, begins, ob, oe)


def test_halo_one_byte_short_is_refused(ctx, apm):
    pats, text, begins = shard_case()
    n, halo, n_seq = len(text), 2 * 70 - 1, len(begins) - 1
    setup(ctx, pats)
    with Dev(ctx, n_seq * len(pats)) as dev:
        d_table = dev.table(begins)
        for lo, hi in ((3000 - halo + 1, 6001), (3000 - halo, 6000)):
            with pytest.raises(apm.ApmError) as e:
                ctx.nearest_seq_shard_device(dev.text(text, lo, hi), lo, hi - lo, n, 3000, 6000, d_table, n_seq, dev.d_keys)
            assert e.value.status == INVALID
        assert dev.keys() == [NONE] * (n_seq * len(pats))


# ---------------------------------------------------------------- 9. the finishing pass on keys the test supplies
def test_snspan_triages_the_keys_it_is_given(ctx):
    text = b"TTTTTTTTTT" + b"ACGTACGTAC" + b"TTTTTTTTTTTT" + b"ACGAACGTAC" + b"TTTTTTTT"
    pats = [b"ACGTACGTAC", b"GGGG"]
    n = len(text)
    begins = [0, 14, 30, 30, n]                                  # sequence 0 ends inside the first copy; sequence 2 is empty
    setup(ctx, pats)
    true = reference(text, pats, begins)
    e1, _, d1 = true[1][2]
    assert e1 != NO_START and true[2][2][0] == 14 and e1 + 1 - 14 < len(pats[0]) + d1, "sequence 1: the span is clamped to the sequence's first byte"
    s7, d7 = R.span(text[30:], pats[1], 3, 11)                   # "GGGG" at end 41 with the bound 3, inside sequence 3
    assert R.span(text[30:], pats[0], 0, 11) == (None, 1) and s7 is not None and d7 == 3
    keys = [N.key(0, 19), NONE,          # sequence 0: an end of sequence 1 -> a made-up key; NONE
            true[0][2], N.key(4, 19),    # sequence 1: the true key; d >= m of "GGGG"
            NONE, N.key(0, 30),          # sequence 2 (empty): NONE; every end is outside it
            N.key(0, 41), N.key(3, 41)]  # sequence 3: d too small for this end (d* = 1); d larger than needed
    want_ends = [(NO_START, 0, DIST_INVALID), (NO_START, 1, 4), true[1][2], (NO_START, 1, DIST_INVALID),
                 (NO_START, 0, 10), (NO_START, 1, DIST_INVALID), (41, 0, 0), (41, 1, 3)]
    want_starts = want_ends[:2] + [true[2][2]] + want_ends[3:6] + [(NO_START, 0, 1), (30 + s7, 1, d7)]
    with Dev(ctx, len(keys)) as dev:
        dev.reset(keys)
        d_text, d_table = dev.text(text), dev.table(begins)
        ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, 4, dev.d_keys, dev.d_end, dev.d_start)
        assert [l for l, _ in ctx.launch_times()] == ["snspan"]
        assert dev.ends() == want_ends
        assert dev.starts() == want_starts
        assert dev.keys() == keys                                # only read
        # without d_start only the ends are written
        dev.reset(keys)
        ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, 4, dev.d_keys, dev.d_end, None)
        assert dev.ends() == want_ends and dev.starts() == [None] * len(keys)
        # a span the shard text does not cover: the end record is written, the start entry keeps its guard
        cut = 18
        assert true[2][2][0] < cut <= e1
        dev.reset(true[0])
        ctx.nearest_seq_records_device(dev.text(text, cut, n), cut, n - cut, n, d_table, 4, dev.d_keys, dev.d_end, dev.d_start)
        assert dev.ends() == true[1]
        covered = [e == NO_START or st >= cut for (e, _, _), (st, _, _) in zip(true[1], true[2])]
        assert not covered[2] and covered[3:] == [False] + [True] * 4
        assert dev.starts() == [st if c else None for st, c in zip(true[2], covered)]


# ---------------------------------------------------------------- 10. positions beyond 2^32
def test_positions_beyond_32_bits(ctx):
    rs = np.random.RandomState(51)
    pats = [dna(rs, 24), dna(rs, 90)]
    halo, n_total = 2 * 90 - 1, 1 << 33
    off = (1 << 32) + 4099
    t = bytearray(dna(rs, 4096))
    for at in (300, 1500, 2600, 3500):                           # a copy of each pattern, one substitution, in several sequences
        for j, p in enumerate(pats):
            s = bytearray(p)
            s[5] = ord("A") if s[5] != ord("A") else ord("C")
            t[at + 150 * j:at + 150 * j + len(p)] = s
    t = bytes(t)
    local = [0, 1000, 1000, 2500, 3400, len(t)]                  # sequence 0 begins at 0 of T, far in front of the shard
    begins = [0] + [off + b for b in local[1:-1]] + [n_total]
    n_seq = len(begins) - 1
    setup(ctx, pats)
    ob, oe = off + halo, off + len(t) - 1
    want = SR.keys(t, pats, local, halo, len(t) - 1, off)
    ends, starts = SR.records(t, pats, local, off)               # (every copy lies behind the halo: the best ends are the shard's own)
    assert want == [NONE if e == NO_START else N.key(d, e) for e, _, d in ends]
    assert [k == NONE for k in want] == [r // 2 == 1 for r in range(10)], "but for the empty sequence every pair has an answer"
    assert all(N.key_end(k) >> 32 == 1 and N.key_dist(k) == 1 for k in want if k != NONE)
    with Dev(ctx, n_seq * 2) as dev:
        d_text, d_table = dev.text(t, mis=1), dev.table(begins)
        ctx.nearest_seq_shard_device(d_text, off, len(t), n_total, ob, oe, d_table, n_seq, dev.d_keys)
        assert dev.keys() == want
        ctx.nearest_seq_records_device(d_text, off, len(t), n_total, d_table, n_seq, dev.d_keys, dev.d_end, dev.d_start)
        assert dev.ends() == ends
        assert dev.starts() == starts
        assert starts[0] == (ends[0][0] + 1 - len(pats[0]), 0, 1)


# ---------------------------------------------------------------- 11. the host-level call
def fasta_case():
    rs = np.random.RandomState(81)
    seq = [dna(rs, 130), dna(rs, 700), b"", dna(rs, 900), dna(rs, 40)]
    pats = [seq[1][290:330], seq[3][100:133], dna(rs, 64), b"NNNN", seq[1][680:700] + seq[3][:20]]
    src = b"\r\n".join(seq[0][i:i + 60] for i in range(0, len(seq[0]), 60)).lower() + b"\r\n"     # bytes in front of the first header
    for name, s in zip((b">one first\r\n", b">empty\r\n", b">two\r\n", b">last one\r\n"), seq[1:]):
        src += name + b"".join(s[i:i + 60] + b"\r\n" for i in range(0, len(s), 60)).lower()
    return seq, pats, src


def as_rows(ends, starts):
    return [(i, None if e == NO_START else e, d, None if s == NO_START else s) for (e, i, d), (s, _, _) in zip(ends, starts)]


def test_host_call_on_a_multi_fasta(ctx, apm):
    seq, pats, src = fasta_case()
    flags = apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER
    n_seq, ends, starts = SR.source_records(src, flags, pats)
    P = len(pats)
    assert n_seq == 5 and ends[1 * P + 0][2] == 0 and ends[3 * P + 1][2] == 0 and ends[2 * P] == (NO_START, 0, 40)
    assert 0 < ends[1 * P + 4][2] and 0 < ends[3 * P + 4][2], "the pattern across the boundary matches neither side exactly"
    want = as_rows(ends, starts)
    setup(ctx, pats, 2)
    before = ctx.count_buffer(src)
    ctx.set_text_mode(flags)
    try:
        counted = ctx.count_buffer(src)
        assert ctx.find_nearest_seq_buffer(src) == (5, want)
        assert [l for l, _ in ctx.launch_times()] == ["snear", "snspan"]
        assert ctx.stat("map_ms") > 0                            # the map launches ran behind them
        assert ctx.timing()["n_launches"] >= 2
        # the context's own table stands: apm_get_sequences and apm_locate_buffer work right behind the call
        table, n_tab = ctx.sequences()
        assert n_tab == 5 and [t for _, t in table] == [0, 130, 830, 830, 1730, 1770]
        live = [(r, w) for r, w in enumerate(want) if w[1] is not None]
        locs = ctx.locate([(w[0], w[3]) for _, w in live])
        assert [l[1] for l in locs] == [r // P for r, _ in live]
        assert ctx.find_nearest_seq_buffer(src, spans=False) == (5, [w[:3] for w in want])
        assert ctx.count_buffer(src) == counted                  # the plan is not touched
        for k in (0, 64):                                        # k is not looked at: 64 >= m of four patterns
            setup(ctx, pats, k)
            assert ctx.find_nearest_seq_buffer(src) == (5, want), k
        # without FASTA in the mode: one sequence, the nearest search's answer
        ctx.set_text_mode(apm.APM_TEXT_UPPER)
        plain = b"".join(seq).lower()
        n1, rows = ctx.find_nearest_seq_buffer(plain)
        assert n1 == 1 and rows == ctx.find_nearest_buffer(plain)
        # a header alone, and an empty source
        ctx.set_text_mode(flags)
        assert ctx.find_nearest_seq_buffer(b">only a header\r\n") == (2, [(i, None, len(p), None) for i, p in enumerate(pats)] * 2)
        assert ctx.find_nearest_seq_buffer(b"") == (1, [(i, None, len(p), None) for i, p in enumerate(pats)])
    finally:
        ctx.set_text_mode(0)
    assert ctx.count_buffer(src) == ctx.count_buffer(src) and before == H.oracle_counts(src, pats, 2)


def test_host_call_sizes_and_refusals(ctx, apm):
    import ctypes
    seq, pats, src = fasta_case()
    lib, P = apm.load_library(), len(pats)
    setup(ctx, pats, 2)
    buf = ctypes.create_string_buffer(src, len(src))
    n_seq = ctypes.c_uint64(99)
    ends = (apm.ApmMatch * (4 * P + 2))()
    guard = bytes(range(1, 17)) * (4 * P + 2)
    ctypes.memmove(ends, guard, len(guard))
    # mode 0
    assert lib.apm_find_nearest_seq_buffer(ctx._ctx, buf, len(src), ends, None, 4, ctypes.byref(n_seq)) == STATE
    ctx.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
    try:
        # too few sequences of room: INVALID, the count set, nothing written
        assert lib.apm_find_nearest_seq_buffer(ctx._ctx, buf, len(src), ends, None, 4, ctypes.byref(n_seq)) == INVALID
        assert n_seq.value == 5 and bytes(ends) == guard
        # a count of sequences
        n_seq.value = 99
        assert lib.apm_find_nearest_seq_buffer(ctx._ctx, buf, len(src), None, None, 0, ctypes.byref(n_seq)) == INVALID
        assert n_seq.value == 5
        assert lib.apm_find_nearest_seq_buffer(ctx._ctx, buf, len(src), None, None, 5, ctypes.byref(n_seq)) == INVALID    # NULL arrays with room asked for
        assert lib.apm_find_nearest_seq_buffer(ctx._ctx, buf, len(src), ends, None, 4, None) == INVALID
        # more than the first guess of the Python mirror: the retry
        many = b"".join(b">s%d\nACGT\n" % i for i in range(100))
        n_many, rows = ctx.find_nearest_seq_buffer(many)
        assert n_many == 101 and len(rows) == 101 * P
        assert rows == as_rows(*SR.source_records(many, apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER, pats)[1:])
        # a pattern of 129 bytes
        setup(ctx, [b"ACGT" * 32 + b"A", b"ACGTAC"], 2)
        with pytest.raises(apm.ApmError) as e:
            ctx.find_nearest_seq_buffer(src)
        assert e.value.status == UNSUPPORTED
    finally:
        ctx.set_text_mode(0)


def test_device_calls_refuse_bad_arguments(ctx, apm):
    text = b"ACGT" * 64
    n = len(text)
    setup(ctx, [b"ACGT" * 32 + b"A", b"ACGTAC"], 2)
    with Dev(ctx, 4) as dev:
        d_text, d_table = dev.text(text), dev.table([0, 100, n])
        for call in (lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, n, d_table, 2, dev.d_keys),
                     lambda: ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, 2, dev.d_keys, dev.d_end, dev.d_start)):
            with pytest.raises(apm.ApmError) as e:
                call()
            assert e.value.status == UNSUPPORTED
        setup(ctx, [b"ACGTAC", b"GG"])
        for bad in (lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 9, 8, d_table, 2, dev.d_keys),         # own_begin > own_end
                    lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, 8, d_table, 2, dev.d_keys + 4),     # misaligned keys
                    lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, 8, d_table, 2, None),
                    lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, 8, None, 2, dev.d_keys),
                    lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, 8, d_table + 4, 2, dev.d_keys),
                    lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, 8, d_table, 0, dev.d_keys),         # n_seq == 0
                    lambda: ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, 0, dev.d_keys, dev.d_end, None),
                    lambda: ctx.nearest_seq_records_device(d_text, 0, n, n, None, 2, dev.d_keys, dev.d_end, None),
                    lambda: ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, 2, dev.d_keys, dev.d_end + 8, None),
                    lambda: ctx.nearest_seq_records_device(d_text, 0, n, n, d_table, 2, dev.d_keys, None, None)):
            with pytest.raises(apm.ApmError) as e:
                bad()
            assert e.value.status == INVALID
        for big in (lambda: ctx.nearest_seq_shard_device(d_text, 0, n, (1 << 56) + 1, 0, n, d_table, 2, dev.d_keys),
                    lambda: ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, n, d_table, 1 << 32, dev.d_keys)):
            with pytest.raises(apm.ApmError) as e:
                big()
            assert e.value.status == UNSUPPORTED
        assert dev.keys() == [NONE] * 4 and dev.ends() == [None] * 4 and dev.starts() == [None] * 4


def test_multi_device_context_is_refused(apm):
    rehearse = apm.device_count() < 2                            # two shards on the one device
    if rehearse:
        os.environ["APM_DEVICES"] = "0,0"
    try:
        with apm.ApmContext(n_devices=2) as c:
            c.set_patterns([b"ACGTACGT"], 1)
            with pytest.raises(apm.ApmError) as e:
                c.find_nearest_seq_buffer(b">a\nACGT\n")
            assert e.value.status == UNSUPPORTED
    finally:
        if rehearse:
            del os.environ["APM_DEVICES"]


# ---------------------------------------------------------------- 12. the command-line host
def run_cli(args):
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    return subprocess.run([exe] + args, capture_output=True, text=True)


def test_cli_nearest_per_sequence(tmp_path, apm):
    seq, pats, src = fasta_case()
    pats = [p for p in pats if p != b"NNNN"] + [b"NNNNN"]
    fa = tmp_path / "reads.fa"
    fa.write_bytes(src)
    flags = apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER
    T, _ = SR.TN.normalize(src, flags)
    begins = [t for _, t in SR.SQ.sequences(src, flags)]
    ends, starts = SR.records(T, pats, begins)
    names, P = ["-", "one", "empty", "two", "last"], len(pats)
    want = []
    for i, p in enumerate(pats):
        for s, name in enumerate(names):
            (e, _, d), (st, _, _) = ends[s * P + i], starts[s * P + i]
            what = "none" if e == NO_START else "%d-%d:%d" % (st - begins[s], e - st + 1, d)
            want.append("Nearest occurrence of pattern <%s> in <%s>: %s" % (p.decode(), name, what))
    assert sum(w.endswith("none") for w in want) >= 5 + len(pats) - 1
    for k in ("0", "2", "30"):                                   # the distance is parsed and ignored
        r = run_cli([k, str(fa)] + [p.decode() for p in pats] + ["--fasta", "--upper", "--nearest-per-sequence"])
        assert r.returncode == 0, r.stderr
        assert [l for l in r.stdout.splitlines() if l.startswith("Nearest occurrence")] == want, k
        assert "Number of matches" not in r.stdout
    # nothing in front of the first header: sequence 0 is not listed
    fb = tmp_path / "headed.fa"
    fb.write_bytes(src[src.index(b">"):])
    r = run_cli(["0", str(fb)] + [p.decode() for p in pats] + ["--fasta", "--upper", "--nearest-per-sequence"])
    assert r.returncode == 0, r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith("Nearest occurrence")] == [w for w in want if " in <->" not in w]
    # refused without --fasta, and together with --nearest and the listing flags
    r = run_cli(["2", str(fa)] + [p.decode() for p in pats] + ["--nearest-per-sequence"])
    assert r.returncode == 1 and "--fasta" in r.stderr
    r = run_cli(["2", str(fa)] + [p.decode() for p in pats] + ["--upper", "--nearest-per-sequence"])
    assert r.returncode == 1 and "--fasta" in r.stderr
    for other in ("--nearest", "--positions", "--distances", "--alignments", "--best", "--occurrences", "--occurrence-scripts=all", "--sequences"):
        r = run_cli(["2", str(fa)] + [p.decode() for p in pats] + ["--fasta", "--nearest-per-sequence", other])
        assert r.returncode == 1 and "--nearest-per-sequence" in r.stderr, other
