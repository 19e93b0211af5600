"""The nearest-occurrence search on the GPU: apm_nearest_shard_device, apm_nearest_records_device and
apm_find_nearest_buffer give exactly the keys and records include/apm.h pins ("nearest occurrences").  The truth everywhere
is tests/nearest_ref.py on occ_ref's literal recurrence; every comparison is of the COMPLETE result.  Device buffers carry
preset guard words around the keys and the record arrays, and the tests compare those.  Texts are small, so the segment S
shrinks to about 2 m_max: lane seams everywhere, workgroup seams at 64 and 128 segments."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import nearest_ref as N
import occ_ref as R
import textnorm_ref as TN

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
GUARD = b"\xa5" * 16
MS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)
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
    """device buffers of one test, freed at its end: the shard texts, the guarded keys and the guarded record arrays"""

    def __init__(self, ctx, n_patterns):
        self.ctx, self.P, self.ptrs = ctx, n_patterns, []
        self.base_keys = self.alloc(32 + 8 * n_patterns)
        self.base_end = self.alloc(64 + 16 * n_patterns)
        self.base_start = self.alloc(64 + 16 * n_patterns)
        self.d_keys, self.d_end, self.d_start = self.base_keys + 16, self.base_end + 32, self.base_start + 32
        self.reset()

    def alloc(self, nbytes):
        p = self.ctx.device_alloc(max(nbytes, 16))
        self.ptrs.append(p)
        return p

    def reset(self, keys=None):
        """guards everywhere, the keys preset to NONE (or to `keys`)"""
        keys = [NONE] * self.P if keys is None else keys
        self.ctx.device_upload(self.base_keys, GUARD + struct.pack("<%dQ" % self.P, *keys) + GUARD)
        for base in (self.base_end, self.base_start):
            self.ctx.device_upload(base, GUARD * (self.P + 4))

    def text(self, text, lo=0, hi=None, mis=0):
        """the bytes [lo, hi) of the text at byte `mis` of an allocation with 16 readable bytes around them"""
        hi = len(text) if hi is None else hi
        d = self.alloc(hi - lo + 48)
        self.ctx.device_upload(d, b"\x5a" * (hi - lo + 48))
        if hi > lo:
            self.ctx.device_upload(d + mis, text[lo:hi])
        return d + mis

    def keys(self):
        self.ctx.synchronize()
        raw = self.ctx.device_download(self.base_keys, 32 + 8 * self.P)
        assert raw[:16] == GUARD and raw[-16:] == GUARD, "the guards around d_keys were written"
        return list(struct.unpack("<%dQ" % self.P, raw[16:-16]))

    def records(self, base):
        """[(pos, pattern, dist)], None for an entry that still holds its guard"""
        self.ctx.synchronize()
        raw = self.ctx.device_download(base, 64 + 16 * self.P)
        assert raw[:32] == GUARD * 2 and raw[-32:] == GUARD * 2, "the guards around a record array were written"
        body = raw[32:-32]
        return [None if body[16 * i:16 * i + 16] == GUARD else struct.unpack_from("<QII", body, 16 * i) for i in range(self.P)]

    def ends(self):
        return self.records(self.base_end)

    def starts(self):
        return self.records(self.base_start)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.device_free(p)


def as_tuples(ends, starts):
    """the reference's record pair in the form ApmContext.find_nearest_buffer returns"""
    return [(i, None if e == NO_START else e, d, None if s == NO_START else s) for (e, i, d), (s, _, _) in zip(ends, starts)]


def device_result(ctx, text, n_patterns, mis=0):
    """both device calls over the whole text: (keys, end records, start records)"""
    n = len(text)
    with Dev(ctx, n_patterns) as dev:
        d_text = dev.text(text, mis=mis)
        ctx.nearest_shard_device(d_text, 0, n, n, 0, n, dev.d_keys)
        ctx.nearest_records_device(d_text, 0, n, n, dev.d_keys, dev.d_end, dev.d_start)
        return dev.keys(), dev.ends(), dev.starts()


def check_whole(ctx, text, pats, mis=(0,)):
    """the whole text through both device calls (at every misalignment) and through apm_find_nearest_buffer; -> the reference"""
    ends, starts = N.records(text, pats)
    want_keys = [NONE if e == NO_START else N.key(d, e) for e, _, d in ends]
    for a in mis:
        assert device_result(ctx, text, len(pats), a) == (want_keys, ends, starts), a
    assert ctx.find_nearest_buffer(text) == as_tuples(ends, starts)
    assert ctx.find_nearest_buffer(text, spans=False) == [t[:3] for t in as_tuples(ends, starts)]
    return ends, starts


# ---------------------------------------------------------------- 1. parity: every width, planted and unplanted patterns
@pytest.mark.parametrize("n,seed,mis", [(6000, 11, (0, 1, 7, 15)), (40000, 12, (7,))])
def test_parity(ctx, n, seed, mis):
    pats, text = R.planted(seed, list(MS), 3, n, copies=1)
    rs = np.random.RandomState(seed + 1000)                    # (not the text's own stream)
    pats = pats + [dna(rs, m) for m in (16, 64, 128)]          # unplanted: d about m / 4 .. m / 2
    setup(ctx, pats, 3)
    ends, _ = check_whole(ctx, text, pats, mis)
    assert [l for l, _ in ctx.launch_times()] == ["nearest", "nspan"]
    assert all(e != NO_START for e, _, _ in ends)
    if n == 40000:
        assert ends[-1][2] >= 40, "the unplanted 128-byte pattern exercises a large distance"
        S = int(ctx.stat("nearest_segment"))
        assert S % 16 == 0 and 2 * 128 - 1 <= S <= 16 * (2 * 128 - 1) + 15
        assert n // S >= 128, "the launch has workgroup seams at 64 and at 128 segments"
        assert int(ctx.stat("nearest_lanes")) == -(-n // S) * len(pats)


# ---------------------------------------------------------------- 2. the first end wins
def tie_text(rs, n, p, ends, alter):
    """random DNA with a copy of p, byte `alter` substituted, ending at every end of `ends`"""
    t = bytearray(dna(rs, n))
    s = bytearray(p)
    s[alter] = ord("A") if s[alter] != ord("A") else ord("C")
    for e in ends:
        t[e + 1 - len(p):e + 1] = s
    return bytes(t)


def test_first_end_wins_at_every_seam(ctx):
    rs = np.random.RandomState(21)
    p = dna(rs, 20)
    n = 6400
    setup(ctx, [p])
    ctx.find_nearest_buffer(dna(rs, n))
    S = int(ctx.stat("nearest_segment"))
    assert S >= 2 * len(p) - 1 and 128 * S + 1 + 4 * S < n, S
    for q in (1, 2, 63, 64, 65, 128):
        for delta in (-1, 0, 1):
            first = q * S + delta
            text = tie_text(rs, n, p, (first, first + 3 * S + 1), 9)
            assert N.n_attaining(text, p) >= 2
            ends, _ = check_whole(ctx, text, [p])
            assert ends == [(first, 0, 1)], (q, delta)
            assert int(ctx.stat("nearest_segment")) == S


def test_first_end_wins_on_a_periodic_text(ctx):
    text, p = b"ACG" * 2000, b"ACG" * 6
    assert N.n_attaining(text, p) >= 2
    setup(ctx, [p, b"CGA" * 11, b"GAC" * 42])
    ends, starts = check_whole(ctx, text, [p, b"CGA" * 11, b"GAC" * 42])
    assert ends[0] == (17, 0, 0) and starts[0] == (0, 0, 0)


# ---------------------------------------------------------------- 3. the warm-up is 2 m - 1 bytes, and all of it is needed
@pytest.mark.parametrize("m,d", [(8, 3), (33, 7), (64, 20), (128, 40)])
def test_spread_copy_in_front_of_a_segment_start(ctx, m, d):
    rs = np.random.RandomState(100 + m)
    p = dna(rs, m)
    copy = bytearray()
    cuts = [3 + round(j * (m - 6) / (d - 1)) for j in range(d)]  # d foreign bytes, evenly inside the pattern but for 3 bytes at both ends
    for i, c in enumerate(p):
        copy.append(c)
        copy += b"N" * cuts.count(i + 1)
    assert len(copy) == m + d
    n = 66 * ((2 * m - 1 + 15) // 16 * 16) + 200             # (S, if the chooser takes its smallest)
    setup(ctx, [p])
    ctx.find_nearest_buffer(b"N" * n)
    S = int(ctx.stat("nearest_segment"))
    assert S >= 2 * m - 1 and 65 * S + 2 <= n, S
    for q in (3, 64):
        for delta in (0, 1):
            e = q * S + delta                                  # the copy's last byte: at the segment start, or just behind it
            text = b"N" * (e + 1 - len(copy)) + bytes(copy) + b"N" * (n - e - 1)
            wd, we, ws = N.nearest(text, p)
            assert wd == d and m + d - 2 <= we + 1 - ws <= m + d
            assert ws < q * S - m and q * S <= we <= q * S + 1, "the span starts more than m bytes in front of the segment start"
            check_whole(ctx, text, [p])
            assert int(ctx.stat("nearest_segment")) == S


def test_distance_m_minus_one(ctx):
    p = b"A" * 7 + b"B"
    setup(ctx, [p])
    ctx.find_nearest_buffer(b"C" * 3000)
    S = int(ctx.stat("nearest_segment"))
    for at in (0, 5, S - 1, S, 64 * S, 64 * S + 1, 2999):
        text = b"C" * at + b"B" + b"C" * (2999 - at)
        assert N.nearest(text, p) == (7, at, at)
        check_whole(ctx, text, [p])


# ---------------------------------------------------------------- 4. none
def test_none(ctx):
    setup(ctx, [b"AAAA", b"ACGTACGT"])
    ends, starts = check_whole(ctx, b"C" * 50, [b"AAAA", b"ACGTACGT"])
    assert ends[0] == starts[0] == (NO_START, 0, 4) and ends[1][0] != NO_START
    ends, starts = check_whole(ctx, b"", [b"AAAA", b"ACGTACGT"])
    assert ends == starts == [(NO_START, 0, 4), (NO_START, 1, 8)]
    for text in (b"ACG", b"T", b"GTACGT", b"NNNNNNN"):          # shorter than the pattern: an answer unless no byte is shared
        check_whole(ctx, text, [b"AAAA", b"ACGTACGT"])


# ---------------------------------------------------------------- 5. k is ignored
def test_k_is_ignored(ctx, apm):
    pats, text = R.planted(31, [4, 12, 40, 100], 2, 5000, copies=1)
    want = as_tuples(*N.records(text, pats))
    for k in (0, 3, 5):                                        # 5 >= the shortest pattern
        setup(ctx, pats, k)
        assert ctx.find_nearest_buffer(text) == want, k
    with pytest.raises(apm.ApmError) as e:
        ctx.find_occ_buffer(text, R.ALL)
    assert e.value.status == UNSUPPORTED
    assert ctx.find_nearest_buffer(text) == want
    assert device_result(ctx, text, len(pats))[1:] == N.records(text, pats)


# ---------------------------------------------------------------- 6. shards
def shard_case():
    pats, text = R.planted(41, [9, 33, 70], 3, 9000, copies=2)
    return pats, text


def test_three_shards_share_the_keys(ctx):
    pats, text = shard_case()
    n, halo = len(text), 2 * 70 - 1
    setup(ctx, pats)
    ends, starts = N.records(text, pats)
    want_keys = [N.key(d, e) for e, _, d in ends]
    cuts = [(0, 2999), (2999, 6001), (6001, n)]
    for order in (cuts, cuts[::-1]):
        with Dev(ctx, len(pats)) as dev:
            for ob, oe in order:
                lo, hi = max(0, ob - halo), min(n, oe + 1)     # exactly the bytes the call asks for
                ctx.nearest_shard_device(dev.text(text, lo, hi, mis=3), lo, hi - lo, n, ob, oe, dev.d_keys)
            assert dev.keys() == want_keys
            ctx.nearest_records_device(dev.text(text), 0, n, n, dev.d_keys, dev.d_end, dev.d_start)
            assert (dev.ends(), dev.starts()) == (ends, starts)
    # one shard's keys alone are the reference's of its ends
    with Dev(ctx, len(pats)) as dev:
        ob, oe = cuts[1]
        lo, hi = ob - halo, oe + 1
        ctx.nearest_shard_device(dev.text(text, lo, hi), lo, hi - lo, n, ob, oe, dev.d_keys)
        assert dev.keys() == N.keys(text, pats, ob, oe)


def test_halo_one_byte_short_is_refused(ctx, apm):
    pats, text = shard_case()
    n, halo = len(text), 2 * 70 - 1
    setup(ctx, pats)
    with Dev(ctx, len(pats)) as dev:
        for lo, hi in ((3000 - halo + 1, 6001), (3000 - halo, 6000)):
            with pytest.raises(apm.ApmError) as e:
                ctx.nearest_shard_device(dev.text(text, lo, hi), lo, hi - lo, n, 3000, 6000, dev.d_keys)
            assert e.value.status == INVALID
        assert dev.keys() == [NONE] * len(pats)


def test_nspan_leaves_a_start_another_shard_covers(ctx):
    pats, text = shard_case()
    n = len(text)
    setup(ctx, pats)
    ends, starts = N.records(text, pats)
    keys = [N.key(d, e) for e, _, d in ends]
    i = max(range(len(pats)), key=lambda j: ends[j][0])        # the pattern whose end lies farthest right
    cut = ends[i][0]                                           # a shard [0, cut): it holds the span's bytes but for the end itself
    with Dev(ctx, len(pats)) as dev:
        dev.reset(keys)
        ctx.nearest_records_device(dev.text(text, 0, cut), 0, cut, n, dev.d_keys, dev.d_end, dev.d_start)
        assert dev.ends() == ends
        got = dev.starts()
        assert got[i] is None, "the entry of a span the shard does not cover keeps its guard"
        assert [g for j, g in enumerate(got) if j != i] == [s for j, s in enumerate(starts) if j != i and ends[j][0] < cut]
        ctx.nearest_records_device(dev.text(text, cut - 300, n), cut - 300, n - cut + 300, n, dev.d_keys, dev.d_end, dev.d_start)
        assert dev.starts()[i] == starts[i]
        assert dev.keys() == keys                              # only read


# ---------------------------------------------------------------- 7. positions beyond 2^32
def test_positions_beyond_32_bits(ctx):
    rs = np.random.RandomState(51)
    pats = [dna(rs, 24), dna(rs, 90)]
    halo, n_total = 2 * 90 - 1, 1 << 34
    setup(ctx, pats)
    shard = []
    for off in ((1 << 32) - 2048, (1 << 33) + 5):
        t = bytearray(dna(rs, 4096))
        for j, p in enumerate(pats):                           # the same copy, one substitution, in both shards
            s = bytearray(p)
            s[5] = ord("A") if s[5] != ord("A") else ord("C")
            t[2100 + 700 * j:2100 + 700 * j + len(p)] = s      # (behind 2^32 in the first shard)
        shard.append((off, bytes(t)))
    with Dev(ctx, 2) as dev:
        for off, t in shard[::-1]:                             # the upper shard first: the lower end must still win
            ctx.nearest_shard_device(dev.text(t, mis=1), off, len(t), n_total, off + halo, off + len(t) - 1, dev.d_keys)
        off, t = shard[0]
        want = N.keys(t, pats, halo, len(t) - 1, off)
        assert want == [N.key(1, off + 2100 + 700 * j + len(p) - 1) for j, p in enumerate(pats)]
        assert all(N.key_end(k) >> 32 == 1 for k in want)
        upper = N.keys(shard[1][1], pats, halo, 4095, shard[1][0])
        assert [N.key_dist(k) for k in upper] == [1, 1] and all(N.key_end(k) >> 33 == 1 for k in upper)
        assert dev.keys() == want
        ctx.nearest_records_device(dev.text(t), off, len(t), n_total, dev.d_keys, dev.d_end, dev.d_start)
        assert dev.ends() == [(N.key_end(k), j, 1) for j, k in enumerate(want)]
        assert dev.starts() == [(N.key_end(k) + 1 - len(p), j, 1) for j, (k, p) in enumerate(zip(want, pats))]
        # the upper shard alone
        dev.reset()
        off, t = shard[1]
        ctx.nearest_shard_device(dev.text(t), off, len(t), n_total, off + halo, off + len(t) - 1, dev.d_keys)
        assert dev.keys() == upper


# ---------------------------------------------------------------- 8. made-up keys
def test_nspan_triages_made_up_keys(ctx):
    text = b"TTTTTTTTTT" + b"ACGTACGTAC" + b"TTTTTTTTTTTT" + b"ACGAACGTAC" + b"TTTTTTTT"
    pats = [b"ACGTACGTAC"] * 5 + [b"GGGG"]
    n = len(text)
    setup(ctx, pats)
    keys = [N.key(0, 41),        # d too small for this end: d* = 1 there
            N.key(2, 41),        # d larger than needed: the span rule at k := 2 finds d* = 1
            N.key(10, 19),       # d >= m
            N.key(0, n),         # end >= n_total
            N.key(0, 19),        # a true key
            NONE]
    with Dev(ctx, len(pats)) as dev:
        dev.reset(keys)
        ctx.nearest_records_device(dev.text(text), 0, n, n, dev.d_keys, dev.d_end, dev.d_start)
        assert [l for l, _ in ctx.launch_times()] == ["nspan"]
        assert dev.ends() == [(41, 0, 0), (41, 1, 2), (NO_START, 2, DIST_INVALID), (NO_START, 3, DIST_INVALID), (19, 4, 0), (NO_START, 5, 4)]
        assert R.span(text, pats[0], 0, 41) == (None, 1) and R.span(text, pats[0], 2, 41) == (32, 1)
        assert dev.starts() == [(NO_START, 0, 1), (32, 1, 1), (NO_START, 2, DIST_INVALID), (NO_START, 3, DIST_INVALID), (10, 4, 0), (NO_START, 5, 4)]
        assert dev.keys() == keys
        # without d_start only the ends are written
        dev.reset(keys)
        ctx.nearest_records_device(dev.text(text), 0, n, n, dev.d_keys, dev.d_end, None)
        assert dev.ends()[4] == (19, 4, 0) and dev.starts() == [None] * len(pats)


# ---------------------------------------------------------------- 9. a text mode
def test_fasta_upper_reports_source_offsets(ctx, apm):
    rs = np.random.RandomState(61)
    seq = [dna(rs, 700), dna(rs, 900)]
    pats = [seq[0][290:330], seq[1][100:133], dna(rs, 64), b"NNNN"]
    occ = bytearray(pats[1])
    del occ[7]
    seq[0] = seq[0][:50] + bytes(occ) + seq[0][50 + len(occ):]  # an earlier copy of pattern 1, a byte short: the exact one wins
    src = b""
    for name, s in zip((b">one first\r\n", b">two\r\n"), seq):
        src += name + b"\r\n".join(s[i:i + 60] for i in range(0, len(s), 60)).lower() + b"\r\n"
    T, src_of = TN.normalize(src, TN.FASTA | TN.UPPER)
    assert T == seq[0] + seq[1]
    ends, starts = N.records(T, pats)
    assert ends[0] == (329, 0, 0) and ends[1] == (700 + 132, 1, 0) and ends[2][2] > 10 and ends[3][0] == NO_START
    want = [(i, None if e == NO_START else src_of[e], d, None if s == NO_START else src_of[s]) for (e, i, d), (s, _, _) in zip(ends, starts)]
    setup(ctx, pats, 2)
    ctx.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
    try:
        assert ctx.find_nearest_buffer(src) == want
        assert [l for l, _ in ctx.launch_times()] == ["nearest", "nspan"]
        assert ctx.stat("map_ms") > 0                          # the map launches ran behind them
        assert ctx.find_nearest_buffer(src, spans=False) == [w[:3] for w in want]
        assert ctx.find_nearest_buffer(b">only a header\r\n") == [(i, None, len(p), None) for i, p in enumerate(pats)]
    finally:
        ctx.set_text_mode(0)


# ---------------------------------------------------------------- 10. what the call leaves alone, and what it refuses
def test_counting_calls_are_untouched(ctx):
    pats, text = shard_case()
    setup(ctx, pats, 3)
    before = (ctx.count_buffer(text), [ctx.pattern_kernel(i) for i in range(len(pats))])
    ctx.find_nearest_buffer(text)
    ctx.find_nearest_buffer(text, spans=False)
    assert (ctx.count_buffer(text), [ctx.pattern_kernel(i) for i in range(len(pats))]) == before
    assert before[0] == H.oracle_counts(text, pats, 3)
    t = ctx.timing()
    assert t["n_launches"] >= 1


def test_a_pattern_of_129_bytes_is_refused(ctx, apm):
    text = b"ACGT" * 64
    pats = [b"ACGT" * 32 + b"A", b"ACGTAC"]
    setup(ctx, pats, 2)
    with Dev(ctx, 2) as dev:
        d_text = dev.text(text)
        for call in (lambda: ctx.nearest_shard_device(d_text, 0, len(text), len(text), 0, len(text), dev.d_keys),
                     lambda: ctx.nearest_records_device(d_text, 0, len(text), len(text), dev.d_keys, dev.d_end, dev.d_start),
                     lambda: ctx.find_nearest_buffer(text)):
            with pytest.raises(apm.ApmError) as e:
                call()
            assert e.value.status == UNSUPPORTED
        assert dev.keys() == [NONE, NONE] and dev.ends() == [None, None] and dev.starts() == [None, None]
        setup(ctx, [b"ACGTAC"])
        for bad in (lambda: ctx.nearest_shard_device(d_text, 0, len(text), len(text), 9, 8, dev.d_keys),       # own_begin > own_end
                    lambda: ctx.nearest_shard_device(d_text, 0, len(text), len(text), 0, 8, dev.d_keys + 4),   # misaligned keys
                    lambda: ctx.nearest_shard_device(d_text, 0, len(text), len(text), 0, 8, None),
                    lambda: ctx.nearest_records_device(d_text, 0, len(text), len(text), dev.d_keys, dev.d_end + 8, None),
                    lambda: ctx.nearest_records_device(d_text, 0, len(text), len(text), dev.d_keys, None, None)):
            with pytest.raises(apm.ApmError) as e:
                bad()
            assert e.value.status == INVALID
        with pytest.raises(apm.ApmError) as e:
            ctx.nearest_shard_device(d_text, 0, len(text), (1 << 56) + 1, 0, len(text), dev.d_keys)
        assert e.value.status == UNSUPPORTED


def test_multi_device_context_is_refused(apm):
    rehearse = apm.device_count() < 2                          # two shards on the one device
    if rehearse:
        os.environ["APM_DEVICES"] = "0,0"
    try:
        with apm.ApmContext(n_devices=2) as c:
            c.set_patterns([b"ACGTACGT"], 1)
            with pytest.raises(apm.ApmError) as e:
                c.find_nearest_buffer(b"ACGT" * 64)
            assert e.value.status == UNSUPPORTED
    finally:
        if rehearse:
            del os.environ["APM_DEVICES"]


# ---------------------------------------------------------------- 11. the command-line host
def run_cli(args):
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    return subprocess.run([exe] + args, capture_output=True, text=True)


def render(text, pats):
    ends, starts = N.records(text, pats)
    return ["Nearest occurrence of pattern <%s>: %s" % (p.decode(), "none" if e == NO_START else "%d-%d:%d" % (s, e, d))
            for p, (e, _, d), (s, _, _) in zip(pats, ends, starts)]


def test_cli_nearest(tmp_path):
    pats, text = R.planted(99, [24, 40], 2, 3000, copies=2)
    pats = pats + [b"NNNNN", b"ACGTTGCAGGATCC"]
    path = tmp_path / "text.txt"
    path.write_bytes(text)
    want = render(text, pats)
    assert want[2].endswith(": none") and not want[3].endswith("none")
    for k in ("0", "2", "7"):                                  # the distance is parsed and ignored (7 >= m of a pattern)
        r = run_cli([k, str(path)] + [p.decode() for p in pats] + ["--nearest"])
        assert r.returncode == 0, r.stderr
        assert [l for l in r.stdout.splitlines() if l.startswith("Nearest occurrence")] == want, k
        assert "Number of matches" not in r.stdout
    for other in ("--positions", "--distances", "--alignments", "--best", "--best=2", "--occurrences", "--occurrence-scripts=all", "--sequences"):
        r = run_cli(["2", str(path)] + [p.decode() for p in pats] + ["--nearest", other, "--fasta"])
        assert r.returncode == 1 and "--nearest" in r.stderr, other
    # a FASTA file: offsets in the file
    T = text[:1200]
    src = b">chr1 test\n" + b"\n".join(T[i:i + 50] for i in range(0, 1200, 50)).lower() + b"\n"
    fa = tmp_path / "text.fa"
    fa.write_bytes(src)
    norm, src_of = TN.normalize(src, TN.FASTA | TN.UPPER)
    assert norm == T
    ends, starts = N.records(T, pats)
    lines = ["Nearest occurrence of pattern <%s>: %s" % (p.decode(), "none" if e == NO_START else "%d-%d:%d" % (src_of[s], src_of[e], d))
             for p, (e, _, d), (s, _, _) in zip(pats, ends, starts)]
    r = run_cli(["2", str(fa)] + [p.decode() for p in pats] + ["--nearest", "--fasta", "--upper"])
    assert r.returncode == 0, r.stderr
    assert [l for l in r.stdout.splitlines() if l.startswith("Nearest occurrence")] == lines
