"""The occurrence search on the GPU: apm_occ_shard_device, apm_occ_spans_device and apm_find_occ_buffer report exactly the
ends, distances and spans include/apm.h pins ("occurrence search").  The truth everywhere is tests/occ_ref.py, the literal
recurrence in numpy; every comparison is over the COMPLETE record set, under both flags.  Device buffers carry preset guard
words, and the tests compare those."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import occ_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
ALL, LOCAL_MIN = R.ALL, R.LOCAL_MIN
GUARD = b"\xa5" * 16
MS = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128)
NO_START = R.NO_START
DIST_INVALID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


class Dev:
    """device buffers of one test, freed at its end"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes, data=None):
        p = self.ctx.device_alloc(max(nbytes, 16))
        self.ptrs.append(p)
        if data:
            self.ctx.device_upload(p, data)
        return p

    def text(self, text, lo=0, hi=None, mis=0):
        """the bytes [lo, hi) of the text at byte `mis` of an allocation with 16 readable bytes around them"""
        hi = len(text) if hi is None else hi
        d = self.alloc(hi - lo + 48, b"\x5a" * (hi - lo + 48))
        if hi > lo:
            self.ctx.device_upload(d + mis, text[lo:hi])
        return d + mis

    def counter(self, value=0):
        return self.alloc(16, struct.pack("<QQ", value, 0))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.device_free(p)


def unpack(raw):
    return [(pat, pos, d) for pos, pat, d in (struct.unpack_from("<QII", raw, 16 * i) for i in range(len(raw) // 16))]


def pack(seeds):
    """records with garbage in the fourth dword: the span pass ignores it"""
    return b"".join(struct.pack("<QII", pos, pat, 0xDEAD0000 + q) for q, (pat, pos) in enumerate(seeds))


class Out:
    """a guarded record buffer with its counter and a count vector, shared by the shard calls of one scan"""

    def __init__(self, ctx, dev, cap, n_patterns):
        self.ctx, self.cap, self.P = ctx, cap, n_patterns
        self.d_out = dev.alloc(16 * (cap + 4), GUARD * (cap + 4))
        self.d_n = dev.counter()
        self.d_counts = dev.alloc(8 * n_patterns, b"\0" * (8 * n_patterns))

    def read(self):
        """(records written sorted, *d_n_found, counts); the guards behind the records are checked"""
        self.ctx.synchronize()
        n_found = struct.unpack("<Q", self.ctx.device_download(self.d_n, 8))[0]
        raw = self.ctx.device_download(self.d_out, 16 * (self.cap + 4))
        have = min(n_found, self.cap)
        assert raw[16 * self.cap:] == GUARD * 4, "records behind capacity were written"
        assert raw[16 * have:16 * self.cap] == GUARD * (self.cap - have), "records beyond *d_n_found were written"
        counts = list(struct.unpack("<%dQ" % self.P, self.ctx.device_download(self.d_counts, 8 * self.P)))
        return sorted(unpack(raw[:16 * have])), n_found, counts


def scan(ctx, text, n_patterns, flags, cap, ob=0, oe=None):
    """one whole-text shard call; (records sorted, n_found, counts)"""
    n = len(text)
    with Dev(ctx) as dev:
        out = Out(ctx, dev, cap, n_patterns)
        ctx.occ_shard_device(dev.text(text), 0, n, n, ob, n if oe is None else oe, flags, out.d_out, cap, out.d_n, out.d_counts)
        return out.read()


def counts_of(recs, n_patterns):
    c = [0] * n_patterns
    for r in recs:
        c[r[0]] += 1
    return c


def setup(ctx, pats, k):
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)


_ref = {}


def ref(key, text, pats, k, flags):
    """the reference records of a case, computed once"""
    if (key, flags) not in _ref:
        _ref[(key, flags)] = R.records(text, pats, k, flags)
    return _ref[(key, flags)]


def check_spans(text, pats, k, got):
    """got: [(pattern, end, dist, start)] -- starts are the reference's, and the span has the distance reported"""
    for i, e, d, s in got:
        ws, wd = R.span(text, pats[i], k, e)
        assert (s, d) == (ws, wd), (i, e)
        assert R.global_dist(pats[i], text[s:e + 1]) == d, (i, e)


# ---------------------------------------------------------------- 1. planted copies with substitutions and indels
_planted = {}


def planted_case(m, k):
    if (m, k) not in _planted:
        _planted[(m, k)] = R.planted(1000 * m + k, [m], k, 8192 if m < 96 else 12288, copies=8)
    return _planted[(m, k)]


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("m", MS)
def test_planted(ctx, m, k):
    """W = 1..4 at the word seams; 16 copies of lengths m - k .. m + k at start residues 0..15 mod 16"""
    if k >= m:
        with pytest.raises(H.pkg().ApmError) as e:
            setup(ctx, [b"A" * m], k)
            ctx.find_occ_buffer(b"ACGT" * 8, ALL)
        assert e.value.status == UNSUPPORTED
        return
    pats, text = planted_case(m, k)
    setup(ctx, pats, k)
    for flags in (ALL, LOCAL_MIN):
        want = ref(("planted", m, k), text, pats, k, flags)
        assert want, "the planted copies must be found"
        got, n_found, counts = scan(ctx, text, 1, flags, len(want) + 8)
        assert got == want, (m, k, flags)
        assert n_found == len(want) and counts == [len(want)]
        # the host-level call: the same ends, sorted, each with its start
        rec, total, cnt = ctx.find_occ_buffer(text, flags, capacity=len(want) + 8)
        assert [r[:3] for r in rec] == want and total == len(want) and cnt == [len(want)]
        check_spans(text, pats, k, rec if flags == LOCAL_MIN else rec[:: max(1, len(rec) // 64)])
    labels = [l for l, _ in ctx.launch_times()]
    assert labels == ["occ", "span"]
    t = ctx.timing()
    assert t["text_bytes"] == len(text) and t["n_launches"] == 2 and t["kernel_ms"] > 0
    S = int(ctx.stat("occ_segment"))
    assert S % 16 == 0 and S >= m + k
    assert ctx.stat("occ_lanes") == -(-len(text) // S)


# ---------------------------------------------------------------- 2. seams between lanes, waves and workgroups
def test_seams(ctx):
    """occurrences that end at q S - 1, q S and q S + 1 and ones that begin just in front of a boundary, q at lane
    boundaries and at the boundaries of a wave = a workgroup's 64 segments; the boundaries move with own_begin"""
    k = 2
    rs = np.random.RandomState(77)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats = [a[rs.randint(0, 4, size=m)].tobytes() for m in (20, 33, 70)]
    setup(ctx, pats, k)
    probe = a[rs.randint(0, 4, size=4096)].tobytes()
    ctx.find_occ_buffer(probe, ALL, capacity=16, spans=False)
    S = int(ctx.stat("occ_segment"))
    assert S >= 72 and S % 16 == 0
    n = 64 * S * 3 + S // 2                                   # more than three workgroups' ends
    assert n <= 400 << 10
    text = bytearray(a[rs.randint(0, 4, size=n)].tobytes())
    for q in (1, 2, 63, 64, 65, 127, 128, 129, 191, 192):    # ends at q S: lane seams, and q = 64, 128, 192: workgroup seams
        p = bytearray(pats[q % 3])
        if q % 2:
            del p[len(p) // 2]                                # a net deletion: length m - 1
        text[q * S + 1 - len(p):q * S + 1] = p
    for q in (3, 66, 130):                                    # begins two bytes in front of a boundary
        p = bytearray(pats[q % 3])
        p.insert(5, ord("A"))                                 # a net insertion: length m + 1
        text[q * S - 2:q * S - 2 + len(p)] = p
    text = bytes(text)
    for flags in (ALL, LOCAL_MIN):
        want = ref("seams", text, pats, k, flags)
        ends = {e for _, e, _ in want}
        assert all(q * S in ends for q in (64, 128, 192))     # (the exact copies at the workgroup seams)
        for ob in (0, 1, 2, S - 1, 64 * S - 1):               # a planted end q S is a segment's first, last, second ... end
            w = [r for r in want if r[1] >= ob]
            got, n_found, counts = scan(ctx, text, 3, flags, len(w) + 8, ob=ob)
            assert got == w, (flags, ob)
            assert n_found == len(w) and counts == counts_of(w, 3)
            assert int(ctx.stat("occ_segment")) == S
        assert -(-n // (64 * S)) >= 3


# ---------------------------------------------------------------- 3. the shard contract
def shard_case():
    return R.planted(4242, [33, 97], 3, 8192, copies=4)


def test_three_shards_one_buffer(ctx):
    """unaligned own ranges, the minimal left halo, text_off > 0, a d_text that is not 16-byte aligned: the whole-text scan"""
    pats, text = shard_case()
    k, n, m_max = 3, len(shard_case()[1]), 97
    setup(ctx, pats, k)
    cuts = [0, 2731, 5555, n]
    for flags in (ALL, LOCAL_MIN):
        want = ref("shards", text, pats, k, flags)
        whole, _, _ = scan(ctx, text, 2, flags, len(want) + 8)
        assert whole == want
        with Dev(ctx) as dev:
            out = Out(ctx, dev, len(want) + 8, 2)
            for s in range(3):
                ob, oe = cuts[s], cuts[s + 1]
                lo, hi = max(0, ob - m_max - k), min(n, oe + 1)
                d_text = dev.text(text, lo, hi, mis=(5, 9, 3)[s])
                assert d_text % 16
                ctx.occ_shard_device(d_text, lo, hi - lo, n, ob, oe, flags, out.d_out, out.cap, out.d_n, out.d_counts)
            got, n_found, counts = out.read()
            assert got == want and n_found == len(want) and counts == counts_of(want, 2)


def test_halo_one_byte_short_is_refused(ctx, apm):
    pats, text = shard_case()
    k, n, m_max = 3, len(text), 97
    setup(ctx, pats, k)
    ob, oe = 2731, 5555
    lo, hi = ob - m_max - k, oe + 1
    with Dev(ctx) as dev:
        out = Out(ctx, dev, 64, 2)
        for tlo, thi in ((lo + 1, hi), (lo, hi - 1)):        # the left halo, then the look-ahead byte
            with pytest.raises(apm.ApmError) as e:
                ctx.occ_shard_device(dev.text(text, tlo, thi), tlo, thi - tlo, n, ob, oe, ALL, out.d_out, out.cap, out.d_n, out.d_counts)
            assert e.value.status == INVALID
        assert out.read() == ([], 0, [0, 0])
        # at the ends of the whole text nothing beyond it is asked for
        ctx.occ_shard_device(dev.text(text, 0, 100), 0, 100, n, 0, 99, ALL, out.d_out, out.cap, out.d_n, out.d_counts)
        ctx.occ_shard_device(dev.text(text, n - 300, n), n - 300, 300, n, n - 200, n + 50, ALL, out.d_out, out.cap, out.d_n, out.d_counts)
        got, _, _ = out.read()
        assert got == [r for r in ref("shards", text, pats, k, ALL) if r[1] < 99 or r[1] >= n - 200]


@pytest.mark.parametrize("n", [1, 2, 5, 19, 20])
def test_texts_shorter_than_the_pattern(ctx, n):
    pats, k = [b"ACGTACGTACGTACGTACGA", b"AC"], 1
    setup(ctx, pats, k)
    text = (b"ACGTACGTACGTACGTACGA" * 2)[1:1 + n]
    for flags in (ALL, LOCAL_MIN):
        want = R.records(text, pats, k, flags)
        got, n_found, counts = scan(ctx, text, 2, flags, 64)
        assert got == want and n_found == len(want) and counts == counts_of(want, 2)
        rec, total, _ = ctx.find_occ_buffer(text, flags, capacity=64)
        assert [r[:3] for r in rec] == want and total == len(want)
        check_spans(text, pats, k, rec)


def test_capacity_below_the_matches(ctx):
    pats, text = shard_case()
    setup(ctx, pats, 3)
    want = ref("shards", text, pats, 3, ALL)
    cap = len(want) // 3
    assert cap >= 4
    got, n_found, counts = scan(ctx, text, 2, ALL, cap)       # (read() compares the guard words)
    assert n_found == len(want) and counts == counts_of(want, 2)
    assert len(got) == cap and set(got) <= set(want)
    rec, total, cnt = ctx.find_occ_buffer(text, ALL, capacity=cap)
    assert total == len(want) and cnt == counts_of(want, 2) and len(rec) == cap
    assert {r[:3] for r in rec} <= set(want)
    total_only = ctx.find_occ_buffer(text, ALL, capacity=0)
    assert total_only[0] == [] and total_only[1] == len(want)


# ---------------------------------------------------------------- 4. closed form, prose, other bytes
def test_closed_form(ctx):
    n = 4096
    text, pats, k = b"A" * n, [b"A" * 20], 3
    setup(ctx, pats, k)
    got, n_found, counts = scan(ctx, text, 1, ALL, n)
    assert n_found == n - 16 == len(got) and counts == [n - 16]
    assert got == [(0, e, max(0, 19 - e)) for e in range(16, n)]
    rec, total, cnt = ctx.find_occ_buffer(text, LOCAL_MIN)
    assert rec == [(0, 19, 0, 0)] and total == 1 and cnt == [1]


PROSE = (b"It was the best of times, it was the worst of times, it was the age of wisdom,\nit was the age of foolishness, "
         b"it was the epoch of belief, it was the epoch of incredulity,\r\nit was the season of Light, it was the season of Darkness ")


def test_prose_and_bytes_outside_dna(ctx):
    """bytes that share their 2-bit codes, 0x00, 0xFF and line breaks: the Eq tables are indexed by the full byte"""
    rs = np.random.RandomState(5)
    blob = bytes(rs.randint(0, 256, size=2048, dtype=np.int64).astype(np.uint8))
    text = PROSE * 6 + blob + b"\x00\xff\n\x00\xff\n" * 40 + PROSE.upper() * 2 + b"xx aAaAqQqQaAzA " + b"AaAaQqQq" * 50
    pats = [b"the age of wisdom", b"it was the epoch of beleif", b"\x00\xff\n\x00\xff\n\x00\xfe", b"aAaAqQqQaAaA", blob[100:171]]
    k = 2
    setup(ctx, pats, k)
    for flags in (ALL, LOCAL_MIN):
        want = ref("prose", text, pats, k, flags)
        assert {i for i, _, _ in want} == set(range(5))
        got, n_found, counts = scan(ctx, text, 5, flags, len(want) + 8)
        assert got == want and n_found == len(want) and counts == counts_of(want, 5)
    rec, _, _ = ctx.find_occ_buffer(text, LOCAL_MIN)
    assert [r[:3] for r in rec] == ref("prose", text, pats, k, LOCAL_MIN)
    check_spans(text, pats, k, rec)


def test_window_matches_are_occurrences(ctx):
    """every record (i, j, d) of apm_find_all_dist_buffer with j + m <= n has an ALL record (i, j + m - 1) with distance <= d"""
    pats, text = shard_case()
    k, n = 3, len(text)
    setup(ctx, pats, k)
    windows, total = ctx.find_all_dist_buffer(text)
    assert total == len(windows) and windows
    occ, _, _ = ctx.find_occ_buffer(text, ALL, spans=False)
    dist = {(i, e): d for i, e, d in occ}
    full = [(i, j, d) for i, j, d in windows if j + len(pats[i]) <= n]
    assert full
    for i, j, d in full:
        assert dist.get((i, j + len(pats[i]) - 1), k + 1) <= d, (i, j, d)


# ---------------------------------------------------------------- 5. the span pass on made-up records
def test_spans_triage_made_up_records(ctx):
    pats, text = shard_case()
    k, n = 3, len(text)
    setup(ctx, pats, k)
    real = ref("shards", text, pats, k, LOCAL_MIN)
    covered_lo, covered_hi = 1000, 6000                       # the shard text handed to the pass
    inside = [(i, e) for i, e, _ in real if e - len(pats[i]) - k + 1 >= covered_lo and e < covered_hi]
    outside = [(i, e) for i, e, _ in real if e < covered_lo or e >= covered_hi]
    straddle = [(0, covered_lo + 10), (1, covered_lo)]        # the end is inside, the columns in front of it are not
    none = [(0, 3001), (1, 4003)]
    assert inside and outside and all(R.span(text, pats[i], k, e)[0] is None for i, e in none)
    seeds = inside + [(2, 50), (7, 3000)] + outside + [(0, n), (1, n + 99), (0, 1 << 40)] + none + straddle
    preset = b"".join(struct.pack("<QII", 0x1111111111111111, 0x22222222, 0x33333333 + q) for q in range(len(seeds) + 2))
    with Dev(ctx) as dev:
        d_text = dev.text(text, covered_lo, covered_hi, mis=7)
        d_rec, d_n = dev.alloc(16 * len(seeds), pack(seeds)), dev.counter(len(seeds) + 5)   # (*d_n_rec may exceed capacity)
        d_span = dev.alloc(len(preset), preset)
        ctx.occ_spans_device(d_text, covered_lo, covered_hi - covered_lo, n, d_rec, len(seeds), d_n, d_span)
        ctx.synchronize()
        raw = ctx.device_download(d_span, len(preset))
        assert ctx.device_download(d_rec, 16 * len(seeds)) == pack(seeds)                    # the records are only read
        assert [l for l, _ in ctx.launch_times()] == ["span"]
    assert raw[16 * len(seeds):] == preset[16 * len(seeds):], "entries at or beyond capacity were written"
    for q, (i, e) in enumerate(seeds):
        pos, pat, d = struct.unpack_from("<QII", raw, 16 * q)
        if i >= 2 or e >= n:
            assert (pos, pat, d) == (NO_START, i, DIST_INVALID), (i, e)
        elif (i, e) in outside or (i, e) in straddle:
            assert raw[16 * q:16 * q + 16] == preset[16 * q:16 * q + 16], (i, e)
        elif (i, e) in none:
            assert (pos, pat, d) == (NO_START, i, k + 1), (i, e)
        else:
            ws, wd = R.span(text, pats[i], k, e)
            assert (pos, pat, d) == (ws, i, wd), (i, e)


# ---------------------------------------------------------------- 6. a text mode
def test_fasta_upper_reports_source_offsets(ctx, apm):
    rs = np.random.RandomState(31)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    seq = [a[rs.randint(0, 4, size=s)].tobytes() for s in (700, 900)]
    pats = [seq[0][290:330], seq[1][100:133]]
    occ = bytearray(pats[0])
    del occ[7]                                                 # one more copy, a byte short, in the second sequence
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
            rec, total, cnt = ctx.find_occ_buffer(src, flags)
            assert rec == [(i, keep[e], d, keep[s]) for i, e, d, s in want], flags
            assert total == len(want) and cnt == counts_of(want, 2)
        assert (0, keep[329], 0, keep[290]) in rec and any(r[0] == 0 and r[2] == 1 for r in rec)
        assert [l for l, _ in ctx.launch_times()] == ["occ", "span"]
    finally:
        ctx.set_text_mode(0)


# ---------------------------------------------------------------- 7. errors, and what the call leaves alone
def test_errors(ctx, apm):
    text = b"ACGT" * 64
    with Dev(ctx) as dev:
        out = Out(ctx, dev, 16, 2)
        d_text = dev.text(text)

        def refused(status, flags=ALL):
            with pytest.raises(apm.ApmError) as e:
                ctx.occ_shard_device(d_text, 0, len(text), len(text), 0, len(text), flags, out.d_out, out.cap, out.d_n, out.d_counts)
            assert e.value.status == status
            with pytest.raises(apm.ApmError) as e:
                ctx.find_occ_buffer(text, flags)
            assert e.value.status == status
            if status == UNSUPPORTED:                          # (the span pass has no flags)
                with pytest.raises(apm.ApmError) as e:
                    ctx.occ_spans_device(d_text, 0, len(text), len(text), out.d_out, out.cap, out.d_n, out.d_out)
                assert e.value.status == status

        setup(ctx, [b"ACGT" * 32 + b"A", b"ACGTAC"], 2)        # m = 129
        refused(UNSUPPORTED)
        setup(ctx, [b"ACGTACGT", b"ACG"], 3)                   # k >= m
        refused(UNSUPPORTED)
        setup(ctx, [b"ACGTACGT", b"ACGA"], 1)
        refused(INVALID, flags=2)
        refused(INVALID, flags=0x80000001)
        assert out.read() == ([], 0, [0, 0])                   # nothing was written


def test_multi_device_context_is_refused(apm):
    if apm.device_count() < 2:
        pytest.skip("one device visible")
    with apm.ApmContext(n_devices=2) as c:
        c.set_patterns([b"ACGTACGT"], 1)
        with pytest.raises(apm.ApmError) as e:
            c.find_occ_buffer(b"ACGT" * 64, ALL)
        assert e.value.status == UNSUPPORTED


def test_counting_calls_are_untouched(ctx):
    pats, text = shard_case()
    setup(ctx, pats, 3)
    before = (ctx.count_buffer(text), [ctx.pattern_kernel(i) for i in range(2)])
    ctx.find_occ_buffer(text, LOCAL_MIN)
    ctx.find_occ_buffer(text, ALL, spans=False)
    assert (ctx.count_buffer(text), [ctx.pattern_kernel(i) for i in range(2)]) == before
    assert before[0] == H.oracle_counts(text, pats, 3)


# ---------------------------------------------------------------- 8. the command-line host
def run_cli(args):
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    return subprocess.run([exe] + args, capture_output=True, text=True)


def render(text, pats, k, flags):
    recs = R.records_with_starts(text, pats, k, flags)
    lines = ["Number of matches for pattern <%s>: %d" % (p.decode(), sum(r[0] == i for r in recs)) for i, p in enumerate(pats)]
    for i, p in enumerate(pats):
        lines.append("Occurrences for pattern <%s>:" % p.decode() + "".join(" %d-%d:%d" % (s, e, d) for j, e, d, s in recs if j == i))
    return lines


def test_cli_occurrences(tmp_path):
    pats, text = R.planted(99, [24, 40], 2, 3000, copies=2)
    path = tmp_path / "text.txt"
    path.write_bytes(text)
    base = ["2", str(path)] + [p.decode() for p in pats]
    for flag, flags in (("--occurrences", LOCAL_MIN), ("--occurrences=best", LOCAL_MIN), ("--occurrences=all", ALL)):
        r = run_cli(base + [flag])
        assert r.returncode == 0, r.stderr
        lines = [l for l in r.stdout.splitlines() if l.startswith(("Number of matches", "Occurrences for"))]
        assert lines == render(text, pats, 2, flags), flag
    for other in ("--positions", "--distances", "--alignments", "--best", "--best=2"):
        r = run_cli(base + ["--occurrences", other])
        assert r.returncode == 1 and "--occurrences" in r.stderr, other
    assert run_cli(base + ["--occurrences=worst"]).returncode == 1


def test_cli_occurrences_fasta_sequences(tmp_path):
    seq = R.planted(98, [30], 2, 600, copies=1)
    pats, body = seq
    src = b">chr1 test\n" + b"\n".join(body[i:i + 50] for i in range(0, 300, 50)).lower() + b"\n>chr2\n" + \
          b"\n".join(body[i:i + 50] for i in range(300, 600, 50)) + b"\n"
    path = tmp_path / "text.fa"
    path.write_bytes(src)
    T = body
    recs = R.records_with_starts(T, pats, 2, LOCAL_MIN)
    assert recs
    r = run_cli(["2", str(path), pats[0].decode(), "--fasta", "--upper", "--sequences", "--occurrences"])
    assert r.returncode == 0, r.stderr
    want = []
    for _, e, d, s in recs:
        if (s < 300) == (e < 300):                             # inside one sequence
            want.append("%s:%d-%d:%d" % ("chr1" if s < 300 else "chr2", s % 300, e - s + 1, d))
    line = [l for l in r.stdout.splitlines() if l.startswith("Occurrences for")]
    assert line == ["Occurrences for pattern <%s>:" % pats[0].decode() + "".join(" " + w for w in want)]
    assert "Number of matches for pattern <%s>: %d" % (pats[0].decode(), len(recs)) in r.stdout
