"""The occurrence search per sequence on the GPU: apm_occ_seq_shard_device, apm_occ_seq_spans_device and
apm_find_occ_seq_buffer give exactly the records include/apm.h pins ("occurrence search per sequence").  The truth everywhere
is tests/seqocc_ref.py -- occ_ref on every sequence as a text of its own; every comparison is exact and of the COMPLETE
result.  Device buffers carry preset guard words in front of and behind the records, the spans and the sequence array, and
the tests compare those.  Texts are 4 .. 24 KiB, so the segment S shrinks to about m_max + k: lane seams every S bytes,
workgroup seams at 64 and 128 segments."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import occ_ref as R
import seqocc_ref as SR
from test_occ_align_gpu import script as pinned_script

pytestmark = pytest.mark.gpu

INVALID, STATE, UNSUPPORTED = -1, -8, -6
ALL, LOCAL_MIN = SR.ALL, SR.LOCAL_MIN
GUARD = b"\xa5" * 16
NO_START = SR.NO_START
DIST_INVALID = 0xFFFFFFFF
SEQ_INVALID = 0xFFFFFFFF
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


def setup(ctx, pats, k):
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)


def dna(rs, n, alphabet=DNA):
    return alphabet[rs.randint(0, len(alphabet), size=n)].tobytes()


def counts_of(recs, n_patterns):
    c = [0] * n_patterns
    for r in recs:
        c[r[0]] += 1
    return c


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

    def table(self, begins):
        """the apm_seq entries of t_begin[0 .. n_seq]; hdr_off holds a value nothing may depend on"""
        flat = []
        for s, b in enumerate(begins):
            flat += [0xDEAD000000000000 + s, b]
        return self.alloc(16 * len(begins), struct.pack("<%dQ" % len(flat), *flat))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx.device_free(p)


class Out:
    """the guarded buffers of one scan and its span pass: `cap` end records with their counter and count vector, `cap` span
    records and `cap` sequence words, each between two guards of 32 bytes"""

    def __init__(self, ctx, dev, cap, n_patterns, n_found=0):
        self.ctx, self.cap, self.P = ctx, cap, n_patterns
        self.b_out = dev.alloc(64 + 16 * cap, GUARD * (cap + 4))
        self.b_span = dev.alloc(64 + 16 * cap, GUARD * (cap + 4))
        self.b_seq = dev.alloc(64 + 4 * cap, GUARD * 4 + b"\xa5" * (4 * cap))
        self.d_out, self.d_span, self.d_seq = self.b_out + 32, self.b_span + 32, self.b_seq + 32
        self.d_n = dev.alloc(16, struct.pack("<QQ", n_found, 0))
        self.d_counts = dev.alloc(8 * n_patterns, b"\0" * (8 * n_patterns))

    def put(self, recs):
        """made-up records (pattern, end) with garbage in the fourth dword: the span pass ignores it"""
        raw = b"".join(struct.pack("<QII", pos, pat, 0xDEAD0000 + q) for q, (pat, pos) in enumerate(recs))
        self.ctx.device_upload(self.d_out, raw)
        return raw

    def _body(self, base, width):
        self.ctx.synchronize()
        raw = self.ctx.device_download(base, 64 + width * self.cap)
        assert raw[:32] == GUARD * 2 and raw[-32:] == GUARD * 2, "the guards around a device buffer were written"
        return raw[32:-32]

    def n_found(self):
        self.ctx.synchronize()
        return struct.unpack("<Q", self.ctx.device_download(self.d_n, 8))[0]

    def raw_records(self, base):
        """[(pattern, pos, dist)] in buffer order, None for an entry that still holds its guard"""
        body = self._body(base, 16)
        out = []
        for i in range(self.cap):
            pos, pat, d = struct.unpack_from("<QII", body, 16 * i)
            out.append(None if body[16 * i:16 * i + 16] == GUARD else (pat, pos, d))
        return out

    def seqs(self):
        """the sequence words in buffer order, None for a word that still holds its guard"""
        body = self._body(self.b_seq, 4)
        return [None if body[4 * i:4 * i + 4] == b"\xa5" * 4 else struct.unpack_from("<I", body, 4 * i)[0] for i in range(self.cap)]

    def read(self):
        """(records written sorted, *d_n_found, counts); nothing beyond min(*d_n_found, cap) is written"""
        n_found = self.n_found()
        recs = self.raw_records(self.b_out)
        have = min(n_found, self.cap)
        assert all(r is not None for r in recs[:have]) and all(r is None for r in recs[have:]), "records beyond *d_n_found were written"
        counts = list(struct.unpack("<%dQ" % self.P, self.ctx.device_download(self.d_counts, 8 * self.P)))
        return sorted(recs[:have]), n_found, counts

    def rows(self):
        """[(pattern, end, dist, start, seq)] sorted, of the records, spans and sequence words written"""
        n_found = self.n_found()
        have = min(n_found, self.cap)
        recs, spans, seqs = self.raw_records(self.b_out), self.raw_records(self.b_span), self.seqs()
        assert all(x is None for x in spans[have:]) and all(x is None for x in seqs[have:]), "entries beyond the records were written"
        rows = []
        for r, sp, sq in zip(recs[:have], spans[:have], seqs[:have]):
            assert sp is not None and sq is not None and sp[0] == r[0] and sp[2] == r[2], (r, sp, sq)
            rows.append(r + (None if sp[1] == NO_START else sp[1], sq))
        return sorted(rows)


def scan(ctx, text, n_patterns, begins, flags, cap, ob=0, oe=None, mis=0):
    """one whole-text shard call under the table; (records sorted, n_found, counts)"""
    n = len(text)
    with Dev(ctx) as dev:
        out = Out(ctx, dev, cap, n_patterns)
        ctx.occ_seq_shard_device(dev.text(text, mis=mis), 0, n, n, ob, n if oe is None else oe, dev.table(begins), len(begins) - 1, flags,
                                 out.d_out, cap, out.d_n, out.d_counts)
        return out.read()


def scan_with_spans(ctx, text, n_patterns, begins, flags, cap):
    """the scan and the span pass behind it; [(pattern, end, dist, start, seq)] sorted"""
    n = len(text)
    with Dev(ctx) as dev:
        out = Out(ctx, dev, cap, n_patterns)
        d_text, d_table = dev.text(text), dev.table(begins)
        ctx.occ_seq_shard_device(d_text, 0, n, n, 0, n, d_table, len(begins) - 1, flags, out.d_out, cap, out.d_n, out.d_counts)
        ctx.occ_seq_spans_device(d_text, 0, n, n, d_table, len(begins) - 1, out.d_out, cap, out.d_n, out.d_span, out.d_seq)
        return out.rows()


def with_spans(text, pats, k, recs, begins):
    return [(i, e, d) + SR.span(text, pats[i], k, e, begins)[::2] for i, e, d in recs]


def check_whole(ctx, text, pats, k, begins, spans=True, mis=(0,)):
    """the whole text through the device calls under both flags; -> the reference {flags: records}"""
    want = SR.records_both(text, pats, k, begins)
    P = len(pats)
    for flags in (ALL, LOCAL_MIN):
        w = want[flags]
        for a in mis:
            got, n_found, counts = scan(ctx, text, P, begins, flags, len(w) + 8, mis=a)
            assert got == w, (flags, a, begins[:8])
            assert n_found == len(w) and counts == counts_of(w, P)
    if spans:
        w = want[LOCAL_MIN]
        rows = scan_with_spans(ctx, text, P, begins, LOCAL_MIN, len(w) + 8)
        assert rows == with_spans(text, pats, k, w, begins)
        for i, e, d, start, s in rows:
            assert begins[s] <= start <= e < begins[s + 1], "a span leaves its sequence"
    return want


def segment_of(ctx, n, n_patterns):
    """S of a launch over n ends with the current pattern set"""
    with Dev(ctx) as dev:
        out = Out(ctx, dev, 4, n_patterns)
        ctx.occ_seq_shard_device(dev.text(b"\x00" * n), 0, n, n, 0, n, dev.table([0, n]), 1, ALL, out.d_out, 4, out.d_n, out.d_counts)
        ctx.synchronize()
    return int(ctx.stat("seqocc_segment"))


def near_copies(rs, n, p, step):
    """random DNA with a near copy of p every `step` bytes: what a walk wrongly keeps from the far side of a boundary shows"""
    t = bytearray(dna(rs, n))
    m = len(p)
    for at in range(5, n - m, step):
        t[at:at + m] = p
        if m > 4:
            t[at + at % m] = ord("N")
    return bytes(t)


# ---------------------------------------------------------------- 1. one sequence: the whole-text calls
def test_one_sequence_equals_the_whole_text_calls(ctx):
    pats, text = R.planted(51, [9, 33, 70, 128], 3, 9000, copies=2)
    k, n, P = 3, len(text), 4
    setup(ctx, pats, k)
    for flags in (ALL, LOCAL_MIN):
        want = R.records(text, pats, k, flags)
        assert want
        cap = len(want) + 8
        with Dev(ctx) as dev:
            d_text = dev.text(text, mis=5)
            whole, per = Out(ctx, dev, cap, P), Out(ctx, dev, cap, P)
            ctx.occ_shard_device(d_text, 0, n, n, 0, n, flags, whole.d_out, cap, whole.d_n, whole.d_counts)
            ctx.occ_spans_device(d_text, 0, n, n, whole.d_out, cap, whole.d_n, whole.d_span)
            d_table = dev.table([0, n])
            ctx.occ_seq_shard_device(d_text, 0, n, n, 0, n, d_table, 1, flags, per.d_out, cap, per.d_n, per.d_counts)
            assert [l for l, _ in ctx.launch_times()] == ["socc"]
            ctx.occ_seq_spans_device(d_text, 0, n, n, d_table, 1, per.d_out, cap, per.d_n, per.d_span, per.d_seq)
            assert [l for l, _ in ctx.launch_times()] == ["sspan"]
            assert per.read() == whole.read() == (want, len(want), counts_of(want, P))
            rows = per.rows()
            spans = sorted(r + (None if sp[1] == NO_START else sp[1],)
                           for r, sp in zip(whole.raw_records(whole.b_out)[:len(want)], whole.raw_records(whole.b_span)[:len(want)]))
            assert [r[:4] for r in rows] == spans and all(r[4] == 0 for r in rows)
            assert spans == R.records_with_starts(text, pats, k, flags) if flags == LOCAL_MIN else len(spans) == len(want)
    assert int(ctx.stat("seqocc_segment")) == int(ctx.stat("occ_segment"))
    assert int(ctx.stat("seqocc_lanes")) == int(ctx.stat("occ_lanes"))


# ---------------------------------------------------------------- 2. one boundary against lane and workgroup seams
@pytest.mark.parametrize("q", (1, 63, 64, 65, 128))
def test_boundary_against_seams(ctx, q):
    rs = np.random.RandomState(200 + q)
    m, k, n = 20, 2, 6400
    p = dna(rs, m)
    setup(ctx, [p], k)
    S = segment_of(ctx, n, 1)
    assert S % 16 == 0 and m + k <= S and 129 * S + 2 * S < n, S
    text = near_copies(rs, n, p, m + 7)
    # the boundary at the seam, beside it, and inside the warm-up of the lane that begins at the seam
    for delta in (-(m + k) - 1, -(m + k), -(m + k) + 1, -m, -1, 0, 1):
        want = check_whole(ctx, text, [p], k, [0, q * S + delta, n], spans=delta == 0)
        assert want[ALL] and int(ctx.stat("seqocc_segment")) == S
    check_whole(ctx, text, [p], k, [0, q * S, q * S, q * S, q * S + 1, n])      # empties and a 1-byte sequence at the seam


# ---------------------------------------------------------------- 3. random tables, every width
def test_random_boundaries_every_width(ctx):
    n, k = 12 * 1024, 3
    lens = [4, 31, 32, 33, 64, 65, 96, 97, 127, 128]
    pats, text = R.planted(71, lens, k, n, copies=2)
    rs = np.random.RandomState(1071)
    cuts = [int(c) for c in rs.randint(0, n + 1, size=34)]
    cuts += cuts[:3] + [0, n, n]                                 # empties: inside, at the first byte, behind the last
    begins = SR.begins_of(cuts, n)
    assert len(begins) - 1 == 41 and sum(a == b for a, b in zip(begins, begins[1:])) >= 6
    setup(ctx, pats, k)
    want = check_whole(ctx, text, pats, k, begins, mis=(0, 7))
    S = int(ctx.stat("seqocc_segment"))
    assert S % 16 == 0 and 128 + k <= S and n // S >= 65, "the launch has a workgroup seam at 64 segments"
    assert int(ctx.stat("seqocc_lanes")) == -(-n // S) * len(pats)
    assert all(c > 0 for c in counts_of(want[LOCAL_MIN], len(pats)))
    # a boundary cuts at least one whole-text occurrence away
    assert want[ALL] != R.records(text, pats, k, ALL)


# ---------------------------------------------------------------- 4. the masked case, one per column width
@pytest.mark.parametrize("m", (7, 40, 70, 100))
def test_a_crossing_copy_hides_the_hit_inside_the_sequence(ctx, m):
    """the GATTACA shape: an exact copy of p with its first two bytes in front of the boundary.  The whole-text search
    reports it at distance 0; per sequence the end is the real hit at distance 2, the copy's last m - 2 bytes"""
    rs = np.random.RandomState(300 + m)
    k, n = 2, 4096
    p = dna(rs, m, np.frombuffer(b"AGT", dtype=np.uint8))        # no C: the filler shares no byte with it
    setup(ctx, [p], k)
    S = segment_of(ctx, n, 1)
    # the boundary at a lane seam, one byte off it, and in the middle of a lane
    for c in (5 * S, 64 * S + 1 if 64 * S + m < n else 9 * S + 1, 7 * S + S // 2):
        t = bytearray(b"C" * n)
        t[c - 2:c - 2 + m] = p
        text, end = bytes(t), c + m - 3
        begins = [0, 10, c, n]
        want = check_whole(ctx, text, [p], k, begins)
        assert want[LOCAL_MIN] == [(0, end, 2)] and want[ALL] == [(0, end, 2)]
        assert scan_with_spans(ctx, text, 1, begins, LOCAL_MIN, 8) == [(0, end, 2, c, 2)]
        assert R.records_with_starts(text, [p], k, LOCAL_MIN) == [(0, end, 0, c - 2)]
        with Dev(ctx) as dev:                                    # the whole-text call reports the crossing copy
            out = Out(ctx, dev, 16, 1)
            ctx.occ_shard_device(dev.text(text), 0, n, n, 0, n, LOCAL_MIN, out.d_out, 16, out.d_n, out.d_counts)
            assert out.read()[0] == [(0, end, 0)]
        # one edit fewer and nothing is left of it
        setup(ctx, [p], 1)
        assert scan(ctx, text, 1, begins, ALL, 8) == ([], 0, [0])
        setup(ctx, [p], k)


# ---------------------------------------------------------------- 5. tiny sequences
def test_many_tiny_sequences(ctx):
    rs = np.random.RandomState(41)
    lens = rs.randint(0, 7, size=1500)
    begins = [0] + [int(x) for x in np.cumsum(lens)]
    n = begins[-1]
    assert n >= 4096
    two = np.frombuffer(b"AC", dtype=np.uint8)
    text = dna(rs, n, two)
    pats = [dna(rs, m, two) for m in (2, 3, 4, 5, 6, 8)]
    setup(ctx, pats, 1)
    want = check_whole(ctx, text, pats, 1, begins)
    S = int(ctx.stat("seqocc_segment"))
    assert S // 6 >= 2 and (lens == 0).sum() > 150 and (lens == 1).sum() > 150, "a lane crosses boundaries, runs of empty sequences among them"
    got = counts_of(want[ALL], len(pats))
    assert got[0] > 0 and got[4] > 0 and got[5] == 0, "m = 8 at k = 1 fits no sequence: every one is shorter than m - k"


# ---------------------------------------------------------------- 6. LOCAL_MIN at a sequence's first and last byte
def test_local_min_at_the_first_and_the_last_byte_of_a_sequence(ctx):
    p = b"ACGTTGCATG"
    k, n = 2, 4096
    setup(ctx, [p, b"G"], 0)
    t = bytearray(b"C" * n)
    t[1000:1010] = p                                             # sequence 1 ends with p, and p goes on behind the boundary
    t[1010:1020] = p
    t[2000] = ord("G")                                           # sequence 3 begins with G; sequence 4 is that one byte again
    t[2001] = ord("G")
    text = bytes(t)
    begins = [0, 500, 1010, 2000, 2001, 2002, n]
    setup(ctx, [p, b"G"], 0)
    want = check_whole(ctx, text, [p, b"G"], 0, begins)
    assert (0, 1009, 0) in want[LOCAL_MIN] and (0, 1019, 0) in want[LOCAL_MIN]
    assert (1, 2000, 0) in want[LOCAL_MIN] and (1, 2001, 0) in want[LOCAL_MIN], "E_s = m in front of a sequence's first byte"
    assert R.records(text, [b"G"], 0, LOCAL_MIN).count((0, 2001, 0)) == 0, "the whole text's plateau keeps its first end only"
    # a falling score at the last byte: E_s(e + 1) >= E_s(e) is true by definition there
    setup(ctx, [p], k)
    begins = [0, 1008, n]                                        # sequence 0 ends two bytes short of the copy's end
    want = check_whole(ctx, text, [p], k, begins)
    assert (0, 1007, 2) in want[LOCAL_MIN] and (0, 1007, 2) in want[ALL]
    assert (0, 1007, 2) not in R.records(text, [p], k, LOCAL_MIN)


# ---------------------------------------------------------------- 7. capacity
def shard_case():
    pats, text = R.planted(41, [9, 33, 70], 3, 9000, copies=2)
    begins = [0, 450, 450, 2500, 5200, 5203, 8000, len(text)]
    return pats, text, begins


_shard_ref = {}


def shard_ref():
    if not _shard_ref:
        pats, text, begins = shard_case()
        _shard_ref.update(SR.records_both(text, pats, 3, begins))
    return _shard_ref


def test_capacity_below_the_records(ctx):
    pats, text, begins = shard_case()
    setup(ctx, pats, 3)
    want = shard_ref()[ALL]
    cap = len(want) // 3
    assert cap >= 4
    got, n_found, counts = scan(ctx, text, 3, begins, ALL, cap)  # (read() compares the guard words)
    assert n_found == len(want) and counts == counts_of(want, 3)
    assert len(got) == cap and set(got) <= set(want)
    rows = scan_with_spans(ctx, text, 3, begins, ALL, cap)
    assert len(rows) == cap and {r[:3] for r in rows} <= set(want)
    assert scan(ctx, text, 3, begins, ALL, 0) == ([], len(want), counts_of(want, 3))


# ---------------------------------------------------------------- 8. shards
@pytest.mark.parametrize("cuts", ([(0, 4001), (4001, 9000)], [(0, 2500), (2500, 5201), (5201, 9000)]))
def test_shards_with_left_halos_append_to_one_buffer(ctx, cuts):
    pats, text, begins = shard_case()
    k, n, halo, n_seq = 3, len(text), 70 + 3, len(begins) - 1
    setup(ctx, pats, k)
    for flags in (ALL, LOCAL_MIN):
        want = shard_ref()[flags]
        with Dev(ctx) as dev:
            out = Out(ctx, dev, len(want) + 8, 3)
            d_table = dev.table(begins)
            for j, (ob, oe) in enumerate(cuts):
                lo, hi = max(0, ob - halo), min(n, oe + 1)       # exactly the bytes the call asks for
                ctx.occ_seq_shard_device(dev.text(text, lo, hi, mis=(5, 9, 3)[j]), lo, hi - lo, n, ob, oe, d_table, n_seq, flags,
                                         out.d_out, out.cap, out.d_n, out.d_counts)
            assert out.read() == (want, len(want), counts_of(want, 3))
            # the span pass over one shard's text: what it covers is written, the rest keeps its guard
            lo, hi = cuts[1][0] - halo, n
            ctx.occ_seq_spans_device(dev.text(text, lo, hi), lo, hi - lo, n, d_table, n_seq, out.d_out, out.cap, out.d_n, out.d_span, out.d_seq)
            recs, spans, seqs = out.raw_records(out.b_out), out.raw_records(out.b_span), out.seqs()
            for r, sp, sq in zip(recs[:len(want)], spans, seqs):
                start, d, s = SR.span(text, pats[r[0]], k, r[1], begins)
                if max(r[1] + 1 - (len(pats[r[0]]) + k), begins[s]) >= lo:
                    assert (sp, sq) == ((r[0], start, d), s), r
                else:
                    assert sp is None and sq is None, r
    with Dev(ctx) as dev:                                        # the halo one byte short, then the look-ahead byte missing
        out = Out(ctx, dev, 16, 3)
        ob, oe = cuts[1][0], cuts[1][0] + 1000
        for lo, hi in ((ob - halo + 1, oe + 1), (ob - halo, oe)):
            with pytest.raises(H.pkg().ApmError) as e:
                ctx.occ_seq_shard_device(dev.text(text, lo, hi), lo, hi - lo, n, ob, oe, dev.table(begins), n_seq, ALL, out.d_out, 16, out.d_n, out.d_counts)
            assert e.value.status == INVALID
        assert out.read() == ([], 0, [0, 0, 0])


# ---------------------------------------------------------------- 9. the span pass on records the test supplies
def test_sspan_triages_the_records_it_is_given(ctx):
    pats, text, begins = shard_case()
    k, n, n_seq = 3, len(text), len(begins) - 1
    setup(ctx, pats, k)
    real = shard_ref()[LOCAL_MIN]
    lo, hi = 1000, 6000                                          # the shard text handed to the pass
    cols_lo = lambda i, e: max(e + 1 - (len(pats[i]) + k), begins[SR.seq_of(begins, e)])
    inside = [(i, e) for i, e, _ in real if cols_lo(i, e) >= lo and e < hi]
    outside = [(i, e) for i, e, _ in real if e < lo or e >= hi]
    straddle = [(0, lo + 5), (1, lo)]                            # the end is inside, the columns in front of it are not
    clamped = [(2, 2500 + 10), (1, 5200), (0, 5202)]             # the sequence begins inside the shard text, right in front of the end
    none = [(0, 3001), (1, 4003)]
    assert inside and outside and all(SR.span(text, pats[i], k, e, begins)[0] is None for i, e in none + clamped)
    seeds = inside + [(3, 50), (7, 3000)] + outside + [(0, n), (1, n + 99), (0, 1 << 40)] + none + straddle + clamped
    for with_seq in (True, False):
        with Dev(ctx) as dev:
            out = Out(ctx, dev, len(seeds), 3, n_found=len(seeds) + 5)   # (*d_n_rec may exceed capacity)
            raw = out.put(seeds)
            ctx.occ_seq_spans_device(dev.text(text, lo, hi, mis=7), lo, hi - lo, n, dev.table(begins), n_seq, out.d_out, len(seeds), out.d_n,
                                     out.d_span, out.d_seq if with_seq else None)
            ctx.synchronize()
            assert ctx.device_download(out.d_out, len(raw)) == raw   # the records are only read
            assert [l for l, _ in ctx.launch_times()] == ["sspan"]
            spans, seqs = out.raw_records(out.b_span), out.seqs()
        if not with_seq:
            assert seqs == [None] * len(seeds)
        for q, (i, e) in enumerate(seeds):
            if i >= 3 or e >= n:
                want = ((i, NO_START, DIST_INVALID), SEQ_INVALID)
            elif (i, e) in outside or (i, e) in straddle:
                want = (None, None)
            else:
                start, d, s = SR.span(text, pats[i], k, e, begins)
                want = ((i, NO_START if start is None else start, d), s)
                assert (d == k + 1) == ((i, e) in none + clamped)
            assert (spans[q], seqs[q]) == (want if with_seq else (want[0], None)), (i, e)


# ---------------------------------------------------------------- 10. against the per-sequence nearest search
def test_nearest_per_sequence_is_the_smallest_record_of_each_sequence(ctx):
    pats, text, begins = shard_case()
    k, n, n_seq, P = 3, len(text), len(begins) - 1, 3
    setup(ctx, pats, k)
    with Dev(ctx) as dev:
        d_text, d_table = dev.text(text), dev.table(begins)
        d_keys = dev.alloc(8 * n_seq * P, b"\xff" * (8 * n_seq * P))
        ctx.nearest_seq_shard_device(d_text, 0, n, n, 0, n, d_table, n_seq, d_keys)
        ctx.synchronize()
        keys = struct.unpack("<%dQ" % (n_seq * P), ctx.device_download(d_keys, 8 * n_seq * P))
    recs, n_found, _ = scan(ctx, text, P, begins, ALL, len(shard_ref()[ALL]) + 8)
    assert n_found == len(recs)
    best = {}
    for i, e, d in recs:                                         # sorted by (pattern, end): the first end of the smallest distance
        s = SR.seq_of(begins, e)
        if (s, i) not in best or d < best[(s, i)][0]:
            best[(s, i)] = (d, e)
    near = {(r // P, r % P): (key >> 56, key & ((1 << 56) - 1)) for r, key in enumerate(keys) if key != (1 << 64) - 1 and key >> 56 <= k}
    assert near == best and len(best) >= 6


# ---------------------------------------------------------------- 11. the host-level call
def fasta_case():
    rs = np.random.RandomState(81)
    seq = [dna(rs, 130), dna(rs, 700), b"", dna(rs, 900), dna(rs, 40)]
    occ = bytearray(seq[1][290:330])
    del occ[7]                                                   # one more copy, a byte short, in sequence 3
    seq[3] = seq[3][:520] + bytes(occ) + seq[3][520 + len(occ):]
    cross = seq[1][680:700] + seq[3][:20]                        # exact across the boundary of sequences 1 and 3
    pats = [seq[1][290:330], seq[3][100:133], cross, seq[3][:18]]
    src = b"\r\n".join(seq[0][i:i + 60] for i in range(0, len(seq[0]), 60)).lower() + b"\r\n"     # bytes in front of the first header
    for name, s in zip((b">one first\r\n", b">empty\r\n", b">two\r\n", b">last one\r\n"), seq[1:]):
        src += name + b"".join(s[i:i + 60] + b"\r\n" for i in range(0, len(s), 60)).lower()
    return seq, pats, src


def apply_script(p, t, text):
    """the script consumes the pattern and the text bytes exactly; -> the number of edits"""
    x = y = edits = 0
    for count, op in re.findall(r"(\d+)([=XID])", text):
        for _ in range(int(count)):
            if op in "=X":
                assert (p[y] == t[x]) == (op == "=")
                x, y = x + 1, y + 1
            elif op == "I":
                x += 1
            else:
                y += 1
            edits += op != "="
    assert (x, y) == (len(t), len(p))
    return edits


def test_host_call_on_a_multi_fasta(ctx, apm):
    seq, pats, src = fasta_case()
    flags = apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER
    T, src_of = SR.TN.normalize(src, flags)
    begins = [t for _, t in SR.SQ.sequences(src, flags)]
    assert T == b"".join(seq) and begins == [0, 130, 830, 830, 1730, 1770]
    k, P = 2, len(pats)
    setup(ctx, pats, k)
    before = ctx.count_buffer(src)
    ctx.set_text_mode(flags)
    try:
        counted = ctx.count_buffer(src)
        for occ_flags in (ALL, LOCAL_MIN):
            want = SR.source_records(src, flags, pats, k, occ_flags)
            norm = SR.records_with_starts(T, pats, k, occ_flags, begins)
            rec, total, cnt = ctx.find_occ_seq_buffer(src, occ_flags)
            assert rec == want, occ_flags
            assert total == len(want) and cnt == counts_of(want, P)
            assert [l for l, _ in ctx.launch_times()] == ["socc", "sspan"]
            assert ctx.stat("map_ms") > 0                        # the map launches ran behind them
            assert ctx.find_occ_seq_buffer(src, occ_flags, spans=False) == ([w[:3] for w in want], total, cnt)
            assert [l for l, _ in ctx.launch_times()] == ["socc"]
            # scripts: those of the normalised text, row by row behind the sort
            rows, total_s, cnt_s = ctx.find_occ_seq_buffer(src, occ_flags, scripts=True)
            assert [l for l, _ in ctx.launch_times()] == ["socc", "sspan", "oalign"]
            assert [r[:5] for r in rows] == want and (total_s, cnt_s) == (total, cnt)
            for r, (i, e, d, st, s) in zip(rows, norm):
                assert r[5] == apm.ops_to_script(bytes(pinned_script(pats[i], T[st:e + 1])[1])), r
                assert apply_script(pats[i], T[st:e + 1], r[5]) == d
        # the copy across the boundary is in neither sequence; the whole-text search reports it
        assert not any(r[0] == 2 for r in want)
        assert any(r[0] == 2 and r[2] == 0 for r in ctx.find_occ_buffer(src, LOCAL_MIN)[0])
        assert (0, src_of[130 + 329], 0, src_of[130 + 290], 1) in want and any(r[0] == 0 and r[2] == 1 and r[4] == 3 for r in want)
        assert (3, src_of[830 + 17], 0, src_of[830], 3) in want, "an occurrence at a sequence's first byte, behind an empty sequence"
        # the context's own table stands: apm_get_sequences and apm_locate_buffer work right behind the call
        ctx.find_occ_seq_buffer(src, LOCAL_MIN)
        table, n_tab = ctx.sequences()
        assert n_tab == 5 and [t for _, t in table] == begins
        locs = ctx.locate([(w[0], w[3]) for w in want])
        assert [l[1] for l in locs] == [w[4] for w in want]
        assert ctx.count_buffer(src) == counted                  # the plan is not touched
        # capacity below the records: the first records of the sort need not be the ones kept, the totals stand
        few, total_f, cnt_f = ctx.find_occ_seq_buffer(src, ALL, capacity=3)
        all_rows = SR.source_records(src, flags, pats, k, ALL)
        assert len(few) == 3 and set(few) <= set(all_rows) and total_f == len(all_rows) and cnt_f == counts_of(all_rows, P)
        assert ctx.find_occ_seq_buffer(src, ALL, capacity=0) == ([], total_f, cnt_f)
        # without FASTA in the mode: one sequence, the whole-text search's answer
        ctx.set_text_mode(apm.APM_TEXT_UPPER)
        plain = b"".join(seq).lower()
        rec1, total1, cnt1 = ctx.find_occ_seq_buffer(plain, LOCAL_MIN)
        assert ([r[:4] for r in rec1], total1, cnt1) == ctx.find_occ_buffer(plain, LOCAL_MIN) and all(r[4] == 0 for r in rec1)
        assert any(r[0] == 2 and r[2] == 0 for r in rec1)
        # a header alone, and an empty source
        ctx.set_text_mode(flags)
        assert ctx.find_occ_seq_buffer(b">only a header\r\n") == ([], 0, [0] * P)
        assert ctx.find_occ_seq_buffer(b"") == ([], 0, [0] * P)
    finally:
        ctx.set_text_mode(0)
    assert ctx.count_buffer(src) == before and before == H.oracle_counts(src, pats, k)


def test_host_call_refusals(ctx, apm):
    seq, pats, src = fasta_case()
    lib = apm.load_library()
    setup(ctx, pats, 2)
    buf = ctypes.create_string_buffer(src, len(src))
    cap = 8
    ends, starts = (apm.ApmMatch * cap)(), (apm.ApmMatch * cap)()
    seqs, ops = (ctypes.c_uint32 * cap)(), (ctypes.c_uint32 * (cap * 64))()
    found = ctypes.c_uint64(99)
    call = lambda flags, e, st, sq, op, stride: lib.apm_find_occ_seq_buffer(ctx._ctx, buf, len(src), flags, e, st, sq, cap, ctypes.byref(found), None, op, stride)
    assert call(LOCAL_MIN, ends, starts, seqs, None, 0) == STATE                  # mode 0
    ctx.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
    try:
        words = ctx.occ_align_row_words()
        assert call(LOCAL_MIN, ends, starts, seqs, ops, words) == 0 and found.value > 0
        found.value = 99
        assert call(2, ends, starts, seqs, None, 0) == INVALID                    # unknown flag bits
        assert call(0x80000001, ends, starts, seqs, None, 0) == INVALID
        assert call(LOCAL_MIN, ends, None, seqs, None, 0) == INVALID              # out_seq without out_start
        assert call(LOCAL_MIN, ends, None, None, ops, words) == INVALID           # ops without out_start
        assert call(LOCAL_MIN, ends, starts, None, ops, words - 1) == INVALID     # a short stride
        assert call(LOCAL_MIN, None, None, None, None, 0) == INVALID              # NULL ends with room asked for
        assert lib.apm_find_occ_seq_buffer(ctx._ctx, buf, len(src), LOCAL_MIN, ends, None, None, cap, None, None, None, 0) == INVALID
        assert found.value == 99
        for bad, k in (([b"ACGT" * 32 + b"A", b"ACGTAC"], 2), ([b"ACGTACGT", b"ACG"], 3)):   # m = 129; k >= m
            setup(ctx, bad, k)
            with pytest.raises(apm.ApmError) as e:
                ctx.find_occ_seq_buffer(src)
            assert e.value.status == UNSUPPORTED
    finally:
        ctx.set_text_mode(0)


def test_device_calls_refuse_bad_arguments(ctx, apm):
    text = b"ACGT" * 64
    n = len(text)
    with Dev(ctx) as dev:
        out = Out(ctx, dev, 16, 2)
        d_text, d_table = dev.text(text), dev.table([0, 100, n])
        shard = lambda **kw: ctx.occ_seq_shard_device(kw.get("text", d_text), 0, n, kw.get("n_total", n), kw.get("ob", 0), kw.get("oe", n),
                                                      kw.get("table", d_table), kw.get("n_seq", 2), kw.get("flags", ALL), kw.get("out", out.d_out), 16,
                                                      kw.get("n_found", out.d_n), out.d_counts)
        spans = lambda **kw: ctx.occ_seq_spans_device(d_text, 0, n, kw.get("n_total", n), kw.get("table", d_table), kw.get("n_seq", 2), out.d_out, 16,
                                                      kw.get("n_rec", out.d_n), kw.get("span", out.d_span), kw.get("seq", out.d_seq))

        def refused(call, status):
            with pytest.raises(apm.ApmError) as e:
                call()
            assert e.value.status == status

        for bad, k in (([b"ACGT" * 32 + b"A", b"ACGTAC"], 2), ([b"ACGTACGT", b"ACG"], 3)):   # m = 129; k >= m
            setup(ctx, bad, k)
            refused(shard, UNSUPPORTED)
            refused(spans, UNSUPPORTED)
        setup(ctx, [b"ACGTAC", b"GG"], 1)
        for kw in ({"ob": 9, "oe": 8}, {"flags": 2}, {"flags": 0x80000001}, {"table": None}, {"table": d_table + 4}, {"n_seq": 0}, {"out": None},
                   {"out": out.d_out + 8}, {"n_found": None}):
            refused(lambda: shard(**kw), INVALID)
        for kw in ({"table": None}, {"table": d_table + 4}, {"n_seq": 0}, {"span": None}, {"span": out.d_span + 8}, {"seq": out.d_seq + 2}, {"n_rec": None}):
            refused(lambda: spans(**kw), INVALID)
        for kw in ({"n_total": (1 << 56) + 1}, {"n_seq": 1 << 32}):
            refused(lambda: shard(**kw), UNSUPPORTED)
            refused(lambda: spans(**kw), UNSUPPORTED)
        assert out.read() == ([], 0, [0, 0])                     # nothing was written
        assert out.raw_records(out.b_span) == [None] * 16 and out.seqs() == [None] * 16


def test_multi_device_context_is_refused(apm):
    rehearse = apm.device_count() < 2                            # two shards on the one device
    if rehearse:
        os.environ["APM_DEVICES"] = "0,0"
    try:
        with apm.ApmContext(n_devices=2) as c:
            c.set_patterns([b"ACGTACGT"], 1)
            with pytest.raises(apm.ApmError) as e:
                c.find_occ_seq_buffer(b">a\nACGT\n")
            assert e.value.status == UNSUPPORTED
    finally:
        if rehearse:
            del os.environ["APM_DEVICES"]


# ---------------------------------------------------------------- 12. the command-line host
def run_cli(args):
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    return subprocess.run([exe] + args, capture_output=True, text=True)


def test_cli_occurrences_per_sequence(tmp_path, apm):
    rs = np.random.RandomState(91)
    p = b"GATTACA"
    third = dna(rs, 200, np.frombuffer(b"CT", dtype=np.uint8))
    third = third[:90] + b"GATTGACA" + third[98:]               # one insertion, inside a line break's reach
    src = b">read1 first\nccccccccccga\n>read2\nttacacc\ncccccc\n>read3 last\n" + b"\n".join(third[i:i + 60] for i in range(0, 200, 60)) + b"\n"
    fa = tmp_path / "reads.fa"
    fa.write_bytes(src)
    flags = apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER
    T, _ = SR.TN.normalize(src, flags)
    begins = [t for _, t in SR.SQ.sequences(src, flags)]
    assert begins == [0, 0, 12, 25, 225] and T[:25] == b"CCCCCCCCCCGATTACACCCCCCCC"
    names = ["-", "read1", "read2", "read3"]
    pats = [p, b"CCCCCG"]

    def render(occ_flags, scripts):
        rows = SR.records_with_starts(T, pats, 2, occ_flags, begins)
        lines = ["Number of matches for pattern <%s>: %d" % (q.decode(), sum(r[0] == i for r in rows)) for i, q in enumerate(pats)]
        for i, q in enumerate(pats):
            items = ""
            for j, e, d, st, s in rows:
                if j == i:
                    items += " %s:%d-%d:%d" % (names[s], st - begins[s], e - st + 1, d)
                    if scripts:
                        items += ":" + apm.ops_to_script(bytes(pinned_script(q, T[st:e + 1])[1]))
            lines.append("Occurrences for pattern <%s>:" % q.decode() + items)
        return lines

    best = render(LOCAL_MIN, False)
    assert " read2:0-5:2" in best[2] and " read3:90-8:1" in best[2] and "read1" not in best[2], "the GATTACA case: TTACA, the real hit in read2"
    base = ["2", str(fa)] + [q.decode() for q in pats] + ["--fasta", "--upper"]
    for flag, occ_flags, scripts in (("--occurrences-per-sequence", LOCAL_MIN, False), ("--occurrences-per-sequence=best", LOCAL_MIN, False),
                                     ("--occurrences-per-sequence=all", ALL, False), ("--occurrence-scripts-per-sequence", LOCAL_MIN, True),
                                     ("--occurrence-scripts-per-sequence=all", ALL, True)):
        r = run_cli(base + [flag])
        assert r.returncode == 0, r.stderr
        assert [l for l in r.stdout.splitlines() if l.startswith(("Number of matches", "Occurrences for"))] == render(occ_flags, scripts), flag
    # the whole-text listing reports the crossing occurrence instead
    r = run_cli(base + ["--occurrences"])
    assert r.returncode == 0 and "Occurrences for pattern <GATTACA>: %d-" % src.index(b"ga\n") in r.stdout
    # refused without --fasta, with a bad mode, and together with the other listings
    for flag in ("--occurrences-per-sequence", "--occurrence-scripts-per-sequence"):
        r = run_cli(["2", str(fa)] + [q.decode() for q in pats] + ["--upper", flag])
        assert r.returncode == 1 and "--fasta" in r.stderr and flag in r.stderr
        assert run_cli(base + [flag + "=worst"]).returncode == 1
        for other in ("--positions", "--distances", "--alignments", "--best", "--occurrences", "--occurrence-scripts=all", "--nearest",
                      "--nearest-per-sequence", "--sequences"):
            r = run_cli(base + [flag, other])
            assert r.returncode == 1 and flag in r.stderr, (flag, other)
