"""The sequence index and the locate pass on the GPU: apm_index_sequences_device against the byte-serial reference
(seqindex_ref.sequences) entry for entry, apm_locate_records_device against seqindex_ref.locate record for record, the
host-level calls (apm_locate_buffer, apm_get_sequences) and the CLI's --sequences on a three-sequence CRLF file whose
matches come from the oracle on the normalised text.  Every device-level case runs with the source at an aligned and at
an unaligned device address (lead 0 and 5) and with sentinel bytes around every output."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import seqindex_ref as S
import textnorm_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, STATE = -1, -6, -8
BOTH = R.FASTA | R.UPPER
SENTINEL = 0xA5
GUARD = 64
LEADS = (0, 5)


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


class Source:
    """a source on the device `lead` bytes behind a 16-byte boundary, '>' bytes around it that would count if they were
    read as text, and room for its normalised text"""

    def __init__(self, ctx, src, lead):
        self.ctx, self.n = ctx, len(src)
        self.base = ctx.device_alloc(len(src) + 64)
        self.d_dst = ctx.device_alloc(len(src) + 32)
        ctx.device_memset(self.base, ord(">"), len(src) + 64)
        if src:
            ctx.device_upload(self.base + lead, src)
        ctx.synchronize()
        self.d_src = self.base + lead

    def normalize(self, flags, capacity=None):
        return self.ctx.normalize_device(self.d_src, self.n, flags, self.d_dst, self.n if capacity is None else capacity)

    def close(self):
        self.ctx.device_free(self.base)
        self.ctx.device_free(self.d_dst)


class Guarded:
    """a device buffer of nbytes between two runs of sentinel bytes, itself filled with them"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.base = ctx.device_alloc(nbytes + 2 * GUARD)
        self.ptr = self.base + GUARD
        self.reset()

    def reset(self):
        self.ctx.device_memset(self.base, SENTINEL, self.nbytes + 2 * GUARD)

    def read(self, nbytes=None):
        """the payload's first nbytes (all of it); the rest of the payload and both guards must still be sentinel bytes"""
        self.ctx.synchronize()
        raw = self.ctx.device_download(self.base, self.nbytes + 2 * GUARD)
        used = self.nbytes if nbytes is None else nbytes
        assert raw[:GUARD] == bytes([SENTINEL]) * GUARD, "written in front of the buffer"
        assert raw[GUARD + used:] == bytes([SENTINEL]) * (self.nbytes - used + GUARD), "written behind the entries asked for"
        return raw[GUARD:GUARD + used]

    def close(self):
        self.ctx.device_free(self.base)


def unpack_table(raw):
    return [struct.unpack_from("<QQ", raw, 16 * i) for i in range(len(raw) // 16)]


def unpack_locs(raw):
    return [struct.unpack_from("<QII", raw, 16 * i) for i in range(len(raw) // 16)]


def pack_records(rows, reserved=0x5A5A5A5A):
    return b"".join(struct.pack("<QII", pos, pat, reserved) for pat, pos in rows)


_tables = {}


def ref_table(name, flags):
    if (name, flags) not in _tables:
        _tables[name, flags] = S.sequences(S.layouts()[name], flags)
    return _tables[name, flags]


def index_call(ctx, d_table, capacity):
    """(status, n_seq) of the raw call: *n_seq is set on a refusal too"""
    import ctypes
    n_seq = ctypes.c_uint64(0xDEAD)
    rc = ctx._lib.apm_index_sequences_device(ctx._ctx, ctypes.c_void_p(d_table), capacity, ctypes.byref(n_seq))
    return rc, n_seq.value


# ---------------------------------------------------------------- 1. the table against the reference
@pytest.mark.parametrize("name", sorted(S.layouts()) + ["empty"])
def test_table_on_every_layout(ctx, name):
    src = b"" if name == "empty" else S.layouts()[name]
    for lead in LEADS:
        s = Source(ctx, src, lead)
        try:
            for flags in (BOTH, R.UPPER) if name in ("sq_crlf", "gt_everywhere", "empty") else (BOTH,):
                want = S.sequences(src, flags) if name == "empty" else ref_table(name, flags)
                if flags == R.UPPER:
                    assert len(want) == 2                                    # no FASTA: n_seq == 1
                out = Guarded(ctx, 16 * len(want))
                try:
                    assert s.normalize(flags) == want[-1][1]
                    assert ctx.index_sequences_device(out.ptr, len(want)) == len(want) - 1, (name, lead, flags)
                    assert unpack_table(out.read()) == want, (name, lead, flags)
                    assert ctx.stat("seq_count") == len(want) - 1 and ctx.stat("seq_index_ms") >= 0
                finally:
                    out.close()
        finally:
            s.close()
    if name == "empty":
        assert want == [(S.NO_HEADER, 0), (0, 0)]


# ---------------------------------------------------------------- 2. more blocks than one chunk of the scan
def test_table_beyond_one_scan_chunk(ctx):
    unit = b">r\n" + b"ACGT" * 15 + b"\n"                                     # 64 bytes: one header open, 60 kept bytes
    assert len(unit) == 64
    reps = 4096 * 4096 // 64 + 200                                            # 4096 blocks of 4 KiB and a few more
    src = unit * reps
    assert len(src) > 16 << 20
    idx = np.arange(reps, dtype=np.uint64)
    for lead in LEADS:
        s = Source(ctx, src, lead)
        out = Guarded(ctx, 16 * (reps + 2))
        try:
            assert s.normalize(R.FASTA) == 60 * reps
            assert ctx.index_sequences_device(out.ptr, reps + 2) == reps + 1
            got = np.frombuffer(out.read(), dtype=np.uint64).reshape(-1, 2)
            assert tuple(got[0]) == (S.NO_HEADER, 0) and tuple(got[1]) == (0, 0)
            assert tuple(got[reps]) == (64 * (reps - 1), 60 * (reps - 1)) and tuple(got[reps + 1]) == (len(src), 60 * reps)
            at = 4096 * 4096 // 64                                            # unit `at` begins at the chunk boundary (lead 0)
            for i in (at - 1, at, at + 1, at + 2):                            # entry i + 1 belongs to unit i
                assert tuple(got[i + 1]) == (64 * i, 60 * i), (lead, i)
            assert np.array_equal(got[1:reps + 1, 0], 64 * idx) and np.array_equal(got[1:reps + 1, 1], 60 * idx)
        finally:
            out.close()
            s.close()


# ---------------------------------------------------------------- 3. errors
def test_capacity_one_short_is_refused_and_untouched(ctx):
    name = "sq_crlf"
    want = ref_table(name, BOTH)
    s = Source(ctx, S.layouts()[name], 5)
    out = Guarded(ctx, 16 * len(want))
    try:
        s.normalize(BOTH)
        rc, n_seq = index_call(ctx, out.ptr, len(want) - 1)
        assert rc == INVALID and n_seq == len(want) - 1
        assert out.read(0) == b""                                             # every byte still the sentinel
        rc, n_seq = index_call(ctx, out.ptr, len(want))                       # an exact fit goes through
        assert rc == 0 and n_seq == len(want) - 1
        assert unpack_table(out.read()) == want
    finally:
        out.close()
        s.close()


def test_index_and_locate_without_a_normalisation_are_state_errors(apm):
    with apm.ApmContext(device=0) as fresh:
        buf = Guarded(fresh, 256)
        s = Source(fresh, S.layouts()["sq_crlf"], 0)
        try:
            fresh.set_patterns([b"ACGT"], 0)
            with pytest.raises(apm.ApmError) as e:
                fresh.index_sequences_device(buf.ptr, 16)
            assert e.value.status == STATE
            with pytest.raises(apm.ApmError) as e:
                fresh.locate_records_device(buf.ptr, 1, buf.ptr + 64, buf.ptr + 128, 1, buf.ptr + 192)
            assert e.value.status == STATE
            with pytest.raises(apm.ApmError) as e:                            # a normalisation that fails: the text does not fit
                s.normalize(BOTH, capacity=10)
            assert e.value.status == INVALID
            with pytest.raises(apm.ApmError) as e:
                fresh.index_sequences_device(buf.ptr, 16)
            assert e.value.status == STATE
            assert buf.read(0) == b""
        finally:
            s.close()
            buf.close()


# ---------------------------------------------------------------- 4. locate: every kept byte
LENS = (4, 300)


def _offset_of(src, flags, kind):
    """a source offset on a header byte / a '\\n' / a '\\r' that is not kept, or None"""
    kept = set(R.normalize(src, flags)[1])
    for i, b in enumerate(src):
        if i in kept:
            continue
        if (kind == "nl" and b == 0x0A) or (kind == "cr" and b == 0x0D) or (kind == "header" and b not in (0x0A, 0x0D)):
            return i
    return None


@pytest.mark.parametrize("name", ["sq_crlf", "nl_ends_block_gt_starts_next", "sq_two_headers_in_a_row", "sq_example"])
def test_locate_every_kept_byte(ctx, name):
    src = S.layouts()[name]
    table = ref_table(name, BOTH)
    src_of = R.normalize(src, BOTH)[1]
    rows = [(p, pos) for pos in src_of for p in range(len(LENS))]
    made_up = [(2, src_of[0]), (7, src_of[-1]), (0, len(src)), (1, len(src) + 7), (0, 1 << 40)]
    for kind in ("header", "nl", "cr"):
        at = _offset_of(src, BOTH, kind)
        assert at is not None or (kind == "cr" and name not in ("sq_crlf", "sq_example")), kind
        if at is not None:
            made_up.append((0, at))
    rows += made_up
    want = [S.locate(src, BOTH, table, LENS, pos, p) for p, pos in rows]
    assert want[-len(made_up):] == [S.INVALID] * len(made_up)
    flags_seen = {fl for _, seq, fl in want if seq != S.SEQ_INVALID}
    # (a window that is both: the text ends in a later sequence than the one it starts in -- the 12 kept bytes of the example)
    assert flags_seen >= ({S.SPANS, S.TRUNCATED, S.SPANS | S.TRUNCATED} if name == "sq_example" else {0, S.SPANS, S.TRUNCATED})
    raw = pack_records(rows)
    ctx.set_patterns([b"ACGT", b"ACGT" * 75], 1)
    d_rec, d_n = ctx.device_alloc(len(raw)), ctx.device_alloc(16)
    try:
        ctx.device_upload(d_rec, raw)
        ctx.device_upload(d_n, struct.pack("<Q", len(rows)))
        for lead in LEADS:
            s = Source(ctx, src, lead)
            d_table, d_loc = Guarded(ctx, 16 * len(table)), Guarded(ctx, 16 * len(rows))
            try:
                s.normalize(BOTH)
                assert ctx.index_sequences_device(d_table.ptr, len(table)) == len(table) - 1
                ctx.locate_records_device(d_rec, len(rows), d_n, d_table.ptr, len(table) - 1, d_loc.ptr)
                got = unpack_locs(d_loc.read())
                bad = [(rows[i], got[i], want[i]) for i in range(len(rows)) if got[i] != want[i]]
                assert not bad, (lead, len(bad), bad[:5])
                assert unpack_table(d_table.read()) == table                   # the table is only read
                assert ctx.device_download(d_rec, len(raw)) == raw             # and so are the records
                assert ctx.stat("locate_ms") >= 0
            finally:
                d_table.close()
                d_loc.close()
                s.close()
    finally:
        ctx.device_free(d_rec)
        ctx.device_free(d_n)


# ---------------------------------------------------------------- 5. locate: nothing at or beyond `capacity`
def test_locate_writes_nothing_beyond_capacity(ctx):
    name = "sq_crlf"
    src, table = S.layouts()[name], ref_table(name, BOTH)
    src_of = R.normalize(src, BOTH)[1]
    rows = [(i % 2, pos) for i, pos in enumerate(src_of[:500])]
    cap = 123
    raw = pack_records(rows)
    ctx.set_patterns([b"ACGT", b"ACGT" * 75], 1)
    s = Source(ctx, src, 5)
    d_rec, d_n = ctx.device_alloc(len(raw)), ctx.device_alloc(16)
    d_table, d_loc = Guarded(ctx, 16 * len(table)), Guarded(ctx, 16 * len(rows))
    try:
        ctx.device_upload(d_rec, raw)
        ctx.device_upload(d_n, struct.pack("<Q", len(rows)))                  # *d_n_rec > capacity
        s.normalize(BOTH)
        ctx.index_sequences_device(d_table.ptr, len(table))
        ctx.locate_records_device(d_rec, cap, d_n, d_table.ptr, len(table) - 1, d_loc.ptr)
        got = unpack_locs(d_loc.read(16 * cap))                               # (read: everything behind entry cap - 1 is sentinel)
        assert got == [S.locate(src, BOTH, table, LENS, pos, p) for p, pos in rows[:cap]]
        assert ctx.device_download(d_rec, len(raw)) == raw
    finally:
        for g in (d_table, d_loc, s):
            g.close()
        ctx.device_free(d_rec)
        ctx.device_free(d_n)


# ---------------------------------------------------------------- 6. end to end under apm_set_text_mode
K = 2


@pytest.fixture(scope="module")
def three():
    """a three-sequence CRLF file with lower-case stretches and planted occurrences of a 20-byte pattern: inside sequence 1,
    across the boundary of sequences 1 and 2, in the truncated tail; and of a 33-byte pattern inside sequence 3"""
    rng = random.Random(31)
    P, P2 = R.dna(rng, 20), R.dna(rng, 33)
    seqs = [bytearray(R.dna(rng, n)) for n in (3000, 2500, 1800)]
    inside = bytearray(P)
    inside[7] = next(c for c in b"ACGT" if c != inside[7])                  # one substitution
    seqs[0][1000:1020] = inside
    seqs[0][-10:] = P[:10]
    seqs[1][:10] = P[10:]
    seqs[2][600:633] = P2
    seqs[2][-12:] = P[:12]
    T = b"".join(bytes(q) for q in seqs)
    parts = []
    for i, q in enumerate(seqs):
        low = bytearray(q)
        for a in range(0, len(low), 500):                                   # lower-case stretches, the planted places among them
            low[a:a + 130] = bytes(low[a:a + 130]).lower()
        low[990:1030] = bytes(low[990:1030]).lower()
        parts.append(b">chr%d some description\r\n" % (i + 1) + b"".join(bytes(low[a:a + 60]) + b"\r\n" for a in range(0, len(low), 60)))
    src = b"".join(parts)
    assert R.normalize(src, BOTH)[0] == T and R.normalize(src, R.FASTA)[0] != T
    pats = [P, P2]
    src_of = R.normalize(src, BOTH)[1]
    table = S.sequences(src, BOTH)
    want = []                                                               # (pattern, source offset, distance), sorted
    for i, p in enumerate(pats):
        for j in H.oracle_positions(T, p, K):
            size = min(len(p), len(T) - j)
            want.append((i, src_of[j], H.window_distance(p[:size], T[j:j + size])))
    locs = [S.locate(src, BOTH, table, [len(p) for p in pats], pos, i) for i, pos, _ in want]
    return {"src": src, "T": T, "pats": pats, "table": table, "want": want, "locs": locs}


def test_the_planted_matches_are_what_they_are_meant_to_be(three):
    by = {(i, pos): loc for (i, pos, _), loc in zip(three["want"], three["locs"])}
    src_of = R.normalize(three["src"], BOTH)[1]
    assert by[0, src_of[1000]] == (1000, 1, 0)                                # inside chr1
    assert by[0, src_of[2990]] == (2990, 1, S.SPANS)                          # chr1's last 10 bytes and chr2's first 10
    assert by[0, src_of[len(three["T"]) - 12]] == (1800 - 12, 3, S.TRUNCATED)
    assert by[1, src_of[5500 + 600]] == (600, 3, 0)
    assert {fl for _, _, fl in three["locs"]} >= {0, S.SPANS, S.TRUNCATED}


def test_end_to_end_locations(apm, ctx, three):
    src, pats, want, locs = three["src"], three["pats"], three["want"], three["locs"]
    try:
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, K)
        ctx.set_text_mode(BOTH)
        counts = ctx.count_buffer(src)
        assert counts == [sum(1 for i, _, _ in want if i == q) for q in range(len(pats))]
        for call, shape in ((ctx.find_all_buffer, lambda r: r[:2]), (ctx.find_all_dist_buffer, lambda r: r[:3]),
                            (ctx.find_all_align_buffer, lambda r: r[:3])):
            got, total = call(src, len(want) + 16)
            assert total == len(want) and [tuple(r[:len(shape(want[0]))]) for r in got] == [shape(w) for w in want]
            got_locs = ctx.locate(got)
            assert got_locs == locs
            assert {fl for _, _, fl in got_locs} >= {0, S.SPANS, S.TRUNCATED}  # (not an empty set)
            assert ctx.stat("locate_ms") >= 0 and ctx.stat("seq_count") == 4 # sequence 0 and chr1..chr3
            assert ctx.sequences() == (three["table"], 4)
            assert ctx.sequences(2) == (three["table"][:2], 4)                 # at most `capacity` entries, n_seq exact
            assert call(src, len(want) + 16) == (got, total)                   # records and counts as before the locate call
            assert ctx.count_buffer(src) == counts
        assert ctx.locate([]) == []
        ctx.count_buffer(src)                                                  # a count call normalises too: the table follows it
        assert ctx.locate([(0, want[0][1])]) == [locs[0]]
        ctx.set_text_mode(0)                                                   # a verbatim scan: no normalised text is resident
        ctx.count_buffer(src)
        with pytest.raises(apm.ApmError) as e:
            ctx.locate([(0, want[0][1])])
        assert e.value.status == STATE
    finally:
        ctx.set_text_mode(0)


def test_locate_without_a_text_mode_is_a_state_error(apm, three):
    with apm.ApmContext(device=0) as fresh:
        fresh.set_patterns(three["pats"], K)
        got, _ = fresh.find_all_buffer(three["src"])
        for call in (lambda: fresh.locate(got[:1] or [(0, 0)]), fresh.sequences):
            with pytest.raises(apm.ApmError) as e:
                call()
            assert e.value.status == STATE


def test_multi_device_context_is_unsupported(apm, three):
    os.environ["APM_DEVICES"] = "0,0"
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    with m:
        m.set_patterns(three["pats"], K)
        for call in (lambda: m.locate([(0, 5)]), m.sequences):
            with pytest.raises(apm.ApmError) as e:
                call()
            assert e.value.status == UNSUPPORTED


# ---------------------------------------------------------------- 7. the device pipeline, no host synchronisation in between
@pytest.mark.parametrize("lead", LEADS)
def test_device_pipeline(ctx, three, lead):
    src, pats, want, locs, table = three["src"], three["pats"], three["want"], three["locs"], three["table"]
    cap = len(want) + 16
    ctx.set_text_mode(0)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, K)
    s = Source(ctx, src, lead)
    d_table, d_loc = Guarded(ctx, 16 * len(table)), Guarded(ctx, 16 * cap)
    d_rec, d_n = ctx.device_alloc(16 * cap), ctx.device_alloc(16)
    try:
        ctx.device_memset(d_n, 0, 16)
        n = s.normalize(BOTH)                                                  # (its one synchronisation)
        assert ctx.index_sequences_device(d_table.ptr, len(table)) == len(table) - 1   # (its one synchronisation)
        ctx.find_shard_device(s.d_dst, 0, n, n, 0, n, d_rec, cap, d_n)
        ctx.score_shard_device(s.d_dst, 0, n, n, d_rec, cap, d_n)
        ctx.map_positions_device(d_rec, cap, d_n)
        ctx.locate_records_device(d_rec, cap, d_n, d_table.ptr, len(table) - 1, d_loc.ptr)
        ctx.synchronize()
        assert struct.unpack("<Q", ctx.device_download(d_n, 8))[0] == len(want)
        recs = [struct.unpack_from("<QII", ctx.device_download(d_rec, 16 * len(want)), 16 * i) for i in range(len(want))]
        got = sorted(zip([(pat, pos, dist) for pos, pat, dist in recs], unpack_locs(d_loc.read(16 * len(want)))))
        assert [g[0] for g in got] == want and [g[1] for g in got] == locs
    finally:
        for g in (d_table, d_loc, s):
            g.close()
        ctx.device_free(d_rec)
        ctx.device_free(d_n)


# ---------------------------------------------------------------- 8. the CLI
def test_cli_sequences(three, tmp_path):
    path = tmp_path / "three.fa"
    path.write_bytes(three["src"])
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    pats = [p.decode() for p in three["pats"]]
    base = [exe, "--gpus", "1", "--fasta", "--upper", "--distances", str(K), str(path)] + pats
    r = subprocess.run(base + ["--sequences"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    count_lines = lambda out: [l for l in out.splitlines() if l.startswith("Number of matches")]
    assert count_lines(r.stdout) == count_lines(plain.stdout) and len(count_lines(r.stdout)) == 2   # not adjusted
    for q, p in enumerate(pats):
        items = ["chr%d:%d:%d" % (seq, off, dist) for (i, _, dist), (off, seq, fl) in zip(three["want"], three["locs"]) if i == q and fl == 0]
        assert items
        assert "Positions for pattern <%s>: %s\n" % (p, " ".join(items)) in r.stdout
    assert " chr1:1000:1" in r.stdout                                          # the match inside a sequence
    assert "chr1:2990:" not in r.stdout and "chr3:1788:" not in r.stdout       # spanning and truncated ones are left out
    assert sum(1 for _, _, fl in three["locs"] if fl) >= 2
    r = subprocess.run([exe, "--gpus", "1", "--sequences", str(K), str(path)] + pats, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--fasta" in r.stderr
