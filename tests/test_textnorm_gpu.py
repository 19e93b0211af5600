"""The text modes on the GPU: apm_normalize_device against the byte-serial reference (textnorm_ref.normalize) byte for
byte, apm_map_positions_device against its src_of, and the host-level calls under apm_set_text_mode against the oracle on
the normalised text T with positions mapped through src_of.

Two notes on the end-to-end checks.  The match positions in T come from a bisection over the oracle's own range counts
(helpers.oracle_positions, one DP per window in Python, is run in full for the 20-byte patterns and must agree): that
keeps every test to a few seconds.  "The default mode finds no match for the 75- and 130-byte patterns at k = 0" is
asserted for WHOLE windows: the reference's truncated tail windows at the very end of the file compare a few bytes
only and match by chance in any layout (small_chrY_x100.fa: four such records)."""
import os
import random
import struct
import subprocess

import pytest

import helpers as H
import textnorm_ref as R

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, STATE = -1, -6, -8
FLAGS = (R.FASTA, R.UPPER, R.FASTA | R.UPPER)
SENTINEL = 0xA5
PRESET = 0x5A5A5A5A
CHRY = os.path.join(H.GOLDEN_DIR, "dna", "small_chrY_x100.fa")


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


_ref_cache = {}


def ref(src, flags):
    key = (src, flags)
    if key not in _ref_cache:
        _ref_cache[key] = R.normalize(src, flags)
    return _ref_cache[key]


def fasta_like(seed, n):
    """n bytes, mostly DNA in lines of about 60, lower-case stretches, headers, a few '\\r' and stray '>'"""
    rng = random.Random(seed)
    return bytes(rng.choices(b"ACGTacgtn\n\r>", weights=[60, 60, 60, 60, 8, 8, 8, 8, 2, 5, 1, 2], k=n))


class DeviceText:
    """a source on the device at base + src_mis, and a destination of sentinel bytes whose text goes to base + dst_mis"""

    def __init__(self, ctx, src, src_mis, dst_mis, dst_room=None):
        self.ctx, self.src_mis, self.dst_mis = ctx, src_mis, dst_mis
        self.room = len(src) if dst_room is None else dst_room
        self.d_src = ctx.device_alloc(len(src) + 48)
        self.dst_bytes = dst_mis + self.room + 64 + 16
        self.d_dst = ctx.device_alloc(self.dst_bytes)
        ctx.device_memset(self.d_src, ord(">"), len(src) + 48)     # (bytes around the source that would count if they were read as text)
        ctx.device_memset(self.d_dst, SENTINEL, self.dst_bytes)
        if src:
            ctx.device_upload(self.d_src + src_mis, src)
        ctx.synchronize()
        self.n = len(src)

    def normalize(self, flags, capacity=None):
        return self.ctx.normalize_device(self.d_src + self.src_mis, self.n, flags, self.d_dst + self.dst_mis,
                                         self.room if capacity is None else capacity)

    def dst(self):
        self.ctx.synchronize()
        return self.ctx.device_download(self.d_dst, self.dst_bytes)

    def reset_dst(self):
        self.ctx.device_memset(self.d_dst, SENTINEL, self.dst_bytes)

    def close(self):
        self.ctx.device_free(self.d_src)
        self.ctx.device_free(self.d_dst)


def check_pass(ctx, src, flags_list=FLAGS, src_mis_list=(0, 1, 7), dst_mis_list=(0, 3)):
    """the pass == the reference: out_len, every byte, and nothing in front of or behind the text (the 64-byte sentinel
    behind dst[out_len] and the rest of the buffer)"""
    for src_mis in src_mis_list:
        for dst_mis in dst_mis_list:
            t = DeviceText(ctx, src, src_mis, dst_mis)
            try:
                for flags in flags_list:
                    want = ref(src, flags)[0]
                    t.reset_dst()
                    out_len = t.normalize(flags)
                    got = t.dst()
                    where = (len(src), flags, src_mis, dst_mis)
                    assert out_len == len(want), where
                    assert got[dst_mis:dst_mis + out_len] == want, where
                    assert got[:dst_mis] == bytes([SENTINEL]) * dst_mis, where
                    assert got[dst_mis + out_len:] == bytes([SENTINEL]) * (len(got) - dst_mis - out_len), where
                    assert ctx.stat("norm_src_bytes") == len(src) and ctx.stat("norm_kept_bytes") == out_len
            finally:
                t.close()


# ---------------------------------------------------------------- 1. the pass against the reference
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, 3 * 4096 + 5, (1 << 20) + 3])
def test_source_lengths_alignments_flags(ctx, n):
    src = fasta_like(100 + n % 97, n)
    if n > 100000:
        assert ref(src, R.FASTA)[0] != src and b">" in src[4096:] and len(ref(src, R.FASTA)[0]) < n - n // 100
    check_pass(ctx, src)


@pytest.mark.parametrize("name", sorted(R.layouts()))
def test_layouts(ctx, name):
    src = R.layouts()[name]
    if name == "only_newlines":
        assert ref(src, R.FASTA)[0] == b""
    if name == "gt_starts_block_not_line_start":
        assert src[4096] == 0x3E and 4096 in ref(src, R.FASTA)[1] and 8192 in ref(src, R.FASTA)[1]
    if name == "header_5000":
        so = ref(src, R.FASTA)[1]
        assert not any(4000 <= i < 9000 for i in so) and 3998 in so and 9000 in so
    check_pass(ctx, src, src_mis_list=(0, 7), dst_mis_list=(0, 3))


def test_upper_folds_only_a_to_z(ctx):
    src = bytes(range(256)) * 3
    want = ref(src, R.UPPER)[0]
    assert want[0x60] == 0x60 and want[0x7B] == 0x7B and want[0x61] == 0x41 and want[0x7A] == 0x5A and want[0x80] == 0x80 and want[0xFF] == 0xFF
    assert len(want) == len(src)
    check_pass(ctx, src, flags_list=(R.UPPER,), src_mis_list=(0, 1), dst_mis_list=(0,))


def test_timed_pass_reports_norm_ms(ctx):
    src = fasta_like(5, 300000)
    t = DeviceText(ctx, src, 0, 0)
    try:
        ctx.set_timing(True)
        t.normalize(R.FASTA)
        ctx.synchronize()
        assert 0 < ctx.stat("norm_ms") < 1000
    finally:
        t.close()


# ---------------------------------------------------------------- 2. error paths
def test_destination_too_small_is_refused_and_untouched(apm, ctx):
    src = R.layouts()["fasta50_header_at_0"]
    want = ref(src, R.FASTA)[0]
    t = DeviceText(ctx, src, 0, 0)
    try:
        with pytest.raises(apm.ApmError) as e:
            t.normalize(R.FASTA, capacity=len(want) - 1)
        assert e.value.status == INVALID
        assert t.dst() == bytes([SENTINEL]) * t.dst_bytes
        assert t.normalize(R.FASTA, capacity=len(want)) == len(want)          # an exact fit goes through
        assert t.dst()[:len(want)] == want
        for flags in (0, 4, 7):
            with pytest.raises(apm.ApmError) as e:
                t.normalize(flags)
            assert e.value.status == INVALID, flags
    finally:
        t.close()


def test_map_before_any_normalisation_is_a_state_error(apm):
    with apm.ApmContext(device=0) as fresh:
        d_rec, d_n = fresh.device_alloc(64), fresh.device_alloc(16)
        try:
            fresh.device_upload(d_n, struct.pack("<Q", 1))
            with pytest.raises(apm.ApmError) as e:
                fresh.map_positions_device(d_rec, 1, d_n)
            assert e.value.status == STATE
        finally:
            fresh.device_free(d_rec)
            fresh.device_free(d_n)


# ---------------------------------------------------------------- 3. the map
def _records(rows):
    return b"".join(struct.pack("<QII", pos, pat, PRESET) for pat, pos in rows)


def _unpack(raw):
    return [struct.unpack_from("<QII", raw, 16 * i) for i in range(len(raw) // 16)]


@pytest.mark.parametrize("name,src_mis", [("header_4090_to_4100", 0), ("nl_ends_block_gt_starts_next", 7), ("fasta50_header_at_0", 1)])
def test_map_every_kept_byte(ctx, name, src_mis):
    src = R.layouts()[name]
    assert len(src) >= 3 * 4096 + 5
    want, src_of = ref(src, R.FASTA | R.UPPER)
    t = DeviceText(ctx, src, src_mis, 3)
    n = len(want)
    rows = [(c % 5, c) for c in range(n)] + [(9, n), (9, n + 1), (9, 1 << 40)]      # the last three name no byte of T
    d_rec, d_n = ctx.device_alloc(16 * len(rows)), ctx.device_alloc(16)
    try:
        assert t.normalize(R.FASTA | R.UPPER) == n
        ctx.device_upload(d_rec, _records(rows))
        ctx.device_upload(d_n, struct.pack("<Q", len(rows)))
        ctx.map_positions_device(d_rec, len(rows), d_n)
        ctx.synchronize()
        got = _unpack(ctx.device_download(d_rec, 16 * len(rows)))
        assert [pos for pos, _, _ in got[:n]] == src_of
        assert [(pat, res) for _, pat, res in got] == [(pat, PRESET) for pat, _ in rows]
        assert [pos for pos, _, _ in got[n:]] == [n, n + 1, 1 << 40]
        # capacity below *d_n_rec: the records at and beyond it keep every bit
        cap = n // 2
        ctx.device_upload(d_rec, _records(rows))
        ctx.map_positions_device(d_rec, cap, d_n)
        ctx.synchronize()
        got = _unpack(ctx.device_download(d_rec, 16 * len(rows)))
        assert [pos for pos, _, _ in got[:cap]] == src_of[:cap]
        assert got[cap:] == [(pos, pat, PRESET) for pat, pos in rows[cap:]]
        assert ctx.stat("map_ms") >= 0
    finally:
        t.close()
        ctx.device_free(d_rec)
        ctx.device_free(d_n)


# ---------------------------------------------------------------- 4. beyond 4 GiB
def test_source_beyond_4gib(apm, ctx):
    n = (1 << 32) + (1 << 20)
    seed = 99
    patches = {(1 << 32) - 10: b"\n>a header across the 4 GiB line\nAC\r\nGT\n",
               (1 << 32) + 4090: b"\n>second header, over a block end\nac\n"}
    d_src, d_dst = ctx.device_alloc(n + 32), ctx.device_alloc(n + 32)
    d_rec, d_n = ctx.device_alloc(64), ctx.device_alloc(16)
    try:
        ctx.synth_fill_device(d_src, 0, n, seed)
        ctx.synchronize()
        for off, p in patches.items():
            ctx.device_upload(d_src + off, p)

        def region(r0):
            raw = bytearray(apm.synth_fill_host(r0, 4096, seed))
            for off, p in patches.items():
                if r0 <= off and off + len(p) <= r0 + 4096:
                    raw[off - r0:off - r0 + len(p)] = p
            return bytes(raw)

        regions = [(1 << 32) - 2048, (1 << 32) + 4090 - 2048]
        kept = [R.normalize(region(r0), R.FASTA) for r0 in regions]
        dropped = [4096 - len(k[0]) for k in kept]
        assert dropped == [len(patches[(1 << 32) - 10]) - 4, len(patches[(1 << 32) + 4090]) - 2]
        out_len = ctx.normalize_device(d_src, n, R.FASTA, d_dst, n)
        assert out_len == n - sum(dropped)
        before = 0
        for r0, (want, _), drop in zip(regions, kept, dropped):
            assert ctx.device_download(d_dst + r0 - before, len(want)) == want
            before += drop
        srcs = [(1 << 32) + 5000, (1 << 32) + (1 << 19) + 1, n - 1]
        rows = [(1, s - sum(dropped)) for s in srcs]
        ctx.device_upload(d_rec, _records(rows))
        ctx.device_upload(d_n, struct.pack("<Q", 3))
        ctx.map_positions_device(d_rec, 3, d_n)
        ctx.synchronize()
        assert _unpack(ctx.device_download(d_rec, 48)) == [(s, 1, PRESET) for s in srcs]
        assert ctx.device_download(d_dst + out_len - 16, 16) == apm.synth_fill_host(n - 16, 16, seed)
    finally:
        for d in (d_src, d_dst, d_rec, d_n):
            ctx.device_free(d)


# ---------------------------------------------------------------- 5. end to end under apm_set_text_mode
def _substituted(rng, p, e):
    w = bytearray(p)
    for at in rng.sample(range(len(w)), e):
        w[at] = rng.choice([c for c in b"ACGT" if c != w[at]])
    return bytes(w)


def _positions(text, pat, k):
    """the matching window starts by bisection over the oracle's own range counts (its banded form -- exact for the
    predicate -- where the band is a small part of the pattern)"""
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


@pytest.fixture(scope="module")
def chry():
    src = open(CHRY, "rb").read()
    T, src_of = R.normalize(src, R.FASTA)
    assert len(T) == len(src) - src.count(b"\n") and b"\n" not in T
    rng = random.Random(21)
    pats = []
    for q, m in enumerate((20, 50, 75, 130)):
        for e in range(4):
            at = 50 * (200 + 37 * q + 5 * e) + 41           # 41 + m > 50: the window straddles a line end of the file
            assert src_of[at + m - 1] - src_of[at] >= m
            pats.append(_substituted(rng, T[at:at + m], e))
    return src, T, src_of, pats


_want_cache = {}


def chry_records(chry, k):
    """(pattern, source offset, distance) of every match in T, sorted by (pattern, pos); computed once per k"""
    if k not in _want_cache:
        src, T, src_of, pats = chry
        rec = []
        for i, p in enumerate(pats):
            pos = _positions(T, p, k)
            if len(p) == 20:
                assert pos == H.oracle_positions(T, p, k)               # the bisection is the oracle's scan
            for j in pos:
                size = min(len(p), len(T) - j)
                rec.append((i, src_of[j], H.window_distance(p[:size], T[j:j + size])))
        assert all(d <= k for _, _, d in rec)
        _want_cache[k] = rec
    return _want_cache[k]


@pytest.mark.parametrize("kernel", ["auto", "bitpar"])
@pytest.mark.parametrize("k", [0, 3])
def test_end_to_end_fasta_mode(apm, ctx, chry, k, kernel):
    src, T, src_of, pats = chry
    want = chry_records(chry, k)
    if ("counts", k) not in _want_cache:
        _want_cache["counts", k] = H.oracle_counts(T, pats, k)
    counts = _want_cache["counts", k]
    assert counts == [sum(1 for i, _, _ in want if i == q) for q in range(len(pats))]
    assert all(c >= 1 for q, c in enumerate(counts) if q % 4 <= k)          # the planted copies are found
    try:
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        ctx.set_kernel(kernel)
        ctx.set_text_mode(R.FASTA)
        assert ctx.count_buffer(src) == counts
        got, total = ctx.find_all_align_buffer(src, len(want) + 64)
        assert total == len(want)
        assert [(i, pos, d) for i, pos, d, _ in got] == want
        assert all(sum(1 for op in ops if op != 0) == d for _, _, d, ops in got)
        assert ctx.find_all_buffer(src, len(want) + 64)[0] == [(i, pos) for i, pos, _ in want]
        assert ctx.find_all_dist_buffer(src, len(want) + 64)[0] == want
        with pytest.raises(apm.ApmError) as e:
            ctx.find_buffer(src, 0)
        assert e.value.status == UNSUPPORTED
        with pytest.raises(apm.ApmError) as e:
            ctx.count_synthetic(4096, 1)
        assert e.value.status == UNSUPPORTED
        # the default did not move: verbatim bytes, the 75- and 130-byte patterns cannot match across a line break
        ctx.set_text_mode(0)
        plain, _ = ctx.find_all_align_buffer(src)
        if k == 0:
            # (whole windows: the reference's truncated tail windows at the end of the file compare a few bytes only and
            # match by chance whatever the layout is)
            long_ones = [r for r in plain if len(pats[r[0]]) >= 75]
            assert not [r for r in long_ones if r[1] + len(pats[r[0]]) <= len(src)]
            assert sum(ctx.count_buffer(src)[8:]) == len(long_ones) < 8
        assert ctx.count_buffer(src) == H.oracle_counts(src, pats, k, banded=True)
    finally:
        ctx.set_text_mode(0)
        ctx.set_kernel("auto")


def test_upper_mode_counts_equal_the_upper_case_text(ctx, chry):
    src, T, src_of, pats = chry
    rng = random.Random(22)
    low = bytearray(src)
    for _ in range(300):
        at, run = rng.randrange(len(src) - 400), rng.randint(1, 400)
        low[at:at + run] = bytes(low[at:at + run]).lower()
    low = bytes(low)
    assert low != src and low.upper() == src
    k = 3
    want = H.oracle_counts(T, pats, k)
    try:
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        ctx.set_text_mode(R.FASTA | R.UPPER)
        assert ctx.count_buffer(low) == want
        ctx.set_text_mode(R.FASTA)
        assert ctx.count_buffer(low) == H.oracle_counts(R.normalize(low, R.FASTA)[0], pats, k) != want
    finally:
        ctx.set_text_mode(0)


def test_count_file_through_the_pinned_ring(ctx, tmp_path):
    rng = random.Random(23)
    recs = [R.fasta(rng, 390000, cols=60, header=b">record %d of a generated file\n" % i) for i in range(4)]
    src = b"".join(recs)
    assert len(src) > 3 << 19
    path = tmp_path / "generated.fa"
    path.write_bytes(src)
    T, src_of = R.normalize(src, R.FASTA)
    pats = [T[100055:100075], _substituted(rng, T[389990:390065], 2), T[779990:780010]]     # lines of 60; the second spans two records
    assert src_of[390064] - src_of[389990] > 75 + 20
    k = 2
    want = H.oracle_counts(T, pats, k, banded=True)
    assert all(c >= 1 for c in want)
    try:
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        ctx.set_text_mode(R.FASTA)
        assert ctx.count_file(str(path)) == want
        assert ctx.stat("norm_src_bytes") == len(src) and ctx.stat("norm_kept_bytes") == len(T)
        ctx.set_text_mode(0)
        # the default did not move; no WHOLE window of the file holds the pattern that spans two records (what is left are
        # the reference's truncated tail windows, a few bytes each)
        assert ctx.count_file(str(path)) == H.oracle_counts(src, pats, k, banded=True)
        assert H.oracle_counts(src, [pats[1]], k, banded=True, j_end=len(src) - len(pats[1]) + 1) == [0]
    finally:
        ctx.set_text_mode(0)


def test_cli_fasta_prints_source_offsets(apm, chry):
    src, T, src_of, pats = chry
    p = pats[8]                                                              # 75 bytes, no substitution
    assert len(p) == 75
    pos = [src_of[j] for j in _positions(T, p, 0)]
    assert pos
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    r = subprocess.run([exe, "--gpus", "1", "--fasta", "--positions", "0", CHRY, p.decode()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Number of matches for pattern <%s>: %d\n" % (p.decode(), len(pos)) in r.stdout
    assert "Positions for pattern <%s>: %s\n" % (p.decode(), " ".join(str(x) for x in pos)) in r.stdout
    r = subprocess.run([exe, "--gpus", "1", "--positions", "0", CHRY, p.decode()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Number of matches for pattern <%s>: 0\n" % p.decode() in r.stdout
    assert "Positions for pattern <%s>:\n" % p.decode() in r.stdout


def test_multi_device_context_refuses_a_text_mode(apm):
    os.environ["APM_DEVICES"] = "0,0"
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    with m:
        for partition in ("text", "patterns"):
            m.set_partition(partition)
            with pytest.raises(apm.ApmError) as e:
                m.set_text_mode(R.FASTA)
            assert e.value.status == UNSUPPORTED
            m.set_text_mode(0)
