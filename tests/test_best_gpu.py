"""The best-hit pass on the GPU: apm_best_shard_device and apm_find_best_buffer keep, of the records a find call reports,
exactly the best hits of include/apm.h's rule, scored.  The truth everywhere is tests/best_ref.py: the complete scored
record set from the oracle, the rule applied literally over it."""
import json
import os
import random
import struct
import subprocess

import pytest

import best_ref as B
import helpers as H

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -6
LENS = (16, 23, 40, 130)
GUARD = b"\xa5" * 16


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
        d = self.alloc(hi - lo + 32)
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


def pack(seeds):
    """records with garbage in the fourth dword: the pass ignores it"""
    return b"".join(struct.pack("<QII", pos, pat, 0xDEAD0000 + q) for q, (pat, pos) in enumerate(seeds))


def unpack(raw):
    return [(pat, pos, d) for pos, pat, d in (struct.unpack_from("<QII", raw, 16 * i) for i in range(len(raw) // 16))]


def best_call(ctx, dev, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, r, out_cap, d_out=None, d_n_out=None):
    """one best-hit launch into a fresh (or the given) guarded out buffer; (records written sorted, *d_n_out, d_out)"""
    if d_out is None:
        d_out = dev.alloc(16 * (out_cap + 4), GUARD * (out_cap + 4))
        d_n_out = dev.counter()
    ctx.best_shard_device(d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, r, d_out, out_cap, d_n_out)
    ctx.synchronize()
    n_out = struct.unpack("<Q", ctx.device_download(d_n_out, 8))[0]
    raw = ctx.device_download(d_out, 16 * (out_cap + 4))
    assert raw[16 * out_cap:] == GUARD * 4, "records behind out_capacity were written"
    assert raw[16 * min(n_out, out_cap):16 * out_cap] == GUARD * (out_cap - min(n_out, out_cap)), "records beyond *d_n_out were written"
    return sorted(unpack(raw[:16 * min(n_out, out_cap)])), n_out, d_out


def check_seeds(ctx, text, pats, k, seeds, radii, want_seeds=None):
    """the pass over made-up records `seeds` against the whole text == the rule over them"""
    n = len(text)
    with Dev(ctx) as dev:
        d_text = dev.text(text)
        d_rec, d_n = dev.alloc(16 * len(seeds), pack(seeds)), dev.counter(len(seeds))
        out = {}
        for r in radii:
            want = B.best_hits(text, pats, k, r, seeds if want_seeds is None else want_seeds)
            got, n_out, _ = best_call(ctx, dev, d_text, 0, n, n, d_rec, len(seeds), d_n, r, len(seeds) + 1)
            assert got == want, (k, r)
            assert n_out == len(want)
            out[r] = want
        assert ctx.device_download(d_rec, 16 * len(seeds)) == pack(seeds)          # the records are only read
    return out


def all_records(text, pats, k):
    return [(i, j) for i, j, _ in B.ref_records(text, pats, k)]


def setup(ctx, pats, k):
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)


# ---------------------------------------------------------------- 1. planted texts, behind the find call on one stream
_planted = {}


def planted_case(k):
    if k not in _planted:
        _planted[k] = B.planted(k, LENS, 3000 + k, gaps=3072 if k >= 8 else 4096)
    return _planted[k]


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 7, 8, 12])
def test_planted(ctx, k):
    """BAND 0..3 of the lane form and the wave form; r = 31, 32, 64: one, two and three rounds of the lane form"""
    pats, text = planted_case(k)
    n = len(text)
    assert n <= 8192
    full = B.ref_records(text, pats, k)
    setup(ctx, pats, k)
    cap = len(full) + 8
    sizes = {}
    with Dev(ctx) as dev:
        d_text, d_rec, d_n = dev.text(text), dev.alloc(16 * cap), dev.counter()
        ctx.find_shard_device(d_text, 0, n, n, 0, n, d_rec, cap, d_n, None)
        for r in sorted({0, 1, k // 2, k, 31, 32, 64}):
            want = B.best_hits(text, pats, k, r)
            got, n_out, _ = best_call(ctx, dev, d_text, 0, n, n, d_rec, cap, d_n, r, cap)   # (behind the find call: no synchronisation between)
            assert got == want, (k, r)
            assert n_out == len(want)
            sizes[r] = len(want)
        assert struct.unpack("<Q", ctx.device_download(d_n, 8))[0] == len(full)
    assert sizes[0] == len(full)                                          # r = 0 keeps exactly the records within k
    assert sizes[64] <= sizes[1] <= sizes[0] and sizes[64] >= len(pats)
    if k >= 2:
        assert sizes[1] < sizes[0]                                        # an occurrence leaves a run of records


# ---------------------------------------------------------------- 2. edges
@pytest.mark.parametrize("k", [3, 9])
def test_edges_of_the_text(ctx, k):
    """records at pos < r, records within r of n_total - k, truncated tail windows (size < m)"""
    rng = random.Random(20 + k)
    pats = [B.rand(rng, m) for m in (24, 40, 70)]
    body = B.rand(rng, 600)
    text = bytearray(B.edited(rng, pats[0], 1) + B.rand(rng, 3) + pats[1] + body)
    text += B.edited(rng, pats[1], 2)                                      # a copy that ends with the text: its neighbours' windows are truncated
    text += pats[2][:50]                                                   # a truncated copy of the longest pattern
    text = bytes(text)
    n = len(text)
    setup(ctx, pats, k)
    seeds = all_records(text, pats, k)
    assert any(j < 5 for _, j in seeds) and any(j + len(pats[i]) > n for i, j in seeds) and any(n - k - j <= 5 for _, j in seeds)
    seeds += [(i, j) for i in range(3) for j in range(n - k, n)]         # starts beyond W: decided, but they suppress nobody
    kept = check_seeds(ctx, text, pats, k, seeds, (0, 1, 5, 64))
    assert any(j >= n - k for _, j, _ in kept[0]) and (2, n - 50, 0) in kept[1]


@pytest.mark.parametrize("k", [3, 9])
def test_empty_w_and_k_at_least_m(ctx, k):
    rng = random.Random(30 + k)
    # n_total <= k: W is empty, every start is within k (size <= n <= k) and nothing suppresses
    pats = [B.rand(rng, 20), B.rand(rng, 2)]
    text = B.rand(rng, k)
    setup(ctx, pats, k)
    seeds = [(i, j) for i in range(2) for j in range(k)]
    kept = check_seeds(ctx, text, pats, k, seeds, (0, 1, 64))
    assert len(kept[64]) == len(seeds)
    # k >= m: every window matches; the distances make plateaus
    pats = [B.rand(rng, k), B.rand(rng, 2), B.rand(rng, 30)]
    text = B.rand(rng, 700)
    setup(ctx, pats, k)
    seeds = all_records(text, pats, k)
    assert sum(1 for i, _ in seeds if i == 0) == len(text) - k
    kept = check_seeds(ctx, text, pats, k, seeds, (0, 1, k, 64))
    assert 0 < len(kept[64]) < len(kept[1]) < len(seeds)


# ---------------------------------------------------------------- 3. ties and volume
def test_poly_a_keeps_the_first_start(ctx):
    k, text, pats = 2, b"A" * 6144, [b"A" * 16]
    setup(ctx, pats, k)
    seeds = all_records(text, pats, k)
    assert len(seeds) == 6142
    kept = check_seeds(ctx, text, pats, k, seeds, (1, 64))
    assert kept[1] == kept[64] == [(0, 0, 0)]


def test_acg_tandem_chains(ctx):
    k, text, pats = 3, b"ACG" * 80, [b"ACG" * 6]
    setup(ctx, pats, k)
    seeds = all_records(text, pats, k)
    assert len(seeds) == 237
    kept = check_seeds(ctx, text, pats, k, seeds, (1, 2, 3, 64))
    assert [len(kept[r]) for r in (1, 2, 3, 64)] == [79, 79, 1, 1]


def test_wave_form_grid_stride(ctx):
    """more records than the wave form's grid has workgroups: every start of a 2 KiB poly-A, two patterns, k = 8"""
    k, text, pats = 8, b"A" * 2048, [b"A" * 16, b"A" * 20, b"A" * 19 + b"C"]
    setup(ctx, pats, k)
    seeds = all_records(text, pats, k)
    assert len(seeds) == 3 * 2040
    kept = check_seeds(ctx, text, pats, k, seeds, (1, 8))
    assert kept[8] == [(0, 0, 0), (1, 0, 0), (2, 0, 1), (2, 2048 - 19, 0)]   # (the tail windows lose the C)


# ---------------------------------------------------------------- 4. independence from the set
@pytest.mark.parametrize("k", [3, 8])
def test_independent_of_the_record_set(ctx, k):
    pats, text = planted_case(k)
    n = len(text)
    setup(ctx, pats, k)
    rng = random.Random(40 + k)
    full = all_records(text, pats, k)
    radii = (1, k, 64)
    whole = {r: B.best_hits(text, pats, k, r) for r in radii}
    shuffled = full[:]
    rng.shuffle(shuffled)
    assert check_seeds(ctx, text, pats, k, shuffled, radii) == whole
    half = rng.sample(full, len(full) // 2)
    kept = check_seeds(ctx, text, pats, k, half, radii)
    for r in radii:                                                       # the half's best hits are the whole set's, as far as they are in it
        assert kept[r] == [h for h in whole[r] if (h[0], h[1]) in set(half)]
    twice = full + full[::3]
    kept = check_seeds(ctx, text, pats, k, twice, radii)
    assert len(kept[1]) > len(whole[1]) and set(kept[1]) == set(whole[1])  # a duplicate is kept as often as it comes
    records = set(full)
    made_up = [(i, j) for i in range(len(pats)) for j in rng.sample(range(n), 40) if (i, j) not in records and B.score(text, pats[i], j, k) > k]
    assert len(made_up) > 60
    bad = [(len(pats), 100), (0xFFFFFFFF, 5), (0, n), (1, n + 7), (2, 1 << 40)]
    kept = check_seeds(ctx, text, pats, k, full + made_up + bad, radii)
    assert kept == whole                                                   # non-matches and records that name no window are dropped


# ---------------------------------------------------------------- 5. capacity limits
def test_capacity_limits(ctx):
    k, r = 3, 3
    pats, text = planted_case(k)
    n = len(text)
    setup(ctx, pats, k)
    full = all_records(text, pats, k)
    want = B.best_hits(text, pats, k, r)
    with Dev(ctx) as dev:
        d_text = dev.text(text)
        d_rec, d_n = dev.alloc(16 * len(full), pack(full)), dev.counter(len(full))
        got, n_out, _ = best_call(ctx, dev, d_text, 0, n, n, d_rec, len(full), d_n, r, len(want) - 3)
        assert n_out == len(want)                                         # exact beyond out_capacity
        assert len(got) == len(set(got)) == len(want) - 3 and set(got) <= set(want)
        # *d_n_rec > capacity: the first `capacity` records are decided
        cap = len(full) // 2
        d_n_big = dev.counter(len(full) + 10)
        got, n_out, _ = best_call(ctx, dev, d_text, 0, n, n, d_rec, cap, d_n_big, r, len(want))
        assert got == B.best_hits(text, pats, k, r, full[:cap]) and n_out == len(got)
        # out_capacity 0 with no buffer at all: a count
        d_n_out = dev.counter()
        ctx.best_shard_device(d_text, 0, n, n, d_rec, len(full), d_n, r, None, 0, d_n_out)
        ctx.synchronize()
        assert struct.unpack("<Q", ctx.device_download(d_n_out, 8))[0] == len(want)


def test_bad_arguments(apm, ctx):
    k = 3
    pats, text = planted_case(k)
    n = len(text)
    setup(ctx, pats, k)
    with Dev(ctx) as dev:
        d_text, d_rec, d_n, d_out, d_n_out = dev.text(text), dev.alloc(16 * 8, pack([(0, 0)] * 8)), dev.counter(8), dev.alloc(16 * 8), dev.counter()
        for args in ((65, d_out, 8, d_n_out), (1, d_out + 8, 4, d_n_out), (1, None, 8, d_n_out), (1, d_out, 8, None), (1, d_rec + 16, 4, d_n_out)):
            with pytest.raises(apm.ApmError) as e:
                ctx.best_shard_device(d_text, 0, n, n, d_rec, 8, d_n, *args)
            assert e.value.status == INVALID, args
        ctx.synchronize()
        assert struct.unpack("<Q", ctx.device_download(d_n_out, 8))[0] == 0


# ---------------------------------------------------------------- 6. shards
@pytest.mark.parametrize("k,mis", [(3, 1), (3, 15), (8, 1), (8, 15)])
def test_misaligned_text_and_uncovered_records(ctx, k, mis):
    """d_text at byte 1 and 15 of an allocation; text_off > 0: the records whose neighbourhood the shard does not cover
    are skipped, the others decided as on the whole text"""
    pats, text = planted_case(k)
    n, r = len(text), 5
    setup(ctx, pats, k)
    full = all_records(text, pats, k)
    by_pos = sorted(full, key=lambda rec: rec[1])
    first = next(rec for rec in by_pos if rec[1] >= n // 3)                # the shard starts 2 bytes in front of this record's window
    last = next(rec for rec in reversed(by_pos) if rec[1] + len(pats[rec[0]]) <= n - n // 4)   # ... and ends 2 bytes behind this one's
    lo, hi = first[1] - 2, last[1] + len(pats[last[0]]) + 2
    covered = [(i, j) for i, j in full if max(j, r) - r >= lo and min(n, j + r + len(pats[i])) <= hi]
    assert 0 < len(covered) < len(full)
    assert any(lo <= j and j + len(pats[i]) <= hi for i, j in set(full) - set(covered))   # window inside, neighbourhood not
    with Dev(ctx) as dev:
        d_rec, d_n = dev.alloc(16 * len(full), pack(full)), dev.counter(len(full))
        got, n_out, _ = best_call(ctx, dev, dev.text(text, lo, hi, mis), lo, hi - lo, n, d_rec, len(full), d_n, r, len(full))
        assert got == B.best_hits(text, pats, k, r, covered) and n_out == len(got)
        got, n_out, _ = best_call(ctx, dev, dev.text(text, 0, n, mis), 0, n, n, d_rec, len(full), d_n, r, len(full))
        assert got == B.best_hits(text, pats, k, r) and n_out == len(got)


@pytest.mark.parametrize("k,r", [(3, 3), (3, 64), (8, 8)])
def test_two_shards_one_buffer(ctx, k, r):
    """each shard finds its own starts and decides them against its text, with r bytes of halo in front and
    r + m_max - 1 behind; both append to one buffer: the truth, each record once"""
    pats, text = planted_case(k)
    n = len(text)
    setup(ctx, pats, k)
    want = B.best_hits(text, pats, k, r)
    m_max = max(len(p) for p in pats)
    cut = (n // 2) | 5
    shards = [(0, cut, 0, min(n, cut + r + m_max - 1)), (cut, n, max(0, cut - r), n)]   # (own begin, own end, text begin, text end)
    cap = len(B.ref_records(text, pats, k)) + 8
    with Dev(ctx) as dev:
        d_out, d_n_out = dev.alloc(16 * (cap + 4), GUARD * (cap + 4)), dev.counter()
        for ob, oe, lo, hi in shards:
            d_text, d_rec, d_n = dev.text(text, lo, hi, 3), dev.alloc(16 * cap), dev.counter()
            ctx.find_shard_device(d_text, lo, hi - lo, n, ob, oe, d_rec, cap, d_n, None)
            got, n_out, _ = best_call(ctx, dev, d_text, lo, hi - lo, n, d_rec, cap, d_n, r, cap, d_out, d_n_out)
        assert got == want and n_out == len(want)
        assert any(j < cut for _, j, _ in want) and any(j >= cut for _, j, _ in want)


# ---------------------------------------------------------------- 7. stream order: find -> best -> align, one synchronisation
@pytest.mark.parametrize("k", [3, 8])
def test_find_best_align_on_one_stream(apm, ctx, k):
    pats, text = planted_case(k)
    n, r = len(text), k
    setup(ctx, pats, k)
    want = B.best_hits(text, pats, k, r)
    every, _ = ctx.find_all_align_buffer(text, len(B.ref_records(text, pats, k)) + 8)
    script = {(i, j): (d, ops) for i, j, d, ops in every}
    stride, cap = ctx.align_row_words(), len(every) + 8
    with Dev(ctx) as dev:
        d_text, d_rec, d_n = dev.text(text), dev.alloc(16 * cap), dev.counter()
        d_out, d_n_out, d_ops = dev.alloc(16 * cap), dev.counter(), dev.alloc(4 * stride * cap)
        ctx.find_shard_device(d_text, 0, n, n, 0, n, d_rec, cap, d_n, None)
        ctx.best_shard_device(d_text, 0, n, n, d_rec, cap, d_n, r, d_out, cap, d_n_out)
        ctx.align_shard_device(d_text, 0, n, n, d_out, cap, d_n_out, d_ops, stride)
        ctx.synchronize()
        n_out = struct.unpack("<Q", ctx.device_download(d_n_out, 8))[0]
        assert n_out == len(want)
        rec = unpack(ctx.device_download(d_out, 16 * n_out))
        rows = struct.unpack("<%dI" % (stride * n_out), ctx.device_download(d_ops, 4 * stride * n_out))
        got = sorted((i, j, d, apm.unpack_ops(rows[q * stride:(q + 1) * stride])) for q, (i, j, d) in enumerate(rec))
        assert got == [(i, j, d, script[(i, j)][1]) for i, j, d in want]
        assert all(script[(i, j)][0] == d for i, j, d in want)


# ---------------------------------------------------------------- 8. host level
@pytest.mark.parametrize("k", [3, 8])
def test_find_best_buffer(apm, ctx, k):
    pats, text = planted_case(k)
    setup(ctx, pats, k)
    full = B.ref_records(text, pats, k)
    before = ctx.count_buffer(text)
    assert sum(before) == len(full)
    plain, _ = ctx.find_all_buffer(text, len(full) + 8)
    l_find = [l for l, _ in ctx.launch_times()]
    every, _ = ctx.find_all_align_buffer(text, len(full) + 8)
    script = {(i, j): ops for i, j, _, ops in every}
    for r in (0, 1, k, 64):
        want = B.best_hits(text, pats, k, r)
        got, n_best, n_matches = ctx.find_best_buffer(text, r, len(full) + 8)
        labels = [l for l, _ in ctx.launch_times()]
        assert got == want and n_best == len(want) and n_matches == len(full) == sum(before)
        assert labels == l_find + ["best"] and "score" not in labels       # the scan's launches, then one more
        assert ctx.stat("best_ms") > 0
        got, n_best, n_matches = ctx.find_best_buffer(text, r, len(full) + 8, align=True)
        assert [l for l, _ in ctx.launch_times()] == l_find + ["best", "align"]
        assert got == [(i, j, d, script[(i, j)]) for i, j, d in want] and n_best == len(want) and n_matches == len(full)
    assert ctx.count_buffer(text) == before
    assert ctx.find_all_buffer(text, len(full) + 8)[0] == plain
    # capacity < n_matches: APM_OK, the exact total, a subset of the true best hits
    want = B.best_hits(text, pats, k, 1)
    got, n_best, n_matches = ctx.find_best_buffer(text, 1, len(full) // 2)
    assert n_matches == len(full) and n_best == len(got) and set(got) <= set(want) and got == sorted(set(got))
    # capacity 0: the totals
    assert ctx.find_best_buffer(text, 1, 0) == ([], 0, len(full))
    with pytest.raises(apm.ApmError) as e:
        ctx.find_best_buffer(text, 65, 64)
    assert e.value.status == INVALID
    assert ctx.count_buffer(text) == before


def _fixture():
    with open(os.path.join(H.GOLDEN_DIR, "best_small.json")) as f:
        c = json.load(f)
    with open(os.path.join(H.GOLDEN_DIR, "best_small.fa"), "rb") as f:
        src = f.read()
    return src, [p.encode() for p in c["patterns"]], c["k"]


def test_find_best_buffer_in_a_text_mode(apm, ctx):
    """the pass runs on the normalised text; the positions are source offsets and apm_locate_buffer takes them"""
    src, pats, k = _fixture()
    T, src_of, seq_of, names = B.normalise(src)
    assert len(T) < len(src) and T != src.upper() and len(names) == 3
    setup(ctx, pats, k)
    ctx.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
    try:
        for r in (1, 3):
            want = B.best_hits(T, pats, k, r)
            got, n_best, n_matches = ctx.find_best_buffer(src, r, 4096)
            assert got == [(i, src_of[j], d) for i, j, d in want] and n_best == len(want)
            assert n_matches == len(B.ref_records(T, pats, k))
            assert [l for l, _ in ctx.launch_times()][-1] == "best"
            locs = ctx.locate(got)
            first = {s: seq_of.index(s) for s in set(seq_of)}
            assert [(off, seq) for off, seq, _ in locs] == [(j - first[seq_of[j]], seq_of[j]) for _, j, _ in want]
    finally:
        ctx.set_text_mode(0)


@pytest.mark.parametrize("partition", ["text", "patterns"])
def test_multi_device_context_is_unsupported(apm, partition):
    pats, text = planted_case(3)
    os.environ["APM_DEVICES"] = "0,0"
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    with m:
        m.set_partition(partition)
        m.set_patterns(pats, 3)
        with pytest.raises(apm.ApmError) as e:
            m.find_best_buffer(text, 3, 4096)
        assert e.value.status == UNSUPPORTED
        assert m.find_all_buffer(text, 4096)[1] == len(B.ref_records(text, pats, 3))


# ---------------------------------------------------------------- 9. the CLI
def _positions(out, pats):
    """{pattern index: [item]} of the "Positions for pattern" lines"""
    got = {}
    for q, p in enumerate(pats):
        line = next(l for l in out.splitlines() if l.startswith("Positions for pattern <%s>:" % p.decode()))
        got[q] = line.split(":", 1)[1].split()
    return got


def _apply(script, pat):
    """(window the script turns the pattern into, '?' for text-only bytes; ops that are not '=')"""
    out, y, cost, num = [], 0, 0, ""
    for c in script:
        if c.isdigit():
            num += c
            continue
        for _ in range(int(num)):
            if c in "=XD":
                out.append(pat[y:y + 1] if c == "=" else (b"?" if c == "X" else b""))
                y += 1
            else:
                out.append(b"?")
            cost += c != "="
        num = ""
    assert y == len(pat)
    return b"".join(out), cost


def test_cli_best(tmp_path):
    src, pats, k = _fixture()
    T, src_of, seq_of, names = B.normalise(src)
    path = os.path.join(H.GOLDEN_DIR, "best_small.fa")
    exe = os.path.join(H.PKG_DIR, "host", "apm_parallel")
    base = [exe, "--gpus", "1", "--fasta", "--upper", str(k), path] + [p.decode() for p in pats]

    def run(*flags):
        r = subprocess.run(base + list(flags), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    count_lines = lambda out: [l for l in out.splitlines() if l.startswith("Number of matches")]
    plain = run("--distances")
    full = B.ref_records(T, pats, k)
    assert count_lines(plain) == ["Number of matches for pattern <%s>: %d" % (p.decode(), sum(1 for i, _, _ in full if i == q)) for q, p in enumerate(pats)]
    for flag, r in (("--best", k), ("--best=1", 1), ("--best=0", 0)):
        out = run(flag)
        assert count_lines(out) == count_lines(plain)                      # not thinned
        want = B.best_hits(T, pats, k, r)
        assert _positions(out, pats) == {q: ["%d:%d" % (src_of[j], d) for i, j, d in want if i == q] for q in range(len(pats))}
    assert _positions(run("--best=0"), pats) == _positions(plain, pats)
    out = run("--best", "--alignments", "--sequences")
    assert count_lines(out) == count_lines(plain)
    want = B.best_hits(T, pats, k, k)
    first = {s: seq_of.index(s) for s in set(seq_of)}
    got = _positions(out, pats)
    for q, p in enumerate(pats):
        inside = [(j, d) for i, j, d in want if i == q and j + len(p) <= len(T) and seq_of[j + len(p) - 1] == seq_of[j]]
        assert inside and len(got[q]) == len(inside)
        for item, (j, d) in zip(got[q], inside):
            name, off, dist, script = item.split(":")
            assert (name, int(off), int(dist)) == (names[seq_of[j]], j - first[seq_of[j]], d)
            window, cost = _apply(script, p)
            assert cost == d and len(window) == len(p)
            assert all(w == 63 or w == t for w, t in zip(window, T[j:j + len(p)]))
    for bad in ("--best=65", "--best=x", "--best=", "--best=-1"):
        r = subprocess.run(base + [bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--best" in r.stderr
