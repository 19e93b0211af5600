"""The scoring pass on the GPU: apm_find_all_dist_buffer and apm_score_shard_device write every record's edit distance,
capped at k + 1, into its fourth dword.  The truth everywhere is helpers.window_distance (the oracle pinned to the
reference's levenshtein()) over size = min(m, n - pos) bytes; every comparison is over the complete record set."""
import ctypes
import os
import random
import struct

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

INVALID = 0xFFFFFFFF
PRESET = 0x5A5A5A5A
UNSUPPORTED = -6
DNA = b"ACGT"


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


# ---------------------------------------------------------------- the reference: (pattern, pos, dist), computed once
def _positions(text, pat, k):
    """matching window starts by bisection over the oracle's range counts (its banded form -- exact for the predicate --
    where the band is a small part of the pattern)"""
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


def score(text, pat, pos, k):
    """what a scoring call writes for a window inside the text"""
    size = min(len(pat), len(text) - pos)
    return min(H.window_distance(pat[:size], text[pos:pos + size]), k + 1)


_ref_cache = {}


def ref_records(text, pats, k):
    key = (text, tuple(pats), k)
    if key not in _ref_cache:
        rec = [(i, j, score(text, p, j, k)) for i, p in enumerate(pats) for j in _positions(text, p, k)]
        assert all(d <= k for _, _, d in rec)
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


def dist_call(ctx, text, pats, k, want=None):
    """find_all_dist_buffer == the reference, record for record"""
    want = ref_records(text, pats, k) if want is None else want
    got, total = ctx.find_all_dist_buffer(text, len(want) + 64)
    assert total == len(want)
    assert got == want
    return want


# ---------------------------------------------------------------- 1. planted edits
LENS = (1, 4, 15, 16, 17, 31, 33, 64, 129, 513, 1025)
KS = (0, 1, 2, 3, 6, 7, 8, 9, 16)
_planted_cache = {}


def planted_case(k):
    if k not in _planted_cache:
        _planted_cache[k] = planted(k, LENS, 1000 + k)
    return _planted_cache[k]


def accepted(apm, ctx, pats, k, variant):
    """the patterns whose shape the forced variant accepts at k (the others: APM_ERR_UNSUPPORTED)"""
    keep = []
    for p in pats:
        ctx.set_kernel("auto")
        ctx.set_patterns([p], k)
        try:
            ctx.set_kernel(variant)
            keep.append(p)
        except apm.ApmError as e:
            assert e.status == UNSUPPORTED, e
    ctx.set_kernel("auto")
    return keep


@pytest.mark.parametrize("variant", ["auto", "banded", "nfa", "bitpar", "wavefront", "generic"])
@pytest.mark.parametrize("k", KS)
def test_planted_edits(apm, ctx, k, variant):
    pats, text = planted_case(k)
    full = ref_records(text, pats, k)
    if variant != "auto":
        sub = accepted(apm, ctx, pats, k, variant)
        if not sub:
            return  # (no shape of the list is this variant's at this k: nothing to run)
        index = [pats.index(p) for p in sub]
        want = [(index.index(i), j, d) for i, j, d in full if i in index]
        pats = sub
    else:
        want = full
        for i, p in enumerate(pats):
            mine = [d for q, _, d in want if q == i]
            if k >= len(p):                                          # every window matches
                assert len(mine) == len(text) - k
            elif len(p) >= 15:                                       # the copies at 0 .. k edits are among the matches
                assert min(mine) == 0 and (k == 0 or max(mine) >= 1)
    try:
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        ctx.set_kernel(variant)
        dist_call(ctx, text, pats, k, want)
    finally:
        ctx.set_kernel("auto")


def test_wave_form_with_more_than_64_cells(ctx):
    """m = 200, k = 130: 131 diagonals, three chunks of the wave form; random DNA is within 130 edits of nearly anything"""
    k = 130
    pats, text = planted(k, (200,), 77, edits=(0, 1, 2, 63, 64, 65, 66, 129, 130), gaps=2048)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    want = dist_call(ctx, text, pats, k)
    ds = [d for _, _, d in want]
    assert min(ds) == 0 and max(ds) > 64 and len(want) > len(text) // 2


def test_k_at_least_m_every_window_matches(ctx):
    rng = random.Random(5)
    text = rand(rng, 3000)
    for k, lens in ((3, (1, 2, 3)), (9, (3, 5, 8, 9)), (16, (16, 7))):     # lane form and wave form
        pats = [rand(rng, m) for m in lens]
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        want = dist_call(ctx, text, pats, k)
        assert len(want) == len(pats) * (len(text) - k)
        assert len({d for _, _, d in want}) >= 2


# ---------------------------------------------------------------- 2. truncated tails
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
        want = dist_call(ctx, text, pats, k)
        tails = [(i, j, d) for i, j, d in want if j + len(pats[i]) > len(text)]
        if cut > k:                                                    # (window starts end at n - k)
            assert (pats.index(p), 2000, 0) in tails


@pytest.mark.parametrize("k", [0, 1, 3, 9])
def test_text_shorter_than_the_patterns(ctx, k):
    rng = random.Random(50 + k)
    pats = [rand(rng, m) for m in (20, 31, 64, 200)] + [b"A", b"AC"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    for text in (pats[0][:15], pats[2][:18] + b"T", b"A", b"C", rand(rng, 19)):   # n < m, and a one-byte text
        want = dist_call(ctx, text, pats, k)
        assert len(want) <= len(pats) * max(0, len(text) - k)
        if text == pats[0][:15]:
            assert (0, 0, 0) in want                                    # the whole text is a truncated copy
        if text == b"A" and k == 0:
            assert (4, 0, 0) in want and (5, 0, 0) in want


def test_golden_cfg1_basic_test(ctx):
    c = next(c for c in H.golden()["cases"] if c["name"] == "cfg1_basic_test")
    text, pats, k = H.case_text(c), c["patterns"], c["k"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    want = dist_call(ctx, text, pats, k)
    assert [sum(1 for i, _, _ in want if i == q) for q in range(len(pats))] == c["counts"]


# ---------------------------------------------------------------- 3. low entropy
def test_low_entropy_every_lane_busy(ctx):
    k = 3
    text = b"A" * 4096
    pats = [b"A" * 20, b"A" * 19 + b"C"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    want = [(i, j, score(text, p, j, k)) for i, p in enumerate(pats) for j in range(len(text) - k)]
    assert all(d == 0 for i, _, d in want if i == 0)
    assert all(d == (1 if j + 20 <= len(text) else 0) for i, j, d in want if i == 1)   # the tail windows lose the C
    got, total = ctx.find_all_dist_buffer(text, len(want) + 8)
    assert total == len(want) and got == want


# ---------------------------------------------------------------- 4. foreign records
def _records(rows):
    return b"".join(struct.pack("<QII", pos, pat, PRESET) for pat, pos in rows)


def _unpack(raw):
    return [struct.unpack_from("<QII", raw, 16 * i) for i in range(len(raw) // 16)]


@pytest.mark.parametrize("k", [3, 9])
def test_foreign_records_through_score_shard_device(ctx, k):
    """hand-made records, the fourth dword preset: matches inside the shard, windows farther than k (k + 1), windows that
    cross the shard's ends (untouched), records that name no window (APM_DIST_INVALID); pos and pattern stay as they are"""
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
            (2, 1100), (1, 1234), (0, 2001),                             # inside, random windows: farther than k -> k + 1
            (0, 2977), (1, 2961), (2, 2999), (0, 999), (2, 0), (1, 3000), (0, n - 10),   # cross an end of the shard: untouched
            (3, 1500), (0xFFFFFFFF, 1500), (0, n), (1, 1 << 40)]         # pattern == n_patterns, pos == n_total: invalid
    want = []
    for pat, pos in rows:
        if pat >= len(pats) or pos >= n:
            want.append(INVALID)
        elif pos < off or pos + min(len(pats[pat]), n - pos) > off + length:
            want.append(PRESET)
        else:
            want.append(score(text, pats[pat], pos, k))
    assert want[0] == 0 and 1 <= want[1] <= 2 and want[2] <= k and want.count(k + 1) >= 3 and want.count(PRESET) == 7 and want.count(INVALID) == 4
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    d_text, d_rec, d_n = ctx.device_alloc(length + 16), ctx.device_alloc(16 * (len(rows) + 8)), ctx.device_alloc(16)
    try:
        ctx.device_upload(d_text, text[off:off + length])
        ctx.device_upload(d_rec, _records(rows))
        ctx.device_upload(d_n, struct.pack("<Q", len(rows)))
        ctx.score_shard_device(d_text, off, length, n, d_rec, len(rows), d_n)
        ctx.synchronize()
        got = _unpack(ctx.device_download(d_rec, 16 * len(rows)))
        assert [(pat, pos) for pos, pat, _ in got] == rows               # bit-identical
        assert [d for _, _, d in got] == want
        # *d_n_rec beyond capacity: `capacity` records are scored, the records behind them keep every bit
        cap = 6
        ctx.device_upload(d_rec, _records(rows[:cap + 4]))
        ctx.device_upload(d_n, struct.pack("<Q", cap + 4))
        ctx.score_shard_device(d_text, off, length, n, d_rec, cap, d_n)
        ctx.synchronize()
        got = _unpack(ctx.device_download(d_rec, 16 * (cap + 4)))
        assert [(pat, pos) for pos, pat, _ in got] == rows[:cap + 4]
        assert [d for _, _, d in got] == want[:cap] + [PRESET] * 4
    finally:
        for d in (d_text, d_rec, d_n):
            ctx.device_free(d)


# ---------------------------------------------------------------- 5. two shards, one buffer
def _shard_text(ctx, text, lo, hi, mis):
    d = ctx.device_alloc(hi - lo + 32)
    ctx.device_upload(d + mis, text[lo:hi])
    return d


@pytest.mark.parametrize("k,mis", [(3, 0), (3, 1), (3, 7), (3, 15), (9, 4), (9, 15)])
def test_two_shards_one_buffer(apm, ctx, k, mis):
    """find on both shards, then score against shard 1's text, then against shard 2's, all on one stream without a
    synchronisation in between: every record ends with its distance, whichever shard holds its window"""
    pats, text = planted(k, (16, 33, 64, 129), 70 + k)
    n = len(text)
    want = ref_records(text, pats, k)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    halo = max(len(p) for p in pats) - 1
    cut = (n // 2) | 5
    shards = [(0, cut, 0, min(n, cut + halo)), (cut, n, cut, n)]         # (own begin, own end, text begin, text end)
    cap = len(want) + 16
    d_rec, d_n = ctx.device_alloc(16 * cap), ctx.device_alloc(16)
    bufs = [_shard_text(ctx, text, lo, hi, mis) for _, _, lo, hi in shards]
    try:
        ctx.device_memset(d_n, 0, 16)
        ctx.synchronize()
        for (ob, oe, lo, hi), d in zip(shards, bufs):
            ctx.find_shard_device(d + mis, lo, hi - lo, n, ob, oe, d_rec, cap, d_n, None)
        for (ob, oe, lo, hi), d in zip(shards, bufs):
            ctx.score_shard_device(d + mis, lo, hi - lo, n, d_rec, cap, d_n)
        ctx.synchronize()
        total = struct.unpack("<Q", ctx.device_download(d_n, 8))[0]
        assert total == len(want)
        got = sorted((pat, pos, d) for pos, pat, d in _unpack(ctx.device_download(d_rec, 16 * total)))
        assert got == want
        assert any(j < cut for _, j, _ in want) and any(j >= cut for _, j, _ in want)
    finally:
        for d in bufs + [d_rec, d_n]:
            ctx.device_free(d)


@pytest.mark.parametrize("k", [3, 9])
def test_shard_beyond_8gib_has_64_bit_positions(ctx, k):
    pats, text = planted(k, (17, 64, 31), 80 + k, gaps=2048)
    n = len(text)
    base = (1 << 33) + 5
    want = [(i, j + base, d) for i, j, d in ref_records(text, pats, k)]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    cap = len(want) + 8
    d_text, d_rec, d_n = _shard_text(ctx, text, 0, n, 0), ctx.device_alloc(16 * cap), ctx.device_alloc(16)
    try:
        ctx.device_memset(d_n, 0, 16)
        ctx.find_shard_device(d_text, base, n, base + n, base, base + n, d_rec, cap, d_n, None)
        ctx.score_shard_device(d_text, base, n, base + n, d_rec, cap, d_n)
        ctx.synchronize()
        total = struct.unpack("<Q", ctx.device_download(d_n, 8))[0]
        got = sorted((pat, pos, d) for pos, pat, d in _unpack(ctx.device_download(d_rec, 16 * total)))
        assert got == want and all(pos > 1 << 33 for _, pos, _ in got)
    finally:
        for d in (d_text, d_rec, d_n):
            ctx.device_free(d)


# ---------------------------------------------------------------- 6. multi-device contexts, rehearsed on one GPU
def _mixed(k, lens, n, seed):
    """the mixed set of test_find_all.py's test_multi_device_records_equal_single_device"""
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


@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
@pytest.mark.parametrize("partition", ["text", "patterns"])
def test_multi_device_distances_equal_single_device(apm, ctx, devices, partition):
    k = 3
    pats, text = _mixed(k, (20, 300, 13, 700, 1500), 50000, 8)
    pats.append(pats[0])
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    single = dist_call(ctx, text, pats, k)
    assert {d for _, _, d in single} >= {0, 1}
    os.environ["APM_DEVICES"] = devices
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    with m:
        m.set_partition(partition)
        m.set_patterns(pats, k)
        got, total = m.find_all_dist_buffer(text, 4096)
        assert total == len(single) and got == single
        assert m.find_all_buffer(text, 4096)[0] == [(i, j) for i, j, _ in single]


# ---------------------------------------------------------------- 7. nothing else moved
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
    scored, total_d = _raw_find_all(apm, ctx, text, cap, True)
    t_dist, l_dist = ctx.timing(), [l for l, _ in ctx.launch_times()]
    assert total_d == total == sum(before[0])
    assert [(i, j) for i, j, _ in scored] == [(i, j) for i, j, _ in plain]
    assert [d for _, _, d in scored] == [score(text, pats[i], j, k) for i, j, _ in scored]
    assert any(d for _, _, d in scored) and all(r == 0 for _, _, r in plain)
    assert l_dist.count("score") == 1 and l_dist[-1] == "score" and "score" not in l_find and l_dist[:-1] == l_find
    assert t_dist["n_launches"] == t_find["n_launches"] + 1 and t_dist["kernel_ms"] > 0
    assert state() == before
    # the context's record buffer is reused: the plain call behind a scoring one reports reserved == 0 again
    again, _ = _raw_find_all(apm, ctx, text, cap, False)
    assert again == plain and all(r == 0 for _, _, r in again)


# ---------------------------------------------------------------- 8. the band the wave form serves
def test_band_limit(apm, ctx):
    """half-band min(k/2, m_max - 1) = 2048 is served; 2049 is refused by both scoring calls, the plain calls go on.
    m = 2049 is the shortest pattern that reaches the limit (k/2 = 2048 <= m - 1); k >= m: every window matches."""
    rng = random.Random(9)
    m, k = 2049, 4096
    text = rand(rng, k + 24)
    pats = [rand(rng, m)]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    want = [(0, j, score(text, pats[0], j, k)) for j in range(len(text) - k)]
    assert len(want) == 24 and all(k // 8 < d <= m for _, _, d in want)
    got, total = ctx.find_all_dist_buffer(text, 64)
    assert total == 24 and got == want
    m, k = 2050, 4098
    text = rand(rng, k + 24)
    ctx.set_patterns([rand(rng, m)], k)
    with pytest.raises(apm.ApmError) as e:
        ctx.find_all_dist_buffer(text, 64)
    assert e.value.status == UNSUPPORTED and "2048" in str(e.value)
    d_text, d_rec, d_n = _shard_text(ctx, text, 0, len(text), 0), ctx.device_alloc(64), ctx.device_alloc(16)
    try:
        ctx.device_upload(d_rec, _records([(0, 0)]))
        ctx.device_upload(d_n, struct.pack("<Q", 1))
        with pytest.raises(apm.ApmError) as e:
            ctx.score_shard_device(d_text, 0, len(text), len(text), d_rec, 1, d_n)
        assert e.value.status == UNSUPPORTED
        ctx.synchronize()
        assert _unpack(ctx.device_download(d_rec, 16)) == [(0, 0, PRESET)]
    finally:
        for d in (d_text, d_rec, d_n):
            ctx.device_free(d)
    got, total = ctx.find_all_buffer(text, 64)
    assert total == 24 and got == [(0, j) for j in range(24)]
