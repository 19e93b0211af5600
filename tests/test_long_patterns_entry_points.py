"""GPU (-m gpu): patterns of 129 .. 5000 bytes through EVERY entry point of the library, against the CPU oracle.

The engine has five kernel families beyond 128 bytes, each with truncated-window code of its own:

  A  129 ..  512   8 / 16-word columns (apm_bitpar_wide.hip), tails: apm_launch_tail_wide
  B  513 .. 1024   24 / 32-word one-pass columns (apm_bitpar_xwide_kernel), tails: apm_launch_tail_xwide
  C 1025 .. 2048   apm_bitlong_kernel<uint32_t>, one window per wave, truncated windows in the same kernel
  D 2049 .. 4096   apm_bitlong_kernel<uint64_t>
  E  > 4096, or 1025 .. 4096 over an alphabet whose Eq rows exceed 60 KiB of LDS: GENERIC

test_gpu_parity.py checks them through count_buffer only (aligned text, owner range from 0, one device).  Here every
class goes through owner shards cut at odd offsets with the device text at every residue mod 16, slices of a longer text,
find_buffer, the multi-device context rehearsed on one GPU (text and pattern partition), the link-level shim, the CLI, a
mixed pattern set and the forced kernels.  Every cell pins the kernel id, so a routing change cannot move a class onto
another kernel unnoticed.  Counts are exact integers: no tolerance anywhere.

The recipe (plant()): n = 3 m + 9000 random bytes of the alphabet plus two bytes the pattern never contains; the pattern
with k - 2 substitutions, one deletion and one insertion at 17, n // 2 + 3, n - m - 1 (the last full windows) and
n - m + 40 (only truncated windows left).  The last two overlap: written in that order, the copy at n - m - 1 keeps its
first 41 bytes only, so THREE copies are whole and the oracle must see at least three matches (over the 80-letter and
bigger alphabets it sees exactly three).  plant(c, last_full=True) writes the last two in the other order -- the copy at
n - m - 1 is whole, the truncated one is not -- and the shard test runs that text too.  The loose cases (8 k > m) are
checked by the literal oracle and use a shorter text.

Run time on one MI355X: 102 s for the 173 tests, next to 165 s for the rest of the -m gpu suite.  About 90 s of it are the
class E cells: a GENERIC call costs what one window costs (1.2 s at 2048 bytes .. 7.1 s at 5000, see E_CHEAP), so a
shorter text does not make it cheaper and the class E cases make fewer calls instead.  Classes A .. D take 10 s for the
whole matrix, the literal oracle of the loose cases 4 s."""
import functools
import os
import random
import subprocess
from collections import namedtuple

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
PROSE = b"etaoinshrdlucmfwypvbgkqjxz ,"            # 28 letters, printable
A80 = bytes(range(46, 126))                         # 80 printable letters, no '-'
A200 = bytes(range(1, 201))
A250 = bytes(range(1, 251))
ALPHABETS = {"dna": (DNA, b"N\n"), "prose": (PROSE, b"\n#"), "a80": (A80, b"\n!"),
             "a200": (A200, b"\x00\xff"), "a250": (A250, b"\x00\xff")}   # (pattern letters, text-only bytes)

Case = namedtuple("Case", "cls m k alpha loose kernel")
BITPAR, GENERIC, WAVEFRONT, BANDED, NFA = 3, 1, 2, 4, 5

CASES = [
    Case("A", 129, 9, "dna", False, BITPAR), Case("A", 256, 20, "dna", False, BITPAR), Case("A", 257, 8, "dna", False, BITPAR),
    Case("A", 512, 12, "dna", False, BITPAR), Case("A", 300, 9, "prose", False, BITPAR), Case("A", 400, 11, "a80", False, BITPAR),
    Case("A", 384, 49, "dna", True, BITPAR),
    Case("B", 513, 6, "dna", False, BITPAR), Case("B", 768, 15, "dna", False, BITPAR), Case("B", 769, 8, "dna", False, BITPAR),
    Case("B", 1024, 20, "dna", False, BITPAR), Case("B", 600, 10, "prose", False, BITPAR), Case("B", 900, 13, "a80", False, BITPAR),
    Case("B", 640, 81, "dna", True, BITPAR),
    Case("C", 1025, 5, "dna", False, BITPAR), Case("C", 1500, 14, "dna", False, BITPAR), Case("C", 2048, 19, "dna", False, BITPAR),
    Case("C", 1300, 9, "prose", False, BITPAR), Case("C", 1800, 16, "a80", False, BITPAR),
    Case("C", 1100, 138, "dna", True, BITPAR),
    Case("D", 2049, 7, "dna", False, BITPAR), Case("D", 3000, 20, "dna", False, BITPAR), Case("D", 4096, 11, "dna", False, BITPAR),
    Case("D", 2500, 13, "prose", False, BITPAR), Case("D", 3500, 17, "a80", False, BITPAR),
    Case("D", 2100, 263, "dna", True, BITPAR),
    Case("E", 4097, 6, "dna", False, GENERIC), Case("E", 5000, 18, "dna", False, GENERIC),
    Case("E", 3000, 10, "a200", False, GENERIC),        # class E by alphabet: 201 Eq rows of 128 words > 60 KiB
    Case("E", 2048, 8, "a250", False, GENERIC),         # 251 rows of 64 words > 60 KiB
    Case("E", 1100, 7, "a250", False, GENERIC),         # the same, and the cheapest GENERIC call there is: E_CHEAP
]
TIGHT = [c for c in CASES if not c.loose]
FULL_RESIDUES = {("A", 257), ("B", 769), ("C", 1025), ("D", 2049), ("E", 1100)}   # device text at every residue 1 .. 15 mod 16
# GENERIC keeps its DP column in global memory and one lane walks a whole window: a call costs what its LONGEST window costs,
# however few windows it owns -- measured on an MI355X 1.2 s at m = 2048, 2.4 s at 3000, 4.4 s at 4097, 7.1 s at 5000.  So the
# class E cases run FEWER CALLS, not smaller texts: the shards that hold a planted copy instead of all six (every test
# asserts that the oracle's count of a shard it runs is not zero), and where the class needs just one case a pattern of
# 1100 bytes over 250 letters, which is class E by its alphabet and costs a third of a second per call.
E_A200, E_A250, E_CHEAP = CASES[-3], CASES[-2], CASES[-1]
SLICE_CASES = [c for c in CASES if c.kernel == BITPAR] + [E_CHEAP]
FIND_CASES = [c for c in TIGHT if c.kernel == BITPAR] + [E_A200, E_A250]            # both class E alphabet cases of the issue
MULTI_CASES = [c for c in TIGHT if c.kernel == BITPAR] + [E_CHEAP]
SHIM = {"A": (257, 129), "B": (769, 513), "C": (1025, 513), "D": (2049, 1025), "E": (4097, 2049)}   # odd m: odd n


def _id(c):
    return "%s-%d-k%d-%s%s" % (c.cls, c.m, c.k, c.alpha, "-loose" if c.loose else "")


def _case(cls, m):
    return next(c for c in CASES if c.cls == cls and c.m == m and c.alpha == "dna")


def text_length(c):
    return 4 * c.m + 600 if c.loose else 3 * c.m + 9000   # the literal oracle costs n m^2: a shorter text, all four copies still apart


def plant_offsets(n, m):
    return [17, n // 2 + 3, n - m - 1, n - m + 40]


WHOLE_COPIES = 3


@functools.lru_cache(maxsize=None)
def plant(c, last_full=False):
    """(text, pattern) of a case, from a seed of its own"""
    rnd = random.Random(1000003 * c.m + 101 * c.k + len(c.alpha))
    letters, extra = ALPHABETS[c.alpha]
    m, k, n = c.m, c.k, text_length(c)
    text = bytearray(rnd.choices(letters + extra, k=n))
    head = list(letters) if len(letters) <= m and len(letters) > 80 else []   # the big alphabets: every letter is in the pattern
    pat = bytearray(head + rnd.choices(letters, k=m - len(head)))
    rnd.shuffle(pat)
    offsets = plant_offsets(n, m)
    if last_full:
        offsets[2], offsets[3] = offsets[3], offsets[2]
    for o in offsets:
        w = bytearray(pat)
        for _e in range(k - 2):
            w[rnd.randrange(m)] = rnd.choice(letters)
        del w[m // 3]
        w.insert(2 * m // 3, rnd.choice(letters))
        text[o:o + m] = w[:max(0, min(m, n - o))]
    assert len(text) == n
    return bytes(text), bytes(pat)


_count_cache = {}


def ref_count(text, pat, k, a=0, b=None):
    """the oracle's count of the window starts [a, b): the banded form where the band is narrow (8 k <= m), else the literal one"""
    b = len(text) if b is None else b
    key = (text, pat, k, a, b)
    if key not in _count_cache:
        _count_cache[key] = H.oracle_counts(text, [pat], k, banded=8 * k <= len(pat), j_begin=a, j_end=b)[0]
    return _count_cache[key]


def ref_positions(text, pat, k):
    """the matching window starts, by bisection over the range form of the oracle: a range with a non-zero count is split in
    the middle, the left half counted, the right half's count is the difference"""
    out = []

    def descend(a, b, cnt):
        if cnt == 0:
            return
        if b - a == 1:
            out.append(a)
            return
        mid = (a + b) // 2
        left = ref_count(text, pat, k, a, mid)
        descend(a, mid, left)
        descend(mid, b, cnt - left)

    end = max(0, len(text) - k)
    if end:
        descend(0, end, ref_count(text, pat, k, 0, end))
    return out


def owner_cuts(n, m):
    """odd cuts: one byte after the first copy's start and after the middle copy's, one just in front of the last full
    windows, one inside the last m bytes: the last shard owns truncated windows only, the truncated copy at n - m + 40 among
    them.  Shards 0, 2 and 5 hold a whole copy each; shard 4 holds the one at n - m - 1 in the last_full text."""
    cuts = [0, 18, 1001, n // 2 + 4, (n - m - 7) | 1, (n - m + 8) | 1, n]
    assert cuts == sorted(set(cuts))
    return cuts


def shard_wants(c, last_full=False):
    """the oracle's count of every owner range of owner_cuts (their sum: of the whole text, which costs the literal oracle
    no second pass); asserted to see every whole copy before the GPU is asked"""
    text, pat = plant(c, last_full)
    cuts = owner_cuts(len(text), c.m)
    wants = [ref_count(text, pat, c.k, ob, oe) for ob, oe in zip(cuts[:-1], cuts[1:])]
    assert sum(wants) >= WHOLE_COPIES, (_id(c), wants)
    assert wants[0] >= 1 and wants[2] >= 1 and wants[4 if last_full else 5] >= 1, (_id(c), wants)   # where the copies are
    return cuts, wants


def expected_total(c):
    return sum(shard_wants(c)[1])


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


class DeviceText:
    """text at d + residue of a 16-byte aligned allocation; the bytes around it are copies of `fill` (a pattern: reading
    them as text would make matches)"""

    def __init__(self, ctx, data, residue, fill):
        self.ctx, self.n = ctx, len(data)
        size = len(data) + 64
        self.base = ctx.device_alloc(size)
        assert self.base % 16 == 0
        ctx.device_upload(self.base, (fill * (size // len(fill) + 1))[:size])
        self.ptr = self.base + residue
        ctx.device_upload(self.ptr, data)
        self.d_counts = ctx.device_alloc(8 * 16)

    def count(self, n_patterns, ptr_off, text_off, text_len, n_total, ob, oe):
        ctx = self.ctx
        assert 0 <= ptr_off and ptr_off + text_len <= self.n          # the call stays inside the uploaded text
        ctx.device_memset(self.d_counts, 0, 8 * n_patterns)
        ctx.count_shard_device(self.ptr + ptr_off, text_off, text_len, n_total, ob, oe, self.d_counts)
        ctx.synchronize()
        raw = ctx.device_download(self.d_counts, 8 * n_patterns)
        return [int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(n_patterns)]

    def free(self):
        self.ctx.device_free(self.base)
        self.ctx.device_free(self.d_counts)


def shard_counts(ctx, text, pats, residue, cuts, only=None):
    """[(ob, oe, counts)] through apm_count_shard_device: the whole text resident at `residue` mod 16; shards alternate
    between the whole text (text_off 0) and the text from 1 .. 15 bytes in front of own_begin on (own_begin > text_off > 0);
    only: the shards to run (None: all)"""
    n = len(text)
    dev = DeviceText(ctx, text, residue, pats[-1])
    out = []
    try:
        for i, (ob, oe) in enumerate(zip(cuts[:-1], cuts[1:])):
            if only is not None and i not in only:
                continue
            lo = 0 if (i + residue) % 2 == 0 else max(0, ob - (1 + (residue + 5 * i) % 15))
            out.append((ob, oe, dev.count(len(pats), lo, lo, n - lo, n, ob, oe)))
    finally:
        dev.free()
    return out


def set_one(ctx, c, variant="auto"):
    text, pat = plant(c)
    ctx.set_kernel("auto")
    ctx.set_patterns([pat], c.k)
    ctx.set_kernel(variant)
    return text, pat


def test_case_table_covers_the_issue():
    """the fixed lists: both sides of every class boundary, the alphabets, a loose case per class A .. D"""
    lens = {cls: sorted(c.m for c in CASES if c.cls == cls and c.alpha == "dna" and not c.loose) for cls in "ABCDE"}
    assert lens == {"A": [129, 256, 257, 512], "B": [513, 768, 769, 1024], "C": [1025, 1500, 2048], "D": [2049, 3000, 4096],
                    "E": [4097, 5000]}
    for cls in "ABCD":
        assert {c.alpha for c in CASES if c.cls == cls} == {"dna", "prose", "a80"}
        loose = [c for c in CASES if c.cls == cls and c.loose]
        assert len(loose) == 1 and 8 * loose[0].k > loose[0].m
    assert all(5 <= c.k <= 20 for c in TIGHT)
    assert (E_A200.m, E_A250.m) == (3000, 2048) and 195 <= len(set(plant(E_A200)[1])) <= 200
    assert len(set(plant(E_A250)[1])) >= 240 and len(set(plant(E_CHEAP)[1])) >= 240
    assert len(PROSE) == 28 and len(A80) == 80 and b"-" not in A80 + PROSE
    for c in CASES:
        text, pat = plant(c)
        assert len(pat) == c.m and not set(pat) & set(ALPHABETS[c.alpha][1]) and set(text) & set(ALPHABETS[c.alpha][1])


def test_position_reference_equals_window_by_window_oracle():
    """ref_positions (bisection over oracle ranges) pinned by the full DP per window, on a class A pattern"""
    c = _case("A", 129)
    text, pat = plant(c)
    text = text[:600] + text[-2400:]                       # the first copy, the last ones, the truncated windows (m x m per window is slow)
    want = H.oracle_positions(text, pat, c.k)
    assert len(want) >= 3 and ref_positions(text, pat, c.k) == want


# ---------------------------------------------------------------- (a) owner shards at odd cuts, every residue
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_shards_at_odd_cuts_and_unaligned_device_text(ctx, c):
    cuts, wants = shard_wants(c)
    text, pat = set_one(ctx, c)
    assert ctx.pattern_kernel(0) == c.kernel
    n = len(text)
    assert cuts[-2] > n - c.m and any(x % 2 for x in cuts)
    if c.kernel == GENERIC:   # (see E_CHEAP) shard 0: full windows with the first copy; shard 5: truncated ones with the last
        plan = [(r, {5}) for r in range(1, 16)] + [(3, {0}), (8, {2})] if c is E_CHEAP else [(3, {0}), (12, {5})]
        assert all(wants[i] >= 1 for r, only in plan for i in only)
    else:
        residues = range(1, 16) if (c.cls, c.m) in FULL_RESIDUES else ([5] if c.loose else [1 + c.m % 15, 8, 15])
        plan = [(r, None) for r in residues]
    ran = 0
    for r, only in plan:
        got = shard_counts(ctx, text, [pat], r, cuts, only)
        ran += len(got)
        assert got == [(cuts[i], cuts[i + 1], [wants[i]]) for i in range(6) if only is None or i in only], (_id(c), "residue", r)
    assert ran == sum(6 if only is None else len(only) for r, only in plan)
    if not c.loose and (c.kernel == BITPAR or c is E_CHEAP):   # the text whose copy at n - m - 1 (the last full windows) is whole
        cuts, wants = shard_wants(c, last_full=True)
        text, pat = plant(c, last_full=True)
        for r, only in ([(4, None), (11, None)] if c.kernel == BITPAR else [(4, {4})]):
            got = shard_counts(ctx, text, [pat], r, cuts, only)
            assert got == [(cuts[i], cuts[i + 1], [wants[i]]) for i in range(6) if only is None or i in only], (_id(c), "last full", r)
    ctx.set_kernel("auto")


# ---------------------------------------------------------------- (b) the shard is a slice of a longer text
@pytest.mark.parametrize("c", SLICE_CASES, ids=_id)
def test_slice_of_a_longer_text(ctx, c):
    """text_off != 0 and n_total > text_off + text_len: the slice ends inside the text, so its last windows are FULL ones
    (the bytes behind the slice are pattern copies: a window cut at the slice's end would match); and a slice that does
    hold the global end"""
    cuts, wants = shard_wants(c)
    text, pat = set_one(ctx, c)
    assert ctx.pattern_kernel(0) == c.kernel
    n, m = len(text), c.m
    slices = [(1, 2, False), (2, 3, False), (4, 6, True), (5, 6, True)]       # runs of owner ranges: the counts are their sums
    if c.kernel == GENERIC:
        slices = slices[1:]                                                    # (see E_CHEAP: the slices that hold a copy)
    for i, (s0, s1, to_end) in enumerate(slices):
        ob, oe, want = cuts[s0], cuts[s1], sum(wants[s0:s1])
        assert s0 == 1 or want >= 1
        for r in ([3] if c.loose or c.kernel == GENERIC else [1 + (c.m + i) % 15, 9]):
            pad = 1 + (r + i) % 15
            lo = ob - pad
            hi = n if to_end else oe + m - 1
            assert 0 < lo and hi <= n and (to_end or hi < n)
            dev = DeviceText(ctx, text[lo:hi], r, pat)
            try:
                got = dev.count(1, 0, lo, hi - lo, n, ob, oe)
            finally:
                dev.free()
            assert got == [want], (_id(c), ob, oe, r)
    ctx.set_kernel("auto")


# ---------------------------------------------------------------- (c) match positions
@pytest.mark.parametrize("c", FIND_CASES, ids=_id)
def test_find_buffer_positions(ctx, c):
    """apm_find_buffer on a set of two: the positions are the reference's, total == the count, a small capacity returns a
    subset of that size, the set counts the same afterwards.  The two class E alphabet cases returned
    APM_ERR_UNSUPPORTED (-6) while find_buffer forced BITPAR for every m <= 4096."""
    want = expected_total(c)
    text, pat = plant(c)
    pats = [pat[:33], pat]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, c.k)
    assert ctx.pattern_kernel(1) == c.kernel
    counts = ctx.count_buffer(text)
    assert counts == [ref_count(text, pats[0], c.k), want]
    pos = ref_positions(text, pat, c.k)
    assert len(pos) == want
    got, total = ctx.find_buffer(text, 1, capacity=4096)
    assert total == want and got == pos, _id(c)
    cap = want // 2
    got, total = ctx.find_buffer(text, 1, capacity=cap)
    assert total == want and len(got) == cap and len(set(got)) == cap and set(got) <= set(pos)
    assert ctx.count_buffer(text) == counts
    assert ctx.pattern_kernel(1) == c.kernel
    if c.kernel == BITPAR:                                   # the text with a whole copy in the last full windows
        text, pat = plant(c, last_full=True)
        pos = ref_positions(text, pat, c.k)
        assert len(text) - c.m - 1 in pos
        got, total = ctx.find_buffer(text, 1, capacity=4096)
        assert total == len(pos) and got == pos, (_id(c), "last full")


# ---------------------------------------------------------------- (f) one mixed set
def mixed_set():
    """prefixes of the 4097-byte pattern: every planted copy of it holds a copy of each prefix"""
    c = _case("E", 4097)
    text, pat = plant(c)
    pats = [b"ACG", pat[:20], pat[:40], pat[:100], pat[:257], pat[:769], pat[:1025], pat[:2049], pat]
    # 0: trivial (k >= m), no kernel at all.  BANDED needs k <= 7, and with k <= 7 AUTO sends EVERY pattern of up to 512 bytes to
    # BANDED: in a set that has BANDED patterns the class A length is one of them (alone, with k >= 8, it is BITPAR: CASES)
    kernels = [0, NFA, BANDED, BANDED, BANDED, BITPAR, BITPAR, BITPAR, GENERIC]
    return text, pats, c.k, kernels


def mixed_want(text, pats, k, a=0, b=None):
    return [ref_count(text, p, k, a, b) for p in pats]


def test_mixed_set_by_buffer_and_by_unaligned_shards(ctx):
    """trivial + NFA + two BANDED + one each of B .. E, plus a class A length that AUTO sends to BANDED (see mixed_set), in one
    context: the short ones' sieve pipeline runs with a halo of m_max - 1 = 4096 bytes"""
    text, pats, k, kernels = mixed_set()
    want = mixed_want(text, pats, k)
    assert want[0] == len(text) - k and all(w >= WHOLE_COPIES for w in want[2:]), want
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert [ctx.pattern_kernel(i) for i in range(len(pats))] == kernels
    assert ctx.count_buffer(text) == want
    assert ctx.stat("sieve_on") == 1 and ctx.stat("sieve_candidates") > 0        # the BANDED ones went through the sieve
    n = len(text)
    cuts = owner_cuts(n, 4097)
    ran = 0
    for r, only in ((0, {5}), (13, {0})):         # (the class E pattern: see E_CHEAP) the truncated windows, and the first copy
        for ob, oe, got in shard_counts(ctx, text, pats, r, cuts, only):
            ran += 1
            assert got == mixed_want(text, pats, k, ob, oe) and all(g >= 1 for g in got[2:]), ("residue", r, ob, oe)
    pats, kernels = pats[:-1], kernels[:-1]                                      # without it: every shard, a halo of 2048 bytes
    ctx.set_patterns(pats, k)
    assert [ctx.pattern_kernel(i) for i in range(len(pats))] == kernels
    assert ctx.count_buffer(text) == want[:-1] and ctx.stat("sieve_candidates") > 0
    cuts = owner_cuts(n, 2049)
    for r in (0, 3, 8, 13):
        for ob, oe, got in shard_counts(ctx, text, pats, r, cuts):
            ran += 1
            assert got == mixed_want(text, pats, k, ob, oe), ("residue", r, ob, oe)
    assert ran == 2 + 4 * 6


# ---------------------------------------------------------------- (d) the multi-device context on one GPU
@pytest.fixture(scope="module", params=["0,0,0", "0,0,0,0,0,0,0,0"])
def multi(request, apm):
    os.environ["APM_DEVICES"] = request.param
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    m.n_shards = len(request.param.split(","))
    yield m
    m.close()


@pytest.mark.parametrize("c", MULTI_CASES, ids=_id)
def test_multi_device_text_partition(multi, tmp_path, c):
    """3 and 8 shards of one ~20 KB text: with eight, the m_max - 1 halo of a class D pattern is longer than a shard.
    Buffer and file ingest give the reference's count; positions are global, ascending, unique across the seams."""
    want = expected_total(c)
    text, pat = plant(c)
    multi.set_partition("text")
    multi.set_kernel("auto")
    multi.set_patterns([pat], c.k)
    assert multi.pattern_kernel(0) == c.kernel
    assert multi.count_buffer(text) == [want]
    assert multi.timing()["n_devices"] == multi.n_shards
    f = tmp_path / "text.bin"
    f.write_bytes(text)
    assert multi.count_file(str(f)) == [want]
    got, total = multi.find_buffer(text, 0, capacity=4096)
    assert total == want and got == ref_positions(text, pat, c.k), _id(c)
    assert multi.count_buffer(text) == [want]


def test_multi_device_pattern_partition_mixed_set(multi, tmp_path):
    text, pats, k, kernels = mixed_set()
    want = mixed_want(text, pats, k)
    multi.set_kernel("auto")
    multi.set_partition("patterns")
    try:
        multi.set_patterns(pats, k)
        assert [multi.pattern_kernel(i) for i in range(len(pats))] == kernels
        assert multi.count_buffer(text) == want
        for i in (3, 5, 7):                                  # (the class E pattern's positions: see E_CHEAP)
            got, total = multi.find_buffer(text, i, capacity=4096)
            assert total == want[i] and got == ref_positions(text, pats[i], k), i
        multi.set_patterns(pats[:-1], k)
        f = tmp_path / "text.bin"
        f.write_bytes(text)
        assert multi.count_file(str(f)) == want[:-1]
    finally:
        multi.set_partition("text")


# ---------------------------------------------------------------- (e) the link-level shim and the CLI
@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shim") / "refshim_test")
    subprocess.run(["gcc", "-O1", "-Wall", "-I", os.path.join(H.ROOT, "include"), os.path.join(H.ROOT, "tests", "refshim_test.c"),
                    "-o", exe, "-L", H.PKG_DIR, "-lapm_hip", "-Wl,-rpath," + H.PKG_DIR, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("cls", list("ABCDE"))
def test_reference_entry_points_with_long_patterns(ctx, shim_exe, tmp_path, cls):
    """invoke_kernel / initializeGPU as the reference's hosts call them: n is odd and n / 2 no multiple of 16 (rank 1's
    indexStartMyPiece), two long lengths in front of the pattern the GPU leaves out, so two length groups one after the other.
    Expectations as in test_reference_gpu_entry_points_link_level."""
    m, m2 = SHIM[cls]
    c = _case(cls, m)
    expected_total(c)
    text, pat = plant(c)
    n, k = len(text), c.k
    assert n % 2 == 1 and (n // 2) % 16 != 0
    pats = [pat, pat[:m2], pat[:40]]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert [ctx.pattern_kernel(i) for i in range(3)] == [c.kernel, BITPAR, BANDED if k <= 7 else BITPAR]
    f = tmp_path / "text.txt"
    f.write_bytes(text)
    r = subprocess.run([shim_exe, str(k), str(f)] + [p.decode("latin-1") for p in pats], capture_output=True, timeout=600)
    assert r.returncode == 0 and b"failed" not in r.stderr, r.stderr.decode()[-2000:]
    lines = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in r.stdout.decode().splitlines() if l.strip()}
    want = [ref_count(text, p, k) for p in pats]
    assert want[0] >= WHOLE_COPIES and want[1] >= WHOLE_COPIES
    assert lines["invoke"] == want
    assert lines["invoke34"] == [ref_count(text[:min(n, 3 * n // 4 + len(p) - 1)], p, k) for p in pats]
    for rank, (start, end) in enumerate([(0, n // 2), (n // 2, n)]):
        wdb = [ref_count(text[:min(n, end + (len(p) - 1 if rank == 0 else 0))], p, k, start) for p in pats[:2]] + [0]
        assert lines["db%d" % rank] == wdb, (cls, rank)


CLI = os.path.join(H.PKG_DIR, "host", "apm_parallel")


@pytest.mark.parametrize("gpus", [1, 3])
def test_cli_positions_one_pattern_per_class(ctx, tmp_path, gpus):
    """apm_parallel k file pattern... --positions: one pattern per class (prefixes of the class E one, so each has its
    copies in the text; k = 9, so the class A one is BITPAR); A .. E on one device, A .. D with --gpus 3, where the three
    shards share this GPU (the class E pattern once: see E_CHEAP)"""
    assert os.path.exists(CLI), "host/apm_parallel is not built"
    text, pat = plant(_case("E", 4097))
    k = 9
    pats, kernels = [pat[:257], pat[:769], pat[:1025], pat[:2049], pat], [BITPAR] * 4 + [GENERIC]
    if gpus == 3:
        pats, kernels = pats[:4], kernels[:4]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert [ctx.pattern_kernel(i) for i in range(len(pats))] == kernels
    want = mixed_want(text, pats, k)
    assert all(w >= WHOLE_COPIES for w in want)
    f = tmp_path / "text.txt"
    f.write_bytes(text)
    args = [CLI, str(k), str(f)] + [p.decode() for p in pats] + ["--positions"]
    env = dict(os.environ)
    if gpus > 1:
        args += ["--gpus", str(gpus)]
        env["APM_DEVICES"] = ",".join(["0"] * gpus)
    r = subprocess.run(args, capture_output=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert [int(l.rsplit(": ", 1)[1]) for l in lines if l.startswith("Number of matches")] == want
    pos_lines = [l for l in lines if l.startswith("Positions for pattern")]
    assert len(pos_lines) == len(pats)
    for l, p in zip(pos_lines, pats):
        assert l.startswith("Positions for pattern <%s>:" % p.decode())
        assert [int(x) for x in l.split(">:", 1)[1].split()] == ref_positions(text, p, k), len(p)


# ---------------------------------------------------------------- (g) forced kernels through the shards
@pytest.mark.parametrize("c", [c for c in CASES if c.kernel == BITPAR], ids=_id)
def test_forced_bitpar_shards(ctx, c):
    cuts, wants = shard_wants(c)
    text, pat = set_one(ctx, c, "bitpar")
    assert ctx.pattern_kernel(0) == BITPAR
    for r in (7, 12):
        assert [g[2][0] for g in shard_counts(ctx, text, [pat], r, cuts)] == wants, (_id(c), r)
    ctx.set_kernel("auto")


FORCED_GENERIC_TAIL = 2600   # GENERIC costs m^2 per window in global memory: the last m + 2600 bytes of the text only


@pytest.mark.parametrize("cls,m", [("A", 257), ("B", 769), ("C", 1500), ("D", 3000), ("E", 1100)])
def test_forced_generic_shards(ctx, cls, m):
    """the text shrunk to its end, own ranges at odd cuts: the text with the truncated copy (it lies in the last shard, which
    owns truncated windows only) and the text with the whole copy at n - m - 1 (the shard before it: the last full windows);
    from 1500 bytes on those two shards only (see E_CHEAP)"""
    c = E_CHEAP if cls == "E" else _case(cls, m)
    assert c.m == m
    ctx.set_kernel("generic")
    ctx.set_patterns([plant(c)[1]], c.k)
    assert ctx.pattern_kernel(0) == GENERIC
    ran = 0
    for last_full, key, r in ((False, 4, 5), (True, 3, 10)):
        text, pat = plant(c, last_full)
        text = text[-(m + FORCED_GENERIC_TAIL):]
        n = len(text)
        cuts = [0, 18, 1001, (n - m - 7) | 1, (n - m + 8) | 1, n]
        assert cuts == sorted(set(cuts))
        wants = [ref_count(text, pat, c.k, ob, oe) for ob, oe in zip(cuts[:-1], cuts[1:])]
        assert wants[key] >= 1, (cls, m, wants)
        only = None if m < 1500 else {key}
        got = shard_counts(ctx, text, [pat], r, cuts, only)
        ran += len(got)
        assert [g[2][0] for g in got] == [w for i, w in enumerate(wants) if only is None or i in only], (cls, m, r)
    assert ran == (10 if m < 1500 else 2)
    ctx.set_kernel("auto")


@pytest.mark.parametrize("m", [129, 256])
def test_forced_wavefront_shards(ctx, m):
    c = _case("A", m)
    cuts, wants = shard_wants(c)
    text, pat = set_one(ctx, c, "wavefront")
    assert ctx.pattern_kernel(0) == WAVEFRONT
    for r in (2, 9, 15):
        assert [g[2][0] for g in shard_counts(ctx, text, [pat], r, cuts)] == wants, (m, r)
    ctx.set_kernel("auto")
