"""GPU (-m gpu): the bit-vector kernels where the carry of the column's one addition, (Eq & Pv) + Pv, crosses words and
lanes.

Random DNA never makes that carry pass through a word full of pattern rows (test_bitvec_carry_ref.py), so the sweeps
of test_gpu_parity.py and test_long_patterns_entry_points.py leave the propagate path of every form unrun: the carry
chain of bp_step<W> (W = 2 .. 4 in apm_bitpar.h, 8 / 16 in apm_bitpar_wide.hip), `carry` of bp_step_seq<W> (24 / 32), the
P ballot and the (U + G) ^ U ^ G identity of apm_bitlong_kernel<uint32_t / uint64_t>, and the separately compiled copies
in the three tail kernels and in the record-sink builds.  The three pattern families of bitvec_carry_ref.py drive it:
homopolymer runs, as real genomes have them.

One case per (length, family).  The set holds the three families' patterns of that length (the per-lane kernels loop
over the set, the wave form launches per pattern); the text is the case's family's: 3 m + 3000 bytes of random DNA with
two foreign bytes, and between them the exact window, one with up to four substitutions, deletion + insertion, insertion
+ deletion, the window rotated by a byte, pattern + pattern, and at the very end the pattern's first 2 m / 3 bytes.  The
plants alone are 7 2/3 m bytes, so they do not fit into 3 m + 3000 bytes; the text is the filler plus the plants.

Before the GPU is touched, the big-integer model says for every planted full window that the input reaches the path
(bitvec_carry_ref.condition: the longest run of propagating words, and the number of columns with a run), and what its
distance is.  Census of the seeds in use, over the seven full windows of a case, as (columns with a run >= 1, >= 2,
longest run):

  head+run   longest run = L - 1 at every length: 1 2 2 2 3 | 4 7 | 8 9 15 | 16 23 | 24 31 31 | 32 63 63 | 32 46 63
             for m = 33 64 65 96 128 | 129 256 | 257 300 512 | 513 768 | 769 1000 1024 | 1025 2047 2048 | 2049 3000 4096;
             columns with a run >= 1: 20 .. 25 at m = 33, 48 .. 53 at m = 4096
  runs       m = 257: (188 .. 191, 188 .. 191, 6);  m = 4096: (4031 .. 4033, 3838 .. 3840, 9)
  dna+run    m = 256: (44 .. 45, 44 .. 45, 4);  m = 257: (96 .. 100, 48 .. 49, 4);  m = 2049: (764 .. 770, 365 .. 366, 16)

Then, per case: counts under AUTO, forced BITPAR and forced GENERIC == the oracle (its banded form where 8 k <= m); the
truncated windows; the records of forced BITPAR, binned by 64 window starts and start by start around the copies of
pattern + pattern, == the oracle, and == forced GENERIC's; owner shards cut inside the tiles.  Every comparison is
equality.  Cost per case: the oracle and the census (together 2 s at m = 4096) and, from 2047 bytes on, the two GENERIC
calls, which is why GENERIC runs the case's own pattern alone (see at GENERIC below): 13.5 s at 4096 bytes, less than
7.3 s at 3000, less again elsewhere.

These cases REACH the propagate path; with k <= 12 none of them can DECIDE on it (see at LOOSE at the end of the file):
a build with the P ballot of apm_bitlong_kernel forced to 0 and `carry` of bp_step_seq taken from the word's own sum
passes all of them, and test_wide_bitvector_columns_vs_oracle too.  test_shifted_runs_where_the_propagated_carry_decides
is the one that build fails: at 768, 1024, 1025, 2048, 2049 and 4096 bytes, every kernel that was altered."""
import functools

import pytest

import bitvec_carry_ref as R
import helpers as H

pytestmark = pytest.mark.gpu

BITPAR, GENERIC = 3, 1
# GENERIC keeps its column in global memory and one lane walks a whole window: a call costs, per pattern, what the longest
# window costs (about 1 s at 2048 bytes, 5 s at 4096), however short the text.  It is the second reference of a case's OWN pattern
# and runs that pattern alone; the other two patterns of the set have their own cases at the same length.
LENGTHS = [33, 64, 65, 96, 128,        # W = 2, 3, 4
           129, 256,                   # W = 8
           257, 300, 512,              # W = 16
           513, 768,                   # W = 24
           769, 1000, 1024,            # W = 32
           1025, 2047, 2048,           # one window per wave, 32 rows per lane
           2049, 3000, 4096]           # 64 rows per lane
ALL = ("auto", "bitpar", "generic")
CASES = [(m, 9 if m <= 512 else 12, f, ALL) for m in LENGTHS for f in R.FAMILIES]
CASES += [(m, k, f, ("bitpar",)) for m in (300, 2049) for k in (0, 3) for f in R.FAMILIES]   # AUTO has other kernels for these
TILE = 64                                                                                     # window starts per workgroup of the wave form


def _id(c):
    return "%d-k%d-%s%s" % (c[0], c[1], c[2], "" if len(c[3]) == 3 else "-forced")


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


class Reference:
    """what the CPU says about one case: model census and distances of the planted windows, oracle counts per bin of 64
    window starts"""

    def __init__(self, m, k, family):
        B = R.word_bits(m)
        self.m, self.k, self.family, self.B = m, k, family, B
        self.pats = [R.family_pattern(f, m, B, 0) for f in R.FAMILIES]
        self.fi = R.FAMILIES.index(family)
        self.planted = R.build_text(self.pats[self.fi], k, 0)
        self.text = self.planted.text
        self.n = len(self.text)
        self.banded = 8 * k <= m
        self.end = self.n - k                                   # window starts are [0, n - k)
        self.windows = []                                       # (kind, offset, model distance, census)
        for kind, o in self.planted.full:
            dist, census = R.walk(self.pats[self.fi], self.text[o:o + m], B)
            self.windows.append((kind, o, dist, census))
        self._bins = None

    def count(self, i, a, b):
        b = min(b, self.end)
        return H.oracle_counts(self.text, [self.pats[i]], self.k, banded=self.banded, j_begin=a, j_end=b)[0] if a < b else 0

    @property
    def bins(self):
        if self._bins is None:
            self._bins = [[self.count(i, a, a + TILE) for a in range(0, self.end, TILE)] for i in range(3)]
        return self._bins

    @property
    def want(self):
        return [sum(b) for b in self.bins]

    def range_count(self, i, a, b):
        """the oracle's count of the window starts [a, b): whole bins from the one pass, the ragged ends counted"""
        b = min(b, self.end)
        if a >= b:
            return 0
        a1, b0 = -(-a // TILE) * TILE, b // TILE * TILE
        if a1 > b0:
            return self.count(i, a, b)
        return self.count(i, a, a1) + sum(self.bins[i][a1 // TILE:b0 // TILE]) + self.count(i, b0, b)


@functools.lru_cache(maxsize=4)
def reference(m, k, family):
    return Reference(m, k, family)


def owner_cuts(n, m):
    cuts = sorted({0, 1, 63, 64, 65, m + 7, n - m + 5, n})         # (m + 7 < 63 at m = 33)
    assert cuts[-2] == n - m + 5
    return cuts


def shard_counts(ctx, text, n_patterns, cuts):
    """[counts] per owner range through count_shard_device: the whole text resident at a 16-byte aligned address"""
    n = len(text)
    d_text = ctx.device_alloc(n + 64)
    d_counts = ctx.device_alloc(8 * n_patterns)
    out = []
    try:
        assert d_text % 16 == 0
        ctx.device_upload(d_text, text)
        for ob, oe in zip(cuts[:-1], cuts[1:]):
            ctx.device_memset(d_counts, 0, 8 * n_patterns)
            ctx.count_shard_device(d_text, 0, n, n, ob, oe, d_counts)
            ctx.synchronize()
            raw = ctx.device_download(d_counts, 8 * n_patterns)
            out.append([int.from_bytes(raw[8 * i:8 * i + 8], "little") for i in range(n_patterns)])
    finally:
        ctx.device_free(d_text)
        ctx.device_free(d_counts)
    return out


def test_case_table():
    assert len(LENGTHS) == 21 and len(CASES) == 63 + 12
    assert all(k == (9 if m <= 512 else 12) for m, k, f, v in CASES if len(v) == 3)
    assert sorted({(m, k) for m, k, f, v in CASES if len(v) == 1}) == [(300, 0), (300, 3), (2049, 0), (2049, 3)]


def expectations(case):
    """everything the CPU decides about a case, asserted before any launch: (reference, counts per pattern, owner cuts,
    counts per owner range)"""
    m, k, family, variants = case
    ref = reference(m, k, family)
    text, pats, fi, n = ref.text, ref.pats, ref.fi, ref.n
    assert n == 3 * m + 3000 + 7 * m + len(text) - ref.planted.cut and not set(b"".join(pats)) & set(R.FOREIGN)
    assert set(R.FOREIGN) <= set(text)

    # ---- the input reaches the path: both components of the family's condition, for every planted full window
    assert R.condition(family, m, ref.B) is not None or (family != "head+run" and m < 257)
    for kind, o, dist, census in ref.windows:
        assert R.meets(family, m, ref.B, census), (_id(case), kind, census, R.condition(family, m, ref.B))
    close = [o for kind, o, dist, census in ref.windows if dist <= k]
    assert len(close) >= (7 if k >= 3 else 4)                       # (k = 0: the exact windows only)

    # ---- what the oracle says
    want = ref.want
    assert want[fi] >= len(close)
    size = n - ref.planted.cut                                      # the occurrence cut by the end of the text
    assert k < size < m and ref.planted.cut > n - m and R.walk(pats[fi][:size], text[ref.planted.cut:], ref.B)[0] == 0
    assert ref.range_count(fi, n - m + 1, n - k) >= 1               # 2. the truncated windows see it
    cuts = owner_cuts(n, m)
    assert n - m + 1 <= cuts[-2] <= ref.planted.cut                 # the last shard: truncated windows only, the cut occurrence among them
    shard_want = [[ref.range_count(i, ob, oe) for i in range(3)] for ob, oe in zip(cuts[:-1], cuts[1:])]
    assert [sum(s[i] for s in shard_want) for i in range(3)] == want and shard_want[-1][fi] >= 1
    return ref, want, cuts, shard_want


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_carry_chains(ctx, case):
    m, k, family, variants = case
    ref, want, cuts, shard_want = expectations(case)
    text, pats, fi = ref.text, ref.pats, ref.fi

    # ---- 1. counts
    for variant in (v for v in variants if v != "generic"):
        ctx.set_kernel(variant)
        ctx.set_patterns(pats, k)
        assert [ctx.pattern_kernel(i) for i in range(3)] == [BITPAR] * 3, (variant, _id(case))
        assert ctx.count_buffer(text) == want, (variant, _id(case))

    # ---- 3. records through the record-sink builds
    ctx.set_kernel("bitpar")
    ctx.set_patterns(pats, k)
    rec, total = ctx.find_all_buffer(text, sum(want) + 64)
    assert total == sum(want) == len(rec) and len(set(rec)) == len(rec)
    assert all(0 <= j < ref.end for _, j in rec)
    got_bins = [[0] * len(ref.bins[i]) for i in range(3)]
    for i, j in rec:
        got_bins[i][j // TILE] += 1
    assert got_bins == ref.bins, _id(case)
    got = set(rec)
    s = ref.planted.stretch
    for j in list(range(s - 32, s + 32)) + list(range(s + m - 32, s + m + 32)):   # 128 single starts around the two copies
        for i in range(3):
            assert ((i, j) in got) == (ref.count(i, j, j + 1) == 1), (_id(case), i, j - s)
    if "generic" in variants:                                        # (the case's own pattern alone: see at GENERIC above)
        ctx.set_kernel("generic")
        ctx.set_patterns([pats[fi]], k)
        assert ctx.pattern_kernel(0) == GENERIC
        assert ctx.count_buffer(text) == [want[fi]], ("generic", _id(case))
        g_rec, g_total = ctx.find_all_buffer(text, want[fi] + 64)
        assert g_total == want[fi] and [(fi, j) for _, j in g_rec] == [r for r in rec if r[0] == fi], _id(case)

    # ---- 2. and 4. owner shards cut inside the tiles; the last one holds truncated windows only
    ctx.set_kernel(variants[0])
    ctx.set_patterns(pats, k)
    assert shard_counts(ctx, text, 3, cuts) == shard_want, _id(case)
    ctx.set_kernel("auto")


# ---------------------------------------------------------------- where the propagated carry DECIDES
# With k <= 12 the cases above reach the propagate path in every width class, but no count there can depend on it: a carry
# that passes a whole word joins rows more than B apart, and what it changes lies further than k from the diagonal -- the
# model with the propagated carries taken out (bitvec_carry_ref.walk_losing_propagated_carries) gives the same distance
# for every planted window above.  It does not for the `runs` pattern shifted against itself by more than a word: at shift
# d the distance is 2 d, and without the propagated carries one less from d = B + 3 on (99 at 512 bytes, where fewer runs
# fit).  So k = 2 d - 1 at that shift: the window is NOT a match, and a kernel that loses a propagated carry counts it.
LOOSE = [(512, 99), (768, 35), (1024, 35), (1025, 35), (2048, 35), (2049, 67), (4096, 67)]   # (m, the deciding shift)


@pytest.mark.parametrize("m,d0", LOOSE, ids=["%d-shift%d" % c for c in LOOSE])
def test_shifted_runs_where_the_propagated_carry_decides(ctx, m, d0):
    B, k = R.word_bits(m), 2 * d0 - 1
    pat = R.family_pattern("runs", m, B, 0)
    filler = R.build_text(pat, 12, 1).text[:500]
    text = filler + pat + pat + filler[::-1]
    s, n = len(filler), len(filler) * 2 + 2 * m
    deciding = text[s + d0:s + d0 + m]
    dist, census = R.walk(pat, deciding, B)
    assert dist == k + 1 and census[1] >= m // 2
    assert R.walk_losing_propagated_carries(pat, deciding, B) <= k            # the fault would make it a match

    def count(a, b):
        return H.oracle_counts(text, [pat], k, banded=8 * k <= m, j_begin=a, j_end=b)[0]

    starts = [j for j in range(s - 8, s + 2 * d0 + 8)]
    want_at = {j: count(j, j + 1) for j in starts}
    assert want_at[s + d0] == 0 and want_at[s + d0 - 1] == 1 and want_at[s] == 1
    want = count(0, n)
    for variant in ("auto", "bitpar"):
        ctx.set_kernel(variant)
        ctx.set_patterns([pat], k)
        assert ctx.pattern_kernel(0) == BITPAR
        assert ctx.count_buffer(text) == [want], (variant, m, k)
    rec, total = ctx.find_all_buffer(text, want + 64)
    assert total == want == len(set(rec))
    got = {j for _, j in rec}
    assert {j for j in starts if j in got} == {j for j in starts if want_at[j]}, (m, k)
    ctx.set_kernel("auto")
