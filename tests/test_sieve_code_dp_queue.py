"""The code-filter sieve's window-DP stage (apm_sieve2cfdp_kernel) where its per-wave queue really spans blocks, and at
every k the stage accepts.

Part 1 -- the queue across blocks.  A wave of the sieve scans the 4 KiB blocks w, w + W, w + 2W, ... (W = the pass's wave
count, read off the launch through the statistic "sieve_waves"), and its queue of window-DP entries lives in registers
from one of them to the next.  The text here is sized from W (at least 2 W + 8 blocks, 3 W + 8 where 256 MiB allow it) and
occurrences of the short patterns are planted BY WAVE: first block only (judged blocks later, by the end-of-run flush),
a few in every block, ladders of 2..30 occurrences in the first and the second block (the flush threshold and the
queue-full fallback are crossed somewhere on them), a hit-free block between two loaded ones, occurrences around the
seams of a second and third block, and pairs of patterns whose units meet at one pair index.  AUTO must equal the forced
full-DP BITPAR kernel on the whole text, in the count and in the record form, and the literal CPU oracle around every
planted block.  A second family of plants follows the block grid of a shard call whose owner range is not block aligned.

Part 2 -- every k.  Per k a set with the lengths on both sides of m + 2k <= 30, occurrences with 0..k edits at every
offset around 4 KiB seams, at the text's start and end, two alphabets, against the literal oracle; in a subprocess per
switch setting (candidate-list regions of 1 and 5 entries, no candidate list).  The plan keeps the code filter only
while at most 80 % of a set's key words belong to units the filter cannot judge (build_sieve_plan), and pieces of four
bytes show 256 words each: hence the long lists of companion patterns, whose units show one word each.  A second set
per k holds the upper boundary lengths alone, so that m = 30 - 2k is certain to hold one of the seven slots."""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

BLOCK = 4096
ACGT = b"ACGT"
AMINO = b"ACDEFGHIKLMNPQRSTVWY"      # 20 letters on four 2-bit codes whatever the shift: the DP on codes passes what verify rejects


def _edit(rnd, p, alpha, n_edits):
    p = bytearray(p)
    for _ in range(n_edits):
        r, pos = rnd.random(), rnd.randrange(len(p))
        if r < 0.4:
            p[pos] = rnd.choice(alpha)
        elif r < 0.7 and len(p) > 1:
            del p[pos]
        else:
            p.insert(pos, rnd.choice(alpha))
    return bytes(p)


def _matches_near(text, pos, p, k):
    """some window start within k of pos is a match of p (the oracle's window distance, truncated at the text's end)"""
    n, m = len(text), len(p)
    for j in range(max(0, pos - k), min(pos + k, n - k - 1) + 1):
        size = min(m, n - j)
        if H.window_distance(p[:size], bytes(text[j:j + size])) <= k:
            return True
    return False


def _plant(text, rnd, pos, p, k, alpha, n_edits):
    """an occurrence of p with up to n_edits edits at pos that IS a match (edits that push the fixed-size window beyond k
    are drawn again, with one edit less every few draws)"""
    for attempt in range(24):
        w = _edit(rnd, p, alpha, max(0, n_edits - attempt // 6))
        old = bytes(text[pos:pos + len(w)])
        assert len(old) == len(w), "plant beyond the text"
        text[pos:pos + len(w)] = w
        if _matches_near(text, pos, p, k):
            return len(w)
        text[pos:pos + len(old)] = old
    raise AssertionError("no matching edit found")


def _random_text(seed, n, alpha):
    table = bytes(alpha[b % len(alpha)] for b in range(256))     # (256 = 12 * 20 + 16: near enough to uniform)
    return bytearray(random.Random(seed).randbytes(n).translate(table))


# ================================================================ part 1: the queue across blocks
K = 3
SHORT = [16, 20, 21, 22, 23, 24]      # m + 2k <= 30: their units are the candidates for the seven slots
LONG = [34, 41, 49, 63, 77, 99, 128]  # keep the code filter on (their units are "strong" key words)
CAP_BYTES = 256 << 20
SHARD_LO = BLOCK * 20 + 48            # the shard call's text begins here (16-byte aligned, not block aligned) ...
SHARD_OWN = SHARD_LO + 24             # ... and its owner range here: p_lo = (24 - k / 2) & ~15 = 16
SHARD_G0 = SHARD_LO + 16              # global position of the shard call's block 0
SHARD_SKIP = 21                       # blocks of the text the shard call does not scan (rounded up)


def _part1_patterns():
    rnd = random.Random(4242)
    pats = [bytes(rnd.choice(ACGT) for _ in range(m)) for m in SHORT + LONG]
    n_plain = len(SHORT)
    extra = [pats[1]]                                            # a duplicate of a short pattern
    # Y = R + X[:..]: Y's unit behind its middle starts with the bytes of X's first unit.  In a text "R X" both match, and
    # the two units sit at the same position (d = 0) or at neighbouring ones (d = 1): one pair index, two queue entries --
    # or one entry beside the mask bit of a unit that holds no slot (there are more candidate units than slots)
    pairs = []                                                   # (index of Y, index of X, len(R))
    for xi, m_y, d in ((0, 16, 0), (0, 20, 1), (3, 16, 1), (3, 22, 0), (1, 20, 0), (5, 24, 1), (2, 21, 0)):
        half = 2 * m_y // (K + 1)                                # where Y's third piece starts
        r_len = half - d
        y = bytes(rnd.choice(ACGT) for _ in range(r_len)) + pats[xi][:m_y - r_len]
        assert len(y) == m_y
        pairs.append((len(pats) + len(extra), xi, r_len))
        extra.append(y)
    pats = pats + extra
    shorts = [i for i, p in enumerate(pats) if len(p) + 2 * K <= 30]
    assert len(shorts) == n_plain + 1 + len(pairs)
    return pats, shorts, pairs


def _filler_letter(pats):
    """a letter no pattern holds seven times in nine bytes: a block of it shows the sieve no key word (every key word is
    within one edit of eight or nine pattern bytes)"""
    def worst(letter):
        return max(p[i:i + 9].count(letter) for p in pats for i in range(max(1, len(p) - 8)))
    best = min(ACGT, key=worst)
    assert worst(best) <= 6
    return best


class _Planter:
    """plants occurrences by (wave, block of its run, offset in the block) on the block grid that starts at g0"""

    def __init__(self, text, pats, shorts, pairs, g0, W, wpw, runs, seed):
        self.text, self.pats, self.shorts, self.pairs = text, pats, shorts, pairs
        self.g0, self.W, self.wpw, self.runs = g0, W, wpw, runs
        self.rnd = random.Random(seed)
        self.plants = []          # (position, pattern index, planted bytes, lies on the plant before it)
        self.blocks = set()       # planted blocks of this grid
        self.holes = []           # (begin, end) of the hit-free blocks
        self.filler = _filler_letter(pats)

    def block_start(self, w, r):
        return self.g0 + BLOCK * (w + r * self.W)

    def put(self, pos, pi=None, edits=None, overlay=False):
        pi = self.rnd.choice(self.shorts) if pi is None else pi
        edits = self.rnd.randint(0, K) if edits is None else edits
        ln = _plant(self.text, self.rnd, pos, self.pats[pi], K, ACGT, edits)
        self.plants.append((pos, pi, ln, overlay))
        for b in {(pos - self.g0) // BLOCK, (pos + ln - 1 - self.g0) // BLOCK}:
            self.blocks.add(b)

    def load(self, w, r, count, first=0):
        """`count` occurrences inside block r of wave w's run, 128 bytes apart from offset 128 (+ a few bytes) on"""
        assert first + count <= 30
        for i in range(first, first + count):
            self.put(self.block_start(w, r) + 128 + 128 * i + self.rnd.randrange(32))

    def pair(self, w, r, slot, which, parity):
        """the text R X of a pattern pair, X at an even / odd position"""
        yi, xi, r_len = self.pairs[which]
        xpos = self.block_start(w, r) + 128 + 128 * slot + 40
        xpos += (xpos & 1) ^ parity
        self.put(xpos - r_len, yi, 0)                 # = R + X[:..]
        self.put(xpos, xi, 0, overlay=True)           # (overwrites the tail of Y with the same bytes, and goes on)

    def hole(self, w, r):
        s = self.block_start(w, r)
        self.text[s:s + BLOCK + 16] = bytes([self.filler]) * (BLOCK + 16)
        self.holes.append((s, s + BLOCK + 16))
        self.blocks.add((s - self.g0) // BLOCK)

    def seam(self, at, j, deep):
        """occurrences around the seam at position `at`: one that ends 9..20 bytes in front of it, one across it and one
        16..31 bytes behind it (regions that leave the code strip on either side), or one deep across it"""
        if deep:
            pi = self.rnd.choice(self.shorts)
            self.put(at - 8 - (3 * j) % (len(self.pats[pi]) - 9), pi)
            return
        pi = self.rnd.choice(self.shorts)
        self.put(at - (len(self.pats[pi]) + 2 * K + 17) + j % 12, pi)
        self.put(at - 1 - j % 7)
        self.put(at + 32 + j % 16)

    def run(self):
        W, wpw, R = self.W, self.wpw, self.runs
        N = 40
        step = (W - 128) // N
        assert step >= 48, "too few waves to spread the load patterns over: %d" % W
        sp = [64 + i * step for i in range(N)]
        # first block only: nothing but the end-of-run flush, blocks later, judges these
        self.load(0, 0, 1)
        self.load(wpw - 1, 0, 2)              # the last wave of workgroup 0
        self.load(wpw, 0, 3)                  # the first wave of workgroup 1
        for r in range(R):                    # the last wave overall: a few in every block
            self.load(W - 1, r, 3)
        # ladders: 2, 4, .. 30 occurrences in the first block and as many in the second
        for i in range(15):
            self.load(sp[i], 0, 2 * (i + 1))
            self.load(sp[i], 1, 2 * (i + 1))
        for i, c in ((15, 2), (16, 3), (17, 5)):      # entries carry, grow and leave at the end
            for r in range(R):
                self.load(sp[i], r, c)
        # a hit-free block between two loaded ones (two runs only: behind the loaded ones)
        for i, (c0, c2) in ((18, (5, 6)), (19, (22, 3))):
            self.load(sp[i], 0, c0)
            self.hole(sp[i], 1)
            if R > 2:
                self.load(sp[i], 2, c2)
        # around the seams of second and third blocks, with entries carried from the first (the neighbours' waves too)
        for i in range(20, 28):
            w = sp[i]
            self.load(w, 0, 3 + i % 4)
            self.load(w - 1, 0, 2)
            self.load(w + 1, 0, 2)
            for r in range(1, R):
                j = 2 * (i - 20) + (r - 1)
                self.seam(self.block_start(w, r), j, deep=bool(i & 1))
                self.seam(self.block_start(w, r) + BLOCK, j + 5, deep=not (i & 1))
                self.load(w, r, 2, first=8)
        # pairs of patterns at one pair index, in first and later blocks, next to ordinary occurrences
        for i in range(28, 34):
            w = sp[i]
            for r in range(R):
                for slot in range(0, 2 * len(self.pairs)):
                    self.pair(w, r, 2 * slot, slot % len(self.pairs), (slot // len(self.pairs) + i + r) & 1)
                if (i + r) % 3:
                    self.load(w, r, 2, first=28)
        for i in range(34, 40):                       # mixed loads
            for r in range(R):
                self.load(sp[i], r, self.rnd.randint(1, 12))


class _World:
    pass


@pytest.fixture(scope="module")
def world():
    """patterns, the text sized from the launch geometry and planted by wave (built once), the context, the device text"""
    import torch
    apm = H.pkg()
    pats, shorts, pairs = _part1_patterns()
    wd = _World()
    wd.pats, wd.shorts = pats, shorts
    ctx = apm.ApmContext(device=0)
    try:
        ctx.set_patterns(pats, K)
        assert ctx.stat("sieve_on") == 1 and ctx.stat("sieve_stride") == 1
        cnt = torch.zeros(len(pats), dtype=torch.int64, device="cuda:0")

        def upload(text):
            d = torch.zeros(len(text) + BLOCK + 64, dtype=torch.uint8, device="cuda:0")
            d[:len(text)] = torch.frombuffer(text, dtype=torch.uint8).to("cuda:0")
            assert d.data_ptr() % 16 == 0
            return d

        # size the text from the geometry the launch reports: W grows with the text up to the device's cap
        blocks = 3 * 8192 + 8 + SHARD_SKIP
        for _ in range(8):
            text = _random_text(99, blocks * BLOCK + 1234, ACGT)
            d_text = upload(text)
            ctx.count_shard_device(d_text.data_ptr(), 0, len(text), len(text), 0, len(text), cnt.data_ptr())
            ctx.synchronize()
            W = int(ctx.stat("sieve_waves"))
            assert W > 0 and ctx.stat("sieve_cf") > 0 and ctx.stat("sieve_cf_dp_slots") > 0, "the window-DP stage did not run"
            want = (3 * W if (3 * W + 9 + SHARD_SKIP) * BLOCK <= CAP_BYTES else 2 * W) + 8 + SHARD_SKIP
            if blocks >= want:
                break
            del d_text
            blocks = want
        assert blocks >= 2 * W + 8 + SHARD_SKIP and (blocks + 1) * BLOCK <= CAP_BYTES, (blocks, W)
        wd.W, wd.blocks, wd.runs = W, blocks, 3 if blocks >= 3 * W + 8 + SHARD_SKIP else 2
        wd.wpw = int(ctx.stat("sieve_cf")) // 64                 # waves per workgroup, as launched
        assert W % wd.wpw == 0 and W > 2 * wd.wpw
        # two families of plants: on the whole-text call's block grid (block 0 at position 0) and on the shard call's
        wd.planters = {}
        for name, g0, seed in (("whole", 0, 7), ("shard", SHARD_G0, 8)):
            pl = _Planter(text, pats, shorts, pairs, g0, W, wd.wpw, wd.runs, seed)
            pl.run()
            wd.planters[name] = pl
        spans = sorted([(pos, pos + ln) for pl in wd.planters.values() for pos, pi, ln, overlay in pl.plants if not overlay] +
                       [h for pl in wd.planters.values() for h in pl.holes])
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "plants overlap"
        wd.text = bytes(text)
        wd.n = len(wd.text)
        # every plant is a match, in the final text
        for pl in wd.planters.values():
            for pos, pi, _, _ in pl.plants:
                assert _matches_near(wd.text, pos, pats[pi], K), (pos, pi)
            for s, e in pl.holes:
                assert wd.text[s:e] == bytes([pl.filler]) * (e - s)
        del d_text
        wd.d_text = upload(text)
        wd.ctx, wd.cnt, wd.torch = ctx, cnt, torch
        wd.results = {}
        print("sieve_waves W = %d (%d per workgroup), text %d blocks = %.1f MiB, %d runs per wave, %d + %d plants" % (
            W, wd.wpw, blocks, wd.n / 2**20, wd.runs, len(wd.planters["whole"].plants), len(wd.planters["shard"].plants)))
        yield wd
    finally:
        ctx.close()


def _cut(wd, name):
    n = wd.n
    if name == "whole":
        return 0, n, 0, n                                        # text begin, text end, owner begin, owner end
    hi = n - 777
    return SHARD_LO, hi, SHARD_OWN, hi - 131                     # (a halo of m_max - 1 = 127 bytes behind the owners, and 4 more)


REC_CAP = 1 << 21


def _run(wd, name):
    """counts and sorted records of AUTO and of the forced BITPAR kernel for a cut (run once, shared by the tests)"""
    if name in wd.results:
        return wd.results[name]
    import numpy as np
    torch, c = wd.torch, wd.ctx
    lo, hi, own_b, own_e = _cut(wd, name)
    out = torch.zeros(2 * REC_CAP, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    res = {}
    for variant in ("auto", "bitpar"):
        c.set_kernel(variant)
        wd.cnt.zero_()
        torch.cuda.synchronize()
        c.count_shard_device(wd.d_text.data_ptr() + lo, lo, hi - lo, wd.n, own_b, own_e, wd.cnt.data_ptr())
        c.synchronize()
        counts = wd.cnt.cpu().tolist()
        if variant == "auto":
            stats = {s: c.stat(s) for s in ("sieve_waves", "sieve_cf_dp_slots", "sieve_clist", "sieve_stride", "sieve_cf")}
        wd.cnt.zero_()
        nf.zero_()
        torch.cuda.synchronize()
        c.find_shard_device(wd.d_text.data_ptr() + lo, lo, hi - lo, wd.n, own_b, own_e, out.data_ptr(), REC_CAP, nf.data_ptr(),
                            wd.cnt.data_ptr())
        c.synchronize()
        total = int(nf[0].item())
        assert total <= REC_CAP, total
        rec = out[:2 * total].cpu().numpy().reshape(-1, 2)
        pat, pos = rec[:, 1] & 0xffffffff, rec[:, 0]
        order = np.lexsort((pos, pat))
        res[variant] = dict(counts=counts, rec_counts=wd.cnt.cpu().tolist(), pat=pat[order], pos=pos[order], total=total)
    c.set_kernel("auto")
    res["stats"] = stats
    wd.results[name] = res
    return res


@pytest.mark.parametrize("name", ["whole", "shard"])
def test_queue_spans_blocks_geometry_and_plan(world, name):
    """the text gives every wave at least two blocks (three where 256 MiB allow), as the launch itself reports, and the
    window-DP kernel is the one that ran: a change of geometry or plan cannot turn this module into a one-block test"""
    wd = world
    st = _run(wd, name)["stats"]
    lo, hi, own_b, own_e = _cut(wd, name)
    g0 = 0 if name == "whole" else SHARD_G0
    blocks = -(-(min(hi, own_e + 128 + K // 2) - g0) // BLOCK)
    assert st["sieve_waves"] == wd.W, "the plants were placed for another wave count"
    assert blocks >= 2 * wd.W + 8
    assert st["sieve_cf_dp_slots"] > 0 and st["sieve_clist"] == 1 and st["sieve_stride"] == 1 and st["sieve_cf"] == 64 * wd.wpw
    pl = wd.planters[name]
    assert max(pl.blocks) < blocks and len(pl.blocks) >= 100
    runs_of = {}
    for b in pl.blocks:
        runs_of.setdefault(b % wd.W, set()).add(b // wd.W)
    assert {0, wd.wpw - 1, wd.wpw, wd.W - 1} <= set(runs_of)
    assert sum(1 for r in runs_of.values() if len(r) >= 2) >= 30, "waves with plants in two of their blocks"


@pytest.mark.parametrize("name", ["whole", "shard"])
def test_queue_spans_blocks_counts_equal_bitpar(world, name):
    wd = world
    res = _run(wd, name)
    assert res["auto"]["counts"] == res["bitpar"]["counts"], [len(p) for p in wd.pats]
    lo, hi, own_b, own_e = _cut(wd, name)
    planted = [0] * len(wd.pats)
    for pl in wd.planters.values():
        for pos, pi, _, _ in pl.plants:
            if own_b + K <= pos < own_e - K:
                planted[pi] += 1
    for i in wd.shorts:
        assert planted[i] >= 30 and res["auto"]["counts"][i] >= planted[i], (i, planted[i], res["auto"]["counts"][i])


@pytest.mark.parametrize("name", ["whole", "shard"])
def test_queue_spans_blocks_records_equal_bitpar(world, name):
    import numpy as np
    wd = world
    res = _run(wd, name)
    a, b = res["auto"], res["bitpar"]
    assert a["rec_counts"] == a["counts"] and a["total"] == sum(a["counts"])
    assert b["rec_counts"] == b["counts"] and b["total"] == sum(b["counts"])
    assert a["total"] == b["total"]
    assert np.array_equal(a["pat"], b["pat"]) and np.array_equal(a["pos"], b["pos"])
    key = a["pat"].astype(np.int64) * (1 << 40) + a["pos"]
    assert len(np.unique(key)) == len(key), "a window reported twice"


@pytest.mark.parametrize("name", ["whole", "shard"])
def test_queue_spans_blocks_planted_blocks_equal_literal_oracle(world, name):
    """around every planted block (+- 64 bytes) AUTO's records are the literal oracle's windows: as many per pattern, and
    every one of them a window within k"""
    import numpy as np
    wd = world
    a = _run(wd, name)["auto"]
    lo, hi, own_b, own_e = _cut(wd, name)
    pl = wd.planters[name]
    g0 = pl.g0
    # neighbourhoods of the planted blocks, merged where they touch
    spans = []
    for b in sorted(pl.blocks):
        s, e = max(own_b, g0 + BLOCK * b - 64), min(own_e, wd.n - K, g0 + BLOCK * (b + 1) + 64)
        if spans and s <= spans[-1][1]:
            spans[-1][1] = e
        elif s < e:
            spans.append([s, e])
    first = np.searchsorted(a["pat"], np.arange(len(wd.pats) + 1))
    checked = 0
    for i, p in enumerate(wd.pats):
        pos = a["pos"][first[i]:first[i + 1]]
        for s, e in spans:
            got = pos[np.searchsorted(pos, s):np.searchsorted(pos, e)]
            want = H.oracle_counts(wd.text, [p], K, banded=len(p) > 32, j_begin=s, j_end=e)[0]   # (literal for the short ones)
            assert len(got) == want, (name, len(p), s, e, got.tolist())
            for j in got.tolist():
                assert H.window_distance(p, wd.text[j:j + len(p)]) <= K, (len(p), j)
            checked += want
    assert checked >= len(pl.plants)


# ================================================================ part 2: every k the stage accepts
ROWS = {0: [4, 7, 8, 14, 15, 29, 30, 31], 1: [8, 9, 19, 20, 27, 28, 29], 2: [12, 13, 25, 26, 27], 4: [20, 21, 22, 23]}
# companions beyond m + 2k <= 30 (no slot candidates), enough of them for the plan's 80 % rule (module docstring)
COMPANIONS = {0: [31 + i for i in range(100)], 1: [29 + i % 60 for i in range(150)], 2: [30 + i % 70 for i in range(70)],
              4: [25 + i % 12 for i in range(14)]}
UPPER = {0: [14, 29, 30, 31], 1: [27, 28, 29], 2: [25, 26, 27], 4: [22, 23]}   # the second set's table lengths (k = 0: 14 keeps the sieve per-position)
N2 = 430 * BLOCK - 3001            # 1.7 MiB: a seam per planted offset (419 for k = 0), not a multiple of anything


@functools.lru_cache(maxsize=None)
def _k_case(k, alpha):
    """(text, patterns (the row's lengths first), plants per pattern) -- the same in the parent and in the worker"""
    rnd = random.Random(1000 * k + len(alpha))
    row = ROWS[k]
    pats = [bytes(rnd.choice(alpha) for _ in range(m)) for m in row + COMPANIONS[k]]
    text = _random_text(500 + 10 * k + len(alpha), N2, alpha)
    n = len(text)
    planted = [0] * len(pats)
    seam = 1
    for i, m in enumerate(row):                  # every offset from -(m + 2k + 17) to +17 around a seam, one seam each
        for d in range(-(m + 2 * k + 17), 18):
            _plant(text, rnd, BLOCK * seam + d, pats[i], k, alpha, rnd.randint(0, k))
            planted[i] += 1
            seam += 1
    assert BLOCK * seam + 64 < n
    for i in range(len(row), len(pats)):         # the companions: one occurrence each, inside a block
        _plant(text, rnd, BLOCK * (1 + (i * 3) % 425) + 1500 + i, pats[i], k, alpha, rnd.randint(0, k))
        planted[i] += 1
    slot_max = row.index(30 - 2 * k)
    # the text's start: a window start in 0..k
    _plant(text, rnd, 0 if alpha == ACGT else k, pats[slot_max], k, alpha, k)
    planted[slot_max] += 1
    if alpha == ACGT:                            # an occurrence that ends exactly at the text's end
        p = pats[slot_max]
        text[n - len(p):] = p
        planted[slot_max] += 1
    else:                                        # a truncated one in the tail, behind one that ends where it starts
        p, q = pats[slot_max], pats[row.index(30 - 2 * k) - 1]
        s = len(p) - 3
        assert s > k
        text[n - s:] = p[:s]
        text[n - s - len(q):n - s] = q
        planted[row.index(30 - 2 * k) - 1] += 1
    return bytes(text), pats, planted


def _k_sets(k):
    """pattern indices of the two sets: the whole row + companions, the upper boundary lengths + companions"""
    row = ROWS[k]
    n_all = len(row) + len(COMPANIONS[k])
    return {"row": list(range(n_all)), "upper": [row.index(m) for m in UPPER[k]] + list(range(len(row), n_all))}


def _worker(k):
    apm = H.pkg()
    out = {}
    for alpha in (ACGT, AMINO):
        text, pats, _ = _k_case(k, alpha)
        for sname, idx in _k_sets(k).items():
            with apm.ApmContext(device=0) as ctx:
                ctx.set_patterns([pats[i] for i in idx], k)
                counts = ctx.count_buffer(text)
                stats = {s: ctx.stat(s) for s in ("sieve_on", "sieve_stride", "sieve_cf", "sieve_cf_dp_slots", "sieve_clist", "sieve_waves",
                                                  "sieve_weak_frac")}
                rec, total = ctx.find_all_buffer(text, sum(counts) + 64)
                out["%d:%s" % (len(alpha), sname)] = dict(counts=counts, records=rec, n_found=total, stats=stats,
                                                          kernels=[ctx.pattern_kernel(i) for i in range(len(idx))])
    print(json.dumps(out))


@functools.lru_cache(maxsize=None)
def _k_oracle(k, alpha):
    """the oracle's counts of every pattern: the literal DP for the row's lengths, its banded form (exact for the
    predicate dist <= k, and the only affordable one for some hundred patterns) for the companions"""
    text, pats, _ = _k_case(k, alpha)
    n_row = len(ROWS[k])
    return H.oracle_counts(text, pats[:n_row], k) + H.oracle_counts(text, pats[n_row:], k, banded=True)


ENVS = [{}, {"APM_CLIST_REGION_CAP": "1"}, {"APM_CLIST_REGION_CAP": "5"}, {"APM_SIEVE_CLIST": "0"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join("%s=%s" % (k[4:], v) for k, v in e.items()) or "default")
@pytest.mark.parametrize("k", sorted(ROWS))
def test_every_k_of_the_window_dp_stage_equals_oracle(k, env):
    """counts and records of AUTO equal the oracle's for the lengths on both sides of m + 2k <= 30 (the switches are read
    once per process: a worker per setting).  region caps of 1 and 5: the list region is full while reservations of the
    DP queue are outstanding; no list: slots planned, the DP kernel not chosen"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(k)], capture_output=True, env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert len(got) == 4
    for alpha in (ACGT, AMINO):
        text, pats, planted = _k_case(k, alpha)
        want_all = _k_oracle(k, alpha)
        n = len(text)
        for sname, idx in _k_sets(k).items():
            res = got["%d:%s" % (len(alpha), sname)]
            st = res["stats"]
            where = (k, env, len(alpha), sname, st)
            assert res["kernels"] == [4] * len(idx), "every pattern of the set on the BANDED path"
            assert st["sieve_on"] == 1 and st["sieve_stride"] == 1 and st["sieve_cf"] > 0 and st["sieve_waves"] > 0, where
            assert st["sieve_cf_dp_slots"] > 0, where
            assert st["sieve_clist"] == (0 if env.get("APM_SIEVE_CLIST") == "0" else 1), where
            want = [want_all[i] for i in idx]
            assert res["counts"] == want, where
            assert all(want_all[i] >= planted[i] for i in idx)
            rec = [tuple(x) for x in res["records"]]
            assert res["n_found"] == len(rec) == sum(want) and rec == sorted(set(rec)), where
            per = [0] * len(idx)
            for q, j in rec:                     # as many records as the oracle counts per pattern, each of them a window within k
                per[q] += 1
                p = pats[idx[q]]
                size = min(len(p), n - j)
                assert j < n - k and H.window_distance(p[:size], text[j:j + size]) <= k, (where, len(p), j)
            assert per == want, where


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker(int(sys.argv[1]))
