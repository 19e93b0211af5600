"""The window-DP stage of the code-filter sieve (apm_sieve2cfdp_kernel) at the END OF A BLOCK: the record loop only notes a
slotted record that passes the filter in a pending list of 64 entries per wave; when the block's batches are done the
notes become queue entries, all at once -- one reservation in the workgroup's list region for the block, the range test,
the region's codes and the pair's bit in the (final) mask row read by the queue lane itself, a flush in front when the
queue cannot take the block.  The paths this opens:

1. dense       more wanting records in one block than the pending list holds (the rest takes the bit), and more than the
               queue holds (flush before append);
2. reservation the block-end reservation fails (list regions of 1 and 5 entries) while entries of earlier blocks wait in
               the queue: the pending ones take their bits, the queued ones are released as before;
3. boundaries  regions that start at block offsets -17..-15 and end at 4127..4129: both sides of r >= -16 and
               r + len <= 4128, in the first and the second block of a wave's run;
4. pair        a pending entry whose pair gets its bit later in the same block, from a unit without a slot, in a block
               with more than 64 lookup hits (several batches; the odd position of a hit goes back into the ring).

AUTO must equal the forced full-DP BITPAR kernel on the whole text, in the counts (apm_count_buffer) and in the records
(apm_find_all_buffer), and the literal CPU oracle around every planted block.  The construction is the one of
test_sieve_code_dp_queue.py (K = 3, short lengths 16..24, long companions that keep the code filter on, the text sized from
the statistic "sieve_waves", the filler letter that shows the sieve no key word).  Cases 1-3 use a set whose short
patterns ALL hold a slot (fewer candidate units than slots, asserted): every planted occurrence then makes a pending
entry, whichever units the plan picks.  Case 4 uses the queue test's own set, which has more candidate units than slots.

The switches are read once per process: one worker per setting runs every case and prints what it found."""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H
import test_sieve_code_dp_queue as Q

pytestmark = pytest.mark.gpu

BLOCK, K, ACGT = Q.BLOCK, Q.K, Q.ACGT
SLOTTED = ([16, 20, 24], [16, 24], [24])   # case 1-3: the first of these sets whose plan leaves a slot unused (a pattern has 2..4 units)
SMALL_BLOCKS = 24
PAIR_BLOCKS = 112
DENSE = 127                           # occurrences 32 bytes apart in one block
SETTINGS = {"default": {}, "cap1": {"APM_CLIST_REGION_CAP": "1"}, "cap5": {"APM_CLIST_REGION_CAP": "5"}}
NO_LIST = {"APM_SIEVE_CLIST": "0"}    # the code filter without the window-DP kernel (its survivors leave through the list only)


def _slotted_patterns(lens):
    rnd = random.Random(777)
    return [bytes(rnd.choice(ACGT) for _ in range(m)) for m in lens + Q.LONG]


class _Text:
    """a text with occurrences planted block by block; remembers the planted blocks"""

    def __init__(self, seed, blocks, pats, shorts, plant_seed):
        self.text = Q._random_text(seed, blocks * BLOCK + 1234, ACGT)
        self.pats, self.shorts = pats, shorts
        self.rnd = random.Random(plant_seed)
        self.plants, self.blocks = [], set()
        self.filler = Q._filler_letter(pats)

    def put(self, pos, pi=None, edits=None, overlay=False):
        pi = self.rnd.choice(self.shorts) if pi is None else pi
        edits = self.rnd.randint(0, K) if edits is None else edits
        ln = Q._plant(self.text, self.rnd, pos, self.pats[pi], K, ACGT, edits)
        self.plants.append((pos, pi, ln, overlay))
        self.blocks.update({pos // BLOCK, (pos + ln - 1) // BLOCK})

    def hole(self, b):
        self.text[b * BLOCK:(b + 1) * BLOCK] = bytes([self.filler]) * BLOCK
        self.blocks.add(b)

    def dense(self, b, count=DENSE, skip=()):
        for i in range(count):
            if i not in skip:
                self.put(b * BLOCK + 32 * i)

    def check_plants(self):
        spans = sorted((pos, pos + ln) for pos, pi, ln, overlay in self.plants if not overlay)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "plants overlap"
        text = bytes(self.text)
        for pos, pi, _, _ in self.plants:
            assert Q._matches_near(text, pos, self.pats[pi], K), (pos, pi)
        return text


def _dense_text(pats, shorts):
    """case 1: one block of back-to-back occurrences between two hit-free ones, random blocks around them"""
    t = _Text(31, SMALL_BLOCKS, pats, shorts, 32)
    t.hole(2)
    t.dense(3)
    t.hole(4)
    return t


def _big_text(pats, shorts, W, blocks):
    """cases 2 and 3, planted by wave: wave w scans the blocks w, w + W, ..."""
    t = _Text(33, blocks, pats, shorts, 34)
    step = (W - 64) // 96
    assert step >= 8, W
    waves = [32 + i * step for i in range(96)]
    # case 2: a first block of 1, 3 or 10 occurrences (queued where the region has room), a second one of 40
    for i, first in enumerate((10, 10, 10, 3, 3, 1, 1, 10)):
        w = waves[i]
        for j in range(first):
            t.put(w * BLOCK + 64 + 96 * j + t.rnd.randrange(16))
        for j in range(40):
            t.put((w + W) * BLOCK + 64 + 96 * j + t.rnd.randrange(16))
    # case 3: the region [j - K, j + m + K) of an occurrence at j starts at block offset -17..-15 / ends at 4127..4129
    i = 8
    for r in (0, 1):
        for pi in shorts:
            m = len(pats[pi])
            for edits in (0, K):
                for off in [d + K for d in (-17, -16, -15)] + [e - m - K for e in (4127, 4128, 4129)]:
                    b = waves[i] + r * W
                    i += 1
                    t.put(b * BLOCK + off, pi, edits)
                    t.put(b * BLOCK + 1500 + 8 * (i % 9), None)       # (and an ordinary one in the same block)
    assert i <= len(waves) and waves[-1] + W + 2 < blocks
    return t


def _pair_text(pats, shorts, pairs):
    """case 4: R X texts of the pattern pairs (X at an even and at an odd position) inside blocks that hold some 110 other
    occurrences: more than 64 lookup hits, so the block takes several batches.  Behind them case 3 again for every short
    length of this set, one plant per seam"""
    t = _Text(35, PAIR_BLOCKS, pats, shorts, 36)
    plain = [i for i in shorts if i not in [y for y, _, _ in pairs]]
    t.shorts = plain
    for b, parity0 in ((3, 0), (9, 1)):
        at = [8 + 16 * j for j in range(len(pairs))]                  # the pairs take two places of 32 bytes each
        t.dense(b, skip=set(at) | {a + 1 for a in at})
        for j, (yi, xi, r_len) in enumerate(pairs):
            xpos = b * BLOCK + 32 * at[j] + 28
            xpos += (xpos & 1) ^ ((parity0 + j) & 1)
            t.put(xpos - r_len, yi, 0)
            t.put(xpos, xi, 0, overlay=True)
    b = 12
    for pi in plain:
        m = len(pats[pi])
        for off in [d + K for d in (-17, -16, -15)] + [e - m - K for e in (4127, 4128, 4129)]:
            t.put(b * BLOCK + off, pi, 0)
            b += 2
    assert b < PAIR_BLOCKS
    return t


def _evaluate(ctx, t, full):
    """AUTO against BITPAR on t's text, counts and records; the literal oracle around the planted blocks"""
    text = t.check_plants()
    ctx.set_kernel("auto")
    counts = ctx.count_buffer(text)
    stats = {s: ctx.stat(s) for s in ("sieve_on", "sieve_stride", "sieve_cf", "sieve_cf_dp_slots", "sieve_clist", "sieve_waves",
                                      "sieve_candidates")}
    out = dict(stats=stats, counts=counts, blocks=len(text) // BLOCK, planted_blocks=sorted(t.blocks))
    if not full:
        return out
    rec, total = ctx.find_all_buffer(text, sum(counts) + 64)
    ctx.set_kernel("bitpar")
    b_counts = ctx.count_buffer(text)
    b_rec, b_total = ctx.find_all_buffer(text, sum(b_counts) + 64)
    ctx.set_kernel("auto")
    planted = [0] * len(t.pats)
    for pos, pi, _, _ in t.plants:
        planted[pi] += 1
    out.update(bitpar_counts=b_counts, n_found=total, bitpar_n_found=b_total, n_records=len(rec), records_equal=rec == b_rec,
               records_unique=len(set(rec)) == len(rec), planted=planted)
    # neighbourhoods (+- 64 bytes) of the planted blocks, merged where they touch
    spans, n = [], len(text)
    for b in sorted(t.blocks):
        s, e = max(0, BLOCK * b - 64), min(n - K, BLOCK * (b + 1) + 64)
        if spans and s <= spans[-1][1]:
            spans[-1][1] = e
        else:
            spans.append([s, e])
    by_pat = [[] for _ in t.pats]
    for q, j in rec:
        by_pat[q].append(j)
    wrong, checked = [], 0
    for i, p in enumerate(t.pats):
        for s, e in spans:
            got = [j for j in by_pat[i] if s <= j < e]
            want = H.oracle_counts(text, [p], K, banded=len(p) > 32, j_begin=s, j_end=e)[0]
            if len(got) != want or any(H.window_distance(p, text[j:j + len(p)]) > K for j in got):
                wrong.append((len(p), s, e, want, got))
            checked += want
    out.update(oracle_wrong=wrong[:5], oracle_checked=checked, n_plants=len(t.plants))
    return out


def _worker(mode):
    apm = H.pkg()
    out = {}
    with apm.ApmContext(device=0) as ctx:
        for lens in SLOTTED:
            pats, shorts = _slotted_patterns(lens), list(range(len(lens)))
            ctx.set_patterns(pats, K)
            ctx.count_buffer(Q._random_text(30, 4 * BLOCK, ACGT))
            if 0 < ctx.stat("sieve_cf_dp_slots") < 7:
                break
        out["slotted_lengths"] = lens
        out["dense"] = _evaluate(ctx, _dense_text(pats, shorts), mode == "full")
        if mode == "full":
            # size the text from the geometry the launch reports: W grows with the text up to the device's cap
            blocks = 2 * 8192 + 8
            for _ in range(6):
                ctx.count_buffer(Q._random_text(33, blocks * BLOCK + 1234, ACGT))
                W = int(ctx.stat("sieve_waves"))
                assert W > 0
                if blocks >= 2 * W + 8:
                    break
                blocks = 2 * W + 8
            assert blocks >= 2 * W + 8 and (blocks + 1) * BLOCK <= Q.CAP_BYTES, (blocks, W)
            out["big"] = _evaluate(ctx, _big_text(pats, shorts, W, blocks), True)
            out["big"]["W"] = W
    if mode == "full":
        pats, shorts, pairs = Q._part1_patterns()
        with apm.ApmContext(device=0) as ctx:
            ctx.set_patterns(pats, K)
            out["pair"] = _evaluate(ctx, _pair_text(pats, shorts, pairs), True)
    print(json.dumps(out))


@functools.lru_cache(maxsize=None)
def _run(name, mode="full"):
    env = NO_LIST if name == "nolist" else SETTINGS[name]
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _check(res, slotted, where):
    st = res["stats"]
    assert st["sieve_on"] == 1 and st["sieve_stride"] == 1 and st["sieve_cf"] > 0 and st["sieve_clist"] == 1, (where, st)
    if slotted:      # every candidate unit holds a slot: each planted occurrence makes a pending entry
        assert 0 < st["sieve_cf_dp_slots"] < 7, (where, st)
    else:            # more candidate units than slots: slotted and slotless units side by side
        assert st["sieve_cf_dp_slots"] == 7, (where, st)
    assert res["counts"] == res["bitpar_counts"], where
    assert res["n_found"] == res["bitpar_n_found"] == res["n_records"] == sum(res["counts"]), where
    assert res["records_equal"] and res["records_unique"], where
    assert res["oracle_wrong"] == [] and res["oracle_checked"] >= res["n_plants"], (where, res["oracle_wrong"])
    assert all(c >= p for c, p in zip(res["counts"], res["planted"])), where


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_dense_block_overruns_pending_list_and_queue(setting):
    """case 1: 127 occurrences in one block, each with a pending entry or more"""
    res = _run(setting)["dense"]
    _check(res, True, setting)
    assert sum(res["planted"]) == DENSE and res["blocks"] == SMALL_BLOCKS
    print("short lengths whose units all hold a slot:", _run(setting)["slotted_lengths"])


def test_dense_block_candidates_below_the_filter_alone():
    """the DP stage judged the block's entries instead of sending them all to the bit: with the list on, fewer candidates
    reach the verify launch than the code filter alone hands over (the units of random text that the DP rejects)"""
    with_dp, without = _run("default")["dense"], _run("nolist", "candidates")["dense"]
    assert with_dp["stats"]["sieve_clist"] == 1 and without["stats"]["sieve_clist"] == 0
    assert with_dp["counts"] == without["counts"]
    print("sieve_candidates: %d with the window DP, %d without" % (with_dp["stats"]["sieve_candidates"], without["stats"]["sieve_candidates"]))
    assert with_dp["stats"]["sieve_candidates"] < without["stats"]["sieve_candidates"]


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_block_end_reservation_and_region_boundaries(setting):
    """cases 2 and 3: blocks of 40 occurrences behind blocks of 1, 3 and 10 of the same wave (at region caps of 1 and 5 the
    block-end reservation fails with entries queued), and regions on both sides of the strip's bounds"""
    res = _run(setting)["big"]
    _check(res, True, setting)
    W = res["W"]
    assert res["stats"]["sieve_waves"] == W and res["blocks"] >= 2 * W + 8, "the plants were placed for another wave count"
    runs_of = {}
    for b in res["planted_blocks"]:
        runs_of.setdefault(b % W, set()).add(b // W)
    assert sum(1 for r in runs_of.values() if r >= {0, 1}) >= 8, "waves with plants in their first and their second block"


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_pending_pair_whose_bit_is_set_later_in_the_block(setting):
    """case 4: units of two patterns at one pair index, one with a slot and one without, in blocks of several batches"""
    res = _run(setting)["pair"]
    _check(res, False, setting)


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker(sys.argv[1])
