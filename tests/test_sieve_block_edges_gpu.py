"""The sieve at the EDGES of its blocks: a wave scans four 1 KiB chunks (one 4 KiB block) per trip and drops the hits of
the chunks behind the scanned range -- one scalar mask per block.  Counts through the default path against the oracle's
(helpers.oracle_counts), on ACGT texts of the synthetic fill, at text lengths whose chunk count modulo 4 is 0, 1, 2 and 3
(one of them large enough that every wave of the launch has a last, partial trip), each scanned twice: whole, and with an
owner range that ends in the middle of a chunk while the chunks behind it hold real text.

Patterns of m = 16, 20, 34, 67 and 128 together, at k = 3, 2 and 1, with occurrences of 0..k edits planted
  - ending in the last byte of the owner range,
  - starting in the first chunk behind it (the oracle of the range does not count it, the oracle of the whole text does),
  - across a chunk border and across a block border,
  - within 16 bytes of the text's front.

The 64 KiB case runs again with candidate-list regions of four entries (APM_CLIST_REGION_CAP=4: the overflow rows) and
with the column form of the window DP (APM_CF_DP_DIAG=0: the other kernel over the same body).  Those switches are read
once per process: one worker per setting."""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

CHUNK, BLOCK = 1024, 4096
KIB = 1024
LENGTHS = [KIB - 1, KIB, 4 * KIB - 1, 4 * KIB + 1, 5 * KIB, 7 * KIB + 3, 64 * KIB + 1025, 3 * KIB * KIB + 2049]
KS = [3, 2, 1]
LENS = [16, 20, 34, 67, 128]
ACGT = b"ACGT"
SEED = 0x5EED0012
OVERFLOW_LENGTH = 64 * KIB + 1025
SETTINGS = {"cap4": {"APM_CLIST_REGION_CAP": "4"}, "column": {"APM_CF_DP_DIAG": "0"}}


def _patterns(k):
    rnd = random.Random(1800 + k)
    return [bytes(rnd.choice(ACGT) for _ in range(m)) for m in LENS]


def _edited(rnd, p, budget):
    """p with edits worth `budget`: a substitution costs 1, an insertion or a deletion 2 -- the window of len(p) bytes at
    the planted string's start is then within `budget` of p (the indel's own edit and the byte the window gains or loses)"""
    p = bytearray(p)
    while budget > 0:
        r, pos = rnd.random(), rnd.randrange(len(p))
        if r < 0.5 or budget < 2:
            p[pos] = ACGT[(ACGT.index(p[pos]) + 1 + rnd.randrange(3)) % 4]
            budget -= 1
        elif r < 0.75:
            del p[pos]
            budget -= 2
        else:
            p.insert(pos, rnd.choice(ACGT))
            budget -= 2
    return bytes(p)


def _owner_end(n):
    """an owner end in the middle of a chunk, with a chunk of real text behind that chunk where the text has one"""
    q = (n - 160) // CHUNK          # the last chunk that holds 160 bytes of text or more
    return (q - 1) * CHUNK + 500 if q >= 1 else n - 300


@functools.lru_cache(maxsize=None)
def _case(n, k):
    """(text, patterns, owner end, [(site, position, pattern, length)], oracle counts of the whole text, ... of [0, owner end))"""
    apm = H.pkg()
    text = bytearray(apm.synth_fill_host(0, n, SEED + n))
    pats = _patterns(k)
    oe = _owner_end(n)
    rnd = random.Random(n * 7 + k)
    placed, used = [], []

    def put(site, where, pi, edits):
        """where(length of the planted string) -> its position; left out where it does not fit or meets another plant"""
        w = _edited(rnd, pats[pi], edits)
        pos = where(len(w))
        if pos < 0 or pos + len(w) > n or any(pos < e + 4 and b < pos + len(w) + 4 for b, e in used):
            return
        text[pos:pos + len(w)] = w
        used.append((pos, pos + len(w)))
        placed.append((site, pos, pi, len(w)))

    put("range_end", lambda ln: oe - ln, 4, k)        # its last byte is the range's last
    behind = (oe // CHUNK + 1) * CHUNK                # the first chunk behind the range; a text that ends before it: behind oe
    put("behind", lambda ln: (behind + 5) if behind + 200 <= n else oe + 7, 3, k - 1)
    put("front", lambda ln: 3, (k + 1) % 5, k)
    # across the chunk borders and the block borders inside the range: by half, by its first byte only, by all but its last
    borders = [(c * CHUNK, "chunk") for c in (1, 2, 3, 5, 6, 7)] + [(b * BLOCK, "block") for b in (1, 2, 3, 4, 5, 6)]
    for i, (border, site) in enumerate(borders):
        if border + 200 < oe:
            put(site, lambda ln: border - (ln // 2, 1, ln - 1)[i % 3], (i + k) % 5, i % (k + 1))
    text = bytes(text)
    banded = [len(p) > 32 for p in pats]
    whole = [H.oracle_counts(text, [p], k, banded=b)[0] for p, b in zip(pats, banded)]
    ranged = [H.oracle_counts(text, [p], k, banded=b, j_begin=0, j_end=oe)[0] for p, b in zip(pats, banded)]
    return text, pats, oe, placed, whole, ranged


def _scan(ctx, text, pats, k, oe):
    """[counts of the whole text, counts of the owner range [0, oe)] through apm_count_shard_device"""
    import torch
    n = len(text)
    d_text = torch.zeros(n + BLOCK + 64, dtype=torch.uint8, device="cuda:0")
    d_text[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
    cnt = torch.zeros(len(pats), dtype=torch.int64, device="cuda:0")
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    out = []
    for end in (n, oe):
        cnt.zero_()
        torch.cuda.synchronize()
        ctx.count_shard_device(d_text.data_ptr(), 0, n, n, 0, end, cnt.data_ptr())
        ctx.synchronize()
        out.append(cnt.cpu().tolist())
    return out, {s: ctx.stat(s) for s in ("sieve_on", "sieve_stride", "sieve_cf", "sieve_cf_dp_slots", "sieve_cf_dp_form", "sieve_clist")}


def _check(n, k, got, stats):
    text, pats, oe, placed, whole, ranged = _case(n, k)
    sites = [s for s, _, _, _ in placed]
    print("n %d k %d owner end %d plants %s stats %s" % (n, k, oe, sites, stats))
    print("oracle whole %s range %s, got %s" % (whole, ranged, got))
    # the construction: the plants are there, and the one behind the range is what the two oracle counts differ by
    assert {"range_end", "behind", "front"} <= set(sites), sites
    if n > 5 * KIB:
        assert sites.count("chunk") >= 3 and sites.count("block") >= 1, sites
    for site, pos, pi, ln in placed:
        if site == "behind":
            assert pos >= oe and whole[pi] > ranged[pi], (site, pos, oe)
        else:
            assert pos < oe and ranged[pi] >= 1, (site, pos, oe)
    assert got[0] == whole, (n, k, "whole text")
    assert got[1] == ranged, (n, k, "owner range [0, %d)" % oe)


@pytest.fixture(scope="module")
def ctx():
    with H.pkg().ApmContext(device=0) as c:
        yield c


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", LENGTHS)
def test_counts_at_block_edges(ctx, n, k):
    text, pats, oe = _case(n, k)[:3]
    got, stats = _scan(ctx, text, pats, k, oe)
    _check(n, k, got, stats)
    # the code under test ran: the stride-1 sieve with the code filter and the DIAGONAL window DP (form 2: the kernel whose
    # streaming loop drops the chunks behind the range by the block's mask)
    assert stats["sieve_on"] == 1 and stats["sieve_stride"] == 1 and stats["sieve_cf"] > 0, stats
    assert stats["sieve_cf_dp_slots"] > 0 and stats["sieve_cf_dp_form"] == 2 and stats["sieve_clist"] == 1, stats


def _worker():
    out = {}
    with H.pkg().ApmContext(device=0) as c:
        for k in KS:
            text, pats, oe = _case(OVERFLOW_LENGTH, k)[:3]
            got, stats = _scan(c, text, pats, k, oe)
            out[str(k)] = dict(got=got, stats=stats)
    print(json.dumps(out))


@functools.lru_cache(maxsize=None)
def _run(setting):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, env=dict(os.environ, **SETTINGS[setting]), timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_counts_with_small_list_regions_and_column_form(setting, k):
    res = _run(setting)[str(k)]
    _check(OVERFLOW_LENGTH, k, res["got"], res["stats"])
    assert res["stats"]["sieve_on"] == 1 and res["stats"]["sieve_cf"] > 0 and res["stats"]["sieve_clist"] == 1, res["stats"]
    # the form that ran: the column kernel (1) where it is asked for, the diagonal one (2) with the small list regions
    assert res["stats"]["sieve_cf_dp_form"] == (1 if setting == "column" else 2), res["stats"]


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker()
