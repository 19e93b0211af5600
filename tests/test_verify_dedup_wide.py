"""The verify kernels' dedup of matches (ApmVerifyCore::count_matches): a window counts once, from its first true
(unit, shift) nominator, however many units and shifts nominate it and whichever waves they land in.

With a band (k >= 1) the kernels resolve all the matches of a DP round side by side, one lane per (match, earlier
nominator) pair, in passes of 64 pairs.  The texts here make a round hold many matches (a 16-byte pattern repeated: every
period has several matching windows, each nominated by several units and shifts) and more than 64 pairs (m = 64, k = 7:
up to 55 earlier nominators per match, occurrences planted back to back), put a window's nominators into different waves
(candidate-list regions of 1 and 5 entries dealt one entry per wave; occurrences across 4 KiB seams), and reach the text's
edges (window starts below 20, where the predicate's partner text lies in front of the text; the last full window).
Every caller of count_matches runs them: the list-driven and the mask-driven verify kernels, without the code filter, and
the fused kernel in both its forms (a worker process per switch setting: the switches are read once per process).
Counts equal the literal oracle's; the records of apm_find_all_buffer are distinct, each a window within k, and as many
per pattern as the oracle counts -- the oracle's (pattern, position) set, each exactly once."""
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H

BLOCK = 4096
ACGT = b"ACGT"


def _rand(rnd, m):
    return bytes(rnd.choice(ACGT) for _ in range(m))


def _random_text(seed, n):
    table = bytes(ACGT[b & 3] for b in range(256))
    return bytearray(random.Random(seed).randbytes(n).translate(table))


def _edit(rnd, p, n_edits):
    p = bytearray(p)
    for _ in range(n_edits):
        r, pos = rnd.random(), rnd.randrange(len(p))
        if r < 0.4:
            p[pos] = rnd.choice(ACGT)
        elif r < 0.7:
            del p[pos]
        else:
            p.insert(pos, rnd.choice(ACGT))
    return bytes(p)


def _plant(text, rnd, pos, p, k, n_edits):
    """write an occurrence of p with up to n_edits edits at pos such that some window start within k of pos matches;
    returns its length"""
    n = len(text)
    for attempt in range(32):
        w = _edit(rnd, p, max(0, n_edits - attempt // 4))
        assert 0 <= pos and pos + len(w) <= n, "plant outside the text"
        old = bytes(text[pos:pos + len(w)])
        text[pos:pos + len(w)] = w
        for j in range(max(0, pos - k), min(pos + k, n - len(p)) + 1):
            if H.window_distance(p, bytes(text[j:j + len(p)])) <= k:
                return len(w)
        text[pos:pos + len(old)] = old
    raise AssertionError("no matching edit found")


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (text, patterns, k, indices of the patterns the literal oracle judges; the rest take its banded form)"""
    out = {}
    rnd = random.Random(606)
    # (a) a 16-byte pattern repeated to 64 KiB, alone and beside three random patterns.  (e) comes with it: windows at 0, 1,
    # 15, 16, 17 match, and the last full window is the pattern itself
    p16 = _rand(rnd, 16)
    rep = p16 * (65536 // 16)
    others = [_rand(rnd, m) for m in (20, 23, 64)]
    out["rep16"] = (rep, [p16], 3, [0])
    out["rep16+3"] = (rep, [p16] + others, 3, [0])
    # (b) m = 64, k = 7: runs of occurrences with 0..7 edits back to back; (c) occurrences across 4 KiB seams at
    # 4096 b - m / 2; (e) one in front of position 20 and the pattern itself as the last full window
    k = 7
    p64 = _rand(rnd, 64)
    text = _random_text(607, 32 * BLOCK)
    n = len(text)
    pos = 3                                                 # (e): window starts within k of 3
    for run in range(6):
        for e in range(k + 1):
            pos += _plant(text, rnd, pos, p64, k, e)
        pos = BLOCK * (3 * run + 2) + 1000 + 37 * run        # the next run: inside a block, at an odd offset
    for b in range(1, 31, 2):                               # (c)
        _plant(text, rnd, BLOCK * b - 32, p64, k, b % (k + 1))
    text[n - 64:] = p64
    out["m64k7"] = (bytes(text), [p64], k, [0])
    # (d) a sampled set for the fused form: 16 x 64 bytes, k = 2 -- back-to-back runs, seams, both edges
    k = 2
    pats = [_rand(rnd, 64) for _ in range(16)]
    text = _random_text(608, 32 * BLOCK)
    n = len(text)
    pos = 2
    for i, p in enumerate(pats):
        for e in (0, 1, 2, 2):
            pos += _plant(text, rnd, pos, p, k, e)
        _plant(text, rnd, BLOCK * (2 * i + 1) - 32, p, k, i % (k + 1))
        pos = BLOCK * (2 * i + 1) + 700 + 11 * i
    text[n - 64:] = pats[5]
    out["s16x64k2"] = (bytes(text), pats, k, [])
    for name, (text, pats, k, lit) in out.items():
        assert len(text) <= 1 << 20, name
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name):
    text, pats, k, lit = _cases()[name]
    return [H.oracle_counts(text, [p], k, banded=i not in lit)[0] for i, p in enumerate(pats)]


def _worker():
    apm = H.pkg()
    out = {}
    for name, (text, pats, k, _) in _cases().items():
        with apm.ApmContext(device=0) as ctx:
            ctx.set_patterns(list(pats), k)
            ctx.set_kernel("banded")
            counts = ctx.count_buffer(text)
            stats = {s: ctx.stat(s) for s in ("sieve_on", "sieve_stride", "sieve_cf", "sieve_clist", "sieve_fused")}
            rec, total = ctx.find_all_buffer(text, sum(counts) + 64)
            out[name] = dict(counts=counts, records=rec, n_found=total, stats=stats, kernels=[ctx.pattern_kernel(i) for i in range(len(pats))])
    print(json.dumps(out))


ENVS = [{},
        {"APM_CLIST_MIN_BATCH": "1", "APM_CLIST_REGION_CAP": "1"},
        {"APM_CLIST_MIN_BATCH": "1", "APM_CLIST_REGION_CAP": "5"},
        {"APM_SIEVE_CLIST": "0"},
        {"APM_SIEVE_CF": "0"},
        {"APM_FUSED": "1"},
        {"APM_FUSED": "0"}]


def test_the_texts_hold_what_they_are_for():
    """many matching windows per period; more than 64 (match, earlier nominator) pairs possible per round; matches at both
    edges (the oracle, no GPU work)"""
    rep, pats, k, _ = _cases()["rep16"]
    assert _oracle("rep16")[0] >= 3 * (len(rep) // 16) - 8
    assert H.window_distance(pats[0], rep[1:17]) <= k and H.window_distance(pats[0], rep[len(rep) - 16:]) == 0
    text, pats, k, _ = _cases()["m64k7"]
    assert _oracle("m64k7")[0] >= 6 * 8 + 15 + 1
    assert any(H.window_distance(pats[0], text[j:j + 64]) <= k for j in range(20)) and text[len(text) - 64:] == pats[0]
    text, pats, k, _ = _cases()["s16x64k2"]
    assert all(c >= 5 for c in _oracle("s16x64k2"))
    assert any(H.window_distance(pats[0], text[j:j + 64]) <= k for j in range(20))


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join("%s=%s" % (k[4:], v) for k, v in e.items()) or "default")
def test_each_matching_window_counts_exactly_once(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert sorted(got) == sorted(_cases())
    for name, (text, pats, k, _) in _cases().items():
        res, want, n = got[name], _oracle(name), len(text)
        st = res["stats"]
        where = (name, env, st)
        print(where, res["counts"], want)
        # the verify core ran: every pattern on the BANDED path behind the sieve, in the form the switches ask for
        assert res["kernels"] == [4] * len(pats) and st["sieve_on"] == 1, where
        if not env:      # by default: the mask-driven kernel (one pattern: no code filter, no list), the list-driven one, the fused one
            assert (st["sieve_clist"], st["sieve_fused"]) == {"rep16": (0, 0), "rep16+3": (1, 0), "m64k7": (1, 0), "s16x64k2": (0, 1)}[name], where
        if env.get("APM_FUSED") == "1":
            assert st["sieve_fused"] == 1, where
        elif env.get("APM_FUSED") == "0" or st["sieve_stride"] == 1:
            assert st["sieve_fused"] == 0, where
        if st["sieve_stride"] == 1:
            if env.get("APM_SIEVE_CLIST") == "0":
                assert st["sieve_clist"] == 0, where
            if env.get("APM_SIEVE_CF") == "0":
                assert st["sieve_cf"] == 0, where
        assert res["counts"] == want, where
        rec = [tuple(x) for x in res["records"]]
        assert res["n_found"] == len(rec) == sum(want) and rec == sorted(set(rec)), where
        per = [0] * len(pats)
        for q, j in rec:                                    # each record a window within k: with the counts, the oracle's set
            per[q] += 1
            size = min(len(pats[q]), n - j)
            assert j < n - k and H.window_distance(pats[q][:size], text[j:j + size]) <= k, (where, q, j)
        assert per == want, where


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker()
