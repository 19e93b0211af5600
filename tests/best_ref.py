"""The truth of the best-hit tests: the complete scored record set of a text -- from the oracle's range counts plus
helpers.window_distance, as tests/test_score_gpu.py computes it -- and the rule of include/apm.h ("best hits") applied
literally over a {(pattern, pos): dist} map.  The map stands for s(i, j) on all of W because a start that is not a record
is either outside W or scores k + 1: it never suppresses.  Also the planted texts of test_score_gpu.py, rebuilt here, and
a restatement of the text modes for the host-level tests."""
import random

import helpers as H

DNA = b"ACGT"


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


def planted(k, lens, seed, edits=None, gaps=4096, limit=8192):
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
    assert {s % 16 for s in starts} == set(range(16)) and len(text) <= limit
    return pats, bytes(text)


# ---------------------------------------------------------------- the complete scored record set, computed once per text
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
    """s(i, pos) of the rule: what the scoring pass writes for a window inside the text"""
    size = min(len(pat), len(text) - pos)
    return min(H.window_distance(pat[:size], text[pos:pos + size]), k + 1)


_cache = {}


def ref_records(text, pats, k):
    """[(pattern, pos, dist)] sorted: every record the find calls report, scored"""
    key = (text, tuple(pats), k)
    if key not in _cache:
        rec = [(i, j, score(text, p, j, k)) for i, p in enumerate(pats) for j in _positions(text, p, k)]
        assert all(d <= k for _, _, d in rec)
        _cache[key] = rec
    return _cache[key]


# ---------------------------------------------------------------- the rule
def is_best(scores, i, pos, s0, k, r, n):
    """the three conditions, literally; scores: {(pattern, j): s(pattern, j)} of every j in W that scores <= k"""
    w_end = max(0, n - k)
    if s0 > k:
        return False
    if any(scores.get((i, j), k + 1) <= s0 for j in range(max(0, pos - r), pos) if j < w_end):
        return False
    if any(scores.get((i, j), k + 1) < s0 for j in range(pos + 1, pos + r + 1) if j < w_end):
        return False
    return True


def best_hits(text, pats, k, r, seeds=None):
    """[(pattern, pos, dist)] sorted: the best hits at radius r among `seeds` ([(pattern, pos)], any order, duplicates kept
    as often as they come, records that name no window dropped) -- default: among the complete record set"""
    full = ref_records(text, pats, k)
    scores = {(i, j): d for i, j, d in full}
    n = len(text)
    if seeds is None:
        cand = full
    else:
        cand = [(i, pos, scores[(i, pos)] if (i, pos) in scores else score(text, pats[i], pos, k))
                for i, pos in seeds if i < len(pats) and pos < n]
    return sorted((i, pos, d) for i, pos, d in cand if is_best(scores, i, pos, d, k, r, n))


# ---------------------------------------------------------------- text modes (include/apm.h: "text modes", "sequences")
def normalise(src, fasta=True, upper=True):
    """(T, src_of, seq_of, names): the kept bytes, the source offset of each, per kept byte the index of its sequence, and
    the sequences' names ("-" for the bytes in front of the first header)"""
    kept, src_of, seq_of, names = bytearray(), [], [], ["-"]
    i, line_start, n = 0, True, len(src)
    while i < n:
        c = src[i]
        if fasta and line_start and c == ord(">"):
            e = src.find(b"\n", i)
            e = n if e < 0 else e + 1
            names.append(src[i + 1:e].split()[0].decode() if src[i + 1:e].split() else "")
            i, line_start = e, True
            continue
        line_start = c == ord("\n")
        if not (fasta and c in (ord("\n"), ord("\r"))):
            kept.append(c - 32 if upper and ord("a") <= c <= ord("z") else c)
            src_of.append(i)
            seq_of.append(len(names) - 1)
        i += 1
    return bytes(kept), src_of, seq_of, names
