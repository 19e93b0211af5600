"""Reference of the nearest-occurrence search (include/apm.h: "nearest occurrences"), on occ_ref's literal recurrence:
d = min over e of E(e), e the SMALLEST end that attains it, the start by occ_ref.span at k := d.  "None" -- no end has
E < m (an empty text, or a pattern that shares no byte with it) -- is the record pair (NO_START, i, m).  The key packs
(d, e) so that the smaller key is the better answer."""
import numpy as np

import occ_ref

NO_START = occ_ref.NO_START
NONE = (1 << 64) - 1          # APM_NEAREST_NONE
INVALID = 0xFFFFFFFF          # APM_DIST_INVALID
END_BITS = 56


def key(dist, end):
    return (dist << END_BITS) | end


def key_dist(k):
    return k >> END_BITS


def key_end(k):
    return k & ((1 << END_BITS) - 1)


def nearest(text, p):
    """(d, e, start), or None where no end has E < m"""
    E = occ_ref.ends_scores(text, p)
    if not len(E) or int(E.min()) >= len(p):
        return None
    d = int(E.min())
    e = int(np.argmax(E == d))  # the first end that attains d
    start, ds = occ_ref.span(text, p, d, e)
    assert start is not None and ds == d
    return d, e, start


def n_attaining(text, p):
    """how many ends attain the smallest E (tests that plant ties assert it is >= 2)"""
    E = occ_ref.ends_scores(text, p)
    return int((E == E.min()).sum())


def best_ends(text, pats, lo=0, hi=None):
    """[(d, e) or None] of MANY patterns over the ends [lo, hi): ends_scores' recurrence, column by column, on an
    (m_max + 1, P) array -- one column per pattern, a shorter pattern padded (row y depends on the rows above it alone, so
    E_i is row m_i) -- keeping the running minimum and the first end that attains it, so that no (P, n) table is kept.
    tests check it against `nearest`."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    hi = len(t) if hi is None else min(hi, len(t))
    P, ms = len(pats), np.array([len(p) for p in pats], dtype=np.int64)
    m_max = int(ms.max())
    pat = np.frombuffer(b"".join(bytes(p).ljust(m_max, b"\0") for p in pats), dtype=np.uint8).reshape(P, m_max).T   # (m_max, P)
    neq = {int(c): (pat != c).astype(np.int32) for c in np.unique(t)}
    y = np.arange(m_max + 1, dtype=np.int32)[:, None]
    col = np.repeat(y, P, axis=1)
    new = np.empty((m_max + 1, P), dtype=np.int32)
    best = ms.astype(np.int32).copy()             # only E < m counts
    at = np.full(P, -1, dtype=np.int64)
    lanes = np.arange(P)
    for x in range(hi):
        new[0] = 0
        np.minimum(col[:-1] + neq[int(t[x])], col[1:] + 1, out=new[1:])
        col = y + np.minimum.accumulate(new - y, axis=0)
        if x >= lo:
            cur = col[ms, lanes]
            better = cur < best
            best[better] = cur[better]
            at[better] = x
    return [(int(b), int(a)) if a >= 0 else None for b, a in zip(best, at)]


def records(text, pats):
    """([(pos, pattern, dist)] end records, the same of the start records), in pattern order"""
    ends, starts = [], []
    for i, (p, r) in enumerate(zip(pats, best_ends(text, pats))):
        if r is None:
            ends.append((NO_START, i, len(p)))
            starts.append((NO_START, i, len(p)))
        else:
            start, ds = occ_ref.span(text, p, r[0], r[1])
            assert start is not None and ds == r[0]
            ends.append((r[1], i, r[0]))
            starts.append((start, i, r[0]))
    return ends, starts


def keys(text, pats, lo=0, hi=None, off=0):
    """the keys a scan of the ends [lo, hi) of `text` leaves, an end e reported as off + e"""
    return [NONE if r is None else key(r[0], off + r[1]) for r in best_ends(text, pats, lo, hi)]
