"""Reference of the occurrence search (include/apm.h: "occurrence search"): the literal recurrence
    C[0][x] = 0, C[y][0] = y, C[y][x] = min(C[y-1][x-1] + (p[y-1] != T[x-1]), C[y-1][x] + 1, C[y][x-1] + 1)
in numpy, column by column: new = min(diag, left + 1), then the vertical pass as y + minimum.accumulate(new - y).
E(e) = C[m][e+1]; the reported ends under both flags; the pinned span (d*, the SMALLEST L that attains it)."""
import numpy as np

ALL, LOCAL_MIN = 0, 1
NO_START = (1 << 64) - 1


def ends_scores(text, p):
    """E(e) for every e in [0, n) as an int array"""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    pat = np.frombuffer(bytes(p), dtype=np.uint8)
    m = len(pat)
    y = np.arange(m + 1, dtype=np.int64)
    col = y.copy()
    out = np.empty(len(t), dtype=np.int64)
    new = np.empty(m + 1, dtype=np.int64)
    for x in range(len(t)):
        new[0] = 0
        np.minimum(col[:-1] + (pat != t[x]), col[1:] + 1, out=new[1:])
        col = y + np.minimum.accumulate(new - y)
        out[x] = col[m]
    return out


def reported(E, m, k, flags):
    """the ends reported under `flags`, ascending"""
    n = len(E)
    ok = E <= k
    if flags == LOCAL_MIN and n:
        prev = np.concatenate(([m], E[:-1]))
        nxt = np.concatenate((E[1:], [np.iinfo(np.int64).max]))
        ok &= (prev > E) & (nxt >= E)
    return np.nonzero(ok)[0]


def global_dist(p, s):
    """dist(p, s): the square recurrence, both ends fixed"""
    a = np.frombuffer(bytes(p), dtype=np.uint8)
    y = np.arange(len(a) + 1, dtype=np.int64)
    col = y.copy()
    new = np.empty(len(a) + 1, dtype=np.int64)
    for x, c in enumerate(bytes(s)):
        new[0] = x + 1
        np.minimum(col[:-1] + (a != c), col[1:] + 1, out=new[1:])
        col = y + np.minimum.accumulate(new - y)
    return int(col[len(a)])


def span(text, p, k, e):
    """(start or None, distance): the span record of end e -- d* over L in [1, min(m + k, e + 1)], the smallest L first"""
    m = len(p)
    rp = np.frombuffer(bytes(p)[::-1], dtype=np.uint8)
    y = np.arange(m + 1, dtype=np.int64)
    col = y.copy()
    new = np.empty(m + 1, dtype=np.int64)
    best, at = None, 0
    for L in range(1, min(m + k, e + 1) + 1):
        new[0] = L
        np.minimum(col[:-1] + (rp != text[e + 1 - L]), col[1:] + 1, out=new[1:])
        col = y + np.minimum.accumulate(new - y)
        if best is None or col[m] < best:
            best, at = int(col[m]), L
    if best is not None and best <= k:
        return e + 1 - at, best
    return None, k + 1


def records(text, pats, k, flags, lo=0, hi=None):
    """[(pattern, end, E(end))] sorted, the ends in [lo, hi)"""
    out = []
    for i, p in enumerate(pats):
        E = ends_scores(text, p)
        for e in reported(E, len(p), k, flags):
            if lo <= e and (hi is None or e < hi):
                out.append((i, int(e), int(E[e])))
    return out


def span_many(text, p, k, ends):
    """`span` of MANY ends of one pattern: its columns on an (m + 1, R) array, one column per end; ([start or None],
    [distance]).  tests check it against `span`."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    ends = np.asarray(ends, dtype=np.int64)
    m, n_rec = len(p), len(ends)
    rp = np.frombuffer(bytes(p)[::-1], dtype=np.uint8)[:, None]
    y = np.arange(m + 1, dtype=np.int32)[:, None]
    col = np.repeat(y, n_rec, axis=1)
    new = np.empty((m + 1, n_rec), dtype=np.int32)
    best = np.full(n_rec, np.iinfo(np.int32).max, dtype=np.int32)
    at = np.zeros(n_rec, dtype=np.int64)
    for L in range(1, m + k + 1):
        live = ends + 1 >= L                      # L in [1, min(m + k, e + 1)]
        if not live.any():
            break
        c = t[np.maximum(ends + 1 - L, 0)]
        new[0] = L
        np.minimum(col[:-1] + (rp != c), col[1:] + 1, out=new[1:])
        col = y + np.minimum.accumulate(new - y, axis=0)
        better = live & (col[m] < best)           # the smallest L first
        best[better] = col[m][better]
        at[better] = L
    return ([int(e) + 1 - int(a) if b <= k else None for e, a, b in zip(ends, at, best)],
            [int(b) if b <= k else k + 1 for b in best])


def global_dist_many(p, text, spans):
    """`global_dist`(p, text[s : e + 1]) of MANY spans (s, e): its columns on an (m + 1, R) array; a span that has ended keeps
    its column.  tests check it against `global_dist`."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    s = np.asarray([a for a, _ in spans], dtype=np.int64)
    length = np.asarray([b + 1 - a for a, b in spans], dtype=np.int64)
    m, n_rec = len(p), len(spans)
    a = np.frombuffer(bytes(p), dtype=np.uint8)[:, None]
    y = np.arange(m + 1, dtype=np.int32)[:, None]
    col = np.repeat(y, n_rec, axis=1)
    new = np.empty((m + 1, n_rec), dtype=np.int32)
    for x in range(int(length.max()) if n_rec else 0):
        live = length > x
        c = t[np.minimum(s + x, len(t) - 1)]
        new[0] = x + 1
        np.minimum(col[:-1] + (a != c), col[1:] + 1, out=new[1:])
        col = np.where(live, y + np.minimum.accumulate(new - y, axis=0), col)
    return [int(d) for d in col[m]]


def records_many(text, pats, k):
    """{flags: [(pattern, end, E(end))] sorted} of MANY patterns of one length: ends_scores' recurrence, column by column, on
    an (m + 1, P) array -- one column per pattern -- and `reported`'s predicate on the last three scores, so that no
    (P, n) table is kept.  tests check it against `records`."""
    t = np.frombuffer(bytes(text), dtype=np.uint8)
    P, m = len(pats), len(pats[0])
    assert all(len(p) == m for p in pats)
    pat = np.frombuffer(b"".join(bytes(p) for p in pats), dtype=np.uint8).reshape(P, m).T   # (m, P)
    neq = {int(c): (pat != c).astype(np.int32) for c in np.unique(t)}
    y = np.arange(m + 1, dtype=np.int32)[:, None]
    col = np.repeat(y, P, axis=1)
    new = np.empty((m + 1, P), dtype=np.int32)
    big = np.iinfo(np.int32).max
    e2 = np.full(P, big, dtype=np.int32)          # E(e - 2) while end e - 1 is decided; in front of the text: anything > m
    e1 = np.full(P, m, dtype=np.int32)            # E(-1) = m
    out = {ALL: [], LOCAL_MIN: []}

    def decide(e, prev, cur, nxt):
        ok = cur <= k
        for i in np.nonzero(ok)[0]:
            out[ALL].append((int(i), e, int(cur[i])))
        for i in np.nonzero(ok & (prev > cur) & (nxt >= cur))[0]:
            out[LOCAL_MIN].append((int(i), e, int(cur[i])))

    for x in range(len(t)):
        new[0] = 0
        np.minimum(col[:-1] + neq[int(t[x])], col[1:] + 1, out=new[1:])
        col = y + np.minimum.accumulate(new - y, axis=0)
        cur = col[m]
        if x:
            decide(x - 1, e2, e1, cur)
        e2, e1 = e1, cur.copy()
    if len(t):
        decide(len(t) - 1, e2, e1, np.full(P, big, dtype=np.int32))
    return {f: sorted(r) for f, r in out.items()}


def records_with_starts(text, pats, k, flags):
    return [(i, e, d, span(text, pats[i], k, e)[0]) for i, e, d in records(text, pats, k, flags)]


def planted(seed, lens, k, n, alphabet=b"ACGT", copies=3):
    """a random text of n bytes with, per pattern, copies carrying substitutions AND net insertions / deletions (lengths
    m - k .. m + k), planted at start residues that run through 0..15 mod 16; (patterns, text)"""
    rs = np.random.RandomState(seed)
    a = np.frombuffer(alphabet, dtype=np.uint8)
    text = bytearray(a[rs.randint(0, len(a), size=n)].tobytes())
    pats = [a[rs.randint(0, len(a), size=m)].tobytes() for m in lens]
    slot, q = n // max(1, len(pats) * copies * 2 + 1), 0
    for i, p in enumerate(pats):
        for c in range(copies * 2):
            s = bytearray(p)
            edits = min(k, c % (k + 1)) if k else 0
            kind = c % 3  # 0: substitutions, 1: deletions from the pattern, 2: insertions into it
            for _ in range(edits):
                if kind == 0 or len(s) <= 1:
                    at = rs.randint(0, len(s))
                    s[at] = int(a[(list(a).index(s[at]) + 1) % len(a)]) if s[at] in a else int(a[0])
                elif kind == 1:
                    del s[rs.randint(0, len(s))]
                else:
                    s.insert(rs.randint(0, len(s) + 1), int(a[rs.randint(0, len(a))]))
            at = q * slot
            at += (q % 16 - at % 16) % 16  # start residue q mod 16
            if at + len(s) <= n:
                text[at:at + len(s)] = s
            q += 1
    return pats, bytes(text)
