"""Reference of the nearest-occurrence search per sequence (include/apm.h: "nearest occurrences per sequence"): nearest_ref
applied to every slice T[t_begin[s] : t_begin[s+1]] as a text of its own, ends and starts shifted by t_begin[s].  Row
s * P + i of every result is the pair (sequence s, pattern i).  The host-level path: textnorm_ref / seqindex_ref give T and
the table of a source, and the records' positions go back to source offsets."""
import nearest_ref as N
import seqindex_ref as SQ
import textnorm_ref as TN

NO_START = N.NO_START
NONE = N.NONE
INVALID = N.INVALID


def begins_of(cuts, n):
    """t_begin[0 .. n_seq] of a text of n bytes cut at `cuts` (any order, repeats make empty sequences)"""
    return [0] + sorted(min(c, n) for c in cuts) + [n]


def keys(text, pats, begins, lo=0, hi=None, off=0):
    """the n_seq * P keys a scan of the ends [lo, hi) of `text` leaves; an end e is reported as off + e"""
    hi = len(text) if hi is None else hi
    out = []
    for s in range(len(begins) - 1):
        b, e = begins[s], begins[s + 1]
        if b == e:
            out += [NONE] * len(pats)
        else:
            out += N.keys(text[b:e], pats, max(lo - b, 0), max(min(hi, e) - b, 0), off + b)
    return out


def records(text, pats, begins, off=0):
    """([(pos, pattern, dist)] end records, the same of the start records), n_seq * P each"""
    ends, starts = [], []
    for s in range(len(begins) - 1):
        b = begins[s]
        e_s, s_s = N.records(text[b:begins[s + 1]], pats)
        ends += [(p if p == NO_START else off + b + p, i, d) for p, i, d in e_s]
        starts += [(p if p == NO_START else off + b + p, i, d) for p, i, d in s_s]
    return ends, starts


def source_records(src, flags, pats):
    """(n_seq, ends, starts) of the host-level call on the source `src` in the text mode `flags`: positions are source offsets"""
    T, src_of = TN.normalize(src, flags)
    table = SQ.sequences(src, flags)
    begins = [t for _, t in table]
    ends, starts = records(T, pats, begins)
    back = lambda r: r if r[0] == NO_START else (src_of[r[0]],) + r[1:]
    return len(table) - 1, [back(r) for r in ends], [back(r) for r in starts]


def literal(text, p, b, e):
    """(d, end, start) of pattern p in text[b:e] by the definition, written out: the full DP table of the slice with
    C[y][0] = y, the first end of the smallest E, then the shortest suffix of the slice's prefix that attains it; None
    where no end has E < m"""
    t, m = text[b:e], len(p)
    col = list(range(m + 1))
    best = None
    for x, c in enumerate(t):
        new = [0] * (m + 1)
        for y in range(1, m + 1):
            new[y] = min(col[y - 1] + (p[y - 1] != c), col[y] + 1, new[y - 1] + 1)
        col = new
        if col[m] < m and (best is None or col[m] < best[0]):
            best = (col[m], x)
    if best is None:
        return None
    d, x = best

    def dist(a, s):
        row = list(range(len(s) + 1))
        for i in range(1, len(a) + 1):
            nw = [i] + [0] * len(s)
            for j in range(1, len(s) + 1):
                nw[j] = min(row[j - 1] + (a[i - 1] != s[j - 1]), row[j] + 1, nw[j - 1] + 1)
            row = nw
        return row[len(s)]

    for L in range(1, min(m + d, x + 1) + 1):
        if dist(p, t[x + 1 - L:x + 1]) == d:
            return d, b + x, b + x + 1 - L
    raise AssertionError("no span attains the distance")
