"""Reference of the occurrence search per sequence (include/apm.h: "occurrence search per sequence"): occ_ref applied to every
slice T[t_begin[s] : t_begin[s+1]] as a text of its own, ends and starts shifted by t_begin[s].  The host-level path:
textnorm_ref / seqindex_ref give T and the table of a source, and the records' positions go back to source offsets."""
import bisect

import occ_ref as O
import seqindex_ref as SQ
import textnorm_ref as TN

ALL, LOCAL_MIN = O.ALL, O.LOCAL_MIN
NO_START = O.NO_START


def begins_of(cuts, n):
    """t_begin[0 .. n_seq] of a text of n bytes cut at `cuts` (any order, repeats make empty sequences)"""
    return [0] + sorted(min(c, n) for c in cuts) + [n]


def seq_of(begins, e):
    """s(e): the largest s with t_begin[s] <= e, among the sequences [0, n_seq)"""
    return min(bisect.bisect_right(begins, e) - 1, len(begins) - 2)


def records(text, pats, k, flags, begins, lo=0, hi=None):
    """[(pattern, end, E_s(end))] sorted, the ends in [lo, hi)"""
    out = []
    for s in range(len(begins) - 1):
        b, e = begins[s], begins[s + 1]
        if b < e:
            out += [(i, b + x, d) for i, x, d in O.records(text[b:e], pats, k, flags) if lo <= b + x and (hi is None or b + x < hi)]
    return sorted(out)


def records_both(text, pats, k, begins):
    """{flags: records} under both flags, every slice's scores computed once"""
    out = {ALL: [], LOCAL_MIN: []}
    for s in range(len(begins) - 1):
        b, e = begins[s], begins[s + 1]
        if b == e:
            continue
        for i, p in enumerate(pats):
            E = O.ends_scores(text[b:e], p)
            for flags in out:
                out[flags] += [(i, b + int(x), int(E[x])) for x in O.reported(E, len(p), k, flags)]
    return {f: sorted(r) for f, r in out.items()}


def span(text, p, k, e, begins):
    """(start or None, distance, s(e)): the span record of end e, clamped to its sequence"""
    s = seq_of(begins, e)
    b = begins[s]
    start, d = O.span(text[b:e + 1], p, k, e - b)
    return (None if start is None else b + start), d, s


def records_with_starts(text, pats, k, flags, begins):
    """[(pattern, end, dist, start, seq)] sorted"""
    out = []
    for i, e, d in records(text, pats, k, flags, begins):
        start, ds, s = span(text, pats[i], k, e, begins)
        assert ds == d, (i, e, d, ds)
        out.append((i, e, d, start, s))
    return out


def source_records(src, flags, pats, k, occ_flags):
    """[(pattern, end, dist, start, seq)] of the host-level call on the source `src` in the text mode `flags`, sorted by
    (pattern, end): positions are source offsets"""
    T, src_of = TN.normalize(src, flags)
    begins = [t for _, t in SQ.sequences(src, flags)]
    return [(i, src_of[e], d, src_of[st], s) for i, e, d, st, s in records_with_starts(T, pats, k, occ_flags, begins)]


def literal(text, p, k, flags, begins):
    """[(end, E_s(end))] of ONE pattern by the definition, written out: the full DP table of every slice with C[y][0] = y at
    its first byte, then the report rule on the row m of that table alone"""
    m, out = len(p), []
    for s in range(len(begins) - 1):
        b, e = begins[s], begins[s + 1]
        t = text[b:e]
        C = [[y if x == 0 else 0 for x in range(len(t) + 1)] for y in range(m + 1)]
        for x in range(1, len(t) + 1):
            for y in range(1, m + 1):
                C[y][x] = min(C[y - 1][x - 1] + (p[y - 1] != t[x - 1]), C[y - 1][x] + 1, C[y][x - 1] + 1)
        E = [C[m][x + 1] for x in range(len(t))]
        for x, d in enumerate(E):
            if d > k:
                continue
            if flags == LOCAL_MIN:
                prev = E[x - 1] if x else m
                if not prev > d:
                    continue
                if x + 1 < len(t) and not E[x + 1] >= d:
                    continue
            out.append((b + x, d))
    return out
