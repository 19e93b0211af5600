/*
 * apm_best.h -- arithmetic of the best-hit pass (apm_best.hip): which records of a find call are the best start of their
 * occurrence.  Host and device; tests/host_best_test.cpp compiles it with g++ alone.
 *
 * The rule (include/apm.h pins it): with W = [0, max(0, n_total - k)) the window starts the counting calls count and
 * s(i, j) the scoring pass's score of pattern i at start j (apm_score.h: capped at k + 1), record (i, pos) is a best hit at
 * radius r iff
 *   1. s(i, pos) <= k,
 *   2. every j in W with pos - r <= j < pos has s(i, j) >  s(i, pos),
 *   3. every j in W with pos < j <= pos + r has s(i, j) >= s(i, pos).
 * So a left neighbour suppresses on <=, a right one on <: a plateau keeps its first start.  The decision reads text and
 * pattern only, never the other records.
 *
 * A neighbour's walk needs no cap beyond the record's own score s0: a left neighbour is asked "dist <= s0", a right one
 * "dist < s0" -- caps s0 and s0 - 1 (apm_best_cap).  min(dist, cap + 1) answers either question exactly, and the walks of
 * apm_score.h are exact for every cap up to the k their band was sized for (a band wider than needed is exact as well).
 *
 * Who owns what: the neighbour enumeration, the suppress predicate, the cap, the coverage predicate and the plain-loop
 * decision apm_best_decide live here; the kernels of apm_best.hip call the same pieces and add only how the neighbours
 * are dealt to lanes.  The walks themselves are apm_score.h's.
 */
#ifndef APM_BEST_H
#define APM_BEST_H

#include "apm_score.h"

#ifndef APM_BEST_MAX_RADIUS
#define APM_BEST_MAX_RADIUS 64 /* include/apm.h */
#endif

#define APM_BEST_DROPPED (-1)    /* apm_best_decide: the record's own window is farther than k */
#define APM_BEST_SUPPRESSED (-2) /* ... a neighbour start is a better (or an equal, earlier) start of the occurrence */

/* the end of W */
APM_HD unsigned long long apm_best_w_end(unsigned long long n_total, int k) {
    return n_total > (unsigned long long)k ? n_total - (unsigned long long)k : 0ull;
}

/* is pos + o, o in [-r, r], a neighbour start of the record at pos: another start, inside W */
APM_HD bool apm_best_neighbour(unsigned long long pos, int o, unsigned long long w_end) {
    if (o == 0) return false;
    if (o < 0) return (unsigned long long)(-o) <= pos && pos - (unsigned long long)(-o) < w_end;
    return pos + (unsigned long long)o < w_end;
}

/* the neighbour offsets nearest first, whatever the radius: -1, 1, -2, 2, ...; index i in [0, 2 r) */
APM_HD int apm_best_offset(int i) { return (i & 1) ? (i >> 1) + 1 : -((i >> 1) + 1); }

/* the cap a neighbour at offset o is walked with, given the record's own score s0; < 0: it cannot suppress */
APM_HD int apm_best_cap(int o, int s0) { return o < 0 ? s0 : s0 - 1; }

/* does the neighbour at offset o with score s_nb (capped at any cap >= apm_best_cap(o, s0), plus one) suppress the record */
APM_HD bool apm_best_suppresses(int o, int s_nb, int s0) { return o < 0 ? s_nb <= s0 : s_nb < s0; }

/* the start o bytes from pos (a neighbour: it is inside W) */
APM_HD unsigned long long apm_best_start(unsigned long long pos, int o) {
    return o < 0 ? pos - (unsigned long long)(-o) : pos + (unsigned long long)o;
}

/* size of the window of an m-byte pattern at start j < n_total */
APM_HD int apm_best_size(int m, unsigned long long j, unsigned long long n_total) {
    const unsigned long long left = n_total - j;
    return left < (unsigned long long)m ? (int)left : m;
}

/* coverage: the shard text [text_off, text_off + text_len) holds every byte a decision at radius r may read,
 * [max(pos, r) - r, min(n_total, pos + r + m)) */
APM_HD bool apm_best_covered(unsigned long long pos, int m, int r, unsigned long long n_total, unsigned long long text_off,
                             unsigned long long text_len) {
    const unsigned long long lo = (pos > (unsigned long long)r ? pos : (unsigned long long)r) - (unsigned long long)r;
    unsigned long long hi = pos + (unsigned long long)r + (unsigned long long)m;
    if (hi > n_total) hi = n_total;
    return lo >= text_off && hi >= text_off && hi - text_off <= text_len;
}

/* the lane form's walk at the BAND of the launch (k / 2) with a cap of its own */
template <class Pat, class Txt>
APM_HD int apm_best_score_lane(const Pat &p, const Txt &t, int size, int k, int cap) {
    switch (k / 2) {
    case 0: return apm_score_lane<0>(p, t, size, cap);
    case 1: return apm_score_lane<1>(p, t, size, cap);
    case 2: return apm_score_lane<2>(p, t, size, cap);
    default: return apm_score_lane<3>(p, t, size, cap);
    }
}

/* The decision as a plain loop.  p: the record's pattern of m bytes; t: the text window at pos, with
 * `Txt at(int o) const` = the window o bytes further (the accessors of apm_score.h otherwise); band:
 * APM_SCORE_BAND_CELLS ints for the wave form.  The lane form serves k <= APM_SCORE_LANE_MAX_K, the wave form's emulated
 * lanes beyond -- or wherever wave_form asks for them.  The neighbours are walked nearest first: the result does not
 * depend on the order, the time to the first suppressor does.  Returns the record's score (a best hit),
 * APM_BEST_DROPPED or APM_BEST_SUPPRESSED. */
template <class Pat, class Txt>
inline int apm_best_decide(const Pat &p, const Txt &t, int m, unsigned long long pos, unsigned long long n_total, int k, int r, int *band,
                           bool wave_form = false) {
    const bool wave = wave_form || k > APM_SCORE_LANE_MAX_K;
    const unsigned long long w_end = apm_best_w_end(n_total, k);
    const int size = apm_best_size(m, pos, n_total);
    const int s0 = wave ? apm_score_wave_lanes(p, t, size, k, band) : apm_best_score_lane(p, t, size, k, k);
    if (s0 > k) return APM_BEST_DROPPED;
    for (int i = 0; i < 2 * r; ++i) {
        const int o = apm_best_offset(i), cap = apm_best_cap(o, s0);
        if (cap < 0 || !apm_best_neighbour(pos, o, w_end)) continue;
        const int size_j = apm_best_size(m, apm_best_start(pos, o), n_total);
        const Txt tj = t.at(o);
        const int s = wave ? apm_score_wave_lanes(p, tj, size_j, cap, band) : apm_best_score_lane(p, tj, size_j, k, cap);
        if (apm_best_suppresses(o, s, s0)) return APM_BEST_SUPPRESSED;
    }
    return s0;
}

#if defined(__HIPCC__)
/* ---- the launch (apm_best.hip): the record passes' common block, then where the best hits go ---- */
struct ApmBestArgs : ApmScoreArgs { /* rec is only read */
    uint32_t radius;               /* <= APM_BEST_MAX_RADIUS */
    uint4 *out;                    /* device: the best hits {pos, pattern, score}, appended at *n_out */
    unsigned long long out_cap;    /* records of out */
    unsigned long long *n_out;     /* device: best hits decided so far (may exceed out_cap: those are not written) */
};
hipError_t apm_launch_best(const ApmBestArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_BEST_H */
