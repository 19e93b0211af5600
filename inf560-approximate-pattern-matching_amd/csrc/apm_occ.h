/*
 * apm_occ.h -- arithmetic of the occurrence search (apm_occ.hip): for every text position e the smallest edit distance
 * between the WHOLE pattern and some substring that ends at e (Sellers 1980; Myers 1999, search form), and the span
 * [start, end] of a reported end.  Host and device; tests/host_occ_test.cpp compiles it with g++ alone.
 *
 * Semantics (include/apm.h pins them): with C[0][x] = 0, C[y][0] = y and the cell recurrence of apm_core.h,
 *   E(e) = C[m][e + 1] = min over s <= e + 1 of dist(p, T[s : e + 1)).
 * APM_OCC_ALL reports e iff E(e) <= k; APM_OCC_LOCAL_MIN iff also E(e - 1) > E(e) (E(-1) = m) and E(e + 1) >= E(e) (true
 * by definition at the last byte of the text): a plateau keeps its first end.  Everything needs k < m.
 *
 * The column is apm_core.h's bit-vector column with 0 instead of +1 fed into row 0 (apm_occ_step; bp_step itself is not
 * touched: the scan kernels' digests are pinned).  The step returns the horizontal delta at row m - 1, so the score
 * C[m][x] is carried as an integer and no column is ever counted out.
 *
 * THE WARM-UP LEMMA.  Start a walk at byte x0 > 0 with the column C[y] = y, as if the text began there.  After it has
 * consumed the m + k bytes [e - m - k + 1, e], min(score, k + 1) at e is exact: an alignment of cost <= k spans at most
 * m + k text bytes, and a later start can only raise the score.  At x0 = 0 the walk is exact from its first column.  So
 * the range of ends is cut into segments of S bytes (apm_occ_segment) and every (segment, pattern) walk stands alone:
 * apm_occ_walk starts m + k bytes in front of its first end -- its look-behind column b - 1 is then exact as well --
 * and reads one look-ahead column behind its last.
 *
 * THE SPAN of an end e: d* = min over L in [1, min(m + k, e + 1)] of dist(p, T[e + 1 - L : e + 1)), L* the smallest L that
 * attains it.  apm_occ_span_walk runs the GLOBAL-form column (bp_step / bp_distance as they stand) over the reversed
 * pattern, reading the text backwards from e: after x columns cell(x, m) = dist(p, T[e + 1 - x : e + 1)).  x < m - k needs
 * no special case: cell(x, m) >= m - x > k there.
 */
#ifndef APM_OCC_H
#define APM_OCC_H

#include "apm_core.h"

#ifndef APM_OCC_ALL
#define APM_OCC_ALL 0u /* include/apm.h */
#define APM_OCC_LOCAL_MIN 1u
#define APM_OCC_MAX_PATTERN_LEN 128
#endif
#define APM_OCC_MAX_WORDS (APM_OCC_MAX_PATTERN_LEN / 32)
#define APM_OCC_LANES 64 /* segments per workgroup of the scan: one per lane of a wave */
#define APM_OCC_SLOTS 4  /* patterns per workgroup of the scan: one per wave */

/* words of a pattern's column: the top row m - 1 lies in word W - 1 */
APM_HD int apm_occ_words(int m) { return (m + 31) >> 5; }

/* One text byte in the search form: bp_step with 0 fed into row 0.  W == apm_occ_words(m).  Returns the horizontal delta
 * at row m - 1: C[m][x] - C[m][x - 1]. */
template <int W>
APM_HD int apm_occ_step(uint32_t (&pv)[W], uint32_t (&mv)[W], const uint32_t (&eq)[W], int m) {
    uint32_t xh[W], ph[W], mh[W];
    uint32_t carry = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) {
        const uint32_t t = eq[w] & pv[w];
        const uint64_t s = (uint64_t)t + pv[w] + carry;
        carry = (uint32_t)(s >> 32);
        xh[w] = (((uint32_t)s) ^ pv[w]) | eq[w];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) {
        ph[w] = mv[w] | ~(xh[w] | pv[w]);
        mh[w] = pv[w] & xh[w];
    }
    const uint32_t top = (uint32_t)(m - 1) & 31u;
    const int hd = (int)((ph[W - 1] >> top) & 1u) - (int)((mh[W - 1] >> top) & 1u);
    uint32_t pin = 0u, min_ = 0u; /* row 0 is free: nothing enters at the bottom */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) {
        const uint32_t phs = (ph[w] << 1) | pin;
        const uint32_t mhs = (mh[w] << 1) | min_;
        pin = ph[w] >> 31;
        min_ = mh[w] >> 31;
        const uint32_t xv = eq[w] | mv[w];
        pv[w] = mhs | ~(xv | phs);
        mv[w] = phs & xv;
    }
    return hd;
}

/* the report predicate: c1 = min(E(e), k + 1), c0 / c2 the same of e - 1 / e + 1 (k + 1 in front of the text and behind it) */
APM_HD bool apm_occ_reported(unsigned flags, int c0, int c1, int c2, int k) {
    return c1 <= k && ((flags & APM_OCC_LOCAL_MIN) == 0u || (c0 > c1 && c2 >= c1));
}

/* columns a segment walk runs: m + k of warm-up, S ends, the look-ahead; whole 16-byte blocks */
APM_HD int apm_occ_steps(int S, int m, int k) { return (S + m + k + 1 + 15) & ~15; }

/* The segment walk of one pattern over the ends [b, e), 0 <= b <= e <= n_total (b == e: it reports nothing).
 *   Txt  `void load16(long long x, uint32_t (&w)[4]) const`: the text bytes x .. x + 15 in memory order; bytes outside the
 *        text read as anything, they never reach a column
 *   Eq   `void get(int byte, uint32_t (&eq)[W]) const`: the pattern's match mask of a byte value
 *   Sink `void operator()(bool hit, long long end, int dist)`: called once per column, from code every walk of a wave
 *        runs in step (the kernel's ballot), hit = "end is reported at this distance"
 * It runs `steps` columns (apm_occ_steps of the launch's S: the same for every walk of a wave) from x = b - m - k on; a
 * column in front of the text, or behind this walk's look-ahead, changes nothing.  Returns the ends reported. */
template <int W, class Txt, class Eq, class Sink>
APM_HD unsigned apm_occ_walk(const Txt &t, const Eq &eq, int m, int k, long long b, long long e, long long n_total, unsigned flags, int steps,
                             Sink &sink) {
    uint32_t pv[W], mv[W];
    bp_init<W>(pv, mv);
    const int cap = k + 1;
    const long long last = e < n_total ? e : n_total - 1; /* the last column this walk computes: its look-ahead, if the text has it */
    int score = m, c0 = cap, c1 = cap;                    /* E(-1) = m > k */
    unsigned found = 0;
    long long x = b - (long long)(m + k);
    for (int blk = 0; blk < steps; blk += 16) {
        uint32_t T[4];
        t.load16(x, T);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 16; ++i, ++x) {
            int c2 = cap;
            if (x >= 0 && x <= last) {
                uint32_t q[W];
                eq.get((int)((T[i >> 2] >> (8 * (i & 3))) & 0xffu), q);
                score += apm_occ_step<W>(pv, mv, q, m);
                c2 = score < cap ? score : cap;
            }
            const bool hit = x > b && x <= e && apm_occ_reported(flags, c0, c1, c2, k); /* the end x - 1 */
            sink(hit, x - 1, c1);
            found += hit ? 1u : 0u;
            c0 = c1;
            c1 = c2;
        }
    }
    return found;
}

/* The span walk of an end: `cols` = min(m + k, e + 1) columns of the global form over the reversed pattern.
 *   Eq    as above, of the REVERSED pattern
 *   Back  `int operator()(int i) const`: the text byte at e - i, i < cols
 * *d_star = the smallest cell(x, m), x in [1, cols]; *l_star = the first x that attains it. */
template <int W, class Eq, class Back>
APM_HD void apm_occ_span_walk(const Eq &eq, const Back &back, int m, int cols, int *d_star, int *l_star) {
    uint32_t pv[W], mv[W];
    bp_init<W>(pv, mv);
    int best = 1 << 20, at = 0;
    for (int x = 1; x <= cols; ++x) {
        uint32_t q[W];
        eq.get(back(x - 1), q);
        bp_step<W>(pv, mv, q);
        const int d = bp_distance<W>(pv, mv, m, x);
        if (d < best) {
            best = d;
            at = x;
        }
    }
    *d_star = best;
    *l_star = at;
}

/* columns of the span walk of end e */
APM_HD int apm_occ_span_cols(int m, int k, unsigned long long e) {
    const unsigned long long most = (unsigned long long)(m + k);
    return e + 1ull < most ? (int)(e + 1ull) : (int)most;
}

/* The segment chooser: S bytes of ends per walk for a range of `range` ends, whole 16-byte blocks.  On a large range
 * S = 16 (m_max + k): the warm-up overhead (S + m_max + k) / S is 1.0625, inside the 1.25 asked for (S >= 4 (m_max + k)).  A
 * small range shrinks S, down to m_max + k, until the launch has four workgroups per compute unit: a workgroup walks
 * APM_OCC_LANES segments for APM_OCC_SLOTS patterns. */
APM_HD int apm_occ_segment(int m_max, int k, unsigned long long range, int n_cu, int n_patterns) {
    const unsigned long long lo = (unsigned long long)(m_max + k), hi = 16ull * lo;
    const unsigned long long groups = (unsigned long long)((n_patterns + APM_OCC_SLOTS - 1) / APM_OCC_SLOTS);
    const unsigned long long blocks = 4ull * (unsigned long long)(n_cu > 0 ? n_cu : 1);
    const unsigned long long segs = APM_OCC_LANES * ((blocks + groups - 1) / (groups ? groups : 1));
    unsigned long long s = range / (segs ? segs : 1);
    s = s < lo ? lo : (s > hi ? hi : s);
    return (int)((s + 15ull) & ~15ull);
}

#if defined(__HIPCC__)
#include "apm_score.h"
/* ---- the launches (apm_occ.hip) ---- */
struct ApmOccArgs {
    const uint8_t *text;           /* device: bytes of the global positions [text_off, text_off + text_len) */
    unsigned long long text_off, text_len, n_total;
    unsigned long long e_begin, e_end; /* the ends to decide, e_begin < e_end <= n_total */
    uint32_t segment, n_segments;  /* S; ceil((e_end - e_begin) / S) */
    const uint8_t *image;          /* the record passes' image of the patterns and its {row offset, m} table (apm_score.h) */
    const uint2 *table;
    uint32_t n_patterns;
    int k, m_max;
    unsigned flags;
    uint4 *out;                    /* device: {end, pattern, E(end)}, appended at *n_found */
    unsigned long long cap;
    unsigned long long *n_found;   /* device: ends reported so far (may exceed cap: those are not written) */
    unsigned long long *counts;    /* device: per pattern, added into */
};
hipError_t apm_launch_occ(const ApmOccArgs &a, hipStream_t s);

struct ApmSpanArgs : ApmScoreArgs { /* rec is only read: pos = the end e */
    uint4 *span;                   /* device: span[r] of rec[r] */
};
hipError_t apm_launch_span(const ApmSpanArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_OCC_H */
