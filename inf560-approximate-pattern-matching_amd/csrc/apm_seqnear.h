/*
 * apm_seqnear.h -- arithmetic of the nearest-occurrence search PER SEQUENCE (apm_seqnear.hip): for every sequence of a
 * sequence table and every pattern the smallest E(e) of the occurrence search (apm_occ.h) run on that sequence as a text of
 * its own, and the first end that attains it.  Host and device; tests/host_seqnear_test.cpp compiles it with g++ alone.
 *
 * Semantics (include/apm.h pins them): the table's t_begin[0 .. n_seq] cuts the text into T_s = T[t_begin[s], t_begin[s+1]);
 * C[y][0] = y at the first byte of every sequence; key[s][i] = (d << 56) | e with e an index in T, or APM_NEAREST_NONE.
 *
 * THE WALK of one pattern over the ends [b, e) of a lane.  s_b is the largest s with t_begin[s] <= b (apm_seqnear_find: a
 * bounded binary search, s stays in [0, n_seq); for b < n_total it is never an empty sequence, because the sequence behind
 * an empty one begins at the same byte and is the larger s).  The walk starts at the column x0 = max(b - (2 m - 1),
 * t_begin[s_b]) with C[y] = y and score = m.  If x0 is the sequence's first byte the walk is exact from its first column, as
 * apm_occ.h's lemma says of x0 = 0: nothing in front of it is part of any substring.  Otherwise the 2 m - 1 bytes
 * [x0, b) all lie inside sequence s_b (t_begin[s_b] < x0 and t_begin[s_b + 1] > b), and the warm-up lemma holds as it does for
 * apm_nearest_walk: behind them min(score, m) is exact.
 * At every column x that equals the next boundary t_begin[s + 1] -- in the warm-up or among the lane's ends -- the lane
 * FLUSHES its best key into keys[s][i] (unless it is NONE), moves s to the largest s' with t_begin[s'] <= x (past any empty
 * sequences), and starts again: C[y] = y, score = m, best = NONE.  From there the walk is exact for the new sequence.
 * The sink is the nearest search's: an end x in [b, e) with score < m replaces the best only on a strictly smaller
 * distance, so the first end of the smallest distance stays.  There is no LOCAL_MIN rule, so no look-ahead column.
 * What is left at the end of the walk (*best, *seq) is the caller's to flush: the kernel reduces a wave's keys first where
 * all its lanes ended in the same sequence.
 *
 * The walk runs `steps` columns (apm_seqnear_steps of the launch's S: the same for every walk of a wave) from b - (2 m - 1)
 * on; a column in front of x0 or at or behind e changes nothing.  Columns are counted relative to b - (2 m - 1) in 32-bit
 * integers; a boundary beyond the walk's last column is "never".
 */
#ifndef APM_SEQNEAR_H
#define APM_SEQNEAR_H

#if defined(__HIPCC__)
#include "../../include/apm.h" /* apm_seq; in front of apm_nearest.h, which defines the APM_NEAREST_* macros only where they are missing */
#endif
#include "apm_nearest.h"

/* columns of a per-sequence walk of an m-byte pattern over a segment of S ends: the warm-up and the ends, whole 16-byte blocks */
APM_HD int apm_seqnear_steps(int S, int m) { return (S + 2 * m - 1 + 15) & ~15; }

/* the largest s in [0, n_seq) with begin(s) <= x, 0 if there is none; at most 64 probes, whatever the table holds.
 *   Tab  `unsigned long long begin(unsigned long long s) const`: t_begin[s], s in [0, n_seq] */
template <class Tab>
APM_HD unsigned long long apm_seqnear_find(const Tab &tab, unsigned long long n_seq, unsigned long long x) {
    unsigned long long lo = 0, hi = n_seq;
    for (int i = 0; i < 64 && hi - lo > 1ull; ++i) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (tab.begin(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* The per-sequence walk of one pattern over the ends [b, e), 0 <= b <= e <= n_total (b == e: it reads nothing, flushes
 * nothing and leaves *best = NONE).  Txt and Eq are apm_occ_walk's; Tab as above, n_seq >= 1;
 *   Keys `void operator()(unsigned long long s, unsigned long long key) const`: merge `key` (never NONE) into the key of
 *        sequence s and this walk's pattern; s < n_seq always
 * *best, *seq: the best key of the sequence the walk ended in (NONE: nothing to flush) and that sequence. */
template <int W, class Txt, class Eq, class Tab, class Keys>
APM_HD void apm_seqnear_walk(const Txt &t, const Eq &eq, const Tab &tab, unsigned long long n_seq, const Keys &flush, int m, long long b, long long e,
                             int steps, unsigned long long *best, unsigned long long *seq) {
    const int warm = 2 * m - 1;
    const long long xs = b - (long long)warm; /* column 0 */
    unsigned long long s = 0, key = APM_NEAREST_NONE;
    int c_from = steps, c_to = 0, c_next = -1; /* columns [c_from, c_to) are computed; c_next: the next boundary, -1: never */
    if (b < e) {
        s = apm_seqnear_find(tab, n_seq, (unsigned long long)b);
        const long long first = (long long)tab.begin(s), next = (long long)tab.begin(s + 1ull);
        c_from = first > xs ? (first - xs < (long long)steps ? (int)(first - xs) : steps) : 0;
        c_to = e - xs < (long long)steps ? (int)(e - xs) : steps;
        c_next = next > xs && next - xs < (long long)steps ? (int)(next - xs) : -1;
    }
    uint32_t pv[W], mv[W];
    bp_init<W>(pv, mv);
    int score = m;
    long long x = xs;
    for (int blk = 0; blk < steps; blk += 16) {
        uint32_t T[4];
        t.load16(x, T);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 16; ++i, ++x) {
            const int c = blk + i;
            if (c < c_from || c >= c_to) continue;
            if (c == c_next) { /* x is the first byte of a later sequence: flush, move on, start again */
                if (key != APM_NEAREST_NONE) flush(s, key);
                ++s;
                if (s + 1ull < n_seq && tab.begin(s + 1ull) <= (unsigned long long)x) s = apm_seqnear_find(tab, n_seq, (unsigned long long)x);
                if (s >= n_seq) s = n_seq - 1ull; /* (a table that breaks its promise) */
                const long long next = (long long)tab.begin(s + 1ull);
                c_next = next > x && next - xs < (long long)steps ? (int)(next - xs) : -1;
                bp_init<W>(pv, mv);
                score = m;
                key = APM_NEAREST_NONE;
            }
            uint32_t q[W];
            eq.get((int)((T[i >> 2] >> (8 * (i & 3))) & 0xffu), q);
            score += apm_occ_step<W>(pv, mv, q, m);
            if (c >= warm && score < m && (unsigned)score < APM_NEAREST_DIST(key)) key = apm_nearest_key(score, (unsigned long long)x);
        }
    }
    *best = key;
    *seq = s;
}

#if defined(__HIPCC__)
/* ---- the launches (apm_seqnear.hip) ---- */
struct ApmSeqnearArgs {
    const uint8_t *text;           /* device: bytes of the global positions [text_off, text_off + text_len) */
    unsigned long long text_off, text_len, n_total;
    unsigned long long e_begin, e_end; /* the ends to decide, e_begin < e_end <= n_total */
    uint32_t segment, n_segments;  /* S; ceil((e_end - e_begin) / S) */
    const uint8_t *image;          /* the record passes' image of the patterns and its {row offset, m} table (apm_score.h) */
    const uint2 *table;
    uint32_t n_patterns;
    const apm_seq *seqs;           /* device: n_seq + 1 entries, only t_begin is read */
    unsigned long long n_seq;
    unsigned long long *keys;      /* device: n_seq * n_patterns keys, merged into with atomicMin */
};
hipError_t apm_launch_seqnear(const ApmSeqnearArgs &a, hipStream_t s);

struct ApmSnspanArgs {
    const uint8_t *text;
    unsigned long long text_off, text_len, n_total;
    const uint8_t *image;
    const uint2 *table;
    uint32_t n_patterns;
    const apm_seq *seqs;
    unsigned long long n_seq;
    const unsigned long long *keys; /* device: only read */
    uint4 *end, *start;             /* device: n_seq * n_patterns records each; start may be NULL */
};
hipError_t apm_launch_snspan(const ApmSnspanArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_SEQNEAR_H */
