/*
 * apm_seqocc.h -- arithmetic of the occurrence search PER SEQUENCE (apm_seqocc.hip): the occurrence search (apm_occ.h) with
 * every sequence of a sequence table a text of its own, so that no occurrence begins in one sequence and ends in the next --
 * and none that does can hide an occurrence inside a sequence.  Host and device; tests/host_seqocc_test.cpp compiles it with
 * g++ alone.
 *
 * Semantics (include/apm.h pins them): the table's t_begin[0 .. n_seq] cuts the text into T_s = T[t_begin[s], t_begin[s+1]);
 * E_s is apm_occ.h's recurrence on T_s, C[y][0] = y at the sequence's first byte.  An end e belongs to s(e), the largest s with
 * t_begin[s] <= e.  APM_OCC_ALL reports e iff E_s(e) <= k; APM_OCC_LOCAL_MIN iff also E_s(e - 1) > E_s(e) (E_s = m in front of
 * the sequence's first byte) and E_s(e + 1) >= E_s(e) (true by definition at the sequence's last byte).
 *
 * THE WALK of one pattern over the ends [b, e) of a lane is apm_occ_walk made boundary-aware.  It counts the same columns
 * from b - (m + k) on, so every walk of a wave stays in step, but computes none in front of x0 = max(b - (m + k),
 * t_begin[s_b]), s_b the largest s with t_begin[s] <= b (apm_seqnear_find).  If x0 is the sequence's first byte the walk is
 * exact from its first column; otherwise all m + k bytes [x0, b) lie inside s_b and apm_occ.h's warm-up lemma holds as it
 * stands.  At a column x that is the next boundary t_begin[s + 1] -- in the warm-up, among the ends, or the look-ahead --
 *   1. the pending end x - 1 is decided with c2 = k + 1: it is the last byte of its sequence;
 *   2. the column starts again (C[y] = y, score = m) and s moves to the largest s' with t_begin[s'] <= x, past any empty
 *      sequences;
 *   3. column x is computed afresh, if the walk computes it at all;
 *   4. c0 becomes k + 1, not the old c1: in front of the new sequence's first byte E_s = m > k.
 * Boundaries are tracked as apm_seqnear_walk tracks them: c_next is the next boundary's column relative to b - (m + k) in
 * 32-bit integers, -1 if it lies beyond the walk's last column ("never").  The sink is called exactly once per column, from
 * code every walk of a wave runs in step; only the boundary bookkeeping diverges.
 *
 * THE SPAN of an end e is apm_occ.h's with the columns clamped to the sequence: L in [1, min(m + k, e + 1 - t_begin[s(e)])].
 */
#ifndef APM_SEQOCC_H
#define APM_SEQOCC_H

#if defined(__HIPCC__)
#include "../../include/apm.h" /* apm_seq; in front of the headers that define the APM_* macros only where they are missing */
#endif
#include "apm_occ.h"
#include "apm_seqnear.h"

/* The per-sequence segment walk of one pattern over the ends [b, e), 0 <= b <= e <= n_total (b == e: it reads nothing and
 * reports nothing).  Txt, Eq and Sink are apm_occ_walk's, Tab apm_seqnear_find's; n_seq >= 1; steps = apm_occ_steps of the
 * launch's S.  It reads no text byte outside [x0, min(e, n_total - 1)].  Returns the ends reported. */
template <int W, class Txt, class Eq, class Tab, class Sink>
APM_HD unsigned apm_seqocc_walk(const Txt &t, const Eq &eq, const Tab &tab, unsigned long long n_seq, int m, int k, long long b, long long e,
                                long long n_total, unsigned flags, int steps, Sink &sink) {
    const int cap = k + 1;
    const long long xs = b - (long long)(m + k); /* column 0 */
    unsigned long long s = 0;
    int c_from = steps, c_last = -1, c_next = -1; /* columns [c_from, c_last] are computed; c_next: the next boundary, -1: never */
    if (b < e) {
        s = apm_seqnear_find(tab, n_seq, (unsigned long long)b);
        const long long first = (long long)tab.begin(s), next = (long long)tab.begin(s + 1ull);
        const long long last = e < n_total ? e : n_total - 1; /* the look-ahead, if the text has it */
        c_from = first > xs ? (first - xs < (long long)steps ? (int)(first - xs) : steps) : 0;
        c_last = last - xs < (long long)steps ? (int)(last - xs) : steps - 1;
        c_next = next > xs && next - xs < (long long)steps ? (int)(next - xs) : -1;
    }
    uint32_t pv[W], mv[W];
    bp_init<W>(pv, mv);
    int score = m, c0 = cap, c1 = cap;
    unsigned found = 0;
    long long x = xs;
    for (int blk = 0; blk < steps; blk += 16) {
        uint32_t T[4];
        t.load16(x, T);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 16; ++i, ++x) {
            const int c = blk + i;
            const bool bound = c == c_next;
            if (bound) { /* x is the first byte of a later sequence: move on and start again */
                ++s;
                if (s + 1ull < n_seq && tab.begin(s + 1ull) <= (unsigned long long)x) s = apm_seqnear_find(tab, n_seq, (unsigned long long)x);
                if (s >= n_seq) s = n_seq - 1ull; /* (a table that breaks its promise) */
                const long long next = (long long)tab.begin(s + 1ull);
                c_next = next > x && next - xs < (long long)steps ? (int)(next - xs) : -1;
                bp_init<W>(pv, mv);
                score = m;
            }
            int c2 = cap;
            if (c >= c_from && c <= c_last) {
                uint32_t q[W];
                eq.get((int)((T[i >> 2] >> (8 * (i & 3))) & 0xffu), q);
                score += apm_occ_step<W>(pv, mv, q, m);
                c2 = score < cap ? score : cap;
            }
            const bool hit = x > b && x <= e && apm_occ_reported(flags, c0, c1, bound ? cap : c2, k); /* the end x - 1 */
            sink(hit, x - 1, c1);
            found += hit ? 1u : 0u;
            c0 = bound ? cap : c1;
            c1 = c2;
        }
    }
    return found;
}

/* columns of the span walk of end e in the sequence that begins at `first` <= e */
APM_HD int apm_seqocc_span_cols(int m, int k, unsigned long long e, unsigned long long first) { return apm_occ_span_cols(m, k, e - first); }

#if defined(__HIPCC__)
/* ---- the launches (apm_seqocc.hip) ---- */
struct ApmSeqoccArgs : ApmOccArgs {
    const apm_seq *seqs; /* device: n_seq + 1 entries, only t_begin is read */
    unsigned long long n_seq;
};
hipError_t apm_launch_seqocc(const ApmSeqoccArgs &a, hipStream_t s);

struct ApmSeqspanArgs : ApmSpanArgs {
    const apm_seq *seqs;
    unsigned long long n_seq;
    uint32_t *seq; /* device: seq[r] = s(e) of rec[r], where a span record is written; may be NULL */
};
hipError_t apm_launch_seqspan(const ApmSeqspanArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_SEQOCC_H */
