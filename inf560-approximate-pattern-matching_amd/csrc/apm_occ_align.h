/*
 * apm_occ_align.h -- arithmetic core of the occurrence-script pass (apm_occ_align.hip): the edit script of ONE occurrence,
 * the WHOLE pattern against the text bytes of its span, within k, or "none" beyond.  Host and device;
 * tests/host_occ_align_test.cpp compiles it with g++ alone.
 *
 * The pair (include/apm.h: "occurrence scripts"): p = the pattern's m bytes, t = T[s : e + 1) of L = e + 1 - s bytes,
 * m - k <= L <= m + k.  The script turns p into t in apm_align.h's ops, packing and rule, on a RECTANGULAR matrix: x counts
 * text bytes, y pattern bytes, cell(x, 0) = x, cell(0, y) = y; walk back from (L, m); at (x, y), x, y >= 1:
 *   the diagonal ('=' or 'X')  if cell(x-1, y-1) + (p[y-1] != t[x-1]) == cell(x, y),
 *   else D                     if cell(x, y-1) + 1 == cell(x, y),
 *   else I;
 * at y == 0 emit I until x == 0, at x == 0 emit D until y == 0.  #D - #I = m - L, n_ops = m + #I <= m + k.
 *
 * The align pass's band |x - y| <= k/2 does not hold such a pair (the band of a rectangle is lopsided), and it need not:
 * with m <= 128 and L <= m + k <= 255 the whole matrix is small.  FORWARD: bp_init and L columns of apm_core.h's
 * global-form bp_step over the forward pattern's Eq masks (bp_step and bp_distance as they stand); every column's vertical
 * deltas pv / mv are kept, column 0 .. column L: 2 W words each.  The distance is bp_distance at column L.  WALK BACK: a
 * cell is counted out of its column as bp_distance counts the top one,
 *   cell(x, y) = x + popcount(pv_x & low(y)) - popcount(mv_x & low(y)),      low(y) = the low y bits,
 * and cell(x, y-1) = cell(x, y) - (the vertical delta at bit y - 1 of column x).  p[y-1] != t[x-1] is bit y - 1 of the Eq
 * mask of t[x-1]: the pattern's bytes are not read again.  As in apm_align_walk the ops come last to first, so the walk
 * is done twice (count, then emit from the row's end), 16 ops gathered per dword and stored whole, the last dword's unused
 * high bits zero.
 */
#ifndef APM_OCC_ALIGN_H
#define APM_OCC_ALIGN_H

#include "apm_occ.h"

#ifndef APM_OP_EQ
#define APM_OP_EQ 0 /* include/apm.h, apm_align.h */
#define APM_OP_SUB 1
#define APM_OP_INS 2
#define APM_OP_DEL 3
#endif

/* the most text bytes of an occurrence, and so the trace's columns beside column 0 */
#define APM_OCC_ALIGN_MAX_COLS (2 * APM_OCC_MAX_PATTERN_LEN - 1)

/* the most ops of a script of a pattern of m bytes at distance <= k */
APM_HD int apm_occ_align_max_ops(int m, int k) { return m + k; }
/* dwords of a row that holds a script of the longest pattern behind its count */
APM_HD int apm_occ_align_row_words_of(int m_max, int k) { return 1 + ((apm_occ_align_max_ops(m_max, k) + 15) >> 4); }

APM_HD int apm_occ_align_popc(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

/* cell(x, y), 0 <= y <= 32 W, out of the kept column x */
template <int W, class Trace>
APM_HD int apm_occ_align_cell(const Trace &tr, int x, int y) {
    int d = x;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) {
        const int lo = 32 * w;
        uint32_t mask;
        if (y >= lo + 32) mask = 0xffffffffu;
        else if (y <= lo) mask = 0u;
        else mask = (1u << (y - lo)) - 1u;
        d += apm_occ_align_popc(tr.pv(x, w) & mask) - apm_occ_align_popc(tr.mv(x, w) & mask);
    }
    return d;
}

/* the op the rule takes at (x, y), x, y >= 1 */
template <int W, class Eq, class Txt, class Trace>
APM_HD int apm_occ_align_op(const Eq &eq, const Txt &t, const Trace &tr, int x, int y) {
    const int b = y - 1;
    uint32_t q[W];
    eq.get(t(x - 1), q);
    uint32_t same = 0u; /* (a select per word: a dynamic index into q would put it into scratch) */
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) same = w == (b >> 5) ? (q[w] >> (b & 31)) & 1u : same;
    const int c = apm_occ_align_cell<W>(tr, x, y);
    if (apm_occ_align_cell<W>(tr, x - 1, y - 1) + (same ? 0 : 1) == c) return same ? APM_OP_EQ : APM_OP_SUB;
    const int up = c - (int)((tr.pv(x, b >> 5) >> (b & 31)) & 1u) + (int)((tr.mv(x, b >> 5) >> (b & 31)) & 1u); /* cell(x, y - 1) */
    return up + 1 == c ? APM_OP_DEL : APM_OP_INS;
}

/* The script of one pair.  W == apm_occ_words(m); 1 <= L <= APM_OCC_ALIGN_MAX_COLS; k < m.
 *   Eq     `void get(int byte, uint32_t (&eq)[W]) const`: the FORWARD pattern's match mask of a byte value (apm_occ.h)
 *   Txt    `int operator()(int i) const`: the byte t[i], i < L
 *   Trace  the forward walk's sink and the walk back's source: `void put(int col, int w, uint32_t pv, uint32_t mv)`,
 *          `uint32_t pv(int col, int w) const`, `uint32_t mv(int col, int w) const`, col in [0, L], w < W; `void done()` is
 *          called once between the last put and the first read (the kernel's barrier)
 *   Out    `void store(int word, uint32_t v)`, word >= 1 (apm_align_walk's)
 * Returns n_ops (>= m >= 1), or 0: the pair is farther than k, nothing stored.  (The other "return 0" is apm_align_walk's
 * guard of the row's bounds against a trace that is not one: the rule itself never emits more than m + k ops.) */
template <int W, class Eq, class Txt, class Trace, class Out>
APM_HD int apm_occ_align(const Eq &eq, const Txt &t, int m, int L, int k, Trace &tr, Out &out) {
    uint32_t pv[W], mv[W];
    bp_init<W>(pv, mv);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int w = 0; w < W; ++w) tr.put(0, w, pv[w], mv[w]);
    for (int x = 1; x <= L; ++x) {
        uint32_t q[W];
        eq.get(t(x - 1), q);
        bp_step<W>(pv, mv, q);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int w = 0; w < W; ++w) tr.put(x, w, pv[w], mv[w]);
    }
    if (bp_distance<W>(pv, mv, m, L) > k) return 0;
    tr.done();
    const int max_ops = apm_occ_align_max_ops(m, k);
    int n = 0;
    for (int x = L, y = m; x > 0 || y > 0; ++n) {
        int op = y == 0 ? APM_OP_INS : APM_OP_DEL;
        if (x > 0 && y > 0) op = apm_occ_align_op<W>(eq, t, tr, x, y);
        x -= op != APM_OP_DEL;
        y -= op != APM_OP_INS;
    }
    if (n > max_ops) return 0;
    uint32_t acc = 0u;
    int j = n;
    for (int x = L, y = m; x > 0 || y > 0;) {
        int op = y == 0 ? APM_OP_INS : APM_OP_DEL;
        if (x > 0 && y > 0) op = apm_occ_align_op<W>(eq, t, tr, x, y);
        x -= op != APM_OP_DEL;
        y -= op != APM_OP_INS;
        --j;
        acc |= (uint32_t)op << (2 * (j & 15));
        if ((j & 15) == 0) {
            out.store(1 + (j >> 4), acc);
            acc = 0u;
        }
    }
    return n;
}

#if defined(__HIPCC__)
/* ---- the launch (apm_occ_align.hip) ---- */
/* the record passes' block (shard text, the END records in `rec` -- only read --, patterns, k) and the pass's own */
struct ApmOccAlignArgs : ApmScoreArgs {
    const uint4 *span;             /* device: span[r] of rec[r], only read */
    uint32_t *ops;                 /* device: row r at ops + r * stride */
    uint32_t stride;               /* dwords, >= apm_occ_align_row_words_of(the set's longest pattern, k) */
};
/* A fixed grid sized from the CU count, as the span pass's */
hipError_t apm_launch_occ_align(const ApmOccAlignArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_OCC_ALIGN_H */
