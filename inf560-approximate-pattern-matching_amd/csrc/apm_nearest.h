/*
 * apm_nearest.h -- arithmetic of the nearest-occurrence search (apm_nearest.hip): for every pattern the smallest E(e) of
 * the occurrence search (apm_occ.h) over the whole text and the first end that attains it, with no k.  Host and device;
 * tests/host_nearest_test.cpp compiles it with g++ alone.
 *
 * Semantics (include/apm.h pins them): d_i = min over e of E_i(e), e_i the smallest e with E_i(e) = d_i; an answer exists
 * iff d_i < m_i (E = m_i is the empty substring: no byte of the pattern was found).
 *
 * THE WALK is apm_occ_walk with the bound m - 1 and APM_OCC_ALL: the warm-up is m + (m - 1) = 2 m - 1 bytes, behind it
 * min(score, m) is exact by the warm-up lemma as apm_occ.h states it, and an end is a "hit" iff E(e) <= m - 1.  The walk
 * visits its ends in rising order, so a sink that replaces its best only on a strictly smaller distance keeps the first
 * end of the smallest distance (ApmNearestSink).
 *
 * THE KEY: (d << 56) | e, merged with an unsigned 64-bit minimum.  The smaller key is the smaller distance and, at equal
 * distance, the smaller end, so lanes, waves, segments and shards merge in any order to the same answer.  d <= 127 and
 * e < 2^56, so no key of an answer equals APM_NEAREST_NONE.
 */
#ifndef APM_NEAREST_H
#define APM_NEAREST_H

#include "apm_occ.h"

#ifndef APM_NEAREST_NONE
#define APM_NEAREST_NONE 0xffffffffffffffffull /* include/apm.h */
#define APM_NEAREST_DIST(key) ((unsigned)((unsigned long long)(key) >> 56))
#define APM_NEAREST_END(key) ((unsigned long long)(key) & 0x00ffffffffffffffull)
#endif
#define APM_NEAREST_MAX_TEXT (1ull << 56) /* ends are e < n_total <= 2^56 */

APM_HD unsigned long long apm_nearest_key(int dist, unsigned long long end) { return ((unsigned long long)dist << 56) | end; }

/* the sink of a nearest walk: the best (distance, end) of the hits one lane saw, the first end of the smallest distance */
struct ApmNearestSink {
    unsigned long long best;
    APM_HD ApmNearestSink() : best(APM_NEAREST_NONE) {}
    APM_HD void operator()(bool hit, long long end, int dist) {
        if (hit && (unsigned)dist < APM_NEAREST_DIST(best)) best = apm_nearest_key(dist, (unsigned long long)end);
    }
};

/* columns of a nearest walk of an m-byte pattern over a segment of S ends; S of a launch with the longest pattern m_max */
APM_HD int apm_nearest_steps(int S, int m) { return apm_occ_steps(S, m, m - 1); }
APM_HD int apm_nearest_segment(int m_max, unsigned long long range, int n_cu, int n_patterns) {
    return apm_occ_segment(m_max, m_max - 1, range, n_cu, n_patterns);
}

/* The nearest walk of one pattern over the ends [b, e) (apm_occ_walk's Txt and Eq): the key of its best end, or NONE. */
template <int W, class Txt, class Eq>
APM_HD unsigned long long apm_nearest_walk(const Txt &t, const Eq &eq, int m, long long b, long long e, long long n_total, int steps) {
    ApmNearestSink sink;
    apm_occ_walk<W>(t, eq, m, m - 1, b, e, n_total, APM_OCC_ALL, steps, sink);
    return sink.best;
}

#if defined(__HIPCC__)
/* ---- the launches (apm_nearest.hip) ---- */
struct ApmNearestArgs {
    const uint8_t *text;           /* device: bytes of the global positions [text_off, text_off + text_len) */
    unsigned long long text_off, text_len, n_total;
    unsigned long long e_begin, e_end; /* the ends to decide, e_begin < e_end <= n_total */
    uint32_t segment, n_segments;  /* S; ceil((e_end - e_begin) / S) */
    const uint8_t *image;          /* the record passes' image of the patterns and its {row offset, m} table (apm_score.h) */
    const uint2 *table;
    uint32_t n_patterns;
    unsigned long long *keys;      /* device: one key per pattern, merged into with atomicMin */
};
hipError_t apm_launch_nearest(const ApmNearestArgs &a, hipStream_t s);

struct ApmNspanArgs {
    const uint8_t *text;
    unsigned long long text_off, text_len, n_total;
    const uint8_t *image;
    const uint2 *table;
    uint32_t n_patterns;
    const unsigned long long *keys; /* device: only read */
    uint4 *end, *start;             /* device: n_patterns records each; start may be NULL */
};
hipError_t apm_launch_nspan(const ApmNspanArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_NEAREST_H */
