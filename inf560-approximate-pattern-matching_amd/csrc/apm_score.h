/*
 * apm_score.h -- arithmetic core of the scoring pass (apm_score.hip): the exact distance of ONE (pattern, window) pair,
 * capped at k + 1.  Host and device; tests/host_score_test.cpp compiles it with g++ alone.
 *
 * For a record, size = min(m, n_total - pos) and the score is min(dist(pattern[0:size], text[pos:pos+size]), k + 1), dist the
 * square global unit-cost distance of apm_core.h's recurrence.  Both strings have `size` bytes, so a path of cost <= k
 * holds as many insertions as deletions and never leaves the diagonals |x - y| <= k/2; no path leaves |x - y| <= size - 1
 * to its profit.  A band of half-width h = min(k/2, size - 1) is therefore exact for every dist <= k and can only
 * over-estimate beyond: min(band result, k + 1) is the capped distance.  (A band wider than h is exact as well.)
 *
 * Cell conventions are apm_banded_verify's (apm_device.h): x counts text bytes, y pattern bytes, e[d + h] = cell(x, x + d);
 *   cell(x, y) = min(diag = cell(x-1, y-1) + (p[y-1] != t[x-1]),  left = cell(x-1, y) + 1 = e[d + 1] + 1,  up = cell(x, y-1) + 1)
 * The minimum over a column's band never falls from one column to the next: once it exceeds k the answer is k + 1.
 *
 * Two forms:
 *   lane form  template <BAND>, BAND = k/2 <= 3: one pair per lane, the 2 BAND + 1 cells in registers, 16 columns per
 *              step out of dwords fetched up front, every index static; BAND 0 is a Hamming count
 *   wave form  any h: one pair per wavefront, lane i of chunk c owns diagonal 64 c + i, the band lives in LDS.  The
 *              vertical dependency nv[i] = min(c[i], nv[i-1] + 1), c[i] = min(diag, left), is a prefix minimum,
 *                  nv[i] = i + min over j <= i of (c[j] - j),
 *              one DPP wave scan per column and chunk; the last lane's value is carried into the next chunk.
 *              apm_score_wave_lanes is the same walk as a plain loop over 64 emulated lanes (host).
 *
 * Who owns what: this header owns the forward walk of each form -- apm_score_lane, apm_score_wave, apm_score_wave_lanes --
 * for the scoring pass AND the align pass (apm_align.h).  Each is a template over a trace sink: without one (ApmNoTrace,
 * the scoring pass) it keeps nothing and pays nothing; a sink of apm_align.h is handed the 2-bit direction apm_band_dir
 * of every band cell.  It also owns ApmScoreArgs, the argument block common to the two passes' launches.  What the align
 * pass does with a trace (its ops, walk back, sinks and workspace) is apm_align.h's.
 */
#ifndef APM_SCORE_H
#define APM_SCORE_H

#include "apm_core.h"

#include <stddef.h>

#define APM_SCORE_INF (1 << 20)          /* above every distance (patterns have < 2^16 bytes) */
#define APM_SCORE_LANE_MAX_K 7           /* lane form: k/2 <= 3 */
#define APM_SCORE_MAX_BAND 2048          /* wave form: half-band min(k/2, m_max - 1) it serves (apm.h documents it) */
#define APM_SCORE_BAND_CELLS (64 * ((2 * APM_SCORE_MAX_BAND + 1 + 63) / 64)) /* LDS cells of a wave: whole chunks */

/* byte i of dwords fetched in memory order */
APM_HD int apm_score_byte(const uint32_t *w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu); }
APM_HD int apm_score_min(int a, int b) { return a < b ? a : b; }

/* ---- trace sinks ----
 * The walks below hand a sink the direction of every band cell; ApmNoTrace (no sink) keeps none, and with it the
 * directions are not even worked out.
 *   lane form  `void put(int col, uint32_t w)`, col = x - 1, 2 bits per band cell i = y - x + BAND
 *   wave form  `void put(size_t entry, unsigned long long b0, unsigned long long b1)`, entry = (x - 1) * chunks + c, bit i
 *              of b0 / b1 = bit 0 / 1 of lane i's direction */
struct ApmNoTrace {};
template <class Sink> struct ApmKeepsTrace { static constexpr bool value = true; };
template <> struct ApmKeepsTrace<ApmNoTrace> { static constexpr bool value = false; };

/* the direction of one cell, the op the align pass's rule takes there (apm_align.h documents the rule; 0 '=', 1 'X',
 * 2 'I', 3 'D'): e = cell(x-1, y-1), neq = (p[y-1] != t[x-1]), nv = cell(x, y), nv_up = cell(x, y-1) */
APM_HD int apm_band_dir(int e, int neq, int nv, int nv_up) { return e + neq == nv ? neq : (nv_up + 1 == nv ? 3 : 2); }

/* ---- lane form ----
 * Pat / Txt: `void load16(int off, uint32_t (&w)[4]) const` = bytes off .. off + 15 of the string in memory order.  The
 * pattern is asked at multiples of 16 up to 16 * ceil(size / 16) + 16, the text at multiples of 16 below size; what lies
 * beyond `size` is never part of a cell that counts and may read as anything.  Returns the capped distance; a sink
 * (BAND >= 1 only) gets every column the walk reaches. */
template <int BAND, class Pat, class Txt, class Sink = ApmNoTrace>
APM_HD int apm_score_lane(const Pat &p, const Txt &t, int size, int k, Sink *sink = nullptr) {
    const int cap = k + 1;
    if constexpr (BAND == 0) {
        /* nonzero bytes of text ^ pattern, counted with the carry trick, 16 bytes per step */
        int mism = 0;
        for (int xb = 0; xb < size; xb += 16) {
            uint32_t T[4], P[4];
            t.load16(xb, T);
            p.load16(xb, P);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int valid = size - xb - 4 * i; /* bytes of this dword inside the window */
                const uint32_t mask = valid >= 4 ? 0xffffffffu : (valid <= 0 ? 0u : ((1u << (8 * valid)) - 1u));
                const uint32_t x = (T[i] ^ P[i]) & mask;
                mism += __builtin_popcount((x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u);
            }
            if (mism > k) return cap;
        }
        return mism;
    } else {
        constexpr int NB = 2 * BAND + 1;
        constexpr int INF = APM_SCORE_INF;
        int e[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) e[i] = (i >= BAND && i - BAND <= size) ? (i - BAND) : INF; /* cell(0, d) = d */
        /* pattern bytes 16 (b - 1) .. 16 (b + 2) - 1 around the block b of 16 columns: cell (16 b + xi + 1, . + i - BAND)
           compares pattern byte 16 b + xi + i - BAND = entry 16 + xi + i - BAND of P */
        uint32_t P[12], N[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) P[i] = 0u;
        p.load16(0, N);
#pragma unroll
        for (int i = 0; i < 4; ++i) P[4 + i] = N[i];
        p.load16(16, N);
#pragma unroll
        for (int i = 0; i < 4; ++i) P[8 + i] = N[i];
        for (int xb = 0; xb < size; xb += 16) {
            uint32_t T[4];
            t.load16(xb, T);
            if (xb + 16 < size) p.load16(xb + 32, N); /* the block after the next one's bytes, in flight over this one */
#pragma unroll
            for (int xi = 0; xi < 16; ++xi) {
                const int x = xb + xi + 1;
                if (x <= size) {
                    const int tc = apm_score_byte(T, xi);
                    int up = INF, best = INF;
                    uint32_t tw = 0u;
#pragma unroll
                    for (int i = 0; i < NB; ++i) {
                        const int y = x + i - BAND;
                        const int pc = apm_score_byte(P, 16 + xi + i - BAND);
                        const int neq = (pc != tc) ? 1 : 0;
                        const int diag = e[i] + neq;
                        const int left = (i + 1 < NB) ? e[i + 1] + 1 : INF;
                        int nv = apm_score_min(apm_score_min(diag, left), up + 1);
                        if constexpr (ApmKeepsTrace<Sink>::value) /* (cells outside 1 <= y <= size: never read) */
                            tw |= (uint32_t)apm_band_dir(e[i], neq, nv, up) << (2 * i);
                        if (y < 1) nv = (y == 0) ? x : INF;
                        if (y > size) nv = INF;
                        e[i] = nv;
                        up = nv;
                        best = apm_score_min(best, nv);
                    }
                    if constexpr (ApmKeepsTrace<Sink>::value) sink->put(x - 1, tw);
                    if ((xi & 3) == 3 && best > k) return cap;
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) P[i] = P[i + 4];
#pragma unroll
            for (int i = 0; i < 4; ++i) P[8 + i] = N[i];
        }
        return apm_score_min(e[BAND], cap);
    }
}

/* ---- wave form: what one lane computes for its diagonal g (shared by the device walk and the emulated one) ---- */
/* cell(0, g - h) of the band of nb = 2 h + 1 diagonals; the lanes behind the band (g >= nb) hold INF */
APM_HD int apm_score_band_init(int g, int h, int nb, int size) {
    return (g >= h && g < nb && g - h <= size) ? (g - h) : APM_SCORE_INF;
}
/* c = min(diag, left) of cell (x, y), the vertical dependency left out; e = the diagonal's cell of column x - 1,
 * e_left = that of diagonal g + 1.  Row 0 is cell(x, 0) = x; above it and behind the band nothing exists. */
APM_HD int apm_score_cell(int e, int e_left, int pc, int tc, int x, int y, bool in_band) {
    int c = apm_score_min(e + ((pc != tc) ? 1 : 0), e_left + 1);
    if (y < 1) c = (y == 0) ? x : APM_SCORE_INF;
    if (!in_band) c = APM_SCORE_INF;
    return c;
}

/* The wave form as a plain loop over 64 emulated lanes: the chunks of 64 diagonals, the carry from chunk to chunk, the
 * early exit and the sink's ballots are those of apm_score_wave below.  Pat / Txt: `int byte(int i) const`, i in
 * [0, size) (anything outside may read as anything: those cells do not count).  band: APM_SCORE_BAND_CELLS ints (the
 * wave's LDS).  Returns the capped distance. */
template <class Pat, class Txt, class Sink = ApmNoTrace>
inline int apm_score_wave_lanes(const Pat &p, const Txt &t, int size, int k, int *band, Sink *sink = nullptr) {
    const int INF = APM_SCORE_INF;
    const int h = apm_score_min(k / 2, size - 1), nb = 2 * h + 1, chunks = (nb + 63) >> 6;
    for (int g = 0; g < 64 * chunks; ++g) band[g] = apm_score_band_init(g, h, nb, size);
    for (int x = 1; x <= size; ++x) {
        const int tc = t.byte(x - 1);
        int up = INF, colmin = INF; /* up: the last lane of the chunk below, this column */
        for (int c = 0; c < chunks; ++c) {
            const int fill = c + 1 < chunks ? band[64 * (c + 1)] : INF; /* the left neighbour of lane 63: column x - 1 */
            int cc[64], nv[64], neq[64];
            for (int lane = 0; lane < 64; ++lane) {
                const int g = 64 * c + lane, y = x + g - h;
                const int e_left = lane < 63 ? band[g + 1] : fill;
                const int pc = (y >= 1 && y <= size) ? p.byte(y - 1) : 0;
                neq[lane] = (pc != tc) ? 1 : 0;
                cc[lane] = apm_score_cell(band[g], e_left, pc, tc, x, y, g < nb) - lane;
            }
            for (int lane = 1; lane < 64; ++lane) cc[lane] = apm_score_min(cc[lane], cc[lane - 1]); /* inclusive prefix minimum */
            unsigned long long b0 = 0ull, b1 = 0ull;
            for (int lane = 0; lane < 64; ++lane) {
                const int g = 64 * c + lane, y = x + g - h;
                nv[lane] = g < nb ? apm_score_min(cc[lane] + lane, up + lane + 1) : INF;
                if (g < nb && y >= 0 && y <= size) colmin = apm_score_min(colmin, nv[lane]);
                if constexpr (ApmKeepsTrace<Sink>::value) {
                    const int d = apm_band_dir(band[g], neq[lane], nv[lane], lane ? nv[lane - 1] : up);
                    b0 |= (unsigned long long)(d & 1) << lane;
                    b1 |= (unsigned long long)(d >> 1) << lane;
                }
            }
            if constexpr (ApmKeepsTrace<Sink>::value) sink->put((size_t)(x - 1) * (size_t)chunks + (size_t)c, b0, b1);
            for (int lane = 0; lane < 64; ++lane) band[64 * c + lane] = nv[lane];
            up = nv[63];
        }
        if (colmin > k) return k + 1;
    }
    return apm_score_min(band[h], k + 1);
}

#if defined(__HIPCC__)
/* inclusive prefix minimum over the wave: apm_wave_incl_scan's six DPP steps (apm_wave.h) with min for +; lanes without
 * a source keep the identity */
__device__ __forceinline__ int apm_wave_incl_min_scan(int v) {
    constexpr int ID = 0x3fffffff;
    v = min(v, __builtin_amdgcn_update_dpp(ID, v, 0x111, 0xf, 0xf, false)); // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(ID, v, 0x112, 0xf, 0xf, false)); // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(ID, v, 0x114, 0xf, 0xf, false)); // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(ID, v, 0x118, 0xf, 0xf, false)); // row_shr:8
    v = min(v, __builtin_amdgcn_update_dpp(ID, v, 0x142, 0xa, 0xf, false)); // row_bcast:15 -> rows 1, 3
    v = min(v, __builtin_amdgcn_update_dpp(ID, v, 0x143, 0xc, 0xf, false)); // row_bcast:31 -> rows 2, 3
    return v;
}

/* One pair per wavefront; every lane of the wave calls it with the same arguments (wave-uniform control flow: the DPP
 * steps need all 64 lanes) and gets the same answer, the capped distance.  band: APM_SCORE_BAND_CELLS ints of LDS owned
 * by this wave.  Sink::put is called by every lane with the same arguments (it picks the lane that stores); deciding D
 * needs the upper neighbour's new value, one more DPP shift behind the scan. */
template <class Pat, class Txt, class Sink = ApmNoTrace>
__device__ __forceinline__ int apm_score_wave(const Pat &p, const Txt &t, int size, int k, int *band, int lane, Sink *sink = nullptr) {
    constexpr int INF = APM_SCORE_INF;
    const int h = min(k / 2, size - 1), nb = 2 * h + 1, chunks = (nb + 63) >> 6;
    for (int c = 0; c < chunks; ++c) band[64 * c + lane] = apm_score_band_init(64 * c + lane, h, nb, size);
    __syncthreads();
    for (int x = 1; x <= size; ++x) {
        const int tc = t.byte(x - 1);
        int up = INF, colmin = INF;
        for (int c = 0; c < chunks; ++c) {
            const int g = 64 * c + lane, y = x + g - h;
            const int e = band[g];
            const int fill = c + 1 < chunks ? band[64 * (c + 1)] : INF;
            const int e_left = __builtin_amdgcn_update_dpp(fill, e, 0x130, 0xf, 0xf, false); // wave_shl:1, lane 63 keeps fill
            const int pc = (y >= 1 && y <= size) ? p.byte(y - 1) : 0;
            const int cc = apm_score_cell(e, e_left, pc, tc, x, y, g < nb);
            const int nv = g < nb ? min(apm_wave_incl_min_scan(cc - lane) + lane, up + lane + 1) : INF;
            if (g < nb && y >= 0 && y <= size) colmin = min(colmin, nv);
            if constexpr (ApmKeepsTrace<Sink>::value) {
                const int nv_up = __builtin_amdgcn_update_dpp(up, nv, 0x138, 0xf, 0xf, false); // wave_shr:1, lane 0 keeps the carry
                const int d = apm_band_dir(e, (pc != tc) ? 1 : 0, nv, nv_up);
                sink->put((size_t)(x - 1) * (size_t)chunks + (size_t)c, __builtin_amdgcn_ballot_w64((d & 1) != 0),
                         __builtin_amdgcn_ballot_w64((d & 2) != 0));
            }
            band[g] = nv;
            up = __builtin_amdgcn_readlane(nv, 63);
        }
        __syncthreads(); // (one wave per workgroup: orders the column's LDS stores before the next one's loads)
        if (__builtin_amdgcn_ballot_w64(colmin <= k) == 0ull) return k + 1;
    }
    return min(band[h], k + 1);
}

/* ---- the launch (apm_score.hip); the align pass's launch takes the same block first (ApmAlignArgs) ---- */
struct ApmScoreArgs {
    const uint8_t *text;           /* device: bytes of the global positions [text_off, text_off + text_len) */
    unsigned long long text_off, text_len, n_total;
    uint4 *rec;                    /* device: apm_match records; only the fourth dword is written (align: none) */
    unsigned long long cap;        /* records of rec */
    const unsigned long long *n_rec; /* device: records present (may exceed cap: min(*n_rec, cap) are served) */
    const uint8_t *image;          /* score image: every pattern's raw bytes, rows 16-byte aligned and zero padded */
    const uint2 *table;            /* per pattern {byte offset of its row, m} */
    uint32_t n_patterns;
    int k;
};
/* bytes of a pattern's row in the score image: the lane form fetches whole 16-byte blocks up to two behind the last */
static inline size_t apm_score_row_bytes(size_t m) { return ((m + 15) & ~(size_t)15) + 32; }
hipError_t apm_launch_score(const ApmScoreArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_SCORE_H */
