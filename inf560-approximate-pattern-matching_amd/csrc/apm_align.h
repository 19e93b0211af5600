/*
 * apm_align.h -- arithmetic core of the align pass (apm_align.hip): the edit script of ONE (pattern, window) pair within
 * k, or "none" beyond.  Host and device; tests/host_align_test.cpp compiles it with g++ alone.
 *
 * The pair is the scoring pass's (apm_score.h): size = min(m, n_total - pos), p = pattern[0:size], t = text[pos:pos+size].
 * The script turns p into t, one op per alignment column, from the window's first byte to its last:
 *   0 '='  bytes equal              one byte of each
 *   1 'X'  substitution             one byte of each
 *   2 'I'  the text has a byte the pattern has not      text only
 *   3 'D'  the pattern has a byte the text has not      pattern only
 * Both strings have `size` bytes, so #I == #D and n_ops = size + #I <= size + min(k/2, size - 1).
 *
 * ONE script out of the optimal ones.  With apm_score.h's conventions (x counts text bytes, y pattern bytes,
 * cell(x, 0) = x, cell(0, y) = y) walk back from (size, size); at (x, y), x, y >= 1:
 *   the diagonal ('=' or 'X')  if cell(x-1, y-1) + (p[y-1] != t[x-1]) == cell(x, y),
 *   else D                     if cell(x, y-1) + 1 == cell(x, y),
 *   else I;
 * at y == 0 emit I until x == 0, at x == 0 emit D until y == 0.
 * Band == full matrix: the walk only ever stands on cells of an optimal path of cost <= k, and every such path stays
 * inside |x - y| <= h = min(k/2, size - 1) (apm_score.h's band argument).  A cell on such a path has, in a band of
 * half-width >= h, the full matrix's value (the path's prefix is a band path), and every other band cell can only be
 * larger than its full-matrix value.  So a test "neighbour + cost == cell(x, y)" that holds in the full matrix names a
 * neighbour on an optimal path and holds in the band; one that fails in the full matrix (neighbour + cost > cell) fails
 * in the band all the more.  The rule therefore takes the same step on the band as on the full matrix: the host core,
 * the kernels and the tests' full-matrix reference give the same bits.
 *
 * Who owns what: the forward walk of either form is apm_score.h's (apm_score_lane, apm_score_wave, apm_score_wave_lanes),
 * the scoring pass's own walk instantiated with a sink of this header; it evaluates the rule above per band cell
 * (apm_band_dir: the op the rule takes, 2 bits) and returns the capped distance.  This header owns what is the align
 * pass's alone: the ops, the sinks and readers of the trace, the walk back (apm_align_walk), "farther than k -> 0,
 * nothing stored", and the workspace sizing.
 *
 * Two forms, those of the scoring pass; the trace lives in GLOBAL memory (a per-lane array under dynamic indices would
 * be scratch):
 *   lane form  BAND = k/2 <= 3: per column one 16-bit word, 2 bits per band cell i = y - x + BAND; BAND 0 keeps no
 *              trace, its script is the per-byte compare.  Device layout: column-major across lanes, the halfword of
 *              (column c, lane slot l) at c * rows + l, so the 64 lanes of a wave store side by side.
 *   wave form  per column and chunk of 64 diagonals two 64-bit ballots (bit 0 and bit 1 of the lanes' directions), 16
 *              bytes at (x - 1) * chunks + c.  The walk back is wave-uniform: entry (x - 1) * chunks + (g >> 6), bit g & 63.
 * The walk back yields the ops last to first; it is done twice (count, then emit from the row's end): the trace is
 * L2-resident and the pass runs over matches only.  16 ops per dword are gathered in a register and stored whole, the
 * last dword's unused high bits zero.
 *
 * Workspace budget (APM_ALIGN_WS_BUDGET): the most trace memory a device keeps for the pass.  One trace row of the
 * wave form is m_max * chunks * 16 bytes -- at the scoring pass's limits (m_max = 65535, half-band 2048: 65 chunks)
 * 68.2 MB -- so 80 MiB gives every set the scoring pass accepts at least one row; a lane-form row is 2 m_max bytes, at
 * least 640 of them (512 in whole workgroups).  The budget clamps the records in flight (rows), never what is served.
 */
#ifndef APM_ALIGN_H
#define APM_ALIGN_H

#include "apm_score.h"

/* the ops; apm_band_dir (apm_score.h) yields these codes */
#define APM_OP_EQ 0
#define APM_OP_SUB 1
#define APM_OP_INS 2
#define APM_OP_DEL 3
#define APM_ALIGN_WS_BUDGET ((size_t)80 << 20)

/* the most ops of a script of `size` bytes each at distance <= k */
APM_HD int apm_align_max_ops(int size, int k) { return size + apm_score_min(k / 2, size - 1); }
/* dwords of a row that holds n_ops ops behind its count */
APM_HD int apm_align_words(int n_ops) { return 1 + ((n_ops + 15) >> 4); }

/* The walk back from (size, size) over a trace of a band of half-width h.  Dir: `int at(int x, int g) const` = the
 * direction kept for cell (x, x + g - h), x >= 1.  Out: `void store(int word, uint32_t v)`, word >= 1.  Returns n_ops.
 * (The two "return 0" guard the row's bounds against a trace that is not one: the rule itself never leaves the band
 * and never emits more than max_ops.) */
template <class Dir, class Out>
APM_HD int apm_align_walk(int size, int h, int max_ops, const Dir &dir, Out &out) {
    const int nb = 2 * h + 1;
    int n = 0;
    for (int x = size, y = size; x > 0 || y > 0; ++n) {
        int op = y == 0 ? APM_OP_INS : APM_OP_DEL;
        if (x > 0 && y > 0) {
            const int g = y - x + h;
            if (g < 0 || g >= nb) return 0;
            op = dir.at(x, g);
        }
        x -= op != APM_OP_DEL;
        y -= op != APM_OP_INS;
    }
    if (n > max_ops) return 0;
    uint32_t acc = 0u;
    int j = n;
    for (int x = size, y = size; x > 0 || y > 0;) {
        int op = y == 0 ? APM_OP_INS : APM_OP_DEL;
        if (x > 0 && y > 0) op = dir.at(x, y - x + h);
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

/* ---- lane form ----
 * Pat / Txt: apm_score_lane's.  Trace: the walk's sink and the walk back's source, `void put(int col, uint32_t w)`,
 * `uint32_t get(int col) const`, col in [0, size).  Out: apm_align_walk's.  Returns n_ops, 0: the pair is farther than k
 * (nothing stored). */
template <class Trace>
struct ApmAlignLaneDir {
    const Trace &tr;
    APM_HD int at(int x, int g) const { return (int)((tr.get(x - 1) >> (2 * g)) & 3u); }
};

template <int BAND, class Pat, class Txt, class Trace, class Out>
APM_HD int apm_align_lane(const Pat &p, const Txt &t, int size, int k, Trace &tr, Out &out) {
    if constexpr (BAND == 0) {
        /* no insertion fits k <= 1: the script is the per-byte compare, 16 ops per step */
        if (apm_score_lane<0>(p, t, size, k) > k) return 0;
        for (int xb = 0; xb < size; xb += 16) {
            uint32_t T[4], P[4];
            t.load16(xb, T);
            p.load16(xb, P);
            uint32_t w = 0u;
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (xb + i < size && apm_score_byte(T, i) != apm_score_byte(P, i)) w |= (uint32_t)APM_OP_SUB << (2 * i);
            out.store(1 + (xb >> 4), w);
        }
        return size;
    } else {
        if (apm_score_lane<BAND>(p, t, size, k, &tr) > k) return 0;
        const ApmAlignLaneDir<Trace> dir{tr};
        return apm_align_walk(size, BAND, apm_align_max_ops(size, k), dir, out);
    }
}

/* ---- wave form ---- */
/* the trace entry of (column x, chunk c): two 64-bit words, bit i of word b = bit b of lane i's direction */
struct ApmAlignWaveSinkHost {
    unsigned long long *ws;
    void put(size_t entry, unsigned long long b0, unsigned long long b1) { ws[2 * entry] = b0, ws[2 * entry + 1] = b1; }
};
struct ApmAlignWaveDirHost {
    const unsigned long long *ws;
    int chunks;
    int at(int x, int g) const {
        const unsigned long long *w = ws + 2 * ((size_t)(x - 1) * (size_t)chunks + (size_t)(g >> 6));
        return (int)(((w[0] >> (g & 63)) & 1ull) | (((w[1] >> (g & 63)) & 1ull) << 1));
    }
};

/* The wave form as a plain loop over 64 emulated lanes, apm_align_wave below on the host.  band: APM_SCORE_BAND_CELLS
 * ints; ws: 2 * size * chunks 64-bit words, chunks = (2 min(k/2, size-1) + 64) / 64. */
template <class Pat, class Txt, class Out>
inline int apm_align_wave_lanes(const Pat &p, const Txt &t, int size, int k, int *band, unsigned long long *ws, Out &out) {
    const int h = apm_score_min(k / 2, size - 1), chunks = (2 * h + 64) >> 6;
    ApmAlignWaveSinkHost sink{ws};
    if (apm_score_wave_lanes(p, t, size, k, band, &sink) > k) return 0;
    const ApmAlignWaveDirHost dir{ws, chunks};
    return apm_align_walk(size, h, apm_align_max_ops(size, k), dir, out);
}

#if defined(__HIPCC__)
struct ApmAlignWaveSink {    /* every lane calls put with the same arguments: lane 0 stores the entry */
    uint4 *ws;
    int lane;
    __device__ __forceinline__ void put(size_t entry, unsigned long long b0, unsigned long long b1) {
        if (lane == 0) ws[entry] = make_uint4((uint32_t)b0, (uint32_t)(b0 >> 32), (uint32_t)b1, (uint32_t)(b1 >> 32));
    }
};
struct ApmAlignWaveDir {
    const uint4 *ws;
    int chunks;
    __device__ __forceinline__ int at(int x, int g) const {
        const uint4 v = ws[(size_t)(x - 1) * (size_t)chunks + (size_t)(g >> 6)];
        const uint32_t lo = (g & 32) ? v.y : v.x, hi = (g & 32) ? v.w : v.z;
        return (int)(((lo >> (g & 31)) & 1u) | (((hi >> (g & 31)) & 1u) << 1));
    }
};

/* One pair per wavefront, apm_score_wave's contract: every lane calls it with the same arguments and gets the same
 * answer.  ws: this wave's trace row, size * chunks entries of 16 bytes.  Out::store is called by every lane with the
 * same arguments (it picks the lane that stores). */
template <class Pat, class Txt, class Out>
__device__ __forceinline__ int apm_align_wave(const Pat &p, const Txt &t, int size, int k, int *band, int lane, uint4 *ws, Out &out) {
    const int h = min(k / 2, size - 1), chunks = (2 * h + 64) >> 6;
    ApmAlignWaveSink sink{ws, lane};
    if (apm_score_wave(p, t, size, k, band, lane, &sink) > k) return 0;
    __syncthreads(); // (lane 0's trace stores before every lane's loads of the walk back)
    const ApmAlignWaveDir dir{ws, chunks};
    return apm_align_walk(size, h, apm_align_max_ops(size, k), dir, out);
}

/* ---- the launch (apm_align.hip) ---- */
/* the scoring pass's block (shard text, records -- only read here --, patterns, k) and the align pass's own */
struct ApmAlignArgs : ApmScoreArgs {
    uint32_t *ops;                 /* device: row r at ops + r * stride */
    uint32_t stride;               /* dwords, >= apm_align_words(the set's most ops) */
    void *ws;                      /* trace workspace: lane form rows * m_max halfwords, wave form rows * row_entries uint4 */
    uint32_t m_max;
    unsigned long long row_entries; /* wave form: 16-byte entries of one trace row */
};
/* rows: trace rows of the workspace = lanes (lane form, a multiple of 64) or wavefronts (wave form) of the grid */
hipError_t apm_launch_align(const ApmAlignArgs &a, uint32_t rows, hipStream_t s);
#endif

/* trace rows and bytes of the workspace for a set of longest pattern m_max at k on a device of n_cu compute units */
static inline size_t apm_align_wave_row_entries(int m_max, int k) {
    const int h = apm_score_min(k / 2, m_max - 1);
    return (size_t)m_max * (size_t)((2 * h + 1 + 63) >> 6);
}
static inline uint32_t apm_align_rows(int m_max, int k, int n_cu, int block, size_t *bytes) {
    const size_t budget = APM_ALIGN_WS_BUDGET;
    if (k > APM_SCORE_LANE_MAX_K) {
        const size_t row = apm_align_wave_row_entries(m_max, k) * 16;
        size_t rows = budget / row;
        if (rows < 1) rows = 1;
        if (rows > (size_t)n_cu * 8) rows = (size_t)n_cu * 8;
        *bytes = rows * row;
        return (uint32_t)rows;
    }
    size_t rows = budget / (2 * (size_t)m_max);
    if (rows < 64) rows = 64;
    if (rows > (size_t)n_cu * 4 * (size_t)block) rows = (size_t)n_cu * 4 * (size_t)block;
    rows -= rows % (rows >= (size_t)block ? (size_t)block : 64); /* whole workgroups (below one: whole waves) */
    *bytes = k / 2 ? rows * 2 * (size_t)m_max : 0; /* BAND 0 keeps no trace */
    return (uint32_t)rows;
}

#endif /* APM_ALIGN_H */
