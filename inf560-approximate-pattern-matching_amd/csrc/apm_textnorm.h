/*
 * apm_textnorm.h -- the text-normalisation pass (include/apm.h: APM_TEXT_FASTA, APM_TEXT_UPPER): its per-lane
 * arithmetic, the algebra of its block summaries and the launch arguments.  Everything above the `__HIPCC__` part compiles
 * for host and device: the kernels (apm_textnorm.hip) and tests/host_textnorm_test.cpp run this very code.
 *
 * The pass reads the source in 4 KiB blocks cut on the 16-byte grid of memory (block 0 begins at the 16-byte boundary at
 * or in front of the source pointer), one wavefront per block, four chunks of 64 lanes x 16 bytes.  A lane sees its 16
 * bytes as three 16-bit masks -- '\n', '\r', '>' -- and resolves them without a loop over the bytes:
 *   line starts   LS = (NL << 1) | (the line-start bit handed in by the lane below)
 *   header opens  S  = (LS & GT) | (in header on entry)
 *   header bytes  H  = ((~NL + S) ^ ~NL): adding an opening bit to the run of non-'\n' bytes above it carries through
 *                 the run and stops in the '\n' that ends the header; a carry out of bit 15 is "still in a header"
 *   kept          valid & ~(H | NL | CR)
 * Two headers never open in one run ('>' opens only behind a '\n'), so the carries of one addition do not meet.
 * Bytes outside the source (in front of it in block 0, behind it in the last block) enter as '\n': dropped, and the
 * first source byte is a line start.  Without APM_TEXT_FASTA every valid byte is kept and there is no header state.
 *
 * Across lanes the header state is a two-state machine: a lane with a '\n', or one that opens a header, FIXES the state
 * behind it whatever it was handed; every other lane passes it on.  Two ballots (fixed, the fixed value) give every
 * lane its incoming state: that of the nearest lower fixed lane, or the chunk's own below the first one.  Across blocks
 * the same holds, and a block's summary carries the kept count and the outgoing state for both incoming states.
 */
#ifndef APM_TEXTNORM_H
#define APM_TEXTNORM_H

#include <stdint.h>

#if defined(__HIPCC__)
#define APM_TN_FN __host__ __device__ __forceinline__
#else
#define APM_TN_FN static inline
#endif

#define APM_TN_FASTA 1u /* APM_TEXT_FASTA */
#define APM_TN_UPPER 2u /* APM_TEXT_UPPER */
#define APM_TN_BLOCK 4096u            /* source bytes per block = per wavefront (the sieve's block) */
#define APM_TN_CHUNK 1024u            /* 64 lanes x 16 bytes */
#define APM_TN_STATE_BIT 63           /* map[b]: kept bytes in front of block b, bit 63 = block b is entered inside a header */
#define APM_TN_PREFIX_MASK 0x7fffffffffffffffull

// bit z of the result = byte z of w equals c (exact: no false positive behind a matching byte)
APM_TN_FN uint32_t apm_tn_eq4(uint32_t w, uint32_t c) {
    const uint32_t x = w ^ (c * 0x01010101u);
    const uint32_t nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; // bit 7 of every non-zero byte
    return ((((nz ^ 0x80808080u) >> 7) * 0x00204081u) >> 21) & 15u;
}

APM_TN_FN uint32_t apm_tn_eq16(const uint32_t (&w)[4], uint32_t c) {
    return apm_tn_eq4(w[0], c) | (apm_tn_eq4(w[1], c) << 4) | (apm_tn_eq4(w[2], c) << 8) | (apm_tn_eq4(w[3], c) << 12);
}

// 'a'..'z' -> 'A'..'Z' in the four bytes of w, every other byte value as it is
APM_TN_FN uint32_t apm_tn_upper4(uint32_t w) {
    const uint32_t lo = w & 0x7f7f7f7fu;
    const uint32_t ge_a = lo + 0x1f1f1f1fu; // bit 7: low seven bits >= 0x61
    const uint32_t gt_z = lo + 0x05050505u; // bit 7: low seven bits >= 0x7b
    return w ^ ((ge_a & ~gt_z & ~w & 0x80808080u) >> 2);
}

struct ApmTnMasks { uint32_t nl, cr, gt; }; // 16 bits each, bit i = byte i of the lane

// the lane's masks; valid: bit i = byte i belongs to the source (the others enter as '\n')
APM_TN_FN ApmTnMasks apm_tn_masks(const uint32_t (&w)[4], uint32_t valid) {
    ApmTnMasks m;
    m.nl = (apm_tn_eq16(w, 0x0au) & valid) | (~valid & 0xffffu);
    m.cr = apm_tn_eq16(w, 0x0du) & valid;
    m.gt = apm_tn_eq16(w, 0x3eu) & valid;
    return m;
}

struct ApmTnLane { uint32_t keep, count, h_out; }; // keep mask (16 bits), its popcount, in a header behind the lane

// the lane resolved: h_in = in a header on entry, ls_in = the lane's first byte is a line start
APM_TN_FN ApmTnLane apm_tn_resolve(const ApmTnMasks &m, uint32_t valid, uint32_t flags, uint32_t h_in, uint32_t ls_in) {
    ApmTnLane r;
    if (!(flags & APM_TN_FASTA)) {
        r.keep = valid & 0xffffu;
        r.h_out = 0u;
    } else {
        const uint32_t run = ~m.nl & 0xffffu;
        const uint32_t opens = ((((m.nl << 1) | (ls_in & 1u)) & m.gt) | (h_in & 1u)) & 0xffffu;
        const uint32_t hdr = (run + opens) ^ run;
        r.keep = valid & ~(hdr | m.nl | m.cr) & 0xffffu;
        r.h_out = (hdr >> 16) & 1u;
    }
    r.count = (uint32_t)__builtin_popcount(r.keep);
    return r;
}

// the shared core in one call: the bytes of a lane, the incoming state and the line-start bit -> keep mask, kept count,
// outgoing state
APM_TN_FN ApmTnLane apm_tn_lane(const uint32_t (&w)[4], uint32_t valid, uint32_t flags, uint32_t h_in, uint32_t ls_in) {
    return apm_tn_resolve(apm_tn_masks(w, valid), valid, flags, h_in, ls_in);
}

// a lane fixes the state behind it if it holds a '\n' or opens a header; h_out0: its outgoing state for h_in = 0
APM_TN_FN bool apm_tn_fixes(const ApmTnMasks &m, uint32_t h_out0) { return m.nl != 0u || h_out0 != 0u; }

// incoming state of `lane` from the two ballots of its chunk (fixed: the lanes that fix; value: their h_out0): that of the
// nearest lower fixing lane, else the chunk's; lane == 64: the state behind the chunk
APM_TN_FN uint32_t apm_tn_state_at(uint64_t fixed, uint64_t value, uint32_t lane, uint32_t h_chunk) {
    const uint64_t below = lane >= 64u ? fixed : fixed & ((1ull << lane) - 1ull);
    if (!below) return h_chunk & 1u;
    return (uint32_t)(value >> (63 - __builtin_clzll(below))) & 1u;
}

// position of the n-th (from 0) set bit of a 16-bit mask that has more than n bits set
APM_TN_FN uint32_t apm_tn_select16(uint32_t mask, uint32_t n) {
    uint32_t at = 0u;
    for (uint32_t half = 8u; half; half >>= 1) {
        const uint32_t c = (uint32_t)__builtin_popcount(mask & ((1u << half) - 1u));
        if (n >= c) { n -= c; at += half; mask >>= half; }
    }
    return at;
}

// ---- block summaries: one dword per block ----
// bits 0..12 kept count if entered outside a header, 13..25 if entered inside one, 26 / 27 the outgoing state of the two
APM_TN_FN uint32_t apm_tn_pack_summary(uint32_t cnt0, uint32_t cnt1, uint32_t out0, uint32_t out1) {
    return cnt0 | (cnt1 << 13) | ((out0 & 1u) << 26) | ((out1 & 1u) << 27);
}

// A run of blocks as a function of the state it is entered in: e[x] = kept bytes of the run entered in state x, bit 31 =
// the state behind it.  The scan composes these; a run's count stays below 2^31 (the scan's chunks are 2^12 blocks).
struct ApmTnFn { uint32_t e[2]; };

APM_TN_FN ApmTnFn apm_tn_fn_identity() { ApmTnFn f; f.e[0] = 0u; f.e[1] = 0x80000000u; return f; }

APM_TN_FN ApmTnFn apm_tn_fn_of(uint32_t summary) {
    ApmTnFn f;
    f.e[0] = (summary & 0x1fffu) | (((summary >> 26) & 1u) << 31);
    f.e[1] = ((summary >> 13) & 0x1fffu) | (((summary >> 27) & 1u) << 31);
    return f;
}

// first f, then g
APM_TN_FN ApmTnFn apm_tn_fn_then(const ApmTnFn &f, const ApmTnFn &g) {
    ApmTnFn r;
    r.e[0] = (f.e[0] & 0x7fffffffu) + ((f.e[0] >> 31) ? g.e[1] : g.e[0]);
    r.e[1] = (f.e[1] & 0x7fffffffu) + ((f.e[1] >> 31) ? g.e[1] : g.e[0]);
    return r;
}

// the map entry of a block: `before` kept bytes in front of the scan chunk that is entered in state s, f = the blocks of
// the chunk in front of this one
APM_TN_FN uint64_t apm_tn_map_entry(uint64_t before, uint32_t s, const ApmTnFn &f) {
    const uint32_t e = (s & 1u) ? f.e[1] : f.e[0];
    return (before + (uint64_t)(e & 0x7fffffffu)) | ((uint64_t)(e >> 31) << APM_TN_STATE_BIT);
}

// ---- the source as the kernels see it ----
struct ApmTnSrc {
    const uint8_t *base;   // the 16-byte boundary at or in front of the source's first byte: block b = base + 4096 b
    uint32_t lead;         // bytes between base and the first source byte (0..15)
    uint64_t end;          // lead + source length: offsets [lead, end) from base are the source
    uint64_t n_blocks;     // ceil(end / 4096)
    uint32_t flags;
};

// which of the 16 bytes at offset `at` from base (a multiple of 16) belong to the source
APM_TN_FN uint32_t apm_tn_valid16(const ApmTnSrc &s, uint64_t at) {
    uint32_t v = 0xffffu;
    if (at == 0u) v = (0xffffu << s.lead) & 0xffffu;
    if (at + 16u > s.end) v &= at >= s.end ? 0u : (0xffffu >> (16u - (uint32_t)(s.end - at)));
    return v;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

struct ApmTnArgs {
    ApmTnSrc src;
    uint32_t *summary;            // n_blocks dwords
    unsigned long long *map;      // n_blocks + 1 entries (apm_tn_map_entry; the last = the total, no state bit)
    unsigned long long *total;    // the total once more, for the host
    uint8_t *dst;                 // scatter: the kept bytes, dst[0 .. total)
};

struct ApmTnMapArgs {
    ApmTnSrc src;
    const unsigned long long *map;
    uint4 *rec;                        // apm_match records
    unsigned long long cap;
    const unsigned long long *n_rec;
};

// ---- device helpers of the block-wise kernels (apm_textnorm.hip, apm_seqindex.hip): one wavefront per 4 KiB block ----
// the lane's 16 bytes of each of the block's four chunks; a 16-byte unit wholly outside the source is not fetched
__device__ __forceinline__ void tn_load_block(const ApmTnSrc &s, uint64_t b, uint32_t lane, uint32_t (&w)[4][4], uint32_t (&valid)[4]) {
    uint4 v[4];
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) {
        const uint64_t at = b * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u;
        valid[c] = apm_tn_valid16(s, at);
        v[c] = valid[c] ? *reinterpret_cast<const uint4 *>(s.base + at) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (uint32_t c = 0; c < 4; ++c) { w[c][0] = v[c].x; w[c][1] = v[c].y; w[c][2] = v[c].z; w[c][3] = v[c].w; }
}

// is the block's first byte a line start: block 0 (whose leading bytes outside the source count as '\n'), or behind a '\n'
__device__ __forceinline__ uint32_t tn_block_line_start(const ApmTnSrc &s, uint64_t b) {
    return b == 0 ? 1u : (uint32_t)(s.base[b * APM_TN_BLOCK - 1] == (uint8_t)'\n');
}

struct TnChunk {
    ApmTnMasks m;
    uint32_t ls_in;                    // the lane's first byte is a line start
    unsigned long long fixed, value;   // ballots: the lanes that fix the header state, and to what
};

// one chunk's masks, line starts and ballots; ls: in = line-start bit of the chunk's first byte, out = of the next chunk's
__device__ __forceinline__ TnChunk tn_chunk(const uint32_t (&w)[4], uint32_t valid, uint32_t flags, uint32_t lane, uint32_t &ls) {
    TnChunk t;
    t.m = apm_tn_masks(w, valid);
    const uint32_t last_nl = t.m.nl >> 15;
    const uint32_t below = (uint32_t)__shfl_up((int)last_nl, 1);
    t.ls_in = lane ? below : ls;
    ls = (uint32_t)__builtin_amdgcn_readlane((int)last_nl, 63);
    const uint32_t h_out0 = apm_tn_resolve(t.m, valid, flags, 0u, t.ls_in).h_out;
    t.fixed = __builtin_amdgcn_ballot_w64(apm_tn_fixes(t.m, h_out0));
    t.value = __builtin_amdgcn_ballot_w64(h_out0 != 0u);
    return t;
}

__device__ __forceinline__ uint32_t tn_wave_total(uint32_t incl) { return (uint32_t)__builtin_amdgcn_readlane((int)incl, 63); }

/* apm_textnorm.hip */
hipError_t apm_launch_tn_summary(const ApmTnArgs &a, int n_cu, hipStream_t s);
hipError_t apm_launch_tn_scan(const ApmTnArgs &a, hipStream_t s);
hipError_t apm_launch_tn_scatter(const ApmTnArgs &a, int n_cu, hipStream_t s);
hipError_t apm_launch_tn_map(const ApmTnMapArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_TEXTNORM_H */
