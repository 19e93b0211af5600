/*
 * apm_banded.h -- what the two BANDED filter kernels share by source: the LDS-tile kernel (apm_banded_tile.h, instantiated
 * by apm_banded_tile_b0.hip .. _b3.hip, launched by apm_banded_tile.hip) and the wave-autonomous stream kernel
 * (apm_banded_stream.hip).
 */
#ifndef APM_BANDED_H
#define APM_BANDED_H

#include "apm_device.h"

// ---------------------------------------------------------------------------
// BANDED: exact shortcut for the predicate dist <= k.
//
// (1) Equal-length global alignment with <= k edits has #ins == #del <= k/2, so
//     only the diagonals |x-y| <= band = k/2 can carry it (k<=1: Hamming).
// (2) Pigeonhole: cut the pattern into k+1 disjoint pieces; <= k edits leave one
//     piece intact, and it sits in the window at its own offset shifted by
//     delta in [-band, band].
// (3) Sampling: a piece of length L >= 2*KL-1 contains a KL-byte block that is
//     KL-ALIGNED in the text whatever the window's alignment; so it is enough to
//     look at every KL-th text position (STRIDE = KL) and to know, per piece,
//     its KL shifted sub-keys pattern[a_q + r : a_q + r + KL), r = 0..KL-1.
//     Shorter pieces (L >= KL) use STRIDE = 1 (every position, r = 0).
// A window is a CANDIDATE only if some sub-key occurs at a sampled text position
// consistent with it:  j = position - (a_q + r) - delta.
//
// Workgroup = persistent, software-pipelined walker over tiles of 4096 text
// bytes (16 per lane): the 16-byte buffer loads of tiles t+G and t+2G are in
// flight while tile t is processed out of LDS.  Per tile:
//   filter   each lane fingerprints its 16/STRIDE sampled positions and looks the
//            fingerprint up in an LDS hash table of all sub-keys of the launch
//            (4-way buckets of 32-bit tags + a short overflow list): ~10 VALU
//            ops and one ds_read_b128 per lookup, independent of the key count;
//   enqueue  a tag match pushes (key, position) into an LDS queue;
//   verify   all lanes pop the queue: byte-compare the key (fingerprints can
//            collide), banded DP with early exit over the candidate window,
//            and count it only from its FIRST true (piece, shift) nominator so a
//            window nominated several times is counted once (stateless dedup).
// A queue overflow (adversarial low-entropy text) falls back to a dense pass of
// the same verification over every (sampled position, key) of the tile.
// Per launch the text is read from HBM exactly once (+ halo per tile).
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t apm_fp8(uint32_t lo, uint32_t hi) {
    return lo + (hi << 3); // v_lshl_add_u32; injective on ACGT 8-mers (no carries between bytes)
}
__device__ __forceinline__ uint32_t apm_fp16(uint32_t f_lo, uint32_t f_hi) {
    return f_lo + __umul24(f_hi, 0x9E3779u); // v_mad_u32_u24: 16 text bytes -> 32 bits
}
__device__ __forceinline__ uint32_t apm_slot_hash(uint32_t f) {
    return __umul24(f, 0x9E3779u) + __umul24(f >> 12, 0x85EBCAu); // bucket = top bits, tag = low 16 bits
}

// bucket = top bits, tag = low 16 bits.  A 16-byte fingerprint is already mixed by its mad24;
// an 8-byte one (lo + hi*8, injective but structured) needs the extra multiply-mix.
template <int KL>
__device__ __forceinline__ uint32_t apm_table_hash(uint32_t f) {
    if constexpr (KL == 16) return f;
    else return apm_slot_hash(f);
}


// mask of the key bytes living in the second dword of an (up to) 8-byte key
template <int KL>
__device__ __forceinline__ constexpr uint32_t apm_hi_mask() {
    return KL >= 8 ? 0xffffffffu : (KL <= 4 ? 0u : ((1u << (8 * ((KL - 4) & 3))) - 1u));
}

template <int KL>
__device__ __forceinline__ bool apm_key_equal(const uint8_t *tb, int toff, const uint8_t *pb, int poff) {
    constexpr int ND = (KL + 3) / 4;
    uint32_t x[ND], y[ND];
    apm_lds_dwords<ND>(tb, toff, x);
    apm_lds_dwords<ND>(pb, poff, y);
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < ND; ++i) {
        uint32_t t = x[i] ^ y[i];
        if (i == ND - 1 && (KL & 3)) t &= (1u << (8 * (KL & 3))) - 1u;
        d |= t;
    }
    return d == 0u;
}

// where a candidate window's text bytes come from: the LDS tile (tile kernel) or global memory
// (stream kernel; the bytes were streamed moments ago, so they sit in L2 / Infinity Cache)
struct ApmLdsText {
    const uint8_t *base; // 16-byte aligned LDS buffer
    int off;             // window start inside it
    static constexpr bool kBlocks = false;
    __device__ __forceinline__ bool can16(int) const { return true; }
    __device__ __forceinline__ void load16(uint32_t (&T)[4]) const { apm_lds_dwords<4>(base, off, T); }
    __device__ __forceinline__ int byte(int x) const { return (int)base[off + x]; }
};
struct ApmGlobalText {
    const uint8_t *text; // 16-byte aligned
    int64_t off;         // window start (relative position)
    int64_t limit;       // bytes readable from text (avail_pad)
    static constexpr bool kBlocks = false;
    __device__ __forceinline__ bool can16(int) const { return (off & ~(int64_t)3) + 20 <= limit; }
    __device__ __forceinline__ void load16(uint32_t (&T)[4]) const {
        const uint32_t *a = reinterpret_cast<const uint32_t *>(text + (off & ~(int64_t)3));
        const uint32_t sh = (uint32_t)off & 3u;
        uint32_t w[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) w[i] = a[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) T[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
    }
    __device__ __forceinline__ int byte(int x) const { return (int)text[off + x]; }
};


// ---- hierarchical verification (per-position key classes) ---------------------------------
// The k+1 pigeonhole pieces are paired (0,1), (2,3), ...  With <= k edits in the window some pair
// carries <= 1 edit (or, for even k, the unpaired last piece is intact), and inside such a pair one
// piece is intact while its partner matches the adjoining text with <= 1 edit, anchored at the
// intact piece and free at the far end.  A key hit therefore only needs the expensive window DP if
// (a) the rest of its piece is intact and (b) its partner extends with <= 1 edit -- two short byte
// comparisons that reject almost every random key hit.
// Core for partner pieces of <= 16 bytes (apm_ext1_core16 below): the one edit is located by the first
// mismatching byte i; the three ways to spend it are checked with shifted compares: substitution (P vs T),
// pattern byte without text counterpart (P vs T<<8), one extra text byte (P vs T>>8).  Longer partners (only
// when long patterns joined a per-position class) take the byte loops of apm_ext_fwd / apm_ext_bwd.
// (apm_ext1_core16 lives in apm_core.h: tests/host_core_test.cpp checks it against the byte loops on the host)
// pattern pb[pp..pp+n) vs text read FORWARD from tb[tp]: <= 1 edit, all of the pattern consumed
__device__ __forceinline__ bool apm_ext_fwd(const uint8_t *tb, int tp, const uint8_t *pb, int pp, int n) {
    int i = 0;
    while (i < n && tb[tp + i] == pb[pp + i]) ++i;
    if (i >= n - 1) return true; // no mismatch, or a single substitution at the last byte
    bool ok = true;              // substitution at i
    for (int j = i + 1; j < n && ok; ++j) ok = tb[tp + j] == pb[pp + j];
    if (ok) return true;
    ok = true;                   // pattern byte i has no text counterpart
    for (int j = i + 1; j < n && ok; ++j) ok = tb[tp + j - 1] == pb[pp + j];
    if (ok) return true;
    ok = true;                   // one extra text byte before pattern byte i
    for (int j = i; j < n && ok; ++j) ok = tb[tp + j + 1] == pb[pp + j];
    return ok;
}
// pattern pb[pp..pp+n) vs text read BACKWARD from tb[te-1] (te exclusive): <= 1 edit
__device__ __forceinline__ bool apm_ext_bwd(const uint8_t *tb, int te, const uint8_t *pb, int pp, int n) {
    int i = 0;
    while (i < n && tb[te - 1 - i] == pb[pp + n - 1 - i]) ++i;
    if (i >= n - 1) return true;
    bool ok = true;
    for (int j = i + 1; j < n && ok; ++j) ok = tb[te - 1 - j] == pb[pp + n - 1 - j];
    if (ok) return true;
    ok = true;
    for (int j = i + 1; j < n && ok; ++j) ok = tb[te - j] == pb[pp + n - 1 - j];
    if (ok) return true;
    ok = true;
    for (int j = i; j < n && ok; ++j) ok = tb[te - 2 - j] == pb[pp + n - 1 - j];
    return ok;
}

typedef __attribute__((address_space(3))) uint8_t apm_lds_u8; // LDS byte, for constant-address accesses

#endif
