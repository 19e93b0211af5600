/*
 * apm_wave.h -- the wave-level idioms of the sieve + verify pipeline (apm_sieve.hip, apm_verify.hip), one definition each.
 * Device only.
 */
#ifndef APM_WAVE_H
#define APM_WAVE_H

#include "apm_device.h"

typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) uint32_t apm_lds_u32; // LDS dword, for constant-base accesses

__device__ __forceinline__ uint32_t apm_udot4(uint32_t a, uint32_t b) {
    return __builtin_amdgcn_udot4(a, b, 0u, false); // v_dot4_u32_u8
}

// 2-bit codes of 16 bytes (four dwords): byte z of dword q lands in bits 8 q + 2 z.  The code bits are masked where they
// are (byte >> cs is not formed), one v_dot4_u32_u8 per dword leaves (codes << cs), and the shifts go into the combine:
// 12 instructions instead of 15.
// PAIRS: the combine by pairs (apm_pack16_join, apm_core.h), one instruction fewer -- the diagonal sieve kernel's form
// (five packs per 4 KiB block).  The other kernels keep the term-by-term combine: the registers of the kernels in
// apm_sieve.hip are pinned, and by pairs the record build of apm_fused_kernel<0, true> (apm_verify.hip) goes from 61 to 65
// VGPRs and loses its eighth wave per SIMD.
template <bool PAIRS = false>
__device__ __forceinline__ uint32_t apm_pack16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t cs) {
    const uint32_t mask = 0x03030303u << cs;
    const uint32_t p0 = apm_udot4(x & mask, 0x40100401u), p1 = apm_udot4(y & mask, 0x40100401u);
    const uint32_t p2 = apm_udot4(z & mask, 0x40100401u), p3 = apm_udot4(w & mask, 0x40100401u);
    if constexpr (PAIRS) return apm_pack16_join(p0, p1, p2, p3, cs);
    else return (p0 >> cs) | (p1 << (8u - cs)) | (p2 << (16u - cs)) | (p3 << (24u - cs));
}

// 4 bytes -> 8 code bits (byte z in bits 2z..): shift + and + one v_dot4_u32_u8 with the byte weights 1, 4, 16, 64
__device__ __forceinline__ uint32_t apm_pack4(uint32_t w, uint32_t cs) {
    return apm_udot4((w >> cs) & 0x03030303u, 0x40100401u);
}

// the lane's rank among the set bits of a ballot: the set bits below it
__device__ __forceinline__ uint32_t apm_wave_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Append one round of values to a wave's queue of `count` entries (wave-uniform), no atomics: the lanes that have one
// store in lane order behind the entries there are, and count moves on.  wrap: index mask of a ring (a power of two - 1).
template <typename T>
__device__ __forceinline__ void apm_wave_append(T *dst, uint32_t &count, bool has, uint32_t value, uint32_t wrap = 0xffffffffu) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(has);
    if (has) dst[(count + apm_wave_rank(mask)) & wrap] = (T)value;
    count += (uint32_t)__builtin_popcountll(mask);
}

// inclusive prefix sum over the wave: within the rows of 16 lanes, then across them (six DPP adds)
__device__ __forceinline__ uint32_t apm_wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); // row_bcast:31 -> rows 2, 3
    return v;
}

// Stride-1 lookup of a chunk: the hits of the lane's eight even positions in the 32 KiB bitmap over 18-bit code words that
// LEADS the kernel's LDS (address 0: LDS address = the masked code bits), bit 24 + t = position 2t.  slo: codes of the
// lane's 16 bytes; nx0: of the 8 bytes behind the chunk.  The codes of the 8 bytes behind the LANE's 16 are the low half of
// the next lane's string: one DPP move (wave_shl:1; the last lane keeps `old` = nx0) instead of a second load and two more
// packs.
// MID: positions 8..14 take their words out of ONE funnel shift of the two by plain shifts (apm_lookup2_word, apm_core.h),
// not out of a funnel shift each -- the same bits 2..19; the diagonal sieve kernel's form.  The other kernels keep theirs:
// their registers are pinned (tests/test_verify_resources.py).
template <bool MID = false>
__device__ __forceinline__ uint32_t apm_lookup2_chunk(uint32_t slo, uint32_t nx0) {
    const uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp((int)nx0, (int)slo, 0x130, 0xf, 0xf, false);
    const uint32_t mid = MID ? apm_lookup2_mid(slo, shi) : 0u;
    uint32_t hits = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        // y: the 18-bit code word of position 2t in bits 2..19 -> byte address of its bitmap dword = y & 0x7ffc,
        // bit index = bits 15..19 (a shift by a VGPR uses its low five bits)
        const uint32_t y = MID ? apm_lookup2_word(slo, mid, t) : (t ? __builtin_amdgcn_alignbit(shi, slo, 4u * (uint32_t)t - 2u) : (slo << 2));
        const uint32_t word = *(const apm_lds_u32 *)(uintptr_t)(y & 0x7ffcu);
        hits = __builtin_amdgcn_alignbit(word >> ((y >> 15) & 31u), hits, 1u); // bit 0 of the shifted word enters at the top
    }
    return hits;
}

// Cursor over the key list of a 16-bit code word in a verify image (ApmVerifyArgs::image: bitmap | prefix | r2s | slots).
// cur: bits 0..14 = the payload of the key in hand (key id in the low KBITS bits; above them, sampled sets: the offset r of
// the 8-byte block inside the key's piece), bit 15 = the key is the last of its list, bits 16..31 = index of the list's
// next entry in slots.
struct ApmKeyList {
    const uint32_t *s_bmp;
    const uint16_t *s_prefix, *s_r2s, *s_slots;
    // the first key of code word x (its bit is set in the bitmap): the word's list by rank among the set bits
    __device__ __forceinline__ uint32_t first(uint32_t x) const {
        const uint32_t bit = x >> 11, word = s_bmp[x & 2047u];
        const uint32_t e = s_r2s[(uint32_t)s_prefix[x & 2047u] + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u))];
        return (e & 0x8000u) ? e : ((uint32_t)s_slots[e] | ((e + 1u) << 16));
    }
    __device__ __forceinline__ uint32_t next(uint32_t cur) const { return (uint32_t)s_slots[cur >> 16] | ((cur & 0xffff0000u) + 0x10000u); }
    static __device__ __forceinline__ bool last(uint32_t cur) { return (cur & 0x8000u) != 0u; }
    static __device__ __forceinline__ uint32_t kid(uint32_t cur, uint32_t KBITS) { return cur & ((1u << KBITS) - 1u); }
    static __device__ __forceinline__ uint32_t r(uint32_t cur, uint32_t KBITS) { return (cur & 0x7fffu) >> KBITS; }
};

#endif /* APM_WAVE_H */
