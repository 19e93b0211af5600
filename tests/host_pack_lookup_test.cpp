// Host-side check of the sieve's streaming arithmetic (csrc/apm_core.h): the combine of apm_pack16 (apm_pack16_join) and the
// lookup words of apm_lookup2_chunk (apm_lookup2_mid, apm_lookup2_word) against the forms they replaced and against their
// definitions, all three in plain C++.  No GPU.
#include "apm_core.h"

#include <cstdio>
#include <cstdlib>

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() { return (uint32_t)(apm_splitmix64(rng_state++) >> 16); }

// v_dot4_u32_u8 with the byte weights 1, 4, 16, 64, as apm_pack16 applies it
static uint32_t dot4_weights(uint32_t v) {
    return (v & 0xffu) + 4u * ((v >> 8) & 0xffu) + 16u * ((v >> 16) & 0xffu) + 64u * (v >> 24);
}

// the combine as it was: every dot shifted to its byte, term by term
static uint32_t join_before(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t cs) {
    return (p0 >> cs) | (p1 << (8u - cs)) | (p2 << (16u - cs)) | (p3 << (24u - cs));
}

// the definition: byte z of dword q lands in bits 8 q + 2 z, its code is (byte >> cs) & 3
static uint32_t pack16_definition(const uint32_t (&d)[4], uint32_t cs) {
    uint32_t r = 0;
    for (int q = 0; q < 4; ++q)
        for (int z = 0; z < 4; ++z) r |= (((d[q] >> (8 * z)) >> cs) & 3u) << (8 * q + 2 * z);
    return r;
}

int main() {
    long bad = 0;
    for (int i = 0; i < 1000000; ++i) {
        uint32_t d[4] = {rnd32(), rnd32(), rnd32(), rnd32()};
        if (i % 5 == 0)  // text bytes: letters, where the code bits are few of the set ones
            for (uint32_t &w : d) w = (w & 0x1f1f1f1fu) | 0x40404040u;
        for (uint32_t cs = 0; cs <= 6; ++cs) {
            const uint32_t mask = 0x03030303u << cs;
            const uint32_t p0 = dot4_weights(d[0] & mask), p1 = dot4_weights(d[1] & mask);
            const uint32_t p2 = dot4_weights(d[2] & mask), p3 = dot4_weights(d[3] & mask);
            const uint32_t now = apm_pack16_join(p0, p1, p2, p3, cs);
            if (now != join_before(p0, p1, p2, p3, cs) || now != pack16_definition(d, cs)) {
                if (++bad <= 5) std::printf("pack16: %08x %08x %08x %08x cs %u -> %08x, before %08x, definition %08x\n", d[0], d[1], d[2],
                                            d[3], cs, now, join_before(p0, p1, p2, p3, cs), pack16_definition(d, cs));
            }
        }
    }
    // the eight words of a chunk: what the lookup reads of word t is bits 2..14 (the bitmap dword's byte address) and bits
    // 15..19 (the bit in it) = the 18-bit code word of position 2 t, bits 4 t .. 4 t + 17 of shi:slo
    for (int i = 0; i < 1000000; ++i) {
        uint32_t slo = rnd32(), shi = rnd32();
        if (i % 7 == 0) slo = i % 14 ? 0xffffffffu : 0u;
        if (i % 11 == 0) shi = i % 22 ? 0xffffffffu : 0u;
        const uint64_t both = ((uint64_t)shi << 32) | slo;
        const uint32_t mid = apm_lookup2_mid(slo, shi);
        for (int t = 0; t < 8; ++t) {
            const uint32_t before = t ? (uint32_t)(both >> (4 * t - 2)) : slo << 2;  // (v_alignbit_b32 (shi, slo, 4 t - 2))
            const uint32_t now = apm_lookup2_word(slo, mid, t);
            const uint32_t code = (uint32_t)(both >> (4 * t)) & 0x3ffffu;
            const bool same = (now & 0x7ffcu) == (before & 0x7ffcu) && ((now >> 15) & 31u) == ((before >> 15) & 31u);
            const bool right = (now & 0x7ffcu) == ((code & 0x1fffu) << 2) && ((now >> 15) & 31u) == (code >> 13);
            if (!same || !right) {
                if (++bad <= 10) std::printf("lookup: slo %08x shi %08x t %d -> %08x, before %08x, code word %05x\n", slo, shi, t, now, before, code);
            }
        }
    }
    if (bad) {
        std::printf("%ld mismatches\n", bad);
        return 1;
    }
    std::printf("pack16 combine: 1000000 quadruples at code shifts 0..6; lookup words: 1000000 (slo, shi) pairs, t = 0..7: equal\n");
    return 0;
}
