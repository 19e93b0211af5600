/*
 * apm_verify.hip -- VERIFY, and SIEVE + VERIFY FUSED: the second launch of the pipeline of the per-position key classes of
 * the BANDED path behind the sieve of apm_sieve.hip, or the whole pipeline in one launch.
 *
 *   apm_verify_kernel   mask-driven: a wave walks its run of blocks, compacts the hits into batches of 64 (one
 *                       candidate per lane, dense across block borders: the text comes from global memory).  Key identification by rank
 *                       over the exact 16-bit presence bitmap (two dependent LDS reads, no hashing, no tags),
 *                       piece compare + pair pre-check against global text (bounds-checked buffer loads), the
 *                       survivors of a wave are collected and the banded DP + stateless dedup run on dense lanes.
 *   apm_fused_kernel    the same body; the wave sieves its blocks itself instead of reading the masks of a sieve launch.
 *
 * Both need a 16-byte aligned text pointer and a shard of < 4 GiB, as the sieve does.
 */
#include <algorithm>
#include "apm_wave.h"
#include "apm_sieve.h"
#include "apm_launch.h"

/* tuning constants (each measured on MI355X with tools/ab_libs.sh, one box per comparison) */
#ifndef APM_WORK_CH
#define APM_WORK_CH 8u /* blocks per chunk of the dynamic distribution, per-position sets (2, 8: the same within 3 %; 8 = fewer atomics when most rows are empty) */
#endif
#ifndef APM_WORK_CH8
#define APM_WORK_CH8 8u /* ... sampled sets (8, 16: the same) */
#endif
#ifndef APM_VERIFY_PIPE
#define APM_VERIFY_PIPE 2 /* batches formed ahead of the one in hand (2 beats 1 by 17 % on cfg3: the window loads of batch b+1 then do not wait for the queue reads that form it) */
#endif
#ifndef APM_FUSED_PIPE
#define APM_FUSED_PIPE 1 /* the same for the fused form (1 and 2 equal for sampled sets; 2 costs registers) */
#endif
#ifndef APM_VERIFY_AHEAD
#define APM_VERIFY_AHEAD 2 /* mask rows in flight per wave in front of the block in hand, per-position sets (1, 2, 4: the same within the box-to-box noise; 4 spills in the 72-register instantiation) */
#endif
#ifndef APM_FUSED_S_WAVES
#define APM_FUSED_S_WAVES 6 /* waves per SIMD the sampled fused form with band 1 is compiled for (80 registers; 5: 86 registers, cfg4 0.205 -> 0.198 ms; 7 and 8 fit only without the prefetch and measured 0.200 / 0.210: profiles/r03/cfg4_ab.txt) */
#endif
#ifndef APM_DEDUP_PREFETCH
#define APM_DEDUP_PREFETCH(band, sampled, fused) (!(fused) && !(sampled)) /* the dedup's predicate gets its partner text fetched beside the unit's own (ApmVerifyCore::nominates): \
    six registers more in flight -- the sampled forms with band 1 (80 registers for 6 waves) would lose a wave or spill */
#endif
#ifndef APM_DEDUP_WIDE
#define APM_DEDUP_WIDE(band, sampled, fused) ((band) >= 1) /* which instantiations resolve a round's matches side by side (ApmVerifyCore::count_matches): \
    with a band and without the prefetch it takes 2..6 registers fewer in every one of them (78 against 80 in the list-driven kernel, 80 with the prefetch); at band 0 (k = 0: at most 7 earlier nominators) it costs 3..8 and the two sampled forms a wave of occupancy */
#endif
/* settled, no longer switches: the fused sampled form takes ONE block per sieve step with the NEXT block's 4 KiB in flight
   while this one is sieved and its hits verified -- the access shape of the plain sieve kernels (tools/stream_probe.hip:
   4 KiB per wave and round streams at 6.2 TB/s, 8 KiB at 4.4; two blocks per step without the prefetch had beaten one by
   4 %, four spilled) -- and its blocks are dealt statically (apm_verify_body, STATIC_BLOCKS) */

// ---------------------------------------------------------------------------
// VERIFY
// ---------------------------------------------------------------------------
// text of the shard behind a bounds-checked buffer resource: bytes at or beyond avail_pad (and "negative"
// positions, which wrap to huge offsets) read as zero, for every path alike
struct ApmBufText {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t off; // window start (relative position)
    static constexpr bool kBlocks = true; // the DP fetches its columns 16 at a time (apm_banded_verify)
    __device__ __forceinline__ bool can16(int) const { return true; }
    __device__ __forceinline__ void load16(uint32_t (&T)[4]) const { load16_at(0, T); }
    __device__ __forceinline__ void load16_at(int x0, uint32_t (&T)[4]) const {
        const uint32_t a0 = (off + (uint32_t)x0) & ~3u, sh = (off + (uint32_t)x0) & 3u;
        const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)a0, 0, 0);
        const uint32_t hi = __builtin_amdgcn_raw_buffer_load_b32(rs, (int)(a0 + 16u), 0, 0);
        T[0] = __builtin_amdgcn_alignbyte(lo.y, lo.x, sh);
        T[1] = __builtin_amdgcn_alignbyte(lo.z, lo.y, sh);
        T[2] = __builtin_amdgcn_alignbyte(lo.w, lo.z, sh);
        T[3] = __builtin_amdgcn_alignbyte(hi, lo.w, sh);
    }
    __device__ __forceinline__ int byte(int x) const { return (int)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(off + (uint32_t)x), 0, 0); }
};

// six dwords of text from a 4-byte aligned position a0: bytes [a0, a0 + 24)
struct ApmWin { uint32_t w[6]; };

// The verification core shared by the list-driven verify kernel and the fused kernel: the nomination predicate of a
// unit, the banded DP of the window it implies, and the stateless dedup of matches.  Text comes through a bounds-checked
// buffer resource (zeros outside the shard); the predicate takes the loader of its partner's text as a parameter (the
// fused kernel reads it out of its LDS copy of the block).
// PREFIX: the predicate judges the exact part by its first 16 bytes and the partner by the 16 bytes that adjoin the exact
// part, whatever their lengths (apm_core.h, apm_unit_pred16) -- the
// per-position sets, whose sieve tests nothing beyond them.  The sampled sets keep the full predicate, byte loops over
// parts beyond 16 bytes included: the fused form's register compare may test piece bytes 16..22, so a position at
// which only the prefix form holds need not be delivered, and the dedup would defer to a nominator that never ran.
template <int BAND, bool PREFIX>
struct ApmVerifyCore {
    static constexpr int NSH = 2 * BAND + 1;
    static constexpr bool PAIRS = BAND >= 1;
    const ApmVerifyArgs &a;
    __amdgpu_buffer_rsrc_t rs;
    uint32_t avail;
    const uint32_t *s_kext;
    const uint4 *s_masks;
    const uint8_t *s_pat;
    uint32_t *s_cnt;
    int lane;
    const uint32_t *s_kinfo; // per key (LDS: the DP and the dedup are a chain of dependent reads, and with the sieve's code
    const uint2 *s_pinfo;    // filter in front they are most of what the launch does); per pattern

    __device__ __forceinline__ void load_global(uint32_t a0, ApmWin &o) const {
        const u32x4 lo = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)a0, 0, 0);
        const v2u32 hi = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(a0 + 16u), 0, 0);
        o.w[0] = lo.x; o.w[1] = lo.y; o.w[2] = lo.z; o.w[3] = lo.w; o.w[4] = hi.x; o.w[5] = hi.y;
    }
    __device__ __forceinline__ int gbyte(uint32_t pos) const { // (slow paths only)
        return (int)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)pos, 0, 0);
    }

    // ---- the nomination predicate: key `kid` (one pigeonhole piece) at text position s --------------------
    // piece intact at s, entirely inside the valid text, and (k >= 2) its partner of the pair pre-check within one
    // edit (see apm_banded.h, "hierarchical verification"); PREFIX: of the piece its first 16 bytes, of the
    // partner the 16 bytes that adjoin the piece.
    // `win` = the six text dwords at s & ~3.
    // ONE definition for the candidates of the list and for the dedup's "earlier nominator" test.
    template <typename LoadWin>
    __device__ __forceinline__ bool stage1(uint32_t kid, uint32_t s, const ApmWin &win, LoadWin &&load_win) const {
        typedef unsigned long long u64;
        const uint32_t kx = s_kext[kid];
        const int at = (int)(kx & 0xffffu), len = (int)((kx >> 16) & 0xffu), n = (int)((kx >> 24) & 31u), side = (int)(kx >> 29);
        if ((u64)s + (u64)len > (u64)avail) return false;
        const uint32_t sh = s & 3u;
        uint32_t A[4], B[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) A[i] = __builtin_amdgcn_alignbyte(win.w[i + 1], win.w[i], sh); // text bytes [s, s+16)
        apm_lds_dwords<4>(s_pat, at, B);
        if constexpr (PREFIX) {
            if (!apm_unit_exact16(A, B, len)) return false; // the first min(len, 16) bytes of the exact part are not intact
        } else {
            const uint4 mk = s_masks[len < 16 ? len : 16]; // 0xff for the first min(len, 16) bytes
            if ((((A[0] ^ B[0]) & mk.x) | ((A[1] ^ B[1]) & mk.y) | ((A[2] ^ B[2]) & mk.z) | ((A[3] ^ B[3]) & mk.w)) != 0u) return false; // the exact part is not intact
            for (int x = 16; x < len && !APM_SKIP(a, 2048); ++x) // (pieces beyond 16 bytes: patterns with long pieces in this class)
                if (gbyte(s + (uint32_t)x) != (int)s_pat[at + x]) return false;
        }
        if (!PAIRS || side == 0) return true; // no pre-check (k <= 1) / unpaired last piece (even k)
        if (!PREFIX && n == 31) { // partner longer than 16 bytes: byte loops (definition of the core, apm_ext_fwd / apm_ext_bwd)
            if (APM_SKIP(a, 2048)) return true; // (measurement, with the loop above: what the bytes beyond the 16-byte tests cost)
            const uint32_t kp = a.kpart[kid];
            const int poff = (int)(s_pinfo[s_kinfo[kid] & 0xfffu].x & 0xffffu), ap = (int)(kp & 0xffffu), nn = (int)(kp >> 16), ap1 = ap + nn;
            const bool fwd = side == 1;
            auto T = [&](int i) { return fwd ? gbyte(s + (uint32_t)len + (uint32_t)i) : gbyte(s - 1u - (uint32_t)i); };      // text, read away from the exact part
            auto P = [&](int i) { return fwd ? (int)s_pat[poff + ap + i] : (int)s_pat[poff + ap1 - 1 - i]; };                // partner, same direction
            int i = 0;
            while (i < nn && T(i) == P(i)) ++i;
            if (i >= nn - 1) return true;
            bool ok = true;
            for (int j = i + 1; j < nn && ok; ++j) ok = T(j) == P(j);
            if (ok) return true;
            ok = true;
            for (int j = i + 1; j < nn && ok; ++j) ok = T(j - 1) == P(j);
            if (ok) return true;
            ok = true;
            for (int j = i; j < nn && ok; ++j) ok = T(j + 1) == P(j);
            return ok;
        }
        uint32_t P[4], T[5];
        ApmWin tw;
        if (side == 1) { // partner behind the piece: text read forward from the end of the piece
            const uint32_t tp = s + (uint32_t)len;
            if (len == 0 || APM_SKIP(a, 1024)) tw = win; // (a pair of short pieces as one unit: its text starts at s itself)
            else load_win(tp & ~3u, tw);
            apm_lds_dwords<4>(s_pat, at + len, P);
#pragma unroll
            for (int i = 0; i < 5; ++i) T[i] = __builtin_amdgcn_alignbyte(tw.w[i + 1], tw.w[i], tp & 3u);
        } else { // partner in front of it: both strings byte-reversed, text = the 20 bytes in front of s
            uint32_t Q[4], Wd[5];
            apm_lds_dwords<4>(s_pat, at - 16, Q);
            if (s >= 20u) {
                const uint32_t tp = s - 20u;
                if (APM_SKIP(a, 1024)) tw = win; // (measurement: what the dependent gather costs)
                else load_win(tp & ~3u, tw);
#pragma unroll
                for (int i = 0; i < 5; ++i) Wd[i] = __builtin_amdgcn_alignbyte(tw.w[i + 1], tw.w[i], tp & 3u);
            } else { // the first 20 positions of the shard: bytes in front of text[0] do not exist and read as zero
#pragma unroll
                for (int i = 0; i < 5; ++i) Wd[i] = 0u;
                for (int i = 20 - (int)s; i < 20; ++i) {
                    const uint32_t b = (uint32_t)gbyte(s - 20u + (uint32_t)i);
#pragma unroll
                    for (int d = 0; d < 5; ++d)
                        if ((i >> 2) == d) Wd[d] |= b << (8 * (i & 3));
                }
            }
#pragma unroll
            for (int z = 0; z < 4; ++z) P[z] = apm_bswap(Q[3 - z]);
#pragma unroll
            for (int z = 0; z < 5; ++z) T[z] = apm_bswap(Wd[4 - z]);
        }
        // necessary first: the partner's first four bytes within one edit (a prefix of an alignment with <= 1 edit has
        // <= 1 edit): nonzero-byte masks of P ^ T under the three alignments, 4 bits each; rejects ~9 of 10 random texts
        if (n >= 4) {
            auto nz4 = [](uint32_t x) { return apm_udot4((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7 & 0x01010101u, 0x08040201u); };
            const uint32_t z0 = nz4(P[0] ^ T[0]);
            if (z0 & (z0 - 1u)) { // two or more mismatching bytes under the substitution alignment
                const uint32_t i = (uint32_t)__builtin_ctz(z0); // first mismatching byte: 0..2
                const uint32_t z1 = nz4(P[0] ^ (T[0] << 8));                                  // pattern byte i has no text counterpart
                const uint32_t z2 = nz4(P[0] ^ __builtin_amdgcn_alignbyte(T[1], T[0], 1u));   // one extra text byte before pattern byte i
                if (((z1 >> (i + 1u)) != 0u) && ((z2 >> i) != 0u)) return false;
            }
        }
        if constexpr (PREFIX) return apm_unit_partner16(P, T, n); // (n = 31, beyond 16 bytes: the partner's 16 bytes next to the exact part)
        else return apm_ext1_core16(P, T, n);
    }


    // ---- banded DP of the window a nomination (unit kid at text position s) implies under shift dl ----
    // on a match: wpat = pattern slot, wj = window start, word = rank of (unit, shift) among the window's nominators
    __device__ __forceinline__ bool dp_match(uint32_t kid, uint32_t s, int dl, uint32_t &wpat, uint32_t &wj, uint32_t &word) const {
        const uint32_t ki = s_kinfo[kid];
        const int kpat = (int)(ki & 0xfffu), koff = (int)((ki >> 12) & 0x1ffu), kunit = (int)((ki >> 21) & 7u);
        const uint2 pinf = s_pinfo[kpat];
        const int poff = (int)(pinf.x & 0xffffu), m = (int)(pinf.x >> 16);
        const int64_t je_p = min(a.je, a.nrel - m + 1);
        const int64_t j = (int64_t)s - koff - dl; // candidate window start
        if (j < a.jb || j >= je_p) return false;
        wpat = (uint32_t)kpat;
        wj = (uint32_t)j;
        word = (uint32_t)(kunit * NSH + dl + BAND);
#ifdef APM_MEASURE
        if (APM_SKIP(a, 256)) atomicAdd(&a.stats[2], 1ull); // (bit 8 = collect the statistics: one atomic per DP item distorts the timing)
#endif
        return apm_banded_verify<BAND>(ApmBufText{rs, (uint32_t)j}, s_pat, poff, m, a.k);
    }

    // ---- stateless dedup: a matching window counts only from its FIRST true (unit, shift) nominator.  Matches are
    // rare but come in bursts (an occurrence is nominated by every intact unit, its neighbour windows match too, and
    // they all sit in one wave).  Among the matches of a round a window is kept by its smallest (unit, shift) only;
    // for what is left the predicate is evaluated for every earlier (unit, shift), up to 8 x NSH - 1 per match, each
    // evaluation in a lane of its own with its own text fetches: for all the round's matches at once (WIDE), or match
    // by match (band 0). ----
    // the earlier nominator `idx` (rank among the (unit, shift) pairs of pattern slot bpat) of the window at bj: true?
    template <bool PREF>
    __device__ __forceinline__ bool nominates(uint32_t bpat, uint32_t bj, int idx) const {
        const uint32_t kid = s_pinfo[bpat].y + (uint32_t)(idx / NSH); // (.y: the pattern's first unit)
        const int dd = idx % NSH - BAND;
        const int64_t o = (int64_t)bj + (int)((s_kinfo[kid] >> 12) & 0x1ffu) + dd; // the unit's text position under shift dd
        if (o < 0) return false;
        ApmWin w2;
        load_global((uint32_t)o & ~3u, w2);
        if constexpr (PAIRS && PREF) {
            // the partner's text goes out with the unit's own, not after it: where the predicate will look for it follows from
            // the key alone (stage1: behind the piece, or the 20 bytes in front of it).  A guess only -- the predicate asks for
            // an address and gets the window of that address, from here when the guess was right
            const uint32_t kx = s_kext[kid];
            const uint32_t len = (kx >> 16) & 0xffu, side = kx >> 29;
            // only where the predicate will ask: a paired unit whose partner takes the 16-byte core, not the byte loops
            // (n == 31 without PREFIX), nor the unit's own window (len == 0), nor the zero-filled front of the text (o < 20)
            const bool ask = side != 0u && (PREFIX || ((kx >> 24) & 31u) != 31u) && (side == 1u ? len != 0u : o >= 20);
            // (elsewhere an address beyond the buffer: the bounds check answers zeros without a trip to memory, and a load
            // under a branch of its own would keep its six registers apart -- 20 bytes of scratch in the list-driven kernel)
            const uint32_t pa = ask ? (side == 1u ? (uint32_t)o + len : (uint32_t)o - 20u) & ~3u : 0xffffff00u;
            ApmWin wp;
            load_global(pa, wp);
            return stage1(kid, (uint32_t)o, w2, [&](uint32_t a0, ApmWin &o2) {
                if (a0 == pa) o2 = wp;
                else load_global(a0, o2);
            });
        }
        return stage1(kid, (uint32_t)o, w2, [&](uint32_t a0, ApmWin &o2) { load_global(a0, o2); });
    }

    // WIDE: every (match, earlier nominator) pair of the round is an item with a lane of its own, 64 items per pass --
    // the text fetches of all the round's matches are in flight side by side, where the other form makes two dependent
    // trips to memory per match, one match after the other (a burst of matches in one wave then decides when the
    // launch ends).  Items are numbered match by match in lane order; a lane finds the match of its item by a walk over
    // the round's matches (scalar: a readlane and a running sum each), takes the match's window from its lane, and a
    // true nominator marks the match in a wave-uniform mask.  Matches left unmarked count, each from its own lane.
    // The same predicate over the same pairs in either form: the same windows count.
    template <bool WIDE, bool PREF>
    __device__ __forceinline__ void count_matches(bool hit, uint32_t wpat, uint32_t wj, uint32_t word) const {
        for (unsigned long long m2 = __builtin_amdgcn_ballot_w64(hit); m2; m2 &= m2 - 1ull) {
            const int src = __builtin_ctzll(m2);
            const uint32_t bpat = (uint32_t)__builtin_amdgcn_readlane((int)wpat, src), bj = (uint32_t)__builtin_amdgcn_readlane((int)wj, src);
            const uint32_t bord = (uint32_t)__builtin_amdgcn_readlane((int)word, src);
            if (hit && wpat == bpat && wj == bj && word > bord) hit = false;
        }
        unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);
        if constexpr (WIDE) {
            if (!hm) return; // (wave-uniform)
#ifdef APM_MEASURE
            if (APM_SKIP(a, 32)) return;
#endif
            const unsigned long long pm = __builtin_amdgcn_ballot_w64(hit && word != 0u); // matches with items
            unsigned long long dup = 0ull; // matches with a true earlier nominator
            uint32_t total = 0;
            for (unsigned long long mm = pm; mm; mm &= mm - 1ull) total += (uint32_t)__builtin_amdgcn_readlane((int)word, __builtin_ctzll(mm));
            for (uint32_t base = 0; base < total; base += 64u) {
                const uint32_t t = base + (uint32_t)lane;
                uint32_t msrc = 0, mfirst = 0, run = 0;
                for (unsigned long long mm = pm; mm; mm &= mm - 1ull) { // the last match whose first item is <= t
                    const int src = __builtin_ctzll(mm);
                    if (t >= run) { msrc = (uint32_t)src; mfirst = run; }
                    run += (uint32_t)__builtin_amdgcn_readlane((int)word, src);
                }
                const uint32_t bpat = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(msrc << 2), (int)wpat);
                const uint32_t bj = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(msrc << 2), (int)wj);
                const bool earlier = t < total && nominates<PREF>(bpat, bj, (int)(t - mfirst));
                unsigned long long em = __builtin_amdgcn_ballot_w64(earlier);
                while (em) { // (true nominators are few: a window's intact units)
                    const int l = __builtin_ctzll(em);
                    const uint32_t sl = (uint32_t)__builtin_amdgcn_readlane((int)msrc, l);
                    dup |= 1ull << sl;
                    em &= ~__builtin_amdgcn_ballot_w64(msrc == sl);
                }
            }
            const bool counts = hit && !((dup >> lane) & 1ull);
            if (counts) atomicAdd(&s_cnt[wpat], 1u);
#ifdef APM_REC
            apm_rec_push_wave(a.pos, counts, counts ? a.pats[wpat].index : 0u, (int64_t)wj);
#endif
#ifdef APM_MEASURE
            if (APM_SKIP(a, 256) && counts) atomicAdd(&a.stats[3], 1ull);
#endif
            return;
        }
        while (hm) {
            const int src = __builtin_ctzll(hm);
            hm &= hm - 1ull;
            const uint32_t bpat = (uint32_t)__builtin_amdgcn_readlane((int)wpat, src), bj = (uint32_t)__builtin_amdgcn_readlane((int)wj, src);
            const int n_before = __builtin_amdgcn_readlane((int)word, src); // (unit, shift) pairs in front of this one: < 64
#ifdef APM_MEASURE
            if (APM_SKIP(a, 32)) continue;
#endif
            const bool earlier = lane < n_before && nominates<false>(bpat, bj, lane);
            if (!__builtin_amdgcn_ballot_w64(earlier) && lane == 0) {
                atomicAdd(&s_cnt[bpat], 1u);
#ifdef APM_REC
                apm_rec_push(a.pos, a.pats[bpat].index, (int64_t)bj);
#endif
#ifdef APM_MEASURE
                if (APM_SKIP(a, 256)) atomicAdd(&a.stats[3], 1ull);
#endif
            }
        }
    }

};

__host__ __device__ constexpr int apm_verify_scap(int band) { return ((64 + 2 * band) / (2 * band + 1) + 63 + 7) & ~7; }

// THREADS = 256 or 512: the bigger workgroup shares one LDS image among eight waves -- more waves per CU when the
// image (many keys) limits the workgroups per CU
// SAMPLED: the list comes from the stride-8 sieve (see ApmVerifyArgs::stride)
// FUSED: the hit masks do not come from a sieve launch -- the wave sieves its blocks itself (sv: the sieve's arguments;
// stride 1: its 32 KiB bitmap leads the LDS, the image follows; stride 8: the image's own bitmap is the sieve's) and
// verifies the hits in the same batches of 64 across block borders, the windows gathered from global memory (L2 /
// Infinity Cache: the wave streamed those lines a moment ago).  One launch, the text leaves HBM once, no masks.
// THREADS_T = 0: the workgroup size is the launch's (a multiple of 64).
template <int BAND, int THREADS_T, bool SAMPLED, bool FUSED>
__device__ __forceinline__ void apm_verify_body(const ApmVerifyArgs &a, const ApmSieve2Args *sv, uint8_t *smem) {
    const int THREADS = THREADS_T ? THREADS_T : (int)blockDim.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int NSH = 2 * BAND + 1;
    constexpr uint32_t FLUSH_AT = (64 + NSH - 1) / NSH; // survivors that fill a wave of (survivor, shift) items (capacity of the list: apm_verify_scap)
    (void)FLUSH_AT;
    constexpr int SCAP = apm_verify_scap(BAND);         // capacity of a wave's survivor list: FLUSH_AT - 1 + one round of 64
    uint8_t *s_img = smem + ((FUSED && !SAMPLED) ? 32768 : 0);
    const uint32_t *s_bmp = reinterpret_cast<const uint32_t *>(s_img);
    const uint16_t *s_prefix = reinterpret_cast<const uint16_t *>(s_img + a.o_prefix);
    const uint16_t *s_r2s = reinterpret_cast<const uint16_t *>(s_img + a.o_r2s);
    const uint16_t *s_slots = reinterpret_cast<const uint16_t *>(s_img + a.o_slots);
    const ApmKeyList keys{s_bmp, s_prefix, s_r2s, s_slots};
    const uint32_t *s_kext = reinterpret_cast<const uint32_t *>(s_img + a.o_kext);
    const uint8_t *s_pat = s_img + a.o_pat;
    const uint4 *s_masks = reinterpret_cast<const uint4 *>(s_img + a.o_masks);
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_img + a.image_len);
    uint2 *s_surv = reinterpret_cast<uint2 *>(s_cnt + ((a.n_pats + 3) & ~3)) + wv * SCAP; // this wave's survivors {position, kid}
    uint32_t *s_q = reinterpret_cast<uint32_t *>(reinterpret_cast<uint2 *>(s_cnt + ((a.n_pats + 3) & ~3)) + (THREADS / 64) * SCAP) + wv * 128; // this wave's hit queue

    // the counters a wave starts from -- the length of the block list, of its region of the candidate list -- depend on nothing
    // in LDS: their trip to memory goes out in front of the image's and overlaps it
    const uint32_t my_wave = blockIdx.x * (uint32_t)(THREADS / 64) + (uint32_t)wv;
    const uint32_t n_listed = (!FUSED && a.blist != nullptr) ? *a.blist_ctr : 0xffffffffu;
    // CANDIDATE LIST (ApmVerifyArgs::clist) in front of the rows: region g's batches of 64 entries are dealt statically to the
    // waves g, g + R, g + 2R, ... (R regions; fewer waves than regions: wave w takes regions w, w + W, ... whole) -- the
    // regions of a sieve launch fill evenly (its workgroups walk the text interleaved), so there is nothing to balance
    // A short region is cut into as many batches as it has waves (cfg5: 40 entries for 16 waves): one wave working a
    // dense batch alone walks the longest key list among 64 lanes, a chain of dependent gathers, while the others idle.
    bool cl_on = false;                                  // wave-uniform, like the rest
    uint32_t cl_r = 0, cl_rstep = 0, cl_b = 0, cl_bstep = 1, cl_n = 0, cl_bs = 64;
    if constexpr (!FUSED && !SAMPLED) {
        if (a.clist) {
            const uint32_t R = (uint32_t)a.clist_regions, Wv = (uint32_t)gridDim.x * (uint32_t)(THREADS / 64);
            if (Wv >= R) {
                const uint32_t wpr = Wv / R;
                cl_on = my_wave < wpr * R;
                cl_r = my_wave % R;
                cl_rstep = R; // (one region only)
                cl_b = my_wave / R;
                cl_bstep = wpr;
            } else {
                cl_on = my_wave < R;
                cl_r = my_wave;
                cl_rstep = Wv;
            }
            if (cl_on) {
                cl_n = a.clist_cnt[cl_r];
                if (Wv >= R) {
                    const uint32_t per_wave = (cl_n + cl_bstep - 1u) / cl_bstep;
                    const uint32_t lo = (uint32_t)a.clist_min_batch;
                    cl_bs = per_wave >= 64u ? 64u : (per_wave < lo ? lo : per_wave);
                }
            }
        }
    }
    if constexpr (FUSED && !SAMPLED)
        apm_stage_image(reinterpret_cast<uint4 *>(smem), sv->bitmap, 2048, tid, THREADS);
    apm_stage_image(reinterpret_cast<uint4 *>(s_img), a.image, a.image_len >> 4, tid, THREADS);
    for (int i = tid; i < a.n_pats; i += THREADS) s_cnt[i] = 0u;
    __syncthreads(); // the only workgroup barrier before the final count flush

    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.text), 0, (int)(uint32_t)a.avail_pad, 0x00020000);
    const uint32_t avail = (uint32_t)a.avail;
    const uint32_t cs = (uint32_t)a.code_shift;

    ApmVerifyCore<BAND, !SAMPLED> core{a, rs, avail, s_kext, s_masks, s_pat, s_cnt, lane, reinterpret_cast<const uint32_t *>(s_img + a.o_kinfo),
                             reinterpret_cast<const uint2 *>(s_img + a.o_pinfo)};
    typedef ApmWin Win;
    auto load_win = [&](uint32_t a0, Win &o) __attribute__((always_inline)) { core.load_global(a0, o); };

    // ---- batches of 64 candidates per wave.  One loop, one stage-1 site, one DP site: each trip either runs the
    // DP pass over the wave's survivor list, or moves to the next (batch, parity), or evaluates the predicate once
    // for every lane that still has a key to try at its position. ----
    uint32_t n_surv = 0; // wave-uniform
    uint32_t item_lo = 0; // wave-uniform: shifts of the list's first survivor that an earlier DP pass has taken already
    // the sieve's 4 KiB blocks are dealt to the waves in equal contiguous runs; a wave compacts the hit masks of its
    // blocks (one dword per lane and block) into a queue of positions and takes 64 of them per batch -- dense lanes
    // across block borders, since the text comes from global memory anyway
    constexpr uint32_t STEP = SAMPLED ? 8u : 2u; // bytes between two lookups of the sieve
    // ---- which blocks a wave works on: DYNAMIC.  Equal static runs left the waves finishing anywhere between 0.45 and
    // 1.0 of the kernel's duration (per-wave time stamps, measurement build).  The blocks form chunks of CH; the chunks
    // are split into APM_WORK_GROUPS contiguous ranges, each with its own counter (a single one would serialise: ~90
    // atomics per microsecond chip-wide); wave w belongs to group w % APM_WORK_GROUPS -- every group is a sample of the
    // whole machine, so the groups finish together -- and takes the group's next chunk with one atomic, issued a
    // chunk ahead of its use.  The counters of the NEXT launch are zeroed here (two sets, the host alternates). ----
    // 4 KiB blocks in all; with a block list (ApmVerifyArgs::blist) only the listed ones: entry b of the list is the block
    // -- when the list is short: with most blocks on it (cfg3) the walk over all rows is the shorter chain of loads
    const bool listed = n_listed < (uint32_t)a.n_mask_blocks / 4u || (!FUSED && a.clist != nullptr); // (with a candidate list only the listed blocks have rows at all)
    const uint32_t NB = FUSED ? (uint32_t)((sv->nchunks + 3) >> 2) : (listed ? n_listed : (uint32_t)a.n_mask_blocks);
    // blocks per chunk: a short list is dealt block by block (cfg5: 10 K listed blocks for 4 K waves -- with chunks of 8 most
    // waves got none and the rest walked theirs one load after the other: 0.072 ms against 0.036)
    // (and a short text in chunks small enough that every wave gets a few: 64 MiB in chunks of 8 left two waves of three idle)
    const uint32_t n_waves_launch = (uint32_t)(FUSED ? sv->n_main_blocks : (int)gridDim.x) * (uint32_t)(THREADS / 64);
    const uint32_t ch_fit = NB / (4u * n_waves_launch);
    const uint32_t CH = SAMPLED ? APM_WORK_CH8 : (listed ? 1u : (ch_fit >= APM_WORK_CH ? APM_WORK_CH : (ch_fit < 1u ? 1u : ch_fit)));
    const uint32_t NC = (NB + CH - 1u) / CH;
    // NG = min(APM_WORK_GROUPS, waves of the launch): no group without a wave.  Workgroups go round the XCDs, so the low
    // bits of the wave number alone would tie a group to one XCD and one wave slot: fold the higher bits in
    const uint32_t NG = (uint32_t)a.work_groups, grp = (my_wave ^ (my_wave >> 5)) % NG;
    const uint32_t f_g = (uint32_t)(((uint64_t)NC * grp) / NG), n_g = (uint32_t)(((uint64_t)NC * (grp + 1u)) / NG) - f_g;
    uint32_t *const ctr = a.work + ((uint32_t)a.work_epoch & 1u) * (APM_WORK_GROUPS * APM_WORK_STRIDE) + grp * APM_WORK_STRIDE;
    if (blockIdx.x == 0 && tid < APM_WORK_GROUPS) a.work[(((uint32_t)a.work_epoch + 1u) & 1u) * (APM_WORK_GROUPS * APM_WORK_STRIDE) + (uint32_t)tid * APM_WORK_STRIDE] = 0u;
    auto grab = [&]() __attribute__((always_inline)) -> uint32_t { // (lane 0 holds the answer; read with readfirstlane when it is needed)
        return lane == 0 ? __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    };
    uint32_t grab_v = grab();
    uint32_t it_b = 0, it_end = 0; // the chunk in hand: blocks [it_b, it_end)
    bool it_done = false;
    // fused sampled form: blocks dealt statically, wave w takes blocks w, w + W, ... -- with the register compare in front next
    // to nothing is left to verify, so there is nothing to balance, and the waves of a round read one contiguous stretch of
    // text (the plain sieve's access shape)
    constexpr bool STATIC_BLOCKS = FUSED && SAMPLED;
    const uint32_t n_waves_all = (uint32_t)(FUSED ? sv->n_main_blocks : (int)gridDim.x) * (uint32_t)(THREADS / 64); // (the scanning workgroups: not the tail ones)
    uint32_t st_b = my_wave;
    auto it_next = [&](uint32_t &b) __attribute__((always_inline)) -> bool { // wave-uniform: the wave's next block
        if constexpr (STATIC_BLOCKS) {
            if (st_b >= NB) return false;
            b = st_b;
            st_b += n_waves_all;
            return true;
        }
        if (it_b >= it_end) {
            if (it_done) return false;
            const uint32_t i = (uint32_t)__builtin_amdgcn_readfirstlane((int)grab_v);
            if (i >= n_g) { it_done = true; return false; } // every wave gets here: its group's range is exhausted
            it_b = (f_g + i) * CH;
            it_end = it_b + CH < NB ? it_b + CH : NB;
            grab_v = grab();
        }
        b = it_b++;
        return true;
    };
    // masks of the block in hand and of the AHEAD blocks after it (sparse sampled lists are bound by this chain of loads)
    constexpr int AHEAD = FUSED ? 1 : (SAMPLED ? 4 : APM_VERIFY_AHEAD);
    constexpr uint32_t NONE = 0xffffffffu;
    uint32_t hm = 0, hm_q[AHEAD], hb_q[AHEAD]; // hb_q: their block numbers (wave-uniform)
    if constexpr (!FUSED) {
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) {
            uint32_t b = NONE;
            hb_q[i] = it_next(b) ? (listed ? a.blist[b] : b) : NONE;
            hm_q[i] = hb_q[i] != NONE ? a.masks[(uint64_t)hb_q[i] * 64 + (uint64_t)lane] : 0u;
        }
    }
#ifdef APM_MEASURE
    if (APM_SKIP(a, 512) && lane == 0 && my_wave < APM_STATS_WAVES) a.stats[8 + 2 * my_wave] = wall_clock64();
#endif
    uint32_t blk = 0;    // relative position of the block in hand
    uint32_t qcount = 0; // wave-uniform
    const uint32_t nch32 = FUSED ? (uint32_t)sv->nchunks : 0u;
    const uint32_t tile0 = FUSED ? (uint32_t)sv->tile0 : 0u;
    // hit mask of this lane for the block at relative position b0 (see ApmSieve2Args::masks for the bit layout)
    // FUSED + SAMPLED: one block per sieve step, the next block's text prefetched (a block fills 8 of the 32 mask bits: bits
    // 8 j + t); the pass is bound by the latency of these loads
    constexpr bool PREF = FUSED && SAMPLED;
    u32x4 pf_r[4];      // PREF: the prefetched block's text
    uint32_t pf_sl[4];  // ... the codes of the block in hand (packed before the next block's loads go out: no second copy of the text)
    uint32_t pf_b = 0xffffffffu; // the prefetched block (none)
    bool pf_started = false;
    auto pf_issue = [&](uint32_t b) __attribute__((always_inline)) {
        const uint32_t g = tile0 + b * 4096u + 16u * (uint32_t)lane;
#pragma unroll
        for (int j = 0; j < 4; ++j) pf_r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(g + 1024u * j), 0, 0); // (beyond the text: zeros)
    };
    auto sieve_block = [&](uint32_t b0, uint32_t fb) __attribute__((always_inline)) -> uint32_t {
        const uint32_t g = b0 + 16u * (uint32_t)lane, c0 = fb * 4u;
        uint32_t out = 0;
        if constexpr (SAMPLED) { // one lookup per 8 bytes in the image's bitmap over 16-bit code words (apm_sieve8_kernel)
            uint32_t sl[4]; // codes of the lane's 16 bytes, chunk by chunk (packed when the block was taken up: next_cand)
#pragma unroll
            for (int j = 0; j < 4; ++j) sl[j] = pf_sl[j];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t slo = sl[j];
                const uint32_t w0 = s_bmp[slo & 2047u], w1 = s_bmp[(slo >> 16) & 2047u];
                const uint32_t h = ((w0 >> ((slo >> 11) & 31u)) & 1u) | (((w1 >> (slo >> 27)) & 1u) << 1);
                out |= (c0 + j < nch32 ? h : 0u) << (8 * j);
            }
            // REGISTER COMPARE: a hit says "an 8-byte block of some key's piece, r bytes into the piece, may lie here"; the
            // piece is >= 15 bytes long, so more of it lies inside the lane's own 16 bytes -- compare the codes of that overlap
            // (pattern bytes out of the LDS image, packed like the text) before the hit is queued.  What was queued before
            // -- 0.8 M hits per GiB for cfg4, practically all false, each with two window gathers that missed the caches
            // (1.18 x the text in HBM traffic) -- no longer leaves the lane.  A filter (codes equal is necessary for the
            // piece to be intact at position - r, stage1's first test); lanes work on their own hits, one key at a time.
            {
                uint32_t pend = out, cur = 0, curbit = 0, slo_c = 0, tsel = 0;
                bool act = false;
                for (;;) {
                    if (!act && pend) { // the lane's next hit: key list of its code word by rank
                        curbit = (uint32_t)__builtin_ctz(pend);
                        pend &= pend - 1u;
                        tsel = curbit & 1u;
                        const uint32_t j = curbit >> 3;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (j == (uint32_t)q) slo_c = sl[q];
                        cur = keys.first(tsel ? (slo_c >> 16) : (slo_c & 0xffffu));
                        act = true;
                    }
                    if (!__builtin_amdgcn_ballot_w64(act)) break;
                    if (act && a.o_rc) { // (wave-uniform choice: small sets carry the compare's operands ready made)
                        const uint32_t kid = ApmKeyList::kid(cur, 11u), rr = ApmKeyList::r(cur, 11u);
                        const uint2 rc = reinterpret_cast<const uint2 *>(s_img + a.o_rc)[(kid * 8u + rr) * 2u + tsel];
                        if (((rc.x ^ slo_c) & rc.y) == 0u) act = false; // may be intact: the hit stays
                        else if (ApmKeyList::last(cur)) { act = false; out &= ~(1u << curbit); } // no key of the word fits
                        else cur = keys.next(cur);
                    } else if (act) {
                        const uint32_t kid = ApmKeyList::kid(cur, 11u), rr = ApmKeyList::r(cur, 11u); // (sampled: KBITS = 11)
                        const uint32_t kx = s_kext[kid];
                        const int at = (int)(kx & 0xffffu), len = (int)((kx >> 16) & 0xffu);
                        // lane byte i <-> piece byte i - 8 t + r <-> pattern pool byte at + r - 8 t + i
                        const int sh8 = (int)(8u * tsel) - (int)rr;
                        uint32_t B[4];
                        apm_lds_dwords<4>(s_pat, at - sh8, B);
                        const uint32_t pc = apm_pack4(B[0], cs) | (apm_pack4(B[1], cs) << 8) | (apm_pack4(B[2], cs) << 16) | (apm_pack4(B[3], cs) << 24);
                        const int i0 = sh8 > 0 ? sh8 : 0, i1 = len + sh8 < 16 ? len + sh8 : 16; // the piece covers lane bytes [i0, i1)
                        const uint32_t mhi = i1 >= 16 ? 0xffffffffu : ((1u << (2 * i1)) - 1u), mlo = (1u << (2 * i0)) - 1u;
                        if ((((pc ^ slo_c) & mhi) & ~mlo) == 0u) act = false; // may be intact: the hit stays
                        else if (ApmKeyList::last(cur)) { act = false; out &= ~(1u << curbit); } // no key of the word fits
                        else cur = keys.next(cur);
                    }
                }
            }
        } else { // one lookup per even position in the 32 KiB bitmap over 18-bit code words at LDS address 0 (apm_sieve2_kernel)
            // (chunks behind the scanned range are loaded all the same -- text or zeros -- since the windows of the last
            // valid chunk run into them; only their own hits are dropped)
            u32x4 r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(g + 1024u * j), 0, 0);
            const v2u32 tl = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(b0 + 4096u), 0, 0); // the 8 bytes behind the block
            uint32_t slo[5]; // codes of the lane's 16 bytes, chunk by chunk; [4]: of the 8 bytes behind the block
#pragma unroll
            for (int j = 0; j < 4; ++j) slo[j] = apm_pack16(r[j].x, r[j].y, r[j].z, r[j].w, cs);
            slo[4] = apm_pack4(tl.x, cs) | (apm_pack4(tl.y, cs) << 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // (nx0 of lane 63: the low half of the next chunk's lane 0)
                const uint32_t hits = apm_lookup2_chunk(slo[j], (uint32_t)__builtin_amdgcn_readfirstlane((int)slo[j + 1]));
                out |= (c0 + j < nch32 ? hits >> 24 : 0u) << (8 * j);
                __builtin_amdgcn_sched_barrier(0); // chunk by chunk: the window state of the batches in flight is live here
            }
        }
        return out;
    };
    // the next batch: up to 64 positions (in units of STEP bytes); false once the wave's run is exhausted
    auto next_cand = [&](uint32_t &q, bool &hv) __attribute__((always_inline)) -> bool {
        if constexpr (!FUSED && !SAMPLED) {
            while (cl_on) {
                const uint32_t o = cl_b * cl_bs;
                if (o < cl_n) {
                    const uint32_t nb = cl_n - o < cl_bs ? cl_n - o : cl_bs;
                    hv = (uint32_t)lane < nb;
                    q = hv ? a.clist[(size_t)cl_r * a.clist_cap + o + (uint32_t)lane] : 0u;
                    cl_b += cl_bstep;
                    return true;
                }
                cl_r += cl_rstep;
                cl_b = 0; // (whole regions from here on: cl_bs is 64)
                if (cl_r >= (uint32_t)a.clist_regions) { cl_on = false; break; }
                cl_n = a.clist_cnt[cl_r];
            }
        }
        while (qcount < 64u) {
            if (!__builtin_amdgcn_ballot_w64(hm != 0u)) { // block done: take the prefetched masks of the next one
                if constexpr (FUSED) { // ... or sieve the wave's next block
                    uint32_t b;
                    if constexpr (PREF) {
                        if (!pf_started) {
                            pf_started = true;
                            uint32_t nb;
                            if (it_next(nb)) { pf_b = nb; pf_issue(nb); }
                        }
                        if (pf_b == 0xffffffffu) break;
                        b = pf_b;
#pragma unroll
                        for (int j = 0; j < 4; ++j) pf_sl[j] = apm_pack16(pf_r[j].x, pf_r[j].y, pf_r[j].z, pf_r[j].w, cs);
                        uint32_t nb;
                        if (it_next(nb)) { pf_b = nb; pf_issue(nb); }
                        else pf_b = 0xffffffffu;
                    } else if (!it_next(b)) break;
                    blk = tile0 + b * 4096u;
                    hm = sieve_block(blk, b);
                    continue;
                }
                if (hb_q[0] == NONE) break;
                blk = (uint32_t)(a.tile0 + (int64_t)hb_q[0] * 4096);
                hm = hm_q[0];
#pragma unroll
                for (int i = 0; i + 1 < AHEAD; ++i) { hm_q[i] = hm_q[i + 1]; hb_q[i] = hb_q[i + 1]; }
                {
                    uint32_t b = NONE;
                    hb_q[AHEAD - 1] = it_next(b) ? (listed ? a.blist[b] : b) : NONE;
                    hm_q[AHEAD - 1] = hb_q[AHEAD - 1] != NONE ? a.masks[(uint64_t)hb_q[AHEAD - 1] * 64 + (uint64_t)lane] : 0u;
                }
                continue;
            }
            const bool has = hm != 0u;
            const uint32_t t = has ? (uint32_t)__builtin_ctz(hm) : 0u;
            hm &= hm - 1u;
            apm_wave_append(s_q, qcount, has, (blk + (t >> 3) * 1024u + 16u * (uint32_t)lane + (SAMPLED ? (t & 1u) * 8u : (t & 7u) * 2u)) / STEP);
        }
        q = 0;
        hv = false;
        if (qcount == 0u) return false;
        const uint32_t nb = qcount < 64u ? qcount : 64u;
        hv = (uint32_t)lane < nb;
        if (hv) q = s_q[lane];
        if (qcount > 64u) { // keep the rest for the next batch
            const uint32_t rest = s_q[64 + lane];
            if ((uint32_t)lane < qcount - 64u) s_q[lane] = rest;
        }
        qcount -= nb;
        return true;
    };
    // one batch ahead: the positions of batch b+1 are formed (a matter of registers and LDS) and its text windows are in
    // flight while batch b is worked on (vmcnt counts in order: the loads of the pre-check queue behind them and wait
    // for no more)
    bool done = false, active = false, have = false;
    uint32_t p = 0, str = 0, s = 0, pend = 0;
    uint32_t cur = 0; // the key in hand and the rest of its list (ApmKeyList)
    Win win, win_n, wk; // text at the candidate position (this / the next batch); SAMPLED: at the piece the key in hand implies
    constexpr uint32_t PSH = SAMPLED ? 3u : 1u;    // queue entry -> relative position
    constexpr uint32_t KBITS = SAMPLED ? 11u : 15u; // key id bits of a key-list payload; above them the block's offset in its piece
    uint32_t q_n = 0;
    bool have_n = false;
    bool ex_n = true; // (an empty batch starts the pipeline through the loop's own rotate step)
    constexpr int PIPE = FUSED ? APM_FUSED_PIPE : APM_VERIFY_PIPE;
    uint32_t q_nn = 0; // (PIPE == 2)
    bool have_nn = false, ex_nn = true;
    load_win(0u, win_n);
    for (;;) {
        // the DP pass takes FULL waves of (survivor, shift) items only -- what is left over (fewer than 64 items, possibly
        // part of a survivor's shifts: item_lo) waits at the front of the list for the next pass; everything at the end
        if (n_surv * NSH - item_lo >= 64u || (done && n_surv)) {
            const uint32_t avail_items = n_surv * NSH - item_lo, proc = done ? avail_items : (avail_items & ~63u);
            for (uint32_t w0 = 0; w0 < proc; w0 += 64) { // one (survivor, shift) per lane
                const uint32_t wi = item_lo + w0 + (uint32_t)lane;
                const bool live = w0 + (uint32_t)lane < proc;
                const uint2 e = live ? s_surv[wi / NSH] : make_uint2(0u, 0u);
                const int dl = (int)(wi % NSH) - BAND;
                uint32_t wpat = 0, wj = 0, word = 0;
                bool hit = live && core.dp_match(e.y, e.x, dl, wpat, wj, word);
#ifdef APM_MEASURE
                if (APM_SKIP(a, 64)) hit = false;
#endif
                core.template count_matches<APM_DEDUP_WIDE(BAND, SAMPLED, FUSED), APM_DEDUP_PREFETCH(BAND, SAMPLED, FUSED)>(hit, wpat, wj, word);
            }
            const uint32_t s_first = (item_lo + proc) / NSH, left = n_surv - s_first; // (left <= 22 survivors)
            const uint2 keep = (uint32_t)lane < left ? s_surv[s_first + (uint32_t)lane] : make_uint2(0u, 0u);
            if ((uint32_t)lane < left) s_surv[lane] = keep;
            item_lo = item_lo + proc - s_first * NSH;
            n_surv = left;
        }
        if (done) break;
        // a lane without a key in hand takes up the next of its (at most two) hit positions: key list by rank
        if (!active && pend) {
            const uint32_t par = (pend & 1u) ? 0u : 1u;
            pend &= pend - 1u;
            cur = keys.first((str >> (2u * par)) & 0xffffu);
            s = p + par;
            active = true;
            if constexpr (SAMPLED) { // the block at p lies r bytes inside its piece: the unit's position is p - r
                s = p - ApmKeyList::r(cur, KBITS);
                if (s > p) s = 0xffffffffu; // (in front of the shard: the pre-check's position test rejects it)
                load_win(s & ~3u, wk);
            }
        }
        if (!__builtin_amdgcn_ballot_w64(active)) { // this batch is exhausted: rotate the pipeline
            if (!ex_n) { done = true; continue; }
            p = q_n << PSH; // relative position (even / a multiple of 8)
            have = have_n;
            win = win_n;
            if constexpr (PIPE == 2) {
                ex_n = ex_nn;
                q_n = q_nn;
                have_n = have_nn;
                load_win((q_n << PSH) & ~3u, win_n);
                ex_nn = next_cand(q_nn, have_nn);
            } else {
                ex_n = next_cand(q_n, have_n);
                load_win((q_n << PSH) & ~3u, win_n);
            }
            // code words of the 8-byte windows at p and p + 1 (16 bits each) out of the 12 bytes from p on
            str = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t b4 = __builtin_amdgcn_alignbyte(win.w[i + 1], win.w[i], p & 3u);
                str |= apm_pack4(b4, cs) << (8 * i);
            }
            const uint32_t x0 = str & 0xffffu, x1 = (str >> 2) & 0xffffu;
            pend = have ? (((s_bmp[x0 & 2047u] >> (x0 >> 11)) & 1u) | (SAMPLED ? 0u : (((s_bmp[x1 & 2047u] >> (x1 >> 11)) & 1u) << 1))) : 0u;
#ifdef APM_MEASURE
            if (APM_SKIP(a, 8)) pend = 0;
#endif
            continue;
        }
        bool ok = false;
        if (active) ok = core.stage1(ApmKeyList::kid(cur, KBITS), s, SAMPLED ? wk : win, load_win);
#ifdef APM_MEASURE
        if (APM_SKIP(a, 16)) ok = false;
#endif
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(ok);
#ifdef APM_MEASURE
        if (APM_SKIP(a, 256) && mask && lane == 0) atomicAdd(&a.stats[1], (unsigned long long)__builtin_popcountll(mask));
#endif
        if (mask) { // survivors -> the wave's list (ballot + mbcnt, no atomics); at most FLUSH_AT - 1 + 64 entries
            const uint32_t idx = n_surv + apm_wave_rank(mask);
            if (ok) s_surv[idx] = make_uint2(s, ApmKeyList::kid(cur, KBITS));
            n_surv += (uint32_t)__builtin_popcountll(mask);
        }
        if (active) {
            if (ApmKeyList::last(cur)) active = false;
            else {
                cur = keys.next(cur);
                if constexpr (SAMPLED) {
                    s = p - ApmKeyList::r(cur, KBITS);
                    if (s > p) s = 0xffffffffu; // (in front of the shard: the pre-check's position test rejects it)
                    load_win(s & ~3u, wk);
                }
            }
        }
    }

#ifdef APM_MEASURE
    if (APM_SKIP(a, 512) && lane == 0 && my_wave < APM_STATS_WAVES) a.stats[9 + 2 * my_wave] = wall_clock64();
#endif
    __syncthreads();
    for (int i = tid; i < a.n_pats; i += THREADS) {
        const uint32_t cnt = s_cnt[i];
        if (cnt) atomicAdd(&a.counts[a.pats[i].index], (unsigned long long)cnt);
    }
}

template <int BAND, int THREADS, bool SAMPLED>
__global__ __launch_bounds__(THREADS, (BAND == 1 && THREADS == 256 && !SAMPLED) ? 6 : 4) void apm_verify_kernel(ApmVerifyArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    apm_verify_body<BAND, THREADS, SAMPLED, false>(a, nullptr, smem);
}

static size_t apm_verify_lds_bytes_t(const ApmVerifyArgs &a, int threads) {
    return (size_t)a.image_len + (size_t)((a.n_pats + 3) & ~3) * 4 + (size_t)(threads / 64) * ((size_t)apm_verify_scap(a.band) * 8 + 128 * 4) +
           16; // image + counts + one survivor list and one hit queue per wave
}

// ONE band switch for both kernel families: a family answers fn<BAND>() with its kernel for the band
template <typename Family>
static const void *apm_band_fn(int band, const Family &k) {
    switch (band) {
    case 0: return k.template fn<0>();
    case 1: return k.template fn<1>();
    case 2: return k.template fn<2>();
    case 3: return k.template fn<3>();
    default: return nullptr;
    }
}
struct ApmVerifyFamily {
    int threads, stride;
    template <int BAND>
    const void *fn() const {
        if (threads == 512) return stride == 8 ? (const void *)apm_verify_kernel<BAND, 512, true> : (const void *)apm_verify_kernel<BAND, 512, false>;
        return stride == 8 ? (const void *)apm_verify_kernel<BAND, 256, true> : (const void *)apm_verify_kernel<BAND, 256, false>;
    }
};
static const void *apm_verify_fn(int band, int threads, int stride) { return apm_band_fn(band, ApmVerifyFamily{threads, stride}); }

// workgroup size (256 or 512 threads) and workgroups per CU that put the most waves on a CU for this LDS image
int apm_verify_geometry(const ApmVerifyArgs &a, int *threads) {
    const int blocks = apm_best_geometry([&](int t) { return apm_verify_fn(a.band, t, a.stride); }, 256, 512, 256,
                                         [&](int t) { return apm_verify_lds_bytes_t(a, t); }, 8, 0, threads);
    if (blocks) return blocks;
    *threads = 256;
    return 2;
}

hipError_t apm_launch_verify(const ApmVerifyArgs &a, int threads, int max_blocks, int *work_epoch, hipStream_t s) {
    if (a.n_pats <= 0) return hipSuccess;
    const void *fn = apm_verify_fn(a.band, threads, a.stride);
    if (!fn) return hipErrorInvalidValue;
    ApmVerifyArgs args = a;
    args.n_blocks = max_blocks < 1 ? 1 : max_blocks; // (number of hits unknown on the host: a persistent grid shares the blocks)
#ifdef APM_MEASURE
    if (const char *e = getenv("APM_VERIFY_GRID_PCT")) args.n_blocks = std::max(1, (int)((long)args.n_blocks * atoi(e) / 100)); // occupancy sensitivity
    if (const char *e = getenv("APM_MEASURE_SKIP")) args.skip_mask = atoi(e);
#endif
    args.work_groups = std::min<long>(APM_WORK_GROUPS, (long)args.n_blocks * (threads / 64));
    args.work_epoch = *work_epoch;
    void *kargs[] = {&args};
    const hipError_t e = hipLaunchKernel(fn, dim3((unsigned)args.n_blocks), dim3((unsigned)threads), kargs, apm_verify_lds_bytes_t(a, threads), s);
    if (e == hipSuccess) ++*work_epoch; // only a launch that runs advances it: launch e zeroes the counter set launch e + 1 uses
    return e;
}

// ---------------------------------------------------------------------------
// FUSED: sieve + verify in one launch (apm_verify_body<.., FUSED = true>; see ApmFusedArgs)
// ---------------------------------------------------------------------------
template <int BAND, bool SAMPLED>
__global__ __launch_bounds__(APM_FUSED_MAX_THREADS, SAMPLED ? (BAND == 0 ? 7 : (BAND == 1 ? APM_FUSED_S_WAVES : 5)) : (BAND == 0 ? 6 : 5)) void apm_fused_kernel(ApmFusedArgs f) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if ((int)blockIdx.x >= f.s.n_main_blocks) { // extra workgroups: truncated tail windows (one pattern each)
        apm_tail_body(f.s.tail, (int)blockIdx.x - f.s.n_main_blocks, reinterpret_cast<uint4 *>(smem), (int)threadIdx.x);
        return;
    }
    apm_verify_body<BAND, 0, SAMPLED, true>(f.v, &f.s, smem);
}

struct ApmFusedFamily {
    int stride;
    template <int BAND>
    const void *fn() const { return stride == 8 ? (const void *)apm_fused_kernel<BAND, true> : (const void *)apm_fused_kernel<BAND, false>; }
};
static const void *apm_fused_fn(int band, int stride) { return apm_band_fn(band, ApmFusedFamily{stride}); }

size_t apm_fused_lds_bytes(const ApmFusedArgs &a, int threads) {
    const size_t need = (a.s.stride == 8 ? 0 : 32768) + apm_verify_lds_bytes_t(a.v, threads);
    return need < 4096 + 256 ? 4096 + 256 : need; // (the tail workgroups' tables)
}

// workgroup size (a multiple of 64, <= APM_FUSED_MAX_THREADS) and workgroups per CU that put the most waves on a CU
int apm_fused_geometry(const ApmFusedArgs &a, int *threads) {
    const void *fn = apm_fused_fn(a.v.band, a.s.stride);
    *threads = 0;
    if (!fn) return 0;
    apm_ensure_max_lds(fn);
#ifdef APM_MEASURE
    static const int forced = getenv("APM_FUSED_THREADS") ? atoi(getenv("APM_FUSED_THREADS")) : 0;
#else
    constexpr int forced = 0;
#endif
    return apm_best_geometry([&](int) { return fn; }, APM_FUSED_MAX_THREADS, 256, -64, [&](int t) { return apm_fused_lds_bytes(a, t); }, INT_MAX, forced, threads);
}

hipError_t apm_launch_fused(const ApmFusedArgs &a, int threads, int max_blocks, int *work_epoch, hipStream_t s) {
    if (a.s.nchunks <= 0 || a.v.n_pats <= 0) return hipSuccess;
    const void *fn = apm_fused_fn(a.v.band, a.s.stride);
    if (!fn || threads < 64 || threads > APM_FUSED_MAX_THREADS || (threads & 63)) return hipErrorInvalidValue;
    const size_t lds = apm_fused_lds_bytes(a, threads);
    const int64_t n_fb = (a.s.nchunks + 3) / 4, want = (n_fb + threads / 64 - 1) / (threads / 64);
    const int64_t nb = want < max_blocks ? want : (max_blocks < 1 ? 1 : max_blocks);
    ApmFusedArgs args = a;
    args.s.n_main_blocks = (int)nb;
    args.v.n_blocks = (int)nb;
#ifdef APM_MEASURE
    if (const char *e = getenv("APM_MEASURE_SKIP")) args.v.skip_mask = atoi(e);
#endif
    if (lds > 48 * 1024) apm_ensure_max_lds(fn); // (per device: the geometry query ran on one)
    args.v.work_groups = (int)std::min<int64_t>(APM_WORK_GROUPS, nb * (threads / 64));
    args.v.work_epoch = *work_epoch;
    void *kargs[] = {&args};
    const hipError_t e = hipLaunchKernel(fn, dim3((unsigned)(nb + a.s.n_tail)), dim3((unsigned)threads), kargs, lds, s);
    if (e == hipSuccess) ++*work_epoch; // (as in apm_launch_verify)
    return e;
}
