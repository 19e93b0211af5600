/*
 * apm_banded_stream.hip -- the STREAM form of the BANDED filter (design: apm_banded.h): kernel, its global-text helpers
 * and its launcher.
 */
#include "apm_internal.h"
#include "apm_core.h"
#include "apm_banded.h"

// ---------------------------------------------------------------------------
// STREAM form of the BANDED filter: every WAVE is autonomous -- no LDS text tile, no workgroup
// barrier in the loop.  A wave walks 1 KiB chunks (16 bytes per lane; chunks c, c+W, c+2W, ... for W
// waves in flight) and keeps four buffer loads per lane in flight.  Sampled classes (STRIDE == KL)
// fingerprint the lane's own 16 bytes; per-position classes (STRIDE == 1) also fetch the 8 bytes
// that follow them.  Fingerprints probe the LDS hash table; the hits go to a wave-private LDS queue
// (ballot + mbcnt, no atomics).  When the queue holds a wave's worth of work it is verified on the
// spot against global memory (the bytes were streamed moments ago: L2 / Infinity Cache hits): key
// compare, pair pre-check (per-position classes), banded DP, stateless dedup.
// Requires a 16-byte aligned text pointer (sampling grid = address grid).
// ---------------------------------------------------------------------------
// N dwords of text starting at relative position off (any alignment), zero beyond [0, limit)
template <int N>
__device__ __forceinline__ void apm_gdwords(const uint8_t *text, int64_t limit, int64_t off, uint32_t (&out)[N]) {
    const int64_t a0 = off & ~(int64_t)3;
    const uint32_t sh = (uint32_t)off & 3u;
    uint32_t w[N + 1];
#pragma unroll
    for (int i = 0; i <= N; ++i) {
        const int64_t q = a0 + 4 * i;
        w[i] = (q >= 0 && q + 4 <= limit) ? *reinterpret_cast<const uint32_t *>(text + q) : 0u;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
}
__device__ __forceinline__ int apm_gbyte(const uint8_t *text, int64_t limit, int64_t off) {
    return (off >= 0 && off < limit) ? (int)text[off] : 0x100;
}
// global-text versions of apm_ext_fwd / apm_ext_bwd (see there)
__device__ __forceinline__ bool apm_ext_fwd_g(const uint8_t *text, int64_t limit, int64_t tp, const uint8_t *pb, int pp, int n) {
    int i = 0;
    while (i < n && apm_gbyte(text, limit, tp + i) == (int)pb[pp + i]) ++i;
    if (i >= n - 1) return true;
    bool ok = true;
    for (int j = i + 1; j < n && ok; ++j) ok = apm_gbyte(text, limit, tp + j) == (int)pb[pp + j];
    if (ok) return true;
    ok = true;
    for (int j = i + 1; j < n && ok; ++j) ok = apm_gbyte(text, limit, tp + j - 1) == (int)pb[pp + j];
    if (ok) return true;
    ok = true;
    for (int j = i; j < n && ok; ++j) ok = apm_gbyte(text, limit, tp + j + 1) == (int)pb[pp + j];
    return ok;
}
__device__ __forceinline__ bool apm_ext_bwd_g(const uint8_t *text, int64_t limit, int64_t te, const uint8_t *pb, int pp, int n) {
    int i = 0;
    while (i < n && apm_gbyte(text, limit, te - 1 - i) == (int)pb[pp + n - 1 - i]) ++i;
    if (i >= n - 1) return true;
    bool ok = true;
    for (int j = i + 1; j < n && ok; ++j) ok = apm_gbyte(text, limit, te - 1 - j) == (int)pb[pp + n - 1 - j];
    if (ok) return true;
    ok = true;
    for (int j = i + 1; j < n && ok; ++j) ok = apm_gbyte(text, limit, te - j) == (int)pb[pp + n - 1 - j];
    if (ok) return true;
    ok = true;
    for (int j = i; j < n && ok; ++j) ok = apm_gbyte(text, limit, te - 2 - j) == (int)pb[pp + n - 1 - j];
    return ok;
}

template <int BAND, int KL, int STRIDE>
__global__ __launch_bounds__(APM_BLOCK, (BAND == 0 && STRIDE > 1) ? 7 : ((BAND >= 1 && STRIDE == 1) ? 3 : ((BAND >= 2 || STRIDE == 1) ? 4 : 5)))
void apm_stream_kernel(ApmFilterArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6); // provably wave-uniform: descriptors stay in SGPRs
    if ((int)blockIdx.x >= a.n_main_blocks) { // extra workgroups: truncated tail windows (one pattern each)
        apm_tail_body(a.tail, (int)blockIdx.x - a.n_main_blocks, reinterpret_cast<uint4 *>(smem), tid);
        return;
    }
    constexpr int NSH = 2 * BAND + 1;
    constexpr bool PAIRS = (STRIDE == 1) && (BAND >= 1);
    constexpr int GRP = 4;                        // probes between two flush checks
    constexpr int QW = 64 * GRP + 64;             // wave queue entries: flushed as soon as it holds >= 64
    uint8_t *s_img = smem;
    uint8_t *s_pat = s_img + a.o_pat;
    const uint4 *s_tab = reinterpret_cast<const uint4 *>(s_img + a.o_tab);
    const uint4 *s_kid = reinterpret_cast<const uint4 *>(s_img + a.o_kid);
    const uint32_t *s_ovf = reinterpret_cast<const uint32_t *>(s_img + a.o_ovf);
    const uint32_t *s_kinfo = reinterpret_cast<const uint32_t *>(s_img + a.o_kinfo);
    const uint2 *s_pinfo = reinterpret_cast<const uint2 *>(s_img + a.o_pinfo);
    const uint16_t *s_next = reinterpret_cast<const uint16_t *>(s_img + a.o_next);
    const uint16_t *s_poff = reinterpret_cast<const uint16_t *>(s_img + a.o_poff);
    uint2 *s_queue = reinterpret_cast<uint2 *>(s_img + a.image_len) + wv * QW; // this wave's queue
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_img + a.image_len + 4 * QW * 8);

    apm_stage_image(reinterpret_cast<uint4 *>(s_img), a.image, a.image_len >> 4, tid, APM_BLOCK);
    for (int i = tid; i < a.n_pats; i += APM_BLOCK) s_cnt[i] = 0u;
    __syncthreads(); // the only workgroup barrier before the final count flush

    const uint32_t hshift = 32u - (uint32_t)a.lg_nb;
    const int64_t W = (int64_t)a.n_main_blocks * (APM_BLOCK / 64);
    const int64_t nch = a.ntiles; // 1 KiB chunks from relative position a.tile0 (multiple of 16)
    const uint8_t *text = a.text;
    const int64_t limit = a.avail_pad;

    auto load_chunk = [&](int64_t cc, u32x4 &r, uint2 &e) __attribute__((always_inline)) {
        const int64_t g = a.tile0 + cc * 1024;
        const int64_t lim = cc < nch ? a.avail_pad - g : 0; // chunks past the end: zero records -> zeros, no traffic
        const uint32_t nrec = lim <= 0 ? 0u : (lim > 1040 ? 1040u : (uint32_t)lim);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.text) + (cc < nch ? g : 0), 0, (int)nrec, 0x00020000);
        r = __builtin_amdgcn_raw_buffer_load_b128(rs, 16 * lane, 0, 0); // (nt / sc0 / sc1 cache-policy bits measured: no gain, nt loses 4 %)
        if constexpr (STRIDE == 1) { // the 8 bytes behind the lane's 16 (next lane's / next chunk's head)
            typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));
            const u32x2v x = __builtin_amdgcn_raw_buffer_load_b64(rs, 16 * lane + 16, 0, 0);
            e = make_uint2(x.x, x.y);
        }
    };

    // text[tpos..+KL) == pattern bytes [ppos..+KL) of the pattern stored at s_pat+poff ?
    auto key_at = [&](int64_t tpos, int poff, int ppos) __attribute__((always_inline)) {
        constexpr int ND = (KL + 3) / 4;
        uint32_t x[ND], y[ND];
        apm_lds_dwords<ND>(s_pat, poff + ppos, y);
        apm_gdwords<ND>(text, limit, tpos, x);
        uint32_t dd = 0;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            uint32_t tt = x[i] ^ y[i];
            if (i == ND - 1 && (KL & 3)) tt &= (1u << (8 * (KL & 3))) - 1u;
            dd |= tt;
        }
        return dd == 0u;
    };
    // pair pre-check of piece q found intact at text position tq (see apm_ext_fwd)
    auto group_check = [&](int q, int64_t tq, int aux, int n_pieces, int m, int poff) __attribute__((always_inline)) {
        if constexpr (!PAIRS) {
            return true;
        } else {
            const int aq = (int)s_poff[aux + q];
            const int aq1 = (q + 1 < n_pieces) ? (int)s_poff[aux + q + 1] : m;
            for (int x = KL; x < aq1 - aq; ++x) // rest of the piece behind its key bytes
                if (apm_gbyte(text, limit, tq + x) != (int)s_pat[poff + aq + x]) return false;
            const int p = q ^ 1;
            if (p >= n_pieces) return true; // unpaired last piece (even k)
            uint32_t P[4], T[5]; // (see apm_filter_kernel: one 128-bit core for both directions)
            int n;
            if (p > q) {
                const int ap1 = (p + 1 < n_pieces) ? (int)s_poff[aux + p + 1] : m;
                n = ap1 - aq1;
                if (n > 16) return apm_ext_fwd_g(text, limit, tq + (aq1 - aq), s_pat, poff + aq1, n);
                apm_lds_dwords<4>(s_pat, poff + aq1, P);
                apm_gdwords<5>(text, limit, tq + (aq1 - aq), T);
            } else {
                const int ap = (int)s_poff[aux + p];
                n = aq - ap;
                if (n > 16) return apm_ext_bwd_g(text, limit, tq, s_pat, poff + ap, n);
                uint32_t Q[4], W[5];
                apm_lds_dwords<4>(s_pat, poff + aq - 16, Q);
                apm_gdwords<5>(text, limit, tq - 20, W);
#pragma unroll
                for (int z = 0; z < 4; ++z) P[z] = apm_bswap(Q[3 - z]);
#pragma unroll
                for (int z = 0; z < 5; ++z) T[z] = apm_bswap(W[4 - z]);
            }
            return apm_ext1_core16(P, T, n);
        }
    };

    // ---- verification of one (key, sampled position) nomination over shifts [dl_lo, dl_hi] ----
    auto verify_item = [&](int kid, int64_t pos, int dl_lo, int dl_hi) __attribute__((always_inline)) {
        const uint32_t ki = s_kinfo[kid];
        const int kpat = (int)(ki & 0xfffu), koff = (int)((ki >> 12) & 0x1ffu), kpiece = (int)((ki >> 21) & 7u);
        const uint2 pinf = s_pinfo[kpat];
        const int m = (int)(pinf.x >> 16), aux = (int)pinf.y, poff = (int)(pinf.x & 0xffffu);
        const int n_pieces = a.k + 1;
        if (!key_at(pos, poff, koff)) return; // fingerprint / tag collision
        if (!group_check(kpiece, pos, aux, n_pieces, m, poff)) return;
        const int64_t je_p = min(a.je, a.nrel - m + 1);
        for (int dl = dl_lo; dl <= dl_hi; ++dl) {
            const int64_t j = pos - koff - dl; // candidate window start
            if (j < a.jb || j >= je_p) continue;
            if (!apm_banded_verify<BAND>(ApmGlobalText{text, j, limit}, s_pat, poff, m, a.k)) continue;
            // count the window once: only from its first true (piece, shift) nominator
            bool first = true;
            for (int qq = 0; qq <= kpiece && first; ++qq) {
                const int aq = (int)s_poff[aux + qq];
                for (int dd = -BAND; dd <= BAND; ++dd) {
                    if (qq == kpiece && dd >= dl) break;
                    const int64_t o = j + aq + dd;                                   // piece start under shift dd
                    const int rr = (int)((STRIDE - (o & (STRIDE - 1))) & (STRIDE - 1)); // its sampled (aligned) block
                    if (o + rr >= 0 && key_at(o + rr, poff, aq + rr) && group_check(qq, o, aux, n_pieces, m, poff)) {
                        first = false;
                        break;
                    }
                }
            }
            if (first) {
                atomicAdd(&s_cnt[kpat], 1u);
#ifdef APM_REC
                apm_rec_push(a.pos, a.pats[kpat].index, j);
#endif
            }
        }
    };

    auto flush = [&](uint32_t qcount) __attribute__((always_inline)) {
        const uint32_t nitems = PAIRS ? qcount : qcount * NSH; // PAIRS: the cheap pre-check runs once per entry
        for (uint32_t wi = lane; wi < nitems; wi += 64) {
            const uint2 ent = s_queue[PAIRS ? wi : wi / NSH];
            const int dl_lo = PAIRS ? -BAND : (int)(wi % NSH) - BAND;
            const int dl_hi = PAIRS ? BAND : dl_lo;
            const int64_t pos = (int64_t)ent.x | ((int64_t)ent.y << 32);
            if (pos + KL > a.avail) continue;
            uint32_t fw[(KL + 3) / 4];
            apm_gdwords<(KL + 3) / 4>(text, limit, pos, fw);
            uint32_t fi;
            if constexpr (KL == 16) fi = apm_fp16(apm_fp8(fw[0], fw[1]), apm_fp8(fw[2], fw[3]));
            else if constexpr (KL > 4) fi = apm_fp8(fw[0], fw[1] & apm_hi_mask<KL>());
            else fi = fw[0];
            const uint32_t hh = apm_table_hash<KL>(fi);
            const uint32_t slot = hh >> hshift;
            const uint32_t tag = hh & 0xffffu; // (the bitmap filter queues bare positions)
            uint32_t first = 0xffffffffu; // this lane's matching way, verified with the whole wave
            int n_match = 0;
            {
                const uint4 tg = s_tab[slot], kd = s_kid[slot];
                const uint32_t tw[4] = {tg.x, tg.y, tg.z, tg.w}, kw[4] = {kd.x, kd.y, kd.z, kd.w};
#pragma unroll
                for (int w4 = 3; w4 >= 0; --w4) { // descending: `first` ends up as the lowest matching way
                    const uint32_t khi = kw[w4] >> 16, klo = kw[w4] & 0xffffu;
                    if ((tw[w4] >> 16) == tag && khi != 0xffffu) { first = khi; ++n_match; }
                    if ((tw[w4] & 0xffffu) == tag && klo != 0xffffu) { first = klo; ++n_match; }
                }
                for (int o = 0; o < a.n_ovf; ++o)
                    if (s_ovf[2 * o] == tag) {
                        if (n_match == 0) first = s_ovf[2 * o + 1];
                        ++n_match;
                    }
            }
            if (n_match > 0) {
                uint32_t kid = first & 0x7fffu;
                const bool more = (first & 0x8000u) != 0;
                for (;;) {
                    verify_item((int)kid, pos, dl_lo, dl_hi);
                    if (!more) break;
                    const uint32_t nxt = s_next[kid];
                    if (!nxt) break;
                    kid = nxt - 1u;
                }
            }
            if (n_match > 1) { // several ways carry this tag (rare)
                const uint16_t *tag16 = reinterpret_cast<const uint16_t *>(s_tab + slot);
                const uint16_t *kid16p = reinterpret_cast<const uint16_t *>(s_kid + slot);
                int seen = 0;
#pragma unroll 1
                for (int c = 0; c < 8 + a.n_ovf; ++c) {
                    uint32_t t16, kid16;
                    if (c < 8) {
                        t16 = tag16[c];
                        kid16 = kid16p[c];
                    } else {
                        t16 = s_ovf[2 * (c - 8)];
                        kid16 = s_ovf[2 * (c - 8) + 1];
                    }
                    if (t16 != tag || kid16 == 0xffffu) continue;
                    if (seen++ == 0) continue;
                    uint32_t kid = kid16 & 0x7fffu;
                    const bool more = (kid16 & 0x8000u) != 0;
                    for (;;) {
                        verify_item((int)kid, pos, dl_lo, dl_hi);
                        if (!more) break;
                        const uint32_t nxt = s_next[kid];
                        if (!nxt) break;
                        kid = nxt - 1u;
                    }
                }
            }
        }
    };

    uint32_t qcount = 0; // wave-uniform
    auto drain = [&]() __attribute__((always_inline)) {
        if (qcount >= 64u) {
            flush(qcount);
            qcount = 0;
        }
    };
    // First-level filter of the per-position classes: a presence bitmap over the 2-bit byte codes
    // (b >> code_shift) & 3 of the key bytes (built by the host next to the hash table).  The lane packs
    // the codes of its 24 bytes into a bit string once; the code word of position i is a 2i-bit funnel
    // shift of it and its bit sits in byte x & (NB-1) of the bitmap, bit x >> log2(NB).  Returns the
    // lane's 16-bit hit mask (bit i = position i of its 16 bytes).
    auto pack4 = [&](uint32_t wv4) __attribute__((always_inline)) { // 4 bytes -> 8 code bits
        const uint32_t cd = (wv4 >> a.code_shift) & 0x03030303u;
        const uint32_t u = cd | (cd >> 6);
        return (u | (u >> 12)) & 0xffu;
    };
    constexpr int LB = 13; // log2 of the bitmap's byte count: 8 KiB over 8-byte code words for every key length
    // the bitmap leads the image = the start of dynamic LDS, and this kernel owns no static LDS (tests
    // check the build's resource digest): LDS address 0, a compile-time constant -> no address add per probe
    const apm_lds_u8 *bmp0 = (const apm_lds_u8 *)(uintptr_t)0;
    auto bmp_bit = [&](uint32_t x) __attribute__((always_inline)) { // and, ds_read_u8, 2 x v_bfe_u32
        const uint32_t byte = bmp0[x & ((1u << LB) - 1u)];
        return __builtin_amdgcn_ubfe(byte, __builtin_amdgcn_ubfe(x, LB, 3), 1);
    };
    auto hit_bits = [&](const u32x4 &v, const uint2 &e, int64_t cc) __attribute__((always_inline)) {
        if (APM_SKIP(a, 32)) return (v.x ^ e.x) == 0x12345u ? 1u : 0u; // (measurement build) streaming skeleton only
        uint32_t hits = 0;
        const uint32_t clo = pack4(v.x) | (pack4(v.y) << 8) | (pack4(v.z) << 16) | (pack4(v.w) << 24);
        const uint32_t chi = pack4(e.x) | (pack4(e.y) << 8);
#pragma unroll
        for (int i = 15; i >= 0; --i) // descending: hits = hits << 1 | bit (one v_lshl_or_b32 each)
            hits = (hits << 1) | bmp_bit(i ? __builtin_amdgcn_alignbit(chi, clo, 2u * (uint32_t)i) : clo);
        return (cc < nch && !APM_SKIP(a, 1)) ? hits : 0u;
    };
    // the hit positions of one chunk go to the wave queue, one bit per lane and round (<= 16 rounds of
    // <= 64 positions); the queue is verified as soon as it holds a wave's worth
    auto push_hits = [&](uint32_t hits, int64_t cc) __attribute__((always_inline)) {
        const int64_t pos = a.tile0 + cc * 1024 + 16 * lane;
        while (__builtin_amdgcn_ballot_w64(hits != 0)) {
            const bool has = hits != 0;
            const int i = has ? __builtin_ctz(hits) : 0;
            hits &= hits - 1u; // (0 stays 0)
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(has);
            const uint32_t idx = qcount + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            const int64_t pp = pos + i;
            if (has) s_queue[idx] = make_uint2((uint32_t)pp, (uint32_t)(pp >> 32));
            qcount += (uint32_t)__builtin_popcountll(mask);
            drain();
        }
    };

    // sampled classes: one (stride 16) or two (stride 8) fingerprints per lane and chunk probe the hash
    // table directly (8 x 16-bit tags per bucket, v_pk_min_u16 match); hits are queued on the spot.
    // (A bitmap first level was measured here too: no gain at one or two probes per lane.)
    auto probe = [&](uint32_t fi, int64_t pos, bool valid) __attribute__((always_inline)) {
        const uint32_t h = apm_table_hash<KL>(fi);
        const uint32_t slot = h >> hshift;
        const uint32_t tag = h & 0xffffu;
        const uint32_t rep = tag | (tag << 16);
        const uint4 tg = s_tab[slot];
        const u16x2 m01 = __builtin_elementwise_min(apm_as_u16x2(tg.x ^ rep), apm_as_u16x2(tg.y ^ rep));
        const u16x2 m23 = __builtin_elementwise_min(apm_as_u16x2(tg.z ^ rep), apm_as_u16x2(tg.w ^ rep));
        const u16x2 mm = __builtin_elementwise_min(m01, m23);
        bool hit = (mm.x == 0) | (mm.y == 0);
        for (int o = 0; o < a.n_ovf; ++o) hit |= (s_ovf[2 * o] == tag);
        hit &= valid;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        if (mask) { // rare with long keys
            const uint32_t idx = qcount + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            if (hit) s_queue[idx] = make_uint2((uint32_t)pos, (uint32_t)(pos >> 32));
            qcount += (uint32_t)__builtin_popcountll(mask);
        }
    };
    auto process = [&](const u32x4 &v, int64_t cc) __attribute__((always_inline)) {
        const int64_t pos = a.tile0 + cc * 1024 + 16 * lane;
        const bool valid = cc < nch && !APM_SKIP(a, 1);
        if constexpr (STRIDE == 16) {
            probe(apm_fp16(apm_fp8(v.x, v.y), apm_fp8(v.z, v.w)), pos, valid);
        } else if constexpr (STRIDE == 8) {
            probe(apm_fp8(v.x, v.y), pos, valid);
            probe(apm_fp8(v.z, v.w), pos + 8, valid);
        }
    };

    // four chunks in flight per lane.  Per-position classes: the four bitmap passes only produce hit
    // masks and ONE runtime loop queues them, so the kernel holds a single copy of the verification code.
    int64_t c = (int64_t)blockIdx.x * (APM_BLOCK / 64) + wv;
    if constexpr (STRIDE > 1) {
        // the four chunks a wave has in flight are neighbours (4 KiB contiguous per wave, 16 KiB per workgroup;
        // measured against chunks W apart: same on the HBM-bound cfg2, 7 % faster on cfg4)
        constexpr int64_t CS = 1;
        c *= 4;
        u32x4 r0, r1, r2, r3;
        uint2 e0 = make_uint2(0, 0), e1 = e0, e2 = e0, e3 = e0;
        load_chunk(c, r0, e0);
        load_chunk(c + CS, r1, e1);
        load_chunk(c + 2 * CS, r2, e2);
        load_chunk(c + 3 * CS, r3, e3);
        for (; c < nch; c += 4 * W) {
            { const u32x4 v = r0; load_chunk(c + 4 * W, r0, e0); process(v, c); }
            { const u32x4 v = r1; load_chunk(c + 4 * W + CS, r1, e1); process(v, c + CS); }
            if constexpr (STRIDE == 8) drain(); // four positions queued: keeps the wave queue (LDS) small
            { const u32x4 v = r2; load_chunk(c + 4 * W + 2 * CS, r2, e2); process(v, c + 2 * CS); }
            { const u32x4 v = r3; load_chunk(c + 4 * W + 3 * CS, r3, e3); process(v, c + 3 * CS); }
            drain(); // few verification sites: keeps the loop small and its uniform state in SGPRs
        }
    } else {
        u32x4 r0, r1, r2, r3;
        uint2 e0 = make_uint2(0, 0), e1 = e0, e2 = e0, e3 = e0;
        c *= 4; // (four neighbouring chunks per wave, as above)
        load_chunk(c, r0, e0);
        load_chunk(c + 1, r1, e1);
        load_chunk(c + 2, r2, e2);
        load_chunk(c + 3, r3, e3);
        for (; c < nch; c += 4 * W) {
            uint32_t h0, h1, h2, h3;
            { const u32x4 v = r0; const uint2 e = e0; load_chunk(c + 4 * W, r0, e0); h0 = hit_bits(v, e, c); }
            { const u32x4 v = r1; const uint2 e = e1; load_chunk(c + 4 * W + 1, r1, e1); h1 = hit_bits(v, e, c + 1); }
            { const u32x4 v = r2; const uint2 e = e2; load_chunk(c + 4 * W + 2, r2, e2); h2 = hit_bits(v, e, c + 2); }
            { const u32x4 v = r3; const uint2 e = e3; load_chunk(c + 4 * W + 3, r3, e3); h3 = hit_bits(v, e, c + 3); }
            if (__builtin_amdgcn_ballot_w64((h0 | h1 | h2 | h3) != 0)) {
#pragma unroll 1
                for (int j = 0; j < 4; ++j) push_hits(j == 0 ? h0 : (j == 1 ? h1 : (j == 2 ? h2 : h3)), c + j);
            }
        }
    }
    flush(qcount); // the last partial queue (same single verification site)

    __syncthreads();
    for (int i = tid; i < a.n_pats; i += APM_BLOCK) {
        const uint32_t cnt = s_cnt[i];
        if (cnt) atomicAdd(&a.counts[a.pats[i].index], (unsigned long long)cnt);
    }
}

static size_t apm_stream_lds_bytes(const ApmFilterArgs &a) {
    const size_t qw = (size_t)(64 * 4 + 64); // = QW of the kernel
    size_t b = (size_t)a.image_len + 4 * qw * 8 + (size_t)((a.n_pats + 3) & ~3) * 4 + 16;
    return b < 4608 ? 4608 : b; // the tail workgroups need 256 uint4 + 128 bytes
}

template <int BAND>
static const void *apm_stream_fn_kl(int kl, int stride) {
    if (kl == 16 && stride == 16) return (const void *)apm_stream_kernel<BAND, 16, 16>;
    if (kl == 8 && stride == 8) return (const void *)apm_stream_kernel<BAND, 8, 8>;
    // Per-position classes: the host picks this form only for launches whose keys are expected to hit
    // rarely (few keys per 4^key_len codes).  With frequent candidates the LDS-tile kernel wins clearly
    // (verification against global text: cfg5 20 ms vs 3.6 ms per GiB on MI355X).
    // Wider bands (k >= 4) would spill there and stay on the tile kernel.
    if constexpr (BAND <= 1) {
        if (kl == 8 && stride == 1) return (const void *)apm_stream_kernel<BAND, 8, 1>;
        if (kl == 6 && stride == 1) return (const void *)apm_stream_kernel<BAND, 6, 1>;
        if (kl == 4 && stride == 1) return (const void *)apm_stream_kernel<BAND, 4, 1>;
    }
    return nullptr;
}
static const void *apm_stream_fn(int band, int kl, int stride) {
    switch (band) {
    case 0: return apm_stream_fn_kl<0>(kl, stride);
    case 1: return apm_stream_fn_kl<1>(kl, stride);
    case 2: return apm_stream_fn_kl<2>(kl, stride);
    case 3: return apm_stream_fn_kl<3>(kl, stride);
    default: return nullptr;
    }
}

int apm_stream_blocks_per_cu(const ApmFilterArgs &a) {
    int per_cu = 0;
    const void *fn = apm_stream_fn(a.band, a.key_len, a.stride);
    if (!fn || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, APM_BLOCK, apm_stream_lds_bytes(a)) != hipSuccess || per_cu < 1) {
        (void)hipGetLastError();
        per_cu = 2;
    }
    return per_cu > 8 ? 8 : per_cu;
}

// a.tile0 = first scanned relative position (multiple of 16), a.ntiles = number of 1 KiB chunks
hipError_t apm_launch_stream(const ApmFilterArgs &a, int max_blocks, hipStream_t s) {
    if (a.ntiles <= 0 || a.n_pats <= 0) return hipSuccess;
    const void *fn = apm_stream_fn(a.band, a.key_len, a.stride);
    if (!fn) return hipErrorInvalidValue;
    const int64_t want = (a.ntiles + 3) / 4;
    const int64_t cap = max_blocks < 1 ? 1 : max_blocks;
    const int64_t nb = want < cap ? want : cap;
    ApmFilterArgs args = a;
    args.n_main_blocks = (int)nb;
#ifdef APM_MEASURE
    if (const char *e = getenv("APM_MEASURE_SKIP")) args.skip_mask = atoi(e);
#endif
    void *kargs[] = {&args};
    return hipLaunchKernel(fn, dim3((unsigned)(nb + a.n_tail)), dim3(APM_BLOCK), kargs, apm_stream_lds_bytes(a), s);
}
