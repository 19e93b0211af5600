/*
 * apm_banded_tile.h -- the LDS-tile form of the BANDED filter kernel (design: apm_banded.h).  Its 40 instantiations are the
 * longest compile of the library, so each band is a unit of its own (band 2, the longest, two: apm_banded_tile_b2_dma.hip): apm_banded_tile_b<BAND>.hip
 * includes this header and hands its kernels out through one getter; apm_banded_tile.hip holds the launcher and never
 * sees the template.
 */
#ifndef APM_BANDED_TILE_H
#define APM_BANDED_TILE_H

#include "apm_banded.h"

// DMA = 1: tiles travel HBM -> LDS by LDS-DMA (global_load_lds_dwordx4, no VGPR staging), three LDS
// tile buffers (four for the per-position classes, whose candidates of two consecutive tiles are verified in
// one pass), waits placed by hand (vmcnt(1): the younger tile stays in flight).  Needs a 16-byte aligned text
// pointer.  DMA = 0: register-staged buffer loads, two LDS buffers, compiler-placed waits.
template <int BAND, int KL, int STRIDE, int DMA>
__global__ __launch_bounds__(APM_BLOCK, (BAND == 0 && STRIDE > 1) ? 8 : ((BAND >= 2 && STRIDE == 1 && !DMA) ? 3 : ((BAND >= 3 || (BAND == 2 && STRIDE == 1)) ? 4 : ((BAND >= 1 && STRIDE == 1) ? 4 : 6)))) /* (per-position forms with a band: the LDS-DMA instantiations spilled 8 bytes per lane at 5 waves per SIMD; they are the fallback for unaligned text only since round 2, so they take the registers) */
void apm_filter_kernel(ApmFilterArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= a.n_main_blocks) { // extra workgroups: truncated tail windows (one pattern each)
        apm_tail_body(a.tail, (int)blockIdx.x - a.n_main_blocks, reinterpret_cast<uint4 *>(smem), tid);
        return;
    }
    // LDS: [tile 0 | tile 1 | (tile 2) | launch image (pattern bytes, hash table, key/pattern records) | queue | counts]
    // LDS-DMA: three tile buffers; the per-position classes keep a fourth so that the tile before the current
    // one stays intact and two tiles are verified in ONE pass (see the tile loop)
    constexpr bool TWO_TILES = DMA && STRIDE == 1;
    constexpr int NBUF = DMA ? (TWO_TILES ? 4 : 3) : 2;
    uint8_t *s_tile0 = smem;
    uint8_t *s_tile1 = smem + a.tile_len;
    uint8_t *s_img = smem + NBUF * APM_FILTER_POS;                       // (= a.tile_len, as a constant)
    uint8_t *s_pat = s_img + a.o_pat;                                    // raw pattern bytes
    uint4 *s_tab = reinterpret_cast<uint4 *>(s_img + a.o_tab);           // nb buckets x 8 16-bit tags
    uint4 *s_kid = reinterpret_cast<uint4 *>(s_img + a.o_kid);           // nb x 8 16-bit key ids
    uint32_t *s_ovf = reinterpret_cast<uint32_t *>(s_img + a.o_ovf);     // n_ovf x {tag, kid16}
    uint32_t *s_kinfo = reinterpret_cast<uint32_t *>(s_img + a.o_kinfo); // nk: pat | off<<12 | piece<<21
    uint2 *s_pinfo = reinterpret_cast<uint2 *>(s_img + a.o_pinfo);       // n_pats: {byte_off | m<<16, aux_off}
    const uint16_t *s_next = reinterpret_cast<const uint16_t *>(s_img + a.o_next); // nk: chain links (id+1, 0 = end)
    const uint16_t *s_poff = reinterpret_cast<const uint16_t *>(s_img + a.o_poff); // piece offsets a_q
    uint32_t *s_queue = reinterpret_cast<uint32_t *>(s_img + a.image_len); // 2 x qcap
    uint32_t *s_cnt = s_queue + 2 * a.qcap;
    uint32_t *s_qn = s_cnt + ((a.n_pats + 3) & ~3); // [2] queue counters, [4..7] per-wave survivor counters
    constexpr int SCAP = 128;                       // per-wave list of pre-check survivors (kid | pos << 16)
    uint32_t *s_surv = s_qn + 8;

    // Branch-free tile fetch: ONE raw buffer load of 16 bytes per lane per tile (tile = 4096 bytes),
    // the descriptor's num_records does the bounds check (out-of-range lanes return 0 and move no
    // data).  No other vector-memory operation lives in the tile loop, so the compiler's vmcnt
    // bookkeeping keeps the younger prefetch in flight while the older one is consumed.
    // The descriptor is based on the 16-byte granule that holds text[0] (the bytes in front of an unaligned
    // text pointer lie in the same allocation granule and never belong to a counted window): every lane's
    // 16-byte load then starts on a multiple of 16 from that base, so a load is either wholly in front of the
    // text (-> zeros) or wholly inside -- a load straddling text[0] would be dropped as a whole and lose the
    // first bytes of an unaligned text.
    const int text_sh = (int)(reinterpret_cast<uintptr_t>(a.text) & 15u);
    auto fetch = [&](int t, u32x4 &r0) __attribute__((always_inline)) {
        const int64_t g = a.tile0 + (int64_t)t * a.tile_w - a.front + text_sh; // multiple of 16, >= -32, from the granule base
        const int64_t gb = g > 0 ? g : 0;
        const int64_t lim = a.avail_pad + text_sh - gb;
        const uint32_t nrec = lim <= 0 ? 0u : (lim > 0x7fffffffLL ? 0x7fffffffu : (uint32_t)lim);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.text) - text_sh + gb, 0, (int)nrec, 0x00020000);
        const uint32_t o0 = (uint32_t)((int)(g - gb) + 16 * tid); // negative wraps -> out of range -> 0
        r0 = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)o0, 0, 0);
    };
    auto stash = [&](uint8_t *buf, const u32x4 &r0) __attribute__((always_inline)) {
        *reinterpret_cast<u32x4 *>(buf + 16 * tid) = r0;
    };

    // tile indices fit 32 bits (the launcher refuses more than 2^30 tiles = 4 TiB of text per launch);
    // 64-bit loop state would not fit the SGPR budget and spill
    const int G = a.n_main_blocks;
    const int ntiles = (int)a.ntiles;
    int t = (int)blockIdx.x;
    u32x4 ra0 = {0, 0, 0, 0}, rb0 = {0, 0, 0, 0};

    // LDS-DMA of one tile: lane L's 16 bytes land at (buffer + wave*1024) + 16*L.  Lanes outside the
    // text read a clamped in-range address instead (their bytes are never part of a counted window).
    const uint32_t lds0 = __builtin_amdgcn_groupstaticsize();
    const uint32_t wave_off = __builtin_amdgcn_readfirstlane((uint32_t)tid >> 6) * 1024u;
    const uint32_t lane_off = 16u * (uint32_t)tid;
    auto dma = [&](int tt, int buf) __attribute__((always_inline)) {
        const int64_t gt = a.tile0 + (int64_t)tt * a.tile_w - a.front; // tile start (uniform)
        const uint32_t base = lds0 + (uint32_t)buf * (uint32_t)APM_FILTER_POS + wave_off;
        uint32_t keep;
        if (gt >= 0 && gt + APM_FILTER_POS <= a.avail_pad) { // whole tile inside the text: scalar base + lane offset
            const uint8_t *gbase = a.text + gt;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(lane_off), "s"(base), "s"(gbase)
                         : "memory");
        } else { // edge tile: clamp every lane's address into the text
            int64_t g = gt + 16 * tid;
            const int64_t hi = a.avail_pad - 16;
            g = g > hi ? hi : g;
            g = g < 0 ? 0 : g;
            const uint8_t *gp = a.text + g;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(gp), "s"(base)
                         : "memory");
        }
    };

    if constexpr (DMA) {
        for (int b = 0; b < 3; ++b)
            if (t + b * G < ntiles) dma(t + b * G, b);
    } else {
        if (t < ntiles) fetch(t, ra0);
    }
    // the launch image is ONE contiguous blob laid out like its LDS copy: a single round of
    // 16-byte loads, one wait (separate small copies would chain their HBM latencies)
    for (int i = tid; i < (a.image_len >> 4); i += APM_BLOCK)
        reinterpret_cast<uint4 *>(s_img)[i] = a.image[i];
    for (int i = tid; i < a.n_pats; i += APM_BLOCK) s_cnt[i] = 0u;
    if (tid < 2) s_qn[tid] = 0u;
    if constexpr (!DMA) {
        if (t < ntiles) {
            stash(s_tile0, ra0);
            if (t + G < ntiles) fetch(t + G, ra0);         // A: tile t+G   -> lands in buffer 1
            if (t + 2 * G < ntiles) fetch(t + 2 * G, rb0); // B: tile t+2G -> lands in buffer 0
        }
    }
    __syncthreads(); // (drains the prologue loads, DMA included)

    // verification of one (key, sampled text position, shift) nomination; bumps s_cnt
    // does piece q of the pattern (piece offsets at s_poff[aux..], n_pieces of them, length m, bytes at
    // s_pat+poff) found intact at LDS text offset tq pass the pair pre-check?  (see apm_ext_fwd)
    constexpr bool PAIRS = (STRIDE == 1) && (BAND >= 1);
    auto group_check = [&](const uint8_t *s_tile, int q, int tq, int aux, int n_pieces, int m, int poff) __attribute__((always_inline)) {
        if constexpr (!PAIRS) {
            return true;
        } else {
            const int aq = (int)s_poff[aux + q];
            const int aq1 = (q + 1 < n_pieces) ? (int)s_poff[aux + q + 1] : m;
            for (int x = KL; x < aq1 - aq; ++x) // rest of the piece behind its key bytes
                if (s_tile[tq + x] != s_pat[poff + aq + x]) return false;
            const int p = q ^ 1;
            if (p >= n_pieces) return true; // unpaired last piece (even k)
            // partner piece: after this one (p > q, text read forward from the end of the piece) or before it
            // (read backward from its start, both strings byte-reversed); <= 16 bytes -> one 128-bit core
            uint32_t P[4], T[5];
            int n;
            if (p > q) {
                const int ap1 = (p + 1 < n_pieces) ? (int)s_poff[aux + p + 1] : m;
                n = ap1 - aq1;
                if (n > 16) return apm_ext_fwd(s_tile, tq + (aq1 - aq), s_pat, poff + aq1, n);
                apm_lds_dwords<4>(s_pat, poff + aq1, P);
                apm_lds_dwords<5>(s_tile, tq + (aq1 - aq), T);
            } else {
                const int ap = (int)s_poff[aux + p];
                n = aq - ap;
                if (n > 16) return apm_ext_bwd(s_tile, tq, s_pat, poff + ap, n);
                // a window this tile counts has tq >= front + n - band >= 14: nearer the tile start it is none,
                // and the 20 text bytes in front of tq exist only from tq = 20 on (short partners need 9)
                if (tq < 12 || (tq < 20 && n > 8)) return false;
                uint32_t Q[4], W[5];
                apm_lds_dwords<4>(s_pat, poff + aq - 16, Q);
                const int back = tq < 20 ? 12 : 20;
                apm_lds_dwords<5>(s_tile, tq - back, W); // bytes [tq-back, tq-back+20)
#pragma unroll
                for (int z = 0; z < 4; ++z) P[z] = apm_bswap(Q[3 - z]);
                if (back == 20) {
#pragma unroll
                    for (int z = 0; z < 5; ++z) T[z] = apm_bswap(W[4 - z]);
                } else { // the 12 bytes in front of tq, reversed; n <= 8 looks at 9 of them
                    T[0] = apm_bswap(W[2]);
                    T[1] = apm_bswap(W[1]);
                    T[2] = apm_bswap(W[0]);
                    T[3] = 0u;
                    T[4] = 0u;
                }
            }
            return apm_ext1_core16(P, T, n);
        }
    };

    // stage 1 of a nomination (key, sampled text position): key bytes equal + pair pre-check
    auto stage1_item = [&](const uint8_t *s_tile, int kid, int pos) __attribute__((always_inline)) {
        const uint32_t ki = s_kinfo[kid];
        const int kpat = (int)(ki & 0xfffu), koff = (int)((ki >> 12) & 0x1ffu), kpiece = (int)((ki >> 21) & 7u);
        const uint2 pinf = s_pinfo[kpat];
        const int poff = (int)(pinf.x & 0xffffu);
        if (!apm_key_equal<KL>(s_tile, pos, s_pat, poff + koff)) return false; // fingerprint collision
        return (bool)group_check(s_tile, kpiece, pos, (int)pinf.y, a.k + 1, (int)(pinf.x >> 16), poff);
    };
    // the same for the per-position classes out of ONE packed record per key (a.o_kext): the whole piece in a
    // single masked 16-byte compare, then the partner through the 128-bit core; no walk through kinfo / pinfo /
    // piece offsets (four dependent LDS reads less on the path every candidate takes)
    const uint32_t *s_kext = reinterpret_cast<const uint32_t *>(s_img + a.o_kext);
    auto stage1_fast = [&](const uint8_t *s_tile, int kid, int pos) __attribute__((always_inline)) {
        typedef unsigned long long u64;
        const uint32_t kx = s_kext[kid];
        const int at = (int)(kx & 0xffffu), len = (int)((kx >> 16) & 0xffu), n = (int)((kx >> 24) & 31u), side = (int)(kx >> 29);
        uint32_t A[4], B[4];
        apm_lds_dwords<4>(s_tile, pos, A);
        apm_lds_dwords<4>(s_pat, at, B);
        const u64 ml = len >= 8 ? ~0ull : ((1ull << (8 * len)) - 1ull);
        const u64 mh = len <= 8 ? 0ull : (len >= 16 ? ~0ull : ((1ull << (8 * (len - 8))) - 1ull));
        const u64 dl = (((u64)(A[1] ^ B[1]) << 32) | (A[0] ^ B[0])) & ml, dh = (((u64)(A[3] ^ B[3]) << 32) | (A[2] ^ B[2])) & mh;
        if ((dl | dh) != 0ull) return false; // fingerprint collision, or the piece is not intact
        for (int x = 16; x < len; ++x)       // (pieces beyond 16 bytes: only when long patterns joined this class)
            if (s_tile[pos + x] != s_pat[at + x]) return false;
        if (side == 0) return true;          // unpaired last piece (even k)
        if (n == 31) return (bool)stage1_item(s_tile, kid, pos); // partner longer than 16 bytes: the generic walk
        uint32_t P[4], T[5];
        if (side == 1) {
            apm_lds_dwords<4>(s_pat, at + len, P);
            apm_lds_dwords<5>(s_tile, pos + len, T);
        } else {
            if (pos < 12 || (pos < 20 && n > 8)) return false; // see group_check
            uint32_t Q[4], W[5];
            apm_lds_dwords<4>(s_pat, at - 16, Q);
            const int back = pos < 20 ? 12 : 20;
            apm_lds_dwords<5>(s_tile, pos - back, W);
#pragma unroll
            for (int z = 0; z < 4; ++z) P[z] = apm_bswap(Q[3 - z]);
            if (back == 20) {
#pragma unroll
                for (int z = 0; z < 5; ++z) T[z] = apm_bswap(W[4 - z]);
            } else {
                T[0] = apm_bswap(W[2]);
                T[1] = apm_bswap(W[1]);
                T[2] = apm_bswap(W[0]);
                T[3] = 0u;
                T[4] = 0u;
            }
        }
        return apm_ext1_core16(P, T, n);
    };
    // stage 2: banded DP of the window the nomination implies under shift dl + stateless dedup; bumps s_cnt
    auto dp_item = [&](const uint8_t *s_tile, int64_t base, int kid, int pos, int dl) __attribute__((always_inline)) {
        const uint32_t ki = s_kinfo[kid];
        struct { int pat, off, piece; } key = {(int)(ki & 0xfffu), (int)((ki >> 12) & 0x1ffu), (int)((ki >> 21) & 7u)};
        const uint2 pinf = s_pinfo[key.pat];
        struct { int m, aux_off; } d = {(int)(pinf.x >> 16), (int)pinf.y};
        const int poff = (int)(pinf.x & 0xffffu);
        const int m = d.m;
        const int n_pieces = a.k + 1;
        const int64_t je_p = min(a.je, a.nrel - m + 1);
        const int jr = pos - a.front - key.off - dl; // window start relative to base
        const int64_t j = base + jr;
        if (jr < 0 || jr >= a.tile_w || j < a.jb || j >= je_p) return;
        if (!apm_banded_verify<BAND>(ApmLdsText{s_tile, a.front + jr}, s_pat, poff, m, a.k)) return;
        // count the window once: only from its first true (piece, shift) nominator
        for (int qq = 0; qq <= (int)key.piece; ++qq) {
            const int aq = (int)s_poff[d.aux_off + qq];
            for (int dd = -BAND; dd <= BAND; ++dd) {
                if (qq == (int)key.piece && dd >= dl) break;
                const int o = a.front + jr + aq + dd;           // piece start under shift dd
                const int rr = (STRIDE - (o % STRIDE)) % STRIDE; // its sampled (aligned) block
                if (apm_key_equal<KL>(s_tile, o + rr, s_pat, poff + aq + rr) &&
                    group_check(s_tile, qq, o, d.aux_off, n_pieces, m, poff))
                    return;
            }
        }
        atomicAdd(&s_cnt[key.pat], 1u);
#ifdef APM_REC
        apm_rec_push(a.pos, a.pats[key.pat].index, j);
#endif
    };
    auto verify_item = [&](const uint8_t *s_tile, int64_t base, int kid, int pos, int dl_lo, int dl_hi) __attribute__((always_inline)) {
        if (!stage1_item(s_tile, kid, pos)) return;
        if (APM_SKIP(a, 16)) return; // (measurement build) skip the banded DP
        for (int dl = dl_lo; dl <= dl_hi; ++dl) dp_item(s_tile, base, kid, pos, dl);
    };

    const uint32_t hshift = 32u - (uint32_t)a.lg_nb;
    // resident slot of this workgroup on its CU (workgroups b, b + n_cu, b + 2 n_cu, ... tend to share a CU;
    // a heuristic, only the spread of the verification over the SIMDs depends on it): slots 0,1,2,3 -> 0,2,1,3
    const int slot_on_cu = (int)blockIdx.x / (a.n_cu > 0 ? a.n_cu : 256);
    const int rot0 = 2 * slot_on_cu + (slot_on_cu >> 1);

    // filter + enqueue, barrier, cooperative verification of tile t held in s_tile
    // filter + enqueue of the tile held in s_tile: pushes (tag, position) into queue array `qa`
    // (0/1) under counter s_qn[qc]
    auto filter_tile = [&](const uint8_t *s_tile, int qa, int qc, int tile_bit) __attribute__((always_inline)) {
        const int p0 = tid * 16; // LDS offset of this lane's first position
        uint32_t *queue = s_queue + qa * a.qcap;

        auto probe = [&](uint32_t fi, int pos) __attribute__((always_inline)) { // one hash-table probe
            const uint32_t h = apm_table_hash<KL>(fi);
            const uint32_t slot = h >> hshift;
            const uint32_t tag = h & 0xffffu;
            const uint32_t rep = tag | (tag << 16);
            const uint4 tg = s_tab[slot]; // 8 x 16-bit tags
            const u16x2 m01 = __builtin_elementwise_min(apm_as_u16x2(tg.x ^ rep), apm_as_u16x2(tg.y ^ rep));
            const u16x2 m23 = __builtin_elementwise_min(apm_as_u16x2(tg.z ^ rep), apm_as_u16x2(tg.w ^ rep));
            const u16x2 mm = __builtin_elementwise_min(m01, m23); // v_pk_min_u16: a zero half = tag match
            bool hit = (mm.x == 0) | (mm.y == 0);
            for (int o = 0; o < a.n_ovf; ++o) hit |= (s_ovf[2 * o] == tag);
            if (hit) { // rare with long keys: defer the bucket walk to the cooperative phase
                const uint32_t idx = atomicAdd(&s_qn[qc], 1u);
                if (idx < (uint32_t)a.qcap) queue[idx] = (tag << 16) | (uint32_t)pos;
            }
        };
        if (APM_SKIP(a, 1)) return; // (measurement build) skip the probes
        const uint4 va = *reinterpret_cast<const uint4 *>(s_tile + p0);
        if constexpr (STRIDE == 16) {
            probe(apm_fp16(apm_fp8(va.x, va.y), apm_fp8(va.z, va.w)), p0);
        } else if constexpr (STRIDE == 8) {
            probe(apm_fp8(va.x, va.y), p0);
            probe(apm_fp8(va.z, va.w), p0 + 8);
        } else {
            // every position (KL = 8, 6 or 4 key bytes).  First level = a presence bitmap over the 2-bit byte
            // codes (b >> code_shift) & 3: the lane packs the codes of its 24 bytes into 48 bits once, the
            // key code word of position i is a 2i-bit funnel shift of them, and its bit sits in byte
            // x & (NB-1) of the bitmap (ds_read_u8), bit x >> log2(NB).  ~6 instructions per position instead
            // of a fingerprint + bucket probe; the bucket walk happens in the cooperative phase for the hits.
            const uint2 vb = *reinterpret_cast<const uint2 *>(s_tile + p0 + 16);
            const uint32_t w[6] = {va.x, va.y, va.z, va.w, vb.x, vb.y};
            uint32_t pk[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const uint32_t c = (w[i] >> a.code_shift) & 0x03030303u;
                const uint32_t u = c | (c >> 6);
                pk[i] = (u | (u >> 12)) & 0xffu;
            }
            const uint32_t clo = pk[0] | (pk[1] << 8) | (pk[2] << 16) | (pk[3] << 24);
            const uint32_t chi = pk[4] | (pk[5] << 8);
            constexpr int LB = 13; // log2 of the bitmap's byte count: 8 KiB over 8-byte code words for every key length
            // the bitmap leads the image, and these kernels own no static LDS (tests check the build's
            // resource digest): its LDS address is a compile-time constant -> no address add per probe
            const apm_lds_u8 *bmp0 = (const apm_lds_u8 *)(uintptr_t)(NBUF * APM_FILTER_POS);
            uint32_t hits = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) { // and, ds_read_u8, 2 x v_bfe_u32, v_lshl_or_b32 per position
                const uint32_t x = i ? __builtin_amdgcn_alignbit(chi, clo, 2u * (uint32_t)i) : clo;
                const uint32_t byte = bmp0[x & ((1u << LB) - 1u)];
                hits |= __builtin_amdgcn_ubfe(byte, __builtin_amdgcn_ubfe(x, LB, 3), 1) << i;
            }
            while (hits) {
                const int i = __builtin_ctz(hits);
                hits &= hits - 1u;
                const uint32_t idx = atomicAdd(&s_qn[qc], 1u);
                if (idx < (uint32_t)a.qcap) queue[idx] = (uint32_t)(p0 + i) | ((uint32_t)tile_bit << 12);
            }
        }
    };

    // cooperative verification of the candidates queued for tile t (held in s_tile); the queue must be
    // complete (a barrier since its filter)
    // (the queue may hold the candidates of TWO tiles: bit 12 of an entry's position says which one -- the
    // "even" tile s_tile/t or the "odd" tile s_tile1/t1; callers with one tile pass it twice)
    auto verify_tile = [&](const uint8_t *s_tile, int t, const uint8_t *s_tile1, int t1, int qa, int qc, int rot) __attribute__((always_inline)) {
        // queue entries are dealt to the waves starting at wave `rot` (rotates per tile and workgroup): a short
        // queue keeps one wave busy, and wave i of every resident workgroup sits on SIMD i -- without the
        // rotation the verification of the whole CU would pile up on SIMD 0
        const uint32_t vtid = (uint32_t)(tid - 64 * rot) & (APM_BLOCK - 1);
        const int64_t base = a.tile0 + (int64_t)t * a.tile_w; // first window start of the tile
        const int64_t base1 = a.tile0 + (int64_t)t1 * a.tile_w;
        const uint8_t *const s_tile0v = s_tile;
        const int64_t base0v = base;
        const int p0 = tid * 16;
        constexpr int NF = 16 / STRIDE;
        const uint32_t *queue = s_queue + qa * a.qcap;
        const uint32_t qn = s_qn[qc];
        constexpr int NSH = 2 * BAND + 1;
        // all keys whose tag matches at this sampled position (bucket ways, overflow list, chains);
        // one runtime loop = ONE inlined copy of the verification code
        const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
        auto for_each_key = [&](uint32_t tag, int pos13, int dl_lo, int dl_hi) __attribute__((always_inline)) {
            const int pos = pos13 & 0xfff;
            const uint8_t *s_tile = (pos13 & 0x1000) ? s_tile1 : s_tile0v; // (shadows: this entry's tile)
            const int64_t base = (pos13 & 0x1000) ? base1 : base0v;
            auto handle = [&](int kid) __attribute__((always_inline)) {
                if constexpr (PAIRS) {
                    // pre-check here, banded DP later: the survivors (few per wave) go to a wave-private list so
                    // that the DP runs on dense lanes, one (survivor, shift) each, instead of inside this
                    // divergent walk with the three shifts in sequence
                    if (!stage1_fast(s_tile, kid, pos)) return;
                    if (APM_SKIP(a, 16)) return; // (measurement build) skip the banded DP
                    const uint32_t idx = atomicAdd(&s_qn[4 + wv], 1u);
                    if (idx < (uint32_t)SCAP) s_surv[wv * SCAP + idx] = (uint32_t)kid | ((uint32_t)pos13 << 16);
                    else
                        for (int dl = dl_lo; dl <= dl_hi; ++dl) dp_item(s_tile, base, kid, pos, dl); // list full (rare)
                } else {
                    verify_item(s_tile, base, kid, pos, dl_lo, dl_hi);
                }
            };
            uint32_t fw[(KL + 3) / 4];
            apm_lds_dwords<(KL + 3) / 4>(s_tile, pos, fw);
            uint32_t fi;
            if constexpr (KL == 16) fi = apm_fp16(apm_fp8(fw[0], fw[1]), apm_fp8(fw[2], fw[3]));
            else if constexpr (KL > 4) fi = apm_fp8(fw[0], fw[1] & apm_hi_mask<KL>());
            else fi = fw[0];
            const uint32_t hh = apm_table_hash<KL>(fi);
            const uint32_t slot = hh >> hshift;
            if constexpr (STRIDE == 1) tag = hh & 0xffffu; // (the bitmap filter queues bare positions)
            const uint16_t *tag16 = reinterpret_cast<const uint16_t *>(s_tab + slot);
            const uint16_t *kid16p = reinterpret_cast<const uint16_t *>(s_kid + slot);
            // Find this lane's matching way first (one 16-byte read of the tags, one of the key ids), THEN
            // verify: all lanes of the wave run the checks together instead of once per way index.
            uint32_t first = 0xffffffffu;
            int n_match = 0;
            {
                const uint4 tg = s_tab[slot], kd = s_kid[slot];
                const uint32_t tw[4] = {tg.x, tg.y, tg.z, tg.w}, kw[4] = {kd.x, kd.y, kd.z, kd.w};
#pragma unroll
                for (int wv = 3; wv >= 0; --wv) { // descending: `first` ends up as the lowest matching way
                    const uint32_t khi = kw[wv] >> 16, klo = kw[wv] & 0xffffu;
                    if ((tw[wv] >> 16) == tag && khi != 0xffffu) { first = khi; ++n_match; }
                    if ((tw[wv] & 0xffffu) == tag && klo != 0xffffu) { first = klo; ++n_match; }
                }
                for (int o = 0; o < a.n_ovf; ++o) // ascending: same "first" as the walk below
                    if (s_ovf[2 * o] == tag) {
                        if (n_match == 0) first = s_ovf[2 * o + 1];
                        ++n_match;
                    }
            }
            if (n_match > 0) {
                uint32_t kid = first & 0x7fffu;
                const bool more = (first & 0x8000u) != 0; // heads a chain of keys with the same tag
                for (;;) {
                    handle((int)kid);
                    if (!more) break;
                    const uint32_t nxt = s_next[kid];
                    if (!nxt) break;
                    kid = nxt - 1u;
                }
            }
            if (n_match > 1) { // several ways carry this tag (rare): walk the remaining ones
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
                        handle((int)kid);
                        if (!more) break;
                        const uint32_t nxt = s_next[kid];
                        if (!nxt) break;
                        kid = nxt - 1u;
                    }
                }
            }
        };
        if (APM_SKIP(a, 8)) { // (measurement build) skip verification
        } else if (qn <= (uint32_t)a.qcap) {
            if constexpr (PAIRS) { // work item = queue entry: the cheap pair pre-check runs once per entry ...
                if ((tid & 63) == 0) s_qn[4 + wv] = 0u; // (wave-private: LDS operations of one wave stay in order)
                for (uint32_t wi = vtid; wi < qn; wi += APM_BLOCK) {
                    const uint32_t ent = queue[wi];
                    for_each_key(ent >> 16, (int)(ent & 0xffffu), -BAND, BAND);
                }
                // ... then work item = (survivor, shift) of this wave's list
                __builtin_amdgcn_wave_barrier();
                const uint32_t ns = min(s_qn[4 + wv], (uint32_t)SCAP);
                for (uint32_t wi = (uint32_t)(tid & 63); wi < ns * NSH; wi += 64) {
                    const uint32_t e = s_surv[wv * SCAP + wi / NSH];
                    const bool odd = (e >> 28) & 1u;
                    dp_item(odd ? s_tile1 : s_tile, odd ? base1 : base, (int)(e & 0xffffu), (int)((e >> 16) & 0xfffu), (int)(wi % NSH) - BAND);
                }
            } else { // work item = (queue entry, shift): keeps all lanes busy
                for (uint32_t wi = vtid; wi < qn * NSH; wi += APM_BLOCK) {
                    const uint32_t ent = queue[wi / NSH];
                    const int dl = (int)(wi % NSH) - BAND;
                    for_each_key(ent >> 16, (int)(ent & 0xffffu), dl, dl);
                }
            }
        } else { // queue overflow: dense pass over every (sampled position, key) of the tile(s)
            for (int half = 0; half < (t1 != t ? 2 : 1); ++half)
                for (int i = 0; i < NF; ++i)
                    for (int kid = 0; kid < a.nk; ++kid)
                        verify_item(half ? s_tile1 : s_tile, half ? base1 : base, kid, p0 + i * STRIDE, -BAND, BAND);
        }
    };

    if constexpr (DMA) {
        for (int it = 0; t < ntiles; ++it, t += G) {
            // tile t (DMA issued two iterations ago) must have landed; the DMA of tile t+G stays in flight
            if (t + G < ntiles) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // every wave is past tile t-G now: its buffer takes tile t+2G
            if (it >= 1 && t + 2 * G < ntiles && !APM_SKIP(a, 2)) dma(t + 2 * G, (it + 2) % NBUF);
            const uint8_t *s_tile = smem + (it % NBUF) * APM_FILTER_POS;
            if constexpr (TWO_TILES) {
                // Dense per-position classes: the verification pass is latency bound and its lanes mostly
                // empty, so the candidates of two consecutive tiles share ONE queue and ONE pass (the fourth
                // buffer keeps the even tile intact while the odd one is filtered).
                const int q = (it >> 1) & 1;
                filter_tile(s_tile, q, q, it & 1);
                if ((it & 1) || t + G >= ntiles) {
                    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // A: queue complete (LDS only)
                    if (tid == 0) s_qn[q ^ 1] = 0u; // the next pair's counter (pushed to only after the next barrier)
                    if (it & 1) verify_tile(smem + ((it - 1) % NBUF) * APM_FILTER_POS, t - G, s_tile, t, q, q, ((it >> 1) + rot0) & 3);
                    else verify_tile(s_tile, t, s_tile, t, q, q, ((it >> 1) + rot0) & 3);
                }
            } else {
                filter_tile(s_tile, it & 1, it & 1, 0);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // A: queue complete (LDS only)
                if (tid == 0) s_qn[(it + 1) & 1] = 0u; // next tile's counter (read again only after the next barrier)
                verify_tile(s_tile, t, s_tile, t, it & 1, it & 1, (it + rot0) & 3);
            }
        }
    } else {
        // one iteration: filter tile t, barrier, verify it, then land the registers `r` (tile t+G) in the
        // other buffer and refill them with tile t+3G
        auto iteration = [&](int it, int t, const uint8_t *s_tile, uint8_t *s_other, u32x4 &r0) __attribute__((always_inline)) {
            filter_tile(s_tile, it & 1, it & 1, 0);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // A: queue complete (LDS only)
            if (tid == 0) s_qn[(it + 1) & 1] = 0u; // next iteration's counter (nobody reads it before barrier B)
            verify_tile(s_tile, t, s_tile, t, it & 1, it & 1, (it + rot0) & 3);
            if (t + G < ntiles) {
                stash(s_other, r0);
                if (t + 3 * G < ntiles && !APM_SKIP(a, 2)) fetch(t + 3 * G, r0);
            }
            __syncthreads(); // B
        };
        for (int it = 0; t < ntiles; it += 2, t += 2 * G) {
            iteration(it, t, s_tile0, s_tile1, ra0);
            if (t + G < ntiles) iteration(it + 1, t + G, s_tile1, s_tile0, rb0);
        }
    }
    __syncthreads();

    for (int i = tid; i < a.n_pats; i += APM_BLOCK) {
        const uint32_t c = s_cnt[i];
        if (c) atomicAdd(&a.counts[a.pats[i].index], (unsigned long long)c);
    }
}

// the kernel of one (band, DMA form) for a key class, nullptr if there is none
template <int BAND, int DMA>
static const void *apm_filter_fn_kl(int kl, int stride) {
    if (kl == 16 && stride == 16) return (const void *)apm_filter_kernel<BAND, 16, 16, DMA>;
    if (kl == 8 && stride == 8) return (const void *)apm_filter_kernel<BAND, 8, 8, DMA>;
    if (kl == 8 && stride == 1) return (const void *)apm_filter_kernel<BAND, 8, 1, DMA>;
    if (kl == 6 && stride == 1) return (const void *)apm_filter_kernel<BAND, 6, 1, DMA>;
    if (kl == 4 && stride == 1) return (const void *)apm_filter_kernel<BAND, 4, 1, DMA>;
    return nullptr;
}

#endif
