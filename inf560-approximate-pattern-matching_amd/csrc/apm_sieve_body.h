/*
 * apm_sieve_body.h -- the body of the SIEVE kernels (see apm_sieve.hip), shared by the units that instantiate it:
 * apm_sieve.hip (plain, with the code filter, with the column window DP) and apm_sieve_diag.hip (with the diagonal
 * window DP for k <= 3).  Device code only.
 */
#ifndef APM_SIEVE_BODY_H
#define APM_SIEVE_BODY_H
#include <type_traits>
#include "apm_wave.h"
#include "apm_sieve.h"

#define APM_SIEVE2_BLOCK 512

// ---------------------------------------------------------------------------
// SIEVE
// ---------------------------------------------------------------------------
// CF: with the code filter (ApmSieve2Args::cf_image) -- workgroups of blockDim.x threads, LDS = bitmap | cf image | wave areas
// DP (with CF and the candidate list): the window DP on codes of short patterns' units (ApmSieve2Args::cf_o_dp)
// DIAG (with DP, cf_dp_k <= 3): its diagonal form (apm_code_dp_diag) on the trimmed region [s - off - B, s - off + m + B), B = cf_dp_k / 2
// Args: ApmSieve2Args, or (DIAG) ApmSieve2PoolArgs -- the pooled hand-over of the candidate list when the workgroup ends
template <bool CF, bool DP, bool DIAG = false, typename Args = ApmSieve2Args>
__device__ __forceinline__ void apm_sieve2_body(const Args &a, uint8_t *smem) {
    const int THREADS = CF ? (int)blockDim.x : APM_SIEVE2_BLOCK;
    constexpr bool POOL = std::is_same<Args, ApmSieve2PoolArgs>::value;
    static_assert(!POOL || (DIAG && DP), "the pooled hand-over belongs to the diagonal kernel");
    constexpr uint32_t WAVE_BYTES =APM_CF_WAVE_BYTES + (DP ? APM_CF_DP_PEND_BYTES : 0); // a wave's area (apm_sieve2cf_lds_bytes)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((int)blockIdx.x >= a.n_main_blocks) { // extra workgroups: truncated tail windows (one pattern each)
        apm_tail_body(a.tail, (int)blockIdx.x - a.n_main_blocks, reinterpret_cast<uint4 *>(smem), tid);
        return;
    }
    apm_stage_image(reinterpret_cast<uint4 *>(smem), a.bitmap, 2048, tid, THREADS);
    if constexpr (CF) apm_stage_image(reinterpret_cast<uint4 *>(smem + 32768), a.cf_image, a.cf_len >> 4, tid, THREADS);
    // candidate list (ApmSieve2Args::clist): entries reserved in the workgroup's region | the first reservation that did not fit.
    // DP: entries written | entries reserved (written + waiting in the waves' DP queues; a reservation that does not fit is
    // taken back at once, and what the DP rejects is given back: the region never overflows with entries of finished blocks)
    uint32_t *cl_ctr = reinterpret_cast<uint32_t *>(smem + 32768 + (CF ? a.cf_len + (THREADS / 64) * WAVE_BYTES : 0));
    if (CF && tid == 0) { cl_ctr[0] = 0u; cl_ctr[1] = DP ? 0u : 0xffffffffu; }
    __syncthreads();
    const int64_t W = (int64_t)a.n_main_blocks * (THREADS / 64);
    const int64_t nch = a.nchunks;

    // 16 bytes per lane and chunk; `tl`: the 8 bytes behind the chunk (one address for the whole wave).  Chunks behind the
    // scanned range are loaded all the same -- text or, beyond avail_pad, zeros without traffic -- because the windows of
    // the last valid chunk run into them; only their own hits are dropped.
    // ONE buffer resource over the whole shard (< 4 GiB - 64 MiB, checked by the launcher: the offsets of the chunks a
    // wave loads ahead, up to 4 W beyond the scanned range, do not wrap) and 32-bit offsets: a resource per chunk cost two
    // 64-bit VALU compares per load (the scalar unit has none), ten per block.
    const __amdgpu_buffer_rsrc_t rs_all =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.text), 0, (int)(uint32_t)a.avail_pad, 0x00020000);
    const uint32_t t0_32 = (uint32_t)a.tile0, lane16 = 16u * (uint32_t)lane;
    auto load_chunk = [&](int64_t cc, u32x4 &r) __attribute__((always_inline)) {
        r = __builtin_amdgcn_raw_buffer_load_b128(rs_all, (int)(t0_32 + (uint32_t)cc * 1024u + lane16), 0, 0);
    };
    auto load_tail = [&](int64_t cc, v2u32 &tl) __attribute__((always_inline)) { // the 8 bytes at the start of chunk cc
        tl = __builtin_amdgcn_raw_buffer_load_b64(rs_all, (int)(t0_32 + (uint32_t)cc * 1024u), 0, 0);
    };
    // CF: the halo of the block that starts at chunk cc -- lanes 0, 1: the 32 bytes behind it, lane 2: the 16 bytes in front
    // of it, lane 3 and up: zeros (one load; the resource spans the whole shard: < 4 GiB, zeros outside, and a position in
    // front of the shard wraps to a huge offset = zeros, as for every verify path)
    auto load_halo = [&](int64_t cc, u32x4 &hl) __attribute__((always_inline)) {
        const uint32_t g = (uint32_t)(a.tile0 + cc * 1024);
        const uint32_t off = lane < 2 ? g + 4096u + 16u * (uint32_t)lane : (lane == 2 ? g - 16u : 0xfffffff0u);
        hl = __builtin_amdgcn_raw_buffer_load_b128(rs_all, (int)off, 0, 0);
    };
    const uint32_t cs = (uint32_t)a.code_shift;
    // LEAN: the streaming loop of the diagonal kernel (cfg3's, issue-bound) -- the pack's combine by pairs, lookups 4..7 out
    // of one funnel shift, the range test as one scalar mask per block; 11 VALU instructions fewer in the streaming block of the listing, 13 per
    // block by SQ_INSTS_VALU (the blocks around it shed two).  The kernels of
    // apm_sieve.hip keep the forms their pinned registers were recorded with (tests/test_verify_resources.py).
    constexpr bool LEAN = DIAG;
    auto pack16 = [&](const u32x4 &v) __attribute__((always_inline)) { return apm_pack16<LEAN>(v.x, v.y, v.z, v.w, cs); };
    // hit mask of the lane's eight even positions in chunk cc (apm_lookup2_chunk: the bitmap leads this kernel's LDS -- no
    // static LDS, checked by the tests); the hits of a chunk behind the scanned range are dropped (LEAN: by the block's mask)
    auto hit_bits = [&](uint32_t slo, uint32_t nx0, int64_t cc) __attribute__((always_inline)) {
        uint32_t hits = apm_lookup2_chunk<LEAN>(slo, nx0);
#ifdef APM_MEASURE
        if (APM_SKIP(a, 1)) hits = 0;
#endif
        if constexpr (LEAN) return hits;
        else return cc < nch ? hits : 0u;
    };

    // ---- CODE FILTER (see ApmSieve2Args::cf_image): which of the block's lookup hits can be a nomination at all ----
    const uint2 *cf_tbl = reinterpret_cast<const uint2 *>(smem + 32768);
    const uint2 *cf_rrec = reinterpret_cast<const uint2 *>(smem + 32768 + a.cf_o_rrec);
    const uint2 *cf_lrec = reinterpret_cast<const uint2 *>(smem + 32768 + a.cf_o_lrec);
    uint32_t *st = reinterpret_cast<uint32_t *>(smem + 32768 + a.cf_len + wv * WAVE_BYTES); // the block's codes: dword 0 =
                                                                 // the 16 bytes in front, 1..256 the block, 257..258 the 32 behind, 259 zero
    uint32_t *mk = st + 260;                                     // surviving hit masks, one dword per lane
    uint16_t *rq = reinterpret_cast<uint16_t *>(mk + 64);        // ring of hits: even position / 2 inside the block | 2048: the odd position only
    uint16_t *pend = rq + 128;                                   // DP: the block's pending window-DP entries: position inside the block | slot << 13
    const uint4 *cf_dp = reinterpret_cast<const uint4 *>(smem + 32768 + a.cf_o_dp); // DP: slot table
    // DP: the wave's queue of window-DP entries, lane i holds entry i < qn (wave-uniform): qe = the pair index (relative position
    // / 2, the list entry it becomes; ~0u: dropped), qlo | qhi = codes of the text region from its first byte on (code i in bits
    // 2i.. of the 64 bits, codes 0 .. APM_CF_DP_COLS - 1), bits 28..30 of qhi = the slot.  Entries are reserved in the region.
    uint32_t qe = 0, qlo = 0, qhi = 0, qn = 0;
    // DP: run the window DP on the queue (a wave of entries from several blocks, whose masks have left); what passes leaves as
    // list entries, ONE per pair index (the verify launch identifies every unit at both positions of a pair itself, and its
    // stateless dedup would count a window twice from two entries), and the reservations of the rest are given back
    auto dp_flush = [&]() __attribute__((always_inline)) {
        const bool valid = (uint32_t)lane < qn && qe != 0xffffffffu;
        bool keep = false;
#ifdef APM_MEASURE
        if (APM_SKIP(a, 4)) keep = valid; // (the predicate is not run at all: with bit 2, what the column loop costs)
        else
#endif
        if (valid) {
            const uint4 tb = cf_dp[(qhi >> 28) & 7u];
            if constexpr (DIAG) { // (the codes become bit planes here, once per flush: the queue keeps the two dwords of the column form)
                uint32_t t0, t1;
                apm_code_planes(qlo, qhi & 0x0fffffffu, t0, t1);
                keep = a.cf_dp_k >= 2 ? apm_code_dp_diag<1>(tb.x, tb.y, (int)(tb.z & 0xffu), t0, t1, a.cf_dp_k)
                                      : apm_code_dp_diag<0>(tb.x, tb.y, (int)(tb.z & 0xffu), t0, t1, a.cf_dp_k);
            } else {
                const uint32_t cw[2] = {qlo, qhi};
                keep = apm_code_dp_pass<2>(tb.x, tb.y, (int)(tb.z & 0xffu), cw, a.cf_dp_cols, a.cf_dp_k);
            }
        }
#ifdef APM_MEASURE
        if (APM_SKIP(a, 2)) keep = valid;
#endif
        for (unsigned long long sm = __builtin_amdgcn_ballot_w64(keep); sm;) { // (entries of one pair: both positions, several units)
            const int l = __builtin_ctzll(sm);
            const uint32_t el = (uint32_t)__builtin_amdgcn_readlane((int)qe, l);
            if (keep && qe == el && lane != l) keep = false;
            sm = __builtin_amdgcn_ballot_w64(keep) & ~((2ull << l) - 1ull);
        }
        const unsigned long long km = __builtin_amdgcn_ballot_w64(keep);
        const uint32_t nk = (uint32_t)__builtin_popcountll(km);
        uint32_t base = 0;
        if (lane == 0) {
            if (qn > nk) __hip_atomic_fetch_sub(&cl_ctr[1], qn - nk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (nk) base = __hip_atomic_fetch_add(&cl_ctr[0], nk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if (keep) a.clist[(size_t)blockIdx.x * a.clist_cap + base + apm_wave_rank(km)] = qe;
        qn = 0;
    };
    // hm: the lane's hit mask of the block (bit 8 j + t = lookup t of chunk j); sc[j]: the codes of its 16 bytes of chunk j;
    // hc: codes of the halo bytes this lane loaded.  Returns the mask of the hits that pass the filter.
    // e0: pair index of the block's first position (DP: what queue entries are numbered from)
    auto cf_filter = [&](uint32_t hm, const uint32_t (&sc)[4], uint32_t hc, uint32_t e0) __attribute__((always_inline)) -> uint32_t {
        if (!__builtin_amdgcn_ballot_w64(hm != 0u)) return 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) st[1 + 64 * j + lane] = sc[j];
        if (lane < 4) st[lane < 2 ? 257 + lane : (lane == 2 ? 0 : 259)] = hc;
        mk[lane] = 0u;
        uint32_t qh = 0, qt = 0; // wave-uniform: the ring holds entries [qh, qt)
        uint32_t pn = 0;         // DP, wave-uniform: entries of the pending list
        // nb <= 64 hits, one per lane.  A hit stands for the even position and the odd one behind it: both 16-bit words
        // are looked up; the lane follows the even one if it is a key word, else the odd one; when both are, the odd
        // one goes back into the ring as an entry of its own (rare).
        // Up to 32 hits (most blocks of a sparse set, and the last batch of any block): lanes 0..31 take the even position of
        // entry L, lanes 32..63 the odd one of entry L - 32 -- nothing goes back into the ring, no straggler batch for a
        // handful of odd positions (the both-parities case is common: a unit that tolerates an indel has its neighbour words
        // set too; it cost cfg3 a second batch per block).
        auto run_batch = [&](uint32_t nb) __attribute__((always_inline)) {
#ifdef APM_MEASURE
            if (APM_SKIP(a, 4096)) return; // (the batches do nothing: what is left above bit 1 is strip, prefix scan and ring)
#endif
            const bool split = nb <= 32u; // (wave-uniform)
            const uint32_t ei = split ? ((uint32_t)lane & 31u) : (uint32_t)lane;
            const uint32_t ent = rq[(qh + ei) & 127u];
            const bool valid = ei < nb;
            const bool take0 = !split || lane < 32, take1 = !split || lane >= 32;
            const uint32_t se = 2u * (ent & 2047u), d = 1u + (se >> 4), she = 2u * (se & 15u); // even byte position inside the block
            const uint32_t w0 = st[d], w1 = st[d + 1u];
            const uint32_t x0 = __builtin_amdgcn_alignbit(w1, w0, she) & 0xffffu, x1 = __builtin_amdgcn_alignbit(w1, w0, she + 2u) & 0xffffu;
            const uint2 t0 = cf_tbl[x0 & 2047u], t1 = cf_tbl[x1 & 2047u];
            const bool p0 = valid && take0 && !(ent & 2048u) && ((t0.x >> (x0 >> 11)) & 1u), p1 = valid && take1 && ((t1.x >> (x1 >> 11)) & 1u);
            const unsigned long long both = __builtin_amdgcn_ballot_w64(p0 && p1);
            if (both) { // the odd position waits for a later batch (the ring has room: at most 63 + 64 entries are ever pending)
                const uint32_t idx = qt + apm_wave_rank(both);
                if (p0 && p1) rq[idx & 127u] = (uint16_t)(ent | 2048u);
                qt += (uint32_t)__builtin_popcountll(both);
            }
            bool act = p0 || p1;
            const uint32_t s = se + (p0 ? 0u : 1u); // the position this lane judges
            const uint32_t c0 = __builtin_amdgcn_alignbit(w1, w0, she + (p0 ? 0u : 2u)); // codes of the 16 bytes from s on
            const uint32_t x = p0 ? x0 : x1, word = p0 ? t0.x : t1.x, pre = p0 ? t0.y : t1.y, bit = x >> 11;
            uint2 rec = cf_rrec[act ? pre + (uint32_t)__builtin_popcount(word & ((1u << bit) - 1u)) : 0u];
            uint32_t li = 0; // index of the next record of the word's key list
            bool in_list = false;
            if ((rec.x >> 30) == 3u) { li = rec.x & 0xffffu; in_list = true; rec = cf_lrec[li]; ++li; }
            while (__builtin_amdgcn_ballot_w64(act)) {
                const uint32_t side = rec.x >> 30;
                const uint32_t uu = side == 2u ? s : s + 16u + ((rec.y >> 20) & 0xffu); // 16 + the partner's text position
                const bool vis = uu <= 4128u;
                const uint32_t ua = vis ? uu : 16u;
                uint32_t tw = __builtin_amdgcn_alignbit(st[(ua >> 4) + 1u], st[ua >> 4], 2u * (ua & 15u));
                if (side == 2u) tw = apm_rev_codes(tw);
                const bool ok = apm_cf_pass(rec.x, rec.y, c0, tw, vis);
                bool pass = act && ok;
                if constexpr (DP) {
                    // a unit of a short pattern (its record has a slot): noted in the block's pending list instead of its bit
                    // going into the mask, and the lane walks on through the word's list (a later unit may still pass outright).
                    // The block's end makes queue entries of the notes.  A full pending list: the bit.
                    const uint32_t slot = (rec.y >> 28) & 7u;
                    const bool want = pass && slot != 0u;
                    const unsigned long long wm = __builtin_amdgcn_ballot_w64(want);
                    if (wm) {
                        const uint32_t idx = pn + apm_wave_rank(wm);
                        if (want && idx < 64u) { pend[idx] = (uint16_t)(s | (slot << 13)); pass = false; }
                        pn += (uint32_t)__builtin_popcountll(wm);
                        pn = pn < 64u ? pn : 64u;
                    }
                }
                if (pass) {
                    atomicOr(&mk[(s >> 4) & 63u], 1u << (8u * (s >> 10) + ((s & 15u) >> 1)));
                    act = false;
                } else if (act) {
                    if (!in_list || (rec.y >> 31)) act = false;
                    else { rec = cf_lrec[li]; ++li; }
                }
            }
        };
        // Where the hits go in the ring: a wave prefix sum over the lanes' hit counts (apm_wave_incl_scan), then every lane writes
        // its own hits one after the other -- a round is ctz + store, not ballot + mbcnt + popcount (cfg5: five rounds per
        // block).  The ring is empty here and holds 128; a fuller block takes the round-by-round form below.
        {
            const uint32_t cnt = (uint32_t)__builtin_popcount(hm);
            const uint32_t inc = apm_wave_incl_scan(cnt);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            if (total <= 128u) { // (wave-uniform)
                uint32_t pos = inc - cnt; // (qt == qh == 0: the ring was drained by the block before)
                while (__builtin_amdgcn_ballot_w64(hm != 0u)) {
                    if (hm != 0u) {
                        const uint32_t t = (uint32_t)__builtin_ctz(hm);
                        hm &= hm - 1u;
                        rq[pos & 127u] = (uint16_t)(512u * (t >> 3) + 8u * (uint32_t)lane + (t & 7u));
                        ++pos;
                    }
                }
                qt = total;
                while (qt - qh >= 64u) { run_batch(64u); qh += 64u; }
            }
        }
        while (__builtin_amdgcn_ballot_w64(hm != 0u)) {
            const bool has = hm != 0u;
            const uint32_t t = has ? (uint32_t)__builtin_ctz(hm) : 0u;
            hm &= hm - 1u;
            apm_wave_append(rq, qt, has, 512u * (t >> 3) + 8u * (uint32_t)lane + (t & 7u), 127u);
            while (qt - qh >= 64u) { run_batch(64u); qh += 64u; }
        }
        while (qt != qh) { const uint32_t nb = qt - qh < 64u ? qt - qh : 64u; run_batch(nb); qh += nb; }
        if constexpr (DP) {
            // The block's pending entries join the queue, all at once: the mask is final, the strip still holds the block.  One
            // reservation in the list region for all of them (lane 0, ahead of the reads that hide its latency); a queue that
            // cannot take them runs the DP first.  Lane qn + i reads pending entry i and builds queue entry qn + i itself.
#ifdef APM_MEASURE
            if (APM_SKIP(a, 8192)) pn = 0; // (the pending entries are dropped: no hand-over at the block's end, no flush)
#endif
            if (pn) {
                if (qn + pn > 64u) dp_flush();
                uint32_t room = 0;
                if (lane == 0) room = __hip_atomic_fetch_add(&cl_ctr[1], pn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + pn <= a.clist_cap;
                const uint32_t pi = (uint32_t)lane - qn;
                const bool mine = pi < pn;
                const uint32_t ent = pend[mine ? pi : 0u];
                const uint32_t s = ent & 8191u, slot = ent >> 13;
                const uint32_t info = cf_dp[slot].z;
                // region start inside the block and its length: [s - off - k, s - off + m + k); DIAG: k / 2 in place of k
                const int rk = DIAG ? a.cf_dp_k >> 1 : a.cf_dp_k;
                const int r = (int)s - (int)((info >> 8) & 0xffu) - rk;
                const int rlen = DIAG ? (int)(info & 0xffu) + 2 * rk : (int)(info >> 16);
                const bool inside = r >= -16 && r + rlen <= 4128; // (the region lies in the code strip)
                const uint32_t u = (uint32_t)(r + 16), d = inside ? u >> 4 : 0u, sh = 2u * (u & 15u);
                const uint32_t w0 = st[d], w1 = st[d + 1u], w2 = st[d + 2u];
                const uint32_t lo = __builtin_amdgcn_alignbit(w1, w0, sh);
                const uint32_t hi = (__builtin_amdgcn_alignbit(w2, w1, sh) & 0x0fffffffu) | (slot << 28);
                room = (uint32_t)__builtin_amdgcn_readfirstlane((int)room);
                if (!room && lane == 0) __hip_atomic_fetch_sub(&cl_ctr[1], pn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // the bit, as before: for a region that leaves the strip, and for all of them when the list region is full
                uint32_t *mw = &mk[(s >> 4) & 63u];
                const uint32_t mbit = 1u << (8u * (s >> 10) + ((s & 15u) >> 1));
                if (mine && !(room && inside)) atomicOr(mw, mbit);
                if (room) { // an entry whose pair has its bit in the mask (its own or another unit's) is dropped: list or row, never both
                    const bool drop = (*mw & mbit) != 0u;
                    if (mine) {
                        qe = drop ? 0xffffffffu : e0 + (s >> 1);
                        qlo = lo;
                        qhi = hi;
                    }
                    qn += pn;
                }
            }
        }
        return mk[lane];
    };

    // the wave's non-empty blocks (ApmSieve2Args::blist): lane i holds the i-th pending block number
    uint32_t bl_pend = 0, bl_n = 0; // (bl_n wave-uniform)
    auto bl_flush = [&]() __attribute__((always_inline)) {
        uint32_t base = 0;
        if (lane == 0) base = __hip_atomic_fetch_add(a.blist_ctr, bl_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        if ((uint32_t)lane < bl_n) a.blist[base + (uint32_t)lane] = bl_pend;
        bl_n = 0;
    };
    if (CF && a.blist && blockIdx.x == 0 && tid == 0) *a.blist_ctr_next = 0u; // (nobody counts in the other set during this launch)

    int64_t c = ((int64_t)blockIdx.x * (THREADS / 64) + wv) * 4; // four neighbouring chunks per wave
    u32x4 r0, r1, r2, r3, hl;
    v2u32 tl;
    load_chunk(c, r0);
    load_chunk(c + 1, r1);
    load_chunk(c + 2, r2);
    load_chunk(c + 3, r3);
    if constexpr (CF) load_halo(c, hl);
    else load_tail(c + 4, tl);
    for (; c < nch; c += 4 * W) {
        const uint32_t s0 = pack16(r0), s1 = pack16(r1), s2 = pack16(r2), s3 = pack16(r3);
        uint32_t s4;
        if constexpr (CF) s4 = pack16(hl); // (lane 0: the low half = the 8 bytes behind the block)
        else s4 = apm_pack4(tl.x, cs) | (apm_pack4(tl.y, cs) << 8);
        load_chunk(c + 4 * W, r0);
        load_chunk(c + 4 * W + 1, r1);
        load_chunk(c + 4 * W + 2, r2);
        load_chunk(c + 4 * W + 3, r3);
        if constexpr (CF) load_halo(c + 4 * W, hl);
        else load_tail(c + 4 * W + 4, tl);
        // (chunk by chunk: letting the scheduler interleave the 32 lookups costs more registers than the 8 waves per SIMD leave)
        const uint32_t h0 = hit_bits(s0, (uint32_t)__builtin_amdgcn_readfirstlane((int)s1), c);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t h1 = hit_bits(s1, (uint32_t)__builtin_amdgcn_readfirstlane((int)s2), c + 1);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t h2 = hit_bits(s2, (uint32_t)__builtin_amdgcn_readfirstlane((int)s3), c + 2);
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t h3 = hit_bits(s3, (uint32_t)__builtin_amdgcn_readfirstlane((int)s4), c + 3);
        // the block's hit masks: one coalesced 256-byte store per wave and 4 KiB (see ApmSieve2Args::masks)
        uint32_t hm = (h0 >> 24) | ((h1 >> 24) << 8) | ((h2 >> 24) << 16) | (h3 & 0xff000000u);
        if constexpr (LEAN) {
            // The hits of a chunk behind the scanned range are dropped: chunk j is byte j of the mask, and `left`, the block's
            // chunks inside the range (>= 1 in here; a shard holds fewer than 2^22 chunks, see rs_all), is the wave's: a scalar
            // mask and one AND per block, not a 64-bit vector compare and a select per chunk.
            const uint32_t left = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(nch - c));
            hm &= left >= 4u ? 0xffffffffu : (1u << (8u * left)) - 1u;
        }
        if constexpr (CF) {
            const uint32_t e0b = (uint32_t)((a.tile0 + (c >> 2) * 4096) >> 1); // pair index of the block's first position
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t sc[4] = {s0, s1, s2, s3};
            hm = cf_filter(hm, sc, s4, e0b);
        }
        if constexpr (CF) {
            if (a.clist) { // the survivors leave as list entries, one round per bit of the fullest lane
                const uint32_t e0 = (uint32_t)((a.tile0 + (c >> 2) * 4096) >> 1) + 8u * (uint32_t)lane;
                uint32_t *region = a.clist + (size_t)blockIdx.x * a.clist_cap;
                for (;;) {
                    const bool has = hm != 0u;
                    const unsigned long long mask = __builtin_amdgcn_ballot_w64(has);
                    if (!mask) break;
                    const uint32_t n = (uint32_t)__builtin_popcountll(mask);
                    uint32_t base = 0;
                    if constexpr (DP) { // reserve, then take write positions (see cl_ctr)
                        uint32_t fits = 0;
                        if (lane == 0) {
                            const uint32_t old = __hip_atomic_fetch_add(&cl_ctr[1], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            fits = old + n <= a.clist_cap;
                            if (fits) base = __hip_atomic_fetch_add(&cl_ctr[0], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            else __hip_atomic_fetch_sub(&cl_ctr[1], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                        if (!__builtin_amdgcn_readfirstlane((int)fits)) break; // region full: the rest of the block takes the mask row
                    } else {
                        if (lane == 0) base = __hip_atomic_fetch_add(&cl_ctr[0], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                        if (base + n > a.clist_cap) { // region full: the reservations before this one are the region's entries
                            if (lane == 0) __hip_atomic_fetch_min(&cl_ctr[1], base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            break;
                        }
                    }
                    const uint32_t t = has ? (uint32_t)__builtin_ctz(hm) : 0u;
                    hm &= hm - 1u;
                    if (has)
                        region[base + apm_wave_rank(mask)] = e0 + 512u * (t >> 3) + (t & 7u);
                }
            }
            // the mask row (all of it without a list, what did not fit with one) and the block's entry in the block list
            const bool any = __builtin_amdgcn_ballot_w64(hm != 0u) != 0ull;
            if (!a.clist || any) a.masks[(size_t)(c >> 2) * 64 + (size_t)lane] = hm;
            if (a.blist && any) {
                if ((uint32_t)lane == bl_n) bl_pend = (uint32_t)(c >> 2);
                if (++bl_n == 64u) bl_flush();
            }
        } else {
            a.masks[(size_t)(c >> 2) * 64 + (size_t)lane] = hm; // (without the filter nearly every block has hits: no list)
        }
    }
    if (DP && qn) dp_flush();
    if constexpr (CF) {
        // what is left pending when the wave's run ends leaves with ONE atomic per WORKGROUP: the waves of a launch end
        // together, and 8192 of them adding to one counter took 0.09 ms -- twice the whole sieve of a 256 MiB text (round 3
        // measurement; the adds serialise at ~90 per microsecond).  The per-wave code strips are free by now: each wave
        // parks its pending numbers in its own, thread t then copies entry t % 64 of wave t / 64.
        if (a.blist) { // (workgroup-uniform)
            if ((uint32_t)lane < bl_n) st[lane] = bl_pend;
            if (lane == 0) st[64] = bl_n;
            __syncthreads();
            uint32_t *wg = reinterpret_cast<uint32_t *>(smem + 32768 + a.cf_len); // wave w's strip: wg + w * (WAVE_BYTES / 4)
            const uint32_t nw = (uint32_t)(THREADS / 64);
            uint32_t before = 0, total = 0;
            for (uint32_t w = 0; w < nw; ++w) {
                const uint32_t cw = wg[w * (WAVE_BYTES / 4) + 64];
                if (w < (uint32_t)wv) before += cw;
                total += cw;
            }
            uint32_t *gbase = wg + 65; // (wave 0's strip, behind its own entries)
            if (tid == 0 && total) *gbase = __hip_atomic_fetch_add(a.blist_ctr, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (POOL) {
                // POOLED hand-over (ApmSieve2PoolArgs): the region's entries are final behind the first barrier (every wave has run
                // its last dp_flush); the place in the pool is reserved here, with the block list's, one atomic per workgroup, none
                // for an empty region, and handed round through the same strip
                if (a.cpool && tid == 0) {
                    const uint32_t n = cl_ctr[0];
                    if (n) wg[66] = __hip_atomic_fetch_add(&a.cpool_cnt[blockIdx.x % (uint32_t)a.cpool_n], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __syncthreads();
            if ((uint32_t)lane < bl_n) a.blist[*gbase + before + (uint32_t)lane] = bl_pend;
            if (a.clist && tid == 0) a.clist_cnt[blockIdx.x] = DP ? cl_ctr[0] : (cl_ctr[0] < cl_ctr[1] ? cl_ctr[0] : cl_ctr[1]); // (behind the barrier: every wave has made its reservations)
            if constexpr (POOL) {
                if (a.cpool) { // (workgroup-uniform)
                    const uint32_t n = cl_ctr[0] < a.clist_cap ? cl_ctr[0] : a.clist_cap; // (never above: an entry is reserved before it is written)
                    const uint32_t *region = a.clist + (size_t)blockIdx.x * a.clist_cap;
                    uint32_t *pool = a.cpool + (size_t)(blockIdx.x % (uint32_t)a.cpool_n) * a.cpool_cap + (n ? wg[66] : 0u);
                    // The entries were stored by the other waves of the workgroup, each ahead of the barrier (which waits for the
                    // wave's stores).  Read with relaxed atomic loads of agent scope: they are served by L2, where those stores
                    // went (the vector L1 writes through), never by a line this CU's L1 may hold from before the store.
                    for (uint32_t i = (uint32_t)tid; i < n; i += (uint32_t)THREADS)
                        pool[i] = __hip_atomic_load(&region[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    // (nobody counts in the other set of pool counters during this launch)
                    if (blockIdx.x == 0)
                        for (int i = tid; i < a.cpool_next_n; i += THREADS) a.cpool_cnt_next[i] = 0u;
                }
            }
        }
    }
}

#endif /* APM_SIEVE_BODY_H */
