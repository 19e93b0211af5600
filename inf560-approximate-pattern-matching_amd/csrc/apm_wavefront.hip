/*
 * apm_wavefront.hip -- the WAVEFRONT kernel: the Levenshtein sliding-window DP + per-pattern match count, one
 * anti-diagonal per step.
 *
 * Path replaced (reference file:line):
 *   levenshtein()            src/utils.c:76-99
 *   per-pattern scan loop    src/sequential.c:105-144
 *   (superseded GPU forms:   src/patterns_over_ranks.cu:19-73 ComputeMatches,
 *                            src/database_over_ranks.cu:20-134 searchPattern)
 *
 * Common shape of the tiled scan kernels (this one and BITPAR, apm_bitpar.h): one 256-thread workgroup owns a tile
 * of `tile` consecutive window starts.  It stages tile+halo bytes of text from
 * HBM into LDS with 16-byte coalesced loads ONCE, then runs every pattern of
 * the launch over the LDS copy (1 HBM byte per text position per launch,
 * independent of the number of patterns), reduces matches wave -> workgroup in
 * LDS and issues one 64-bit global atomic per (workgroup, pattern) that has
 * matches.
 */
#include "apm_internal.h"
#include "apm_core.h"
#include <type_traits>
#include "apm_device.h"

// lane l receives lane (l-1)'s value; lane 0 keeps `self` (DPP wave_shr:1, 1 VALU op)
__device__ __forceinline__ int apm_shift_up1(int v) {
    return __builtin_amdgcn_update_dpp(v, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, false);
}

// the same with lane 0 receiving zero: one v_mov_b32_dpp without the copy that keeps `self` (lane 0 is a row-0 lane of
// the wavefront kernel: it never uses what it receives)
__device__ __forceinline__ int apm_shift_up1z(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
}

// ---------------------------------------------------------------------------
// WAVEFRONT: the anti-diagonal kernel BASELINE.json's north_star names.
//
// A pattern of m rows is laid over Lm = ceil(m/R) lanes (R rows per lane);
// S = 64/Lm windows ("streams") sit side by side in one wave64 and advance in
// lockstep.  At step s the lane holding rows r0+1..r0+R works on text column
// x = s - y0 + 1 (y0 = its index inside the stream): the anti-diagonal.  The
// value cell(x, r0) it needs from the lane above was produced one step earlier
// and arrives through one DPP wave_shr:1 move (the "__shfl_up column passing");
// cell(x-1, r0) is last step's arrival.  All values are kept "+1" so that a
// cell costs v_cmp_eq, v_subb, v_min3, v_add.  Ramp-up (s < y0) is exec-masked;
// ramp-down garbage never flows back up.  The last lane of a stream finishes
// cell(m,m) exactly at the last step, m + Lm - 2.
// ---------------------------------------------------------------------------
// packed 16-bit lanes: every register holds the same DP cell of TWO adjacent windows (low / high
// half), so one v_pk_add_u16 / v_pk_min_u16 advances two cells (distances <= 257 fit 16 bits)
typedef unsigned short wf_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t wf_pk_add(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(wf_u16x2, a) + __builtin_bit_cast(wf_u16x2, b));
}
__device__ __forceinline__ uint32_t wf_pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(wf_u16x2, a), __builtin_bit_cast(wf_u16x2, b)));
}

template <int R>
__device__ __forceinline__ uint32_t wf_scan(const uint8_t *s_tile, const uint8_t *s_pat, int m, int k,
                                            int64_t base, int64_t jb, int64_t je_p, int tile, int wave, int lane,
                                            const ApmPosSink &ps, uint32_t pidx) {
    const int Lm = (m + R - 1) / R;
    const int S = 64 / Lm;
    const int sig = lane / Lm;
    const int y0 = lane - sig * Lm;
    const bool live = sig < S;
    const int r0 = y0 * R;
    constexpr uint32_t ONE2 = 0x00010001u;
    uint32_t pch2[R]; // pattern byte of row r0+i in both halves (rows past m: never equal to a text byte)
#pragma unroll
    for (int i = 0; i < R; ++i) pch2[i] = ((r0 + i < m) ? (uint32_t)s_pat[r0 + i] : (uint32_t)(0x100 + i)) * ONE2;
    const bool row0 = (y0 == 0);
    const bool is_res = live && (y0 == Lm - 1);
    const int ires = (m - 1) - (Lm - 1) * R;
    const int nsteps = m + Lm - 1;
    const uint32_t xbase2 = (uint32_t)(2 - y0) * ONE2; // + s*ONE2 = cell(x, 0) + 1 = x + 1 in both halves
    uint32_t one2 = ONE2;
    asm volatile("" : "+v"(one2)); // opaque: keeps min(x, 1) a single v_pk_min_u16 (LLVM would expand it to compares)
    uint32_t cnt = 0;

    for (int g0 = wave * 2 * S; g0 < tile; g0 += (APM_BLOCK / 64) * 2 * S) {
        const int joff = live ? g0 + 2 * sig : g0; // window A = joff (low half), window B = joff + 1 (high half)
        uint32_t cp[R];                            // cell(x-1, r) + 1, packed
#pragma unroll
        for (int i = 0; i < R; ++i) cp[i] = (uint32_t)(r0 + i + 2) * ONE2; // cell(0, r0+i+1) + 1
        uint32_t upprev = (uint32_t)(r0 + 1) * ONE2;                        // cell(0, r0) + 1
        const int cidx = joff - y0;
        // text: the lane keeps the two aligned dwords its column lies in and takes the bytes of windows A and B out of
        // them with ONE v_perm_b32 per step (selector bytes: column & 3 | 0x0c = zero); one aligned ds_read_b32 every
        // four steps, four steps ahead of its use -- no byte reads, no address arithmetic and no LDS wait in the step.
        // (columns in front of the tile occur on masked ramp-up steps only: their dwords are read from offset 0)
        const int cal = cidx & ~3;
        const uint32_t a0 = (uint32_t)(cidx - cal);
        const uint32_t sel0 = 0x0c000c00u | a0 | ((a0 + 1u) << 16); // step i of a block: + i * 0x00010001 (a0 + i + 1 <= 7)
        auto ld = [&](int addr) __attribute__((always_inline)) { return *reinterpret_cast<const uint32_t *>(s_tile + (addr < 0 ? 0 : addr)); };
        uint32_t lo, hi = ld(cal), nx = ld(cal + 4); // (nx: the dword of the NEXT block, on its way while this one is worked on)
        int nxt = cal + 8;

        auto step = [&](int s, uint32_t recv, uint32_t tch2) __attribute__((always_inline)) {
            uint32_t up = row0 ? xbase2 + (uint32_t)s * ONE2 : recv; // cell(x, r0) + 1
            uint32_t dg = upprev;                                    // cell(x-1, r0) + 1
            upprev = up;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const uint32_t left = cp[i];
                const uint32_t neq = wf_pk_min(tch2 ^ pch2[i], one2);            // 0/1 per half
                const uint32_t v = wf_pk_min(wf_pk_add(wf_pk_min(left, up), ONE2), // min(left, up) + 1
                                             wf_pk_add(dg, neq));                 // diag + neq
                dg = left;
                up = v;
                cp[i] = v;
            }
        };
        // MODE 0: every step of the block is a ramp-up step (lanes join one per step); 2: none is; 1: decided per step,
        // and the block may end early (the blocks around s = Lm - 1 and s = nsteps)
        auto block = [&](int s0, auto mode) __attribute__((always_inline)) {
            constexpr int MODE = decltype(mode)::value;
            lo = hi;
            hi = nx;
            nx = ld(nxt);
            nxt += 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int s = s0 + i;
                if (MODE == 1 && s >= nsteps) break;
                const uint32_t tch2 = __builtin_amdgcn_perm(hi, lo, sel0 + (uint32_t)i * 0x00010001u);
                const uint32_t recv = (uint32_t)apm_shift_up1z((int)cp[R - 1]);
                if (MODE == 0 || (MODE == 1 && s < Lm - 1)) {
                    if (s >= y0) step(s, recv, tch2);
                } else {
                    step(s, recv, tch2);
                }
            }
        };
        int s = 0;
        for (; s + 4 <= Lm - 1; s += 4) block(s, std::integral_constant<int, 0>());
        if (s < Lm - 1) { block(s, std::integral_constant<int, 1>()); s += 4; }
        for (; s + 4 <= nsteps; s += 4) block(s, std::integral_constant<int, 2>());
        if (s < nsteps) block(s, std::integral_constant<int, 1>());

        uint32_t res = cp[0];
#pragma unroll
        for (int i = 1; i < R; ++i)
            if (i == ires) res = cp[i];
        const int64_t jA = base + joff, jB = jA + 1;
        const uint32_t thr = (uint32_t)(k + 1);
#ifdef APM_REC
        const bool hitA = is_res && joff < tile && jA >= jb && jA < je_p && (res & 0xffffu) <= thr;
        const bool hitB = is_res && joff + 1 < tile && jB >= jb && jB < je_p && (res >> 16) <= thr;
        cnt += apm_wave_count(hitA);
        cnt += apm_wave_count(hitB);
        apm_rec_push_wave(ps, hitA, pidx, jA);
        apm_rec_push_wave(ps, hitB, pidx, jB);
#else
        cnt += apm_wave_count(is_res && joff < tile && jA >= jb && jA < je_p && (res & 0xffffu) <= thr);
        cnt += apm_wave_count(is_res && joff + 1 < tile && jB >= jb && jB < je_p && (res >> 16) <= thr);
#endif
    }
    return cnt;
}

__global__ __launch_bounds__(APM_BLOCK) void apm_wavefront_kernel(ApmScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile_bytes = (a.tile + a.halo + APM_TILE_SLACK + 15) & ~15;
    uint8_t *s_tile = smem;
    uint8_t *s_pat = smem + tile_bytes;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_pat + ((a.bytes_len + 15) & ~15));
    const int64_t base = a.tile0 + (int64_t)blockIdx.x * a.tile;

    for (int i = tid; i < a.bytes_len; i += APM_BLOCK) s_pat[i] = a.bytes[i];
    for (int i = tid; i < a.n_pats; i += APM_BLOCK) s_cnt[i] = 0u;
    const int nload = (a.tile + a.halo + 31) & ~15;
    for (int i = tid * 16; i < nload; i += APM_BLOCK * 16)
        *reinterpret_cast<uint4 *>(s_tile + i) = apm_load16_guarded(a.text, base + i, a.avail);
    __syncthreads();

    for (int p = 0; p < a.n_pats; ++p) {
        const ApmPatDesc d = a.pats[p];
        const int m = (int)d.m;
        const int64_t je_p = min(a.je, a.nrel - m + 1);
        const uint8_t *pat = s_pat + d.byte_off;
        uint32_t cnt;
        switch (d.w) {
        case 1: cnt = wf_scan<1>(s_tile, pat, m, a.k, base, a.jb, je_p, a.tile, wave, lane, a.pos, d.index); break;
        case 2: cnt = wf_scan<2>(s_tile, pat, m, a.k, base, a.jb, je_p, a.tile, wave, lane, a.pos, d.index); break;
        default: cnt = wf_scan<4>(s_tile, pat, m, a.k, base, a.jb, je_p, a.tile, wave, lane, a.pos, d.index); break;
        }
        if (lane == 0 && cnt) atomicAdd(&s_cnt[p], cnt);
    }
    __syncthreads();
    for (int i = tid; i < a.n_pats; i += APM_BLOCK) {
        const uint32_t c = s_cnt[i];
        if (c) atomicAdd(&a.counts[a.pats[i].index], (unsigned long long)c);
    }
}

size_t apm_wavefront_lds_bytes(const ApmScanArgs &a) {
    const size_t tile_bytes = (size_t)((a.tile + a.halo + APM_TILE_SLACK + 15) & ~15);
    return tile_bytes + (size_t)((a.bytes_len + 15) & ~15) + (size_t)a.n_pats * 4 + 16;
}

hipError_t apm_launch_wavefront(const ApmScanArgs &a, hipStream_t s) {
    const int64_t span = a.je - a.tile0;
    if (span <= 0 || a.n_pats <= 0) return hipSuccess;
    const int64_t nt = (span + a.tile - 1) / a.tile;
    if (nt > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(apm_wavefront_kernel, dim3((unsigned)nt), dim3(APM_BLOCK), apm_wavefront_lds_bytes(a), s, a);
    return hipGetLastError();
}
