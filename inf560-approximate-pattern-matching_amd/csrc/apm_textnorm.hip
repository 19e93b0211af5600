/*
 * apm_textnorm.hip -- the text-normalisation pass (apm_normalize_device) and the position map behind it
 * (apm_map_positions_device); the arithmetic and the layout of the source are apm_textnorm.h's.
 *
 * Three launches turn the source bytes into the kept bytes, none of which waits on another workgroup:
 *   summary  one wavefront per 4 KiB block: the block's kept count and outgoing header state for both incoming states
 *   scan     ONE workgroup composes the summaries in order (apm_tn_fn_then) and writes the map: kept bytes in front of
 *            every block, its incoming state in bit 63, the total behind the last block
 *   scatter  one wavefront per block: the masks again with the state now known, the kept bytes compacted in LDS at the
 *            destination's own 16-byte phase, written with 16-byte stores and a byte-wise head and tail
 * The fourth kernel maps record positions back: a 64-way search of the map for the block, then the select of the
 * (pos - prefix)-th kept byte inside it.
 */
#include "apm_wave.h"
#include "apm_textnorm.h"

#include <algorithm>

namespace {

constexpr uint32_t TN_SCAN_THREADS = 1024, TN_SCAN_PER_THREAD = 4, TN_SCAN_CHUNK = TN_SCAN_THREADS * TN_SCAN_PER_THREAD;

// ---- 1. summary ----
__global__ __launch_bounds__(APM_BLOCK) void apm_tn_summary_kernel(const ApmTnArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * APM_BLOCK + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * APM_BLOCK) >> 6;
    for (uint64_t b = wave; b < a.src.n_blocks; b += n_waves) {
        uint32_t w[4][4], valid[4];
        tn_load_block(a.src, b, lane, w, valid);
        uint32_t ls = tn_block_line_start(a.src, b);
        uint32_t h0 = 0u, h1 = 1u, acc = 0u; // the block entered outside / inside a header; the lane's counts, 16 bits each
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const TnChunk t = tn_chunk(w[c], valid[c], a.src.flags, lane, ls);
            const uint32_t in0 = apm_tn_state_at(t.fixed, t.value, lane, h0), in1 = apm_tn_state_at(t.fixed, t.value, lane, h1);
            acc += apm_tn_resolve(t.m, valid[c], a.src.flags, in0, t.ls_in).count;
            acc += apm_tn_resolve(t.m, valid[c], a.src.flags, in1, t.ls_in).count << 16;
            h0 = apm_tn_state_at(t.fixed, t.value, 64u, h0);
            h1 = apm_tn_state_at(t.fixed, t.value, 64u, h1);
        }
        const uint32_t sum = apm_wave_incl_scan(acc); // (at most 4096 per half: no carry between them)
        if (lane == 63u) a.summary[b] = apm_tn_pack_summary(sum & 0xffffu, sum >> 16, h0, h1);
    }
}

// ---- 2. scan: one workgroup ----
__device__ __forceinline__ ApmTnFn tn_fn_shfl_up(const ApmTnFn &f, int d) {
    ApmTnFn o;
    o.e[0] = (uint32_t)__shfl_up((int)f.e[0], d);
    o.e[1] = (uint32_t)__shfl_up((int)f.e[1], d);
    return o;
}

__global__ __launch_bounds__(TN_SCAN_THREADS) void apm_tn_scan_kernel(const ApmTnArgs a) {
    __shared__ uint32_t s_wave[2][TN_SCAN_THREADS / 64][2]; // the waves' compositions, two iterations' worth
    const uint64_t nb = a.src.n_blocks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 *sum4 = reinterpret_cast<const uint4 *>(a.summary); // (allocated in whole scan chunks)
    unsigned long long before = 0ull; // kept bytes in front of the chunk
    uint32_t state = 0u, par = 0u;    // header state the chunk is entered in
    uint4 cur = nb ? sum4[tid] : make_uint4(0u, 0u, 0u, 0u);
    for (uint64_t c0 = 0; c0 < nb; c0 += TN_SCAN_CHUNK, par ^= 1u) {
        const uint64_t i0 = c0 + (uint64_t)tid * TN_SCAN_PER_THREAD;
        uint4 nxt = cur;
        if (c0 + TN_SCAN_CHUNK < nb) nxt = sum4[(c0 + TN_SCAN_CHUNK) / TN_SCAN_PER_THREAD + tid]; // (in flight over this chunk's scan)
        const uint32_t raw[4] = {cur.x, cur.y, cur.z, cur.w};
        ApmTnFn f[4], incl = apm_tn_fn_identity();
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            f[q] = i0 + q < nb ? apm_tn_fn_of(raw[q]) : apm_tn_fn_identity();
            incl = apm_tn_fn_then(incl, f[q]);
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { // inclusive over the wave
            const ApmTnFn o = tn_fn_shfl_up(incl, d);
            if ((int)lane >= d) incl = apm_tn_fn_then(o, incl);
        }
        if (lane == 63u) { s_wave[par][wave][0] = incl.e[0]; s_wave[par][wave][1] = incl.e[1]; }
        __syncthreads();
        ApmTnFn lower = apm_tn_fn_identity(), all = apm_tn_fn_identity(); // the waves below this one; the whole chunk
        for (uint32_t v = 0; v < TN_SCAN_THREADS / 64; ++v) {
            if (v == wave) lower = all;
            ApmTnFn g;
            g.e[0] = s_wave[par][v][0];
            g.e[1] = s_wave[par][v][1];
            all = apm_tn_fn_then(all, g);
        }
        const ApmTnFn up = tn_fn_shfl_up(incl, 1);
        ApmTnFn ex = lane ? apm_tn_fn_then(lower, up) : lower; // the chunk's blocks in front of this thread's
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (i0 + q < nb) a.map[i0 + q] = apm_tn_map_entry(before, state, ex);
            ex = apm_tn_fn_then(ex, f[q]);
        }
        const uint32_t e = state ? all.e[1] : all.e[0];
        before += e & 0x7fffffffu;
        state = e >> 31;
        cur = nxt;
    }
    if (tid == 0) {
        a.map[nb] = before;
        *a.total = before;
    }
}

// ---- 3. scatter: one wavefront = one workgroup per block ----
__global__ __launch_bounds__(64) void apm_tn_scatter_kernel(const ApmTnArgs a) {
    __shared__ uint4 s_img[(APM_TN_BLOCK + 32u) / 16u]; // the block's kept bytes, image offset q <-> (dst + prefix - pad)[q]
    uint8_t *s_out = reinterpret_cast<uint8_t *>(s_img);
    const uint32_t lane = threadIdx.x;
    for (uint64_t b = blockIdx.x; b < a.src.n_blocks; b += gridDim.x) {
        const unsigned long long e = a.map[b];
        uint8_t *out = a.dst + (e & APM_TN_PREFIX_MASK);
        const uint32_t pad = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
        uint32_t w[4][4], valid[4];
        tn_load_block(a.src, b, lane, w, valid);
        uint32_t ls = tn_block_line_start(a.src, b);
        uint32_t h = (uint32_t)(e >> APM_TN_STATE_BIT), run = pad;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const TnChunk t = tn_chunk(w[c], valid[c], a.src.flags, lane, ls);
            const ApmTnLane r = apm_tn_resolve(t.m, valid[c], a.src.flags, apm_tn_state_at(t.fixed, t.value, lane, h), t.ls_in);
            const uint32_t incl = apm_wave_incl_scan(r.count);
            uint32_t at = run + incl - r.count;
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                uint32_t x = w[c][i >> 2];
                if (a.src.flags & APM_TN_UPPER) x = apm_tn_upper4(x);
                if ((r.keep >> i) & 1u) s_out[at++] = (uint8_t)(x >> (8u * (i & 3u)));
            }
            run += tn_wave_total(incl);
            h = apm_tn_state_at(t.fixed, t.value, 64u, h);
        }
        __syncthreads();
        // image [pad, run) -> out - pad + [pad, run): whole 16-byte units in the middle, bytes in front and behind
        uint8_t *al = out - pad; // (16-byte aligned; nothing in front of `out` is touched)
        const uint32_t q0 = (pad + 15u) & ~15u, q1 = run & ~15u;
        const uint32_t head_end = min(q0, run), tail = max(q1, head_end);
        if (pad + lane < head_end) al[pad + lane] = s_out[pad + lane];
        for (uint32_t u = (q0 >> 4) + lane; u < (q1 >> 4); u += 64u) reinterpret_cast<uint4 *>(al)[u] = s_img[u];
        if (tail + lane < run) al[tail + lane] = s_out[tail + lane];
        __syncthreads(); // (the image is the next block's)
    }
}

// ---- 4. map: one wavefront per record ----
__global__ __launch_bounds__(APM_BLOCK) void apm_tn_map_kernel(const ApmTnMapArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * APM_BLOCK + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * APM_BLOCK) >> 6;
    const unsigned long long have = *a.n_rec, n = have < a.cap ? have : a.cap;
    const uint64_t nb = a.src.n_blocks;
    const unsigned long long total = a.map[nb];
    for (unsigned long long r = wave; r < n; r += n_waves) {
        const uint4 rec = a.rec[r];
        const unsigned long long pos = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)rec.x) |
                                       ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)rec.y) << 32);
        if (pos >= total) continue; // (names no byte of the normalised text: left as it is)
        // the largest b with prefix[b] <= pos, 64 probes a round: prefix[lo] <= pos < prefix[hi] throughout
        uint64_t lo = 0, hi = nb;
        while (hi - lo > 1) {
            const uint64_t step = (hi - lo + 63u) >> 6, idx = lo + lane * step;
            const bool ok = idx < hi && (a.map[idx] & APM_TN_PREFIX_MASK) <= pos;
            const uint64_t j = (uint64_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok)) - 1u; // (lane 0 always holds)
            lo += j * step;
            hi = hi < lo + step ? hi : lo + step;
        }
        const unsigned long long e = a.map[lo];
        const uint32_t want = (uint32_t)(pos - (e & APM_TN_PREFIX_MASK)); // the want-th kept byte of block lo
        uint32_t w[4][4], valid[4];
        tn_load_block(a.src, lo, lane, w, valid);
        uint32_t ls = tn_block_line_start(a.src, lo);
        uint32_t h = (uint32_t)(e >> APM_TN_STATE_BIT), run = 0u;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const TnChunk t = tn_chunk(w[c], valid[c], a.src.flags, lane, ls);
            const ApmTnLane res = apm_tn_resolve(t.m, valid[c], a.src.flags, apm_tn_state_at(t.fixed, t.value, lane, h), t.ls_in);
            const uint32_t incl = apm_wave_incl_scan(res.count);
            const uint32_t first = run + incl - res.count;
            if (want >= first && want < run + incl) {
                const uint64_t at = lo * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u + apm_tn_select16(res.keep, want - first);
                reinterpret_cast<unsigned long long *>(a.rec)[2 * r] = at - a.src.lead;
            }
            run += tn_wave_total(incl);
            h = apm_tn_state_at(t.fixed, t.value, 64u, h);
        }
    }
}

} // namespace

// fixed grids sized from the CU count; every kernel strides over its blocks or records
hipError_t apm_launch_tn_summary(const ApmTnArgs &a, int n_cu, hipStream_t s) {
    const uint64_t want = (a.src.n_blocks + APM_BLOCK / 64 - 1) / (APM_BLOCK / 64);
    hipLaunchKernelGGL(apm_tn_summary_kernel, dim3((unsigned)std::min<uint64_t>(want, (uint64_t)n_cu * 8u)), dim3(APM_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t apm_launch_tn_scan(const ApmTnArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(apm_tn_scan_kernel, dim3(1), dim3(TN_SCAN_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t apm_launch_tn_scatter(const ApmTnArgs &a, int n_cu, hipStream_t s) {
    hipLaunchKernelGGL(apm_tn_scatter_kernel, dim3((unsigned)std::min<uint64_t>(a.src.n_blocks, (uint64_t)n_cu * 32u)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t apm_launch_tn_map(const ApmTnMapArgs &a, int n_cu, hipStream_t s) {
    hipLaunchKernelGGL(apm_tn_map_kernel, dim3((unsigned)n_cu * 8u), dim3(APM_BLOCK), 0, s, a);
    return hipGetLastError();
}
