/*
 * apm_generic.hip -- the small kernels that share nothing but apm_device.h: GENERIC (one DP column per lane, any pattern
 * length), the synthetic text fill, and TAIL (the truncated windows at the end of the text, m <= 128).
 */
#include "apm_internal.h"
#include "apm_core.h"
#include "apm_device.h"

// ---------------------------------------------------------------------------
// GENERIC: literal one-column DP per lane (the loop of utils.c:84-97 with the
// column in a per-thread slice of global scratch, interleaved so that lanes
// touch consecutive addresses).  Any m <= 65535; applies the end-of-text
// truncation of sequential.c:131-134.  Used for the <= m-1 truncated tail
// windows of every pattern and for patterns too long for the tiled kernels.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(APM_BLOCK) void apm_generic_kernel(ApmGenericArgs a) {
    const ApmPatDesc d = a.pats[blockIdx.y];
    const int m = (int)d.m;
    const uint8_t *pat = a.bytes + d.byte_off;
    const int64_t nthreads = (int64_t)gridDim.x * APM_BLOCK;
    const int64_t gtid = (int64_t)blockIdx.x * APM_BLOCK + threadIdx.x;
    uint16_t *col = a.scratch + (int64_t)blockIdx.y * a.col_stride * nthreads + gtid;
    const int64_t first_trunc = a.nrel - m + 1; // first window start that runs past the end of the text
    int64_t jb = a.jb, je = a.je;
    if (a.mode == 0) je = min(je, first_trunc);
    if (a.mode == 1) jb = max(jb, first_trunc);
    uint32_t cnt = 0;
    const int64_t span = je - jb;
    const int64_t rounds = span > 0 ? (span + nthreads - 1) / nthreads : 0;
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t j = jb + r * nthreads + gtid;
        bool hit = false;
        if (j < je) {
            const int64_t rem = a.nrel - j;
            const int size = rem < (int64_t)m ? (int)rem : m; // sequential.c:131-134
            for (int y = 0; y <= size; ++y) col[(int64_t)y * nthreads] = (uint16_t)y;
            for (int x = 1; x <= size; ++x) {
                const uint8_t tc = a.text[j + x - 1];
                int diag = x - 1;
                int up = x;
                col[0] = (uint16_t)x;
                for (int y = 1; y <= size; ++y) {
                    const int left = col[(int64_t)y * nthreads];
                    const int v = apm_min3(left + 1, up + 1, diag + (pat[y - 1] != tc ? 1 : 0));
                    col[(int64_t)y * nthreads] = (uint16_t)v;
                    diag = left;
                    up = v;
                }
            }
            hit = (int)col[(int64_t)size * nthreads] <= a.k;
#ifndef APM_REC
            if (a.pos.out && hit) apm_push_pos(a.pos, j);
#endif
        }
#ifdef APM_REC
        apm_rec_push_wave(a.pos, hit, d.index, j); // (rounds is the same for every lane: convergent)
#endif
        cnt += apm_wave_count(hit);
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&a.counts[d.index], (unsigned long long)cnt);
}

hipError_t apm_launch_generic(const ApmGenericArgs &a, int nbx, int n_pats, hipStream_t s) {
    if (a.je <= a.jb || n_pats <= 0) return hipSuccess;
    hipLaunchKernelGGL(apm_generic_kernel, dim3((unsigned)nbx, (unsigned)n_pats), dim3(APM_BLOCK), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// synthetic text fill: 16 bytes per lane, 16-byte stores
// ---------------------------------------------------------------------------
#ifndef APM_REC /* (no match site: the counting build's copy serves both) */
__global__ __launch_bounds__(APM_BLOCK) void apm_synth_kernel(uint8_t *dst, uint64_t global_off, uint64_t len,
                                                             uint64_t seed) {
    const uint64_t nthreads = (uint64_t)gridDim.x * APM_BLOCK;
    for (uint64_t t = (uint64_t)blockIdx.x * APM_BLOCK + threadIdx.x; t * 16 < len; t += nthreads) {
        const uint64_t o = t * 16;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int b = 0; b < 16; ++b) w[b >> 2] |= (uint32_t)apm_synth_byte(global_off + o + b, seed) << (8 * (b & 3));
        if (o + 16 <= len && ((reinterpret_cast<uintptr_t>(dst + o) & 15u) == 0)) {
            *reinterpret_cast<uint4 *>(dst + o) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int b = 0; o + b < len; ++b) dst[o + b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
}

hipError_t apm_launch_synth(uint8_t *dst, uint64_t global_off, uint64_t len, uint64_t seed, hipStream_t s) {
    if (len == 0) return hipSuccess;
    uint64_t nb = (len / 16 + APM_BLOCK - 1) / APM_BLOCK + 1;
    if (nb > 256 * 32) nb = 256 * 32;
    hipLaunchKernelGGL(apm_synth_kernel, dim3((unsigned)nb), dim3(APM_BLOCK), 0, s, dst, global_off, len, seed);
    return hipGetLastError();
}
#endif

// ---------------------------------------------------------------------------
// TAIL: the <= m-1 truncated windows at the very end of the text
// (sequential.c:131-134: window AND pattern cut to size = n - j), m <= 128.
// One 128-lane workgroup per pattern; each lane runs the 4-word bit-vector
// column for `size` steps over an Eq table built in LDS.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(128) void apm_tail_kernel(ApmTailArgs a) {
    __shared__ uint4 s_eq[256 + 8];
    apm_tail_body(a, (int)blockIdx.x, s_eq, (int)threadIdx.x);
}

hipError_t apm_launch_tail(const ApmTailArgs &a, int n_pats, hipStream_t s) {
    if (n_pats <= 0 || a.je <= a.jb) return hipSuccess;
    hipLaunchKernelGGL(apm_tail_kernel, dim3((unsigned)n_pats), dim3(128), 0, s, a);
    return hipGetLastError();
}
