/*
 * apm_nearest.hip -- the nearest-occurrence search: a scan that reduces, for every pattern, the occurrence search's E(e)
 * over all ends to ONE key (apm_nearest.h: the smallest distance and its first end), and a finishing pass that turns the
 * keys into end and start records.  Compiled once; neither feeds the counting kernels' sinks.
 *
 * Scan ("nearest"): the geometry and the text delivery of the occurrence scan (apm_occ.hip) -- a workgroup is APM_OCC_SLOTS
 * waves, wave w walks pattern blockIdx.y * APM_OCC_SLOTS + w with its Eq table (256 x W words) in its slot of LDS, lane l
 * the segment blockIdx.x * 64 + l, text as per-lane guarded 16-byte streams.  The walk's bound is the wave's own m - 1 (a
 * warm-up of 2 m - 1 bytes), its sink a lane-private best key: no ballot, no append, no atomic per column.  Behind the walk
 * the wave reduces its 64 keys to their minimum and, unless that is NONE, issues one atomicMin on keys[pattern].
 *
 * Finish ("nspan"): one wavefront = workgroup per PATTERN, grid-stride; the key becomes the end record and, where the shard
 * text covers the up to m + d bytes in front of the end, the span record at the bound d -- the reversed pattern's Eq and
 * those bytes in LDS, apm_occ_span_walk, as the span pass of apm_occ.hip does for an end record.
 */
#include "apm_recpass.h"
#include "apm_occ_device.h"
#include "apm_nearest.h"

namespace {

template <int W>
__device__ __forceinline__ unsigned long long nearest_walk(const ApmNearestArgs &a, const uint32_t *tab, int m, long long b, long long e) {
    const ApmOccTxt t{a.text, (long long)a.text_off, (long long)a.text_len};
    return apm_nearest_walk<W>(t, ApmOccEq<W>{tab}, m, b, e, (long long)a.n_total, apm_nearest_steps((int)a.segment, m));
}

__global__ __launch_bounds__(64 * APM_OCC_SLOTS) void apm_nearest_scan_kernel(const ApmNearestArgs a) {
    __shared__ uint32_t s_eq[APM_OCC_SLOTS * kApmOccEqWords];
    const int tid = (int)threadIdx.x, lane = tid & 63, slot = tid >> 6;
    const uint32_t pattern = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.y * APM_OCC_SLOTS + (uint32_t)slot));
    for (int i = tid; i < APM_OCC_SLOTS * kApmOccEqWords; i += 64 * APM_OCC_SLOTS) s_eq[i] = 0u;
    __syncthreads();
    uint32_t *tab = s_eq + slot * kApmOccEqWords;
    int m = 0;
    bool served = false; // (wave-uniform; the host refuses a set with a pattern the scan does not serve)
    if (pattern < a.n_patterns) {
        const uint2 d = a.table[pattern];
        m = (int)d.y;
        served = m >= 1 && m <= APM_OCC_MAX_PATTERN_LEN;
        if (served) apm_occ_build_eq(tab, a.image + d.x, m, false, lane, 64);
    }
    __syncthreads();
    if (!served) return; // (a whole wave)
    // the segment of this lane; a lane behind the last segment walks an empty range, in step with its wave
    const unsigned long long seg = (unsigned long long)blockIdx.x * APM_OCC_LANES + (unsigned long long)lane;
    long long b = (long long)a.e_end, e = (long long)a.e_end;
    if (seg < a.n_segments) {
        b = (long long)(a.e_begin + seg * a.segment);
        e = b + (long long)a.segment < (long long)a.e_end ? b + (long long)a.segment : (long long)a.e_end;
    }
    unsigned long long key = APM_NEAREST_NONE;
    switch (apm_occ_words(m)) { // (wave-uniform)
    case 1: key = nearest_walk<1>(a, tab, m, b, e); break;
    case 2: key = nearest_walk<2>(a, tab, m, b, e); break;
    case 3: key = nearest_walk<3>(a, tab, m, b, e); break;
    default: key = nearest_walk<4>(a, tab, m, b, e); break;
    }
    // the wave's smallest key: a DPP-free butterfly over 64 lanes, both halves of the key travel together; one atomic
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), o, 64);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        key = other < key ? other : key;
    }
    if (lane == 0 && key != APM_NEAREST_NONE) atomicMin(&a.keys[pattern], key);
}

__device__ __forceinline__ uint4 nearest_record(unsigned long long pos, uint32_t pattern, uint32_t dist) {
    return make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), pattern, dist);
}

template <int W>
__device__ __forceinline__ void span_walk(const uint32_t *tab, const uint8_t *bytes, int m, int cols, int *d, int *l) {
    apm_occ_span_walk<W>(ApmOccEq<W>{tab}, ApmSpanBack{bytes}, m, cols, d, l);
}

__global__ __launch_bounds__(64) void apm_nearest_span_kernel(const ApmNspanArgs a) {
    __shared__ uint32_t s_eq[kApmOccEqWords];
    __shared__ uint8_t s_txt[2 * APM_OCC_MAX_PATTERN_LEN]; // m + d <= 2 m - 1 bytes
    const int lane = (int)threadIdx.x;
    const unsigned long long none = 0xffffffffffffffffull; // APM_OCC_NO_START
    for (uint32_t i = blockIdx.x; i < a.n_patterns; i += gridDim.x) {
        unsigned long long key = a.keys[i]; // (the same in every lane: made wave-uniform for the compiler's sake)
        key = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32)) << 32) |
              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key);
        const uint2 d = a.table[i];
        const int m = (int)d.y;
        if (m > APM_OCC_MAX_PATTERN_LEN) continue; // (the host refuses such a set)
        const int dist = (int)APM_NEAREST_DIST(key);
        const unsigned long long e = APM_NEAREST_END(key);
        if (key == APM_NEAREST_NONE || dist >= m || e >= a.n_total) { // no end below m; or a key no scan made
            const uint4 r = nearest_record(none, i, key == APM_NEAREST_NONE ? (uint32_t)m : APM_REC_INVALID);
            if (lane == 0) {
                a.end[i] = r;
                if (a.start) a.start[i] = r;
            }
            continue;
        }
        if (lane == 0) a.end[i] = nearest_record(e, i, (uint32_t)dist);
        if (!a.start) continue;
        const int cols = apm_occ_span_cols(m, dist, e);
        const unsigned long long lo = e + 1ull - (unsigned long long)cols;
        if (lo < a.text_off || e - a.text_off >= a.text_len) continue; // not covered: another shard's
        const int W = apm_occ_words(m);
        for (int j = lane; j < 256 * W; j += 64) s_eq[j] = 0u;
        for (int j = lane; j < cols; j += 64) s_txt[j] = a.text[e - a.text_off - (unsigned long long)j];
        __syncthreads();
        apm_occ_build_eq(s_eq, a.image + d.x, m, true, lane, 64);
        __syncthreads();
        int ds = 0, ls = 0; // (every lane walks the same columns: LDS broadcasts)
        switch (W) {
        case 1: span_walk<1>(s_eq, s_txt, m, cols, &ds, &ls); break;
        case 2: span_walk<2>(s_eq, s_txt, m, cols, &ds, &ls); break;
        case 3: span_walk<3>(s_eq, s_txt, m, cols, &ds, &ls); break;
        default: span_walk<4>(s_eq, s_txt, m, cols, &ds, &ls); break;
        }
        if (lane == 0) a.start[i] = ds <= dist ? nearest_record(e + 1ull - (unsigned long long)ls, i, (uint32_t)ds) : nearest_record(none, i, (uint32_t)(dist + 1));
        __syncthreads(); // (the tables are the next pattern's)
    }
}

} // namespace

hipError_t apm_launch_nearest(const ApmNearestArgs &a, hipStream_t s) {
    const dim3 grid((a.n_segments + APM_OCC_LANES - 1) / APM_OCC_LANES, (a.n_patterns + APM_OCC_SLOTS - 1) / APM_OCC_SLOTS);
    hipLaunchKernelGGL(apm_nearest_scan_kernel, grid, dim3(64 * APM_OCC_SLOTS), 0, s, a);
    return hipGetLastError();
}

// one workgroup per pattern, no more than the span pass's fixed grid
hipError_t apm_launch_nspan(const ApmNspanArgs &a, int n_cu, hipStream_t s) {
    const unsigned most = (unsigned)n_cu * 16u;
    hipLaunchKernelGGL(apm_nearest_span_kernel, dim3(a.n_patterns < most ? a.n_patterns : most), dim3(64), 0, s, a);
    return hipGetLastError();
}
