/*
 * apm_score.hip -- the scoring pass: one launch over a finished buffer of apm_match records that recomputes every
 * record's exact distance (capped at k + 1, apm_score.h) and writes it into the record's fourth dword.  No scan kernel
 * knows the distance -- most decide "within k" only -- so it is worked out here, behind them, for the matches alone.
 *
 * Per record: pattern >= n_patterns or pos >= n_total -> APM_DIST_INVALID; a window [pos, pos + size) that is not wholly
 * inside the shard text -> left untouched (several shards may share one buffer); else the capped distance.  pos and
 * pattern are only read.  The kernels read min(*n_rec, cap) themselves: no host synchronisation in front of the launch.
 * Text bytes are fetched inside [text, text + text_len) only.
 */
#include "apm_device.h"
#include "apm_score.h"

#define APM_SCORE_INVALID 0xffffffffu /* APM_DIST_INVALID of include/apm.h */
#define APM_SCORE_UNTOUCHED 0xfffffffeu /* (internal: apm_score_window's "leave the record alone") */

namespace {

struct ScorePat {      // a pattern's row of the score image: 16-byte aligned, zero padded (apm_score_row_bytes)
    const uint8_t *row;
    __device__ __forceinline__ void load16(int off, uint32_t (&w)[4]) const {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + off);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ int byte(int i) const { return (int)row[i]; }
};

struct ScoreTxt {      // a window of the shard text; nothing outside [0, avail) is fetched
    const uint8_t *text;
    int64_t rel, avail;
    __device__ __forceinline__ void load16(int off, uint32_t (&w)[4]) const {
        const uint4 v = apm_load16_guarded(text, rel + off, avail);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ int byte(int i) const { return (int)text[rel + i]; }
};

// what to do with record r: APM_SCORE_INVALID, APM_SCORE_UNTOUCHED, or 0 with the window's pattern row, text and size set
__device__ __forceinline__ uint32_t apm_score_window(const ApmScoreArgs &a, const uint4 r, ScorePat &p, ScoreTxt &t, int &size) {
    const unsigned long long pos = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
    if (r.z >= a.n_patterns || pos >= a.n_total) return APM_SCORE_INVALID;
    const uint2 d = a.table[r.z];
    const unsigned long long left = a.n_total - pos;
    size = left < (unsigned long long)d.y ? (int)left : (int)d.y; // >= 1
    if (pos < a.text_off || pos - a.text_off > a.text_len || (unsigned long long)size > a.text_len - (pos - a.text_off))
        return APM_SCORE_UNTOUCHED;
    p.row = a.image + d.x;
    t.text = a.text;
    t.rel = (int64_t)(pos - a.text_off);
    t.avail = (int64_t)a.text_len;
    return 0u;
}

__device__ __forceinline__ unsigned long long apm_score_count(const ApmScoreArgs &a) {
    const unsigned long long n = *a.n_rec;
    return n < a.cap ? n : a.cap;
}

// lane form: one record per lane, wave w of the grid takes the records 64 w .. 64 w + 63, then those a grid further
template <int BAND>
__global__ __launch_bounds__(APM_BLOCK) void apm_score_lane_kernel(const ApmScoreArgs a) {
    const unsigned long long n = apm_score_count(a);
    const unsigned long long stride = (unsigned long long)gridDim.x * APM_BLOCK;
    for (unsigned long long idx = (unsigned long long)blockIdx.x * APM_BLOCK + threadIdx.x; idx < n; idx += stride) {
        ScorePat p;
        ScoreTxt t;
        int size = 0;
        uint32_t v = apm_score_window(a, a.rec[idx], p, t, size);
        if (v == APM_SCORE_UNTOUCHED) continue;
        if (v == 0u) v = (uint32_t)apm_score_lane<BAND>(p, t, size, a.k);
        reinterpret_cast<uint32_t *>(a.rec)[4 * idx + 3] = v;
    }
}

// wave form: one record per wavefront = workgroup, the band in its LDS
__global__ __launch_bounds__(64) void apm_score_wave_kernel(const ApmScoreArgs a) {
    __shared__ int band[APM_SCORE_BAND_CELLS];
    const unsigned long long n = apm_score_count(a);
    const int lane = (int)threadIdx.x;
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        uint4 r = a.rec[idx]; // (the same record in every lane: made wave-uniform for the compiler's sake)
        r.x = __builtin_amdgcn_readfirstlane(r.x);
        r.y = __builtin_amdgcn_readfirstlane(r.y);
        r.z = __builtin_amdgcn_readfirstlane(r.z);
        ScorePat p;
        ScoreTxt t;
        int size = 0;
        uint32_t v = apm_score_window(a, r, p, t, size);
        if (v == APM_SCORE_UNTOUCHED) continue;
        if (v == 0u && min(a.k / 2, size - 1) > APM_SCORE_MAX_BAND) continue; // (the host refuses such a set: the band would not fit)
        if (v == 0u) {
            v = (uint32_t)apm_score_wave(p, t, size, a.k, band, lane);
            __syncthreads(); // (the band is the next record's)
        }
        if (lane == 0) reinterpret_cast<uint32_t *>(a.rec)[4 * idx + 3] = v;
    }
}

} // namespace

// Fixed grids sized from the CU count; a launch over few records costs its workgroups one load of the count each.
hipError_t apm_launch_score(const ApmScoreArgs &a, int n_cu, hipStream_t s) {
    if (a.k > APM_SCORE_LANE_MAX_K) {
        hipLaunchKernelGGL(apm_score_wave_kernel, dim3((unsigned)n_cu * 8u), dim3(64), 0, s, a);
        return hipGetLastError();
    }
    const dim3 grid((unsigned)n_cu * 4u), block(APM_BLOCK);
    switch (a.k / 2) {
    case 0: hipLaunchKernelGGL(apm_score_lane_kernel<0>, grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL(apm_score_lane_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(apm_score_lane_kernel<2>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(apm_score_lane_kernel<3>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}
