/*
 * apm_score.hip -- the scoring pass: one launch over a finished buffer of apm_match records that recomputes every
 * record's exact distance (capped at k + 1, apm_score.h) and writes it into the record's fourth dword.  No scan kernel
 * knows the distance -- most decide "within k" only -- so it is worked out here, behind them, for the matches alone.
 *
 * Per record (apm_recpass.h's triage): invalid -> APM_DIST_INVALID; a window that is not wholly inside the shard text ->
 * left untouched; else the capped distance.  pos and pattern are only read.
 */
#include "apm_recpass.h"

namespace {

// lane form: one record per lane, wave w of the grid takes the records 64 w .. 64 w + 63, then those a grid further
template <int BAND>
__global__ __launch_bounds__(APM_BLOCK) void apm_score_lane_kernel(const ApmScoreArgs a) {
    const unsigned long long n = apm_rec_count(a);
    const unsigned long long stride = (unsigned long long)gridDim.x * APM_BLOCK;
    for (unsigned long long idx = (unsigned long long)blockIdx.x * APM_BLOCK + threadIdx.x; idx < n; idx += stride) {
        ApmRecPat p;
        ApmRecTxt t;
        int size = 0;
        uint32_t v = apm_rec_window(a, a.rec[idx], p, t, size);
        if (v == APM_REC_UNTOUCHED) continue;
        if (v == 0u) v = (uint32_t)apm_score_lane<BAND>(p, t, size, a.k);
        reinterpret_cast<uint32_t *>(a.rec)[4 * idx + 3] = v;
    }
}

// wave form: one record per wavefront = workgroup, the band in its LDS
__global__ __launch_bounds__(64) void apm_score_wave_kernel(const ApmScoreArgs a) {
    __shared__ int band[APM_SCORE_BAND_CELLS];
    const unsigned long long n = apm_rec_count(a);
    const int lane = (int)threadIdx.x;
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        const uint4 r = apm_rec_load_uniform(a, idx);
        ApmRecPat p;
        ApmRecTxt t;
        int size = 0;
        uint32_t v = apm_rec_window(a, r, p, t, size);
        if (v == APM_REC_UNTOUCHED) continue;
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
    APM_REC_LAUNCH_LANE(apm_score_lane_kernel, a.k, dim3((unsigned)n_cu * 4u), dim3(APM_BLOCK), s, a);
    return hipGetLastError();
}
