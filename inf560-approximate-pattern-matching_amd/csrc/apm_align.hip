/*
 * apm_align.hip -- the align pass: one launch over a finished buffer of apm_match records that works out every record's
 * edit script (apm_align.h: the canonical one of the optimal scripts) and writes it into the record's row of `ops`.  It
 * runs behind the scan and the scoring pass, for the matches alone; the records are only read.
 *
 * Per record (apm_recpass.h's triage): invalid -> word 0 = APM_DIST_INVALID; a window that is not wholly inside the
 * shard text -> row untouched; a window farther than k -> word 0 = 0; else word 0 = n_ops and the ops behind it.  Every
 * lane (lane form) or wavefront (wave form) of the grid owns one trace row of the workspace and reuses it for its next
 * record.
 */
#include "apm_recpass.h"
#include "apm_align.h"

namespace {

struct LaneTrace {     // a lane's trace row: column c at c * rows + slot
    uint16_t *ws;
    size_t rows;
    __device__ __forceinline__ void put(int col, uint32_t w) { ws[(size_t)col * rows] = (uint16_t)w; }
    __device__ __forceinline__ uint32_t get(int col) const { return ws[(size_t)col * rows]; }
};

struct LaneOut {       // a record's row of ops
    uint32_t *row;
    __device__ __forceinline__ void store(int word, uint32_t v) { row[word] = v; }
};

struct WaveOut {       // the same, every lane calling: one lane stores
    uint32_t *row;
    int lane;
    __device__ __forceinline__ void store(int word, uint32_t v) { if (lane == 0) row[word] = v; }
};

// lane form: one record per lane; the grid has exactly `rows` lanes, lane `slot` owns trace row `slot`
template <int BAND>
__global__ __launch_bounds__(APM_BLOCK) void apm_align_lane_kernel(const ApmAlignArgs a) {
    const unsigned long long n = apm_rec_count(a);
    const unsigned long long rows = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long slot = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneTrace tr{reinterpret_cast<uint16_t *>(a.ws) + slot, (size_t)rows};
    for (unsigned long long idx = slot; idx < n; idx += rows) {
        ApmRecPat p;
        ApmRecTxt t;
        int size = 0;
        uint32_t v = apm_rec_window(a, a.rec[idx], p, t, size);
        if (v == 0u && (uint32_t)size > a.m_max) v = APM_REC_UNTOUCHED; // (never: the trace rows are sized for the set's longest pattern)
        if (v == APM_REC_UNTOUCHED) continue;
        LaneOut out{a.ops + idx * a.stride};
        if (v == 0u) v = (uint32_t)apm_align_lane<BAND>(p, t, size, a.k, tr, out);
        out.row[0] = v;
    }
}

// wave form: one record per wavefront = workgroup, the band in its LDS, workgroup b owns trace row b
__global__ __launch_bounds__(64) void apm_align_wave_kernel(const ApmAlignArgs a) {
    __shared__ int band[APM_SCORE_BAND_CELLS];
    const unsigned long long n = apm_rec_count(a);
    const int lane = (int)threadIdx.x;
    uint4 *ws = reinterpret_cast<uint4 *>(a.ws) + (size_t)blockIdx.x * (size_t)a.row_entries;
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        const uint4 r = apm_rec_load_uniform(a, idx);
        ApmRecPat p;
        ApmRecTxt t;
        int size = 0;
        uint32_t v = apm_rec_window(a, r, p, t, size);
        if (v == 0u && (uint32_t)size > a.m_max) v = APM_REC_UNTOUCHED; // (never: the trace rows are sized for the set's longest pattern)
        if (v == APM_REC_UNTOUCHED) continue;
        if (v == 0u && min(a.k / 2, size - 1) > APM_SCORE_MAX_BAND) continue; // (the host refuses such a set: the band would not fit)
        WaveOut out{a.ops + idx * a.stride, lane};
        if (v == 0u) {
            v = (uint32_t)apm_align_wave(p, t, size, a.k, band, lane, ws, out);
            __syncthreads(); // (the band and the trace row are the next record's)
        }
        if (lane == 0) out.row[0] = v;
    }
}

} // namespace

// The grid is the workspace's: `rows` lanes (lane form, whole workgroups) or `rows` wavefronts (wave form), which the
// runtime sized from the budget and the CU count (apm_align_rows); a launch over few records costs its workgroups one
// load of the count each.
hipError_t apm_launch_align(const ApmAlignArgs &a, uint32_t rows, hipStream_t s) {
    if (rows == 0) return hipErrorInvalidValue;
    if (a.k > APM_SCORE_LANE_MAX_K) {
        hipLaunchKernelGGL(apm_align_wave_kernel, dim3(rows), dim3(64), 0, s, a);
        return hipGetLastError();
    }
    const dim3 block(rows < APM_BLOCK ? rows : APM_BLOCK), grid(rows / block.x);
    APM_REC_LAUNCH_LANE(apm_align_lane_kernel, a.k, grid, block, s, a);
    return hipGetLastError();
}
