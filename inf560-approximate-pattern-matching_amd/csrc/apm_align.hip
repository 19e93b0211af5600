/*
 * apm_align.hip -- the align pass: one launch over a finished buffer of apm_match records that works out every record's
 * edit script (apm_align.h: the canonical one of the optimal scripts) and writes it into the record's row of `ops`.  It
 * runs behind the scan and the scoring pass, for the matches alone; the records are only read.
 *
 * Per record (the scoring pass's triage): pattern >= n_patterns or pos >= n_total -> word 0 = APM_DIST_INVALID; a window
 * that is not wholly inside the shard text -> row untouched; a window farther than k -> word 0 = 0; else word 0 = n_ops
 * and the ops behind it.  The kernels read min(*n_rec, cap) themselves: no host synchronisation in front of the launch.
 * Text bytes are fetched inside [text, text + text_len) only.  Every lane (lane form) or wavefront (wave form) of the
 * grid owns one trace row of the workspace and reuses it for its next record.
 */
#include "apm_device.h"
#include "apm_align.h"

#define APM_ALIGN_INVALID 0xffffffffu /* APM_DIST_INVALID of include/apm.h */
#define APM_ALIGN_UNTOUCHED 0xfffffffeu /* (internal: "leave the row alone") */

namespace {

struct AlignPat {      // a pattern's row of the score image: 16-byte aligned, zero padded (apm_score_row_bytes)
    const uint8_t *row;
    __device__ __forceinline__ void load16(int off, uint32_t (&w)[4]) const {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + off);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ int byte(int i) const { return (int)row[i]; }
};

struct AlignTxt {      // a window of the shard text; nothing outside [0, avail) is fetched
    const uint8_t *text;
    int64_t rel, avail;
    __device__ __forceinline__ void load16(int off, uint32_t (&w)[4]) const {
        const uint4 v = apm_load16_guarded(text, rel + off, avail);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ int byte(int i) const { return (int)text[rel + i]; }
};

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

// apm_score.hip's apm_score_window: what to do with record r -- APM_ALIGN_INVALID, APM_ALIGN_UNTOUCHED, or 0 with the
// window's pattern row, text and size set
__device__ __forceinline__ uint32_t apm_align_window(const ApmAlignArgs &a, const uint4 r, AlignPat &p, AlignTxt &t, int &size) {
    const unsigned long long pos = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
    if (r.z >= a.n_patterns || pos >= a.n_total) return APM_ALIGN_INVALID;
    const uint2 d = a.table[r.z];
    const unsigned long long left = a.n_total - pos;
    size = left < (unsigned long long)d.y ? (int)left : (int)d.y; // >= 1
    if (pos < a.text_off || pos - a.text_off > a.text_len || (unsigned long long)size > a.text_len - (pos - a.text_off))
        return APM_ALIGN_UNTOUCHED;
    if ((uint32_t)size > a.m_max) return APM_ALIGN_UNTOUCHED; // (never: the trace rows are sized for the set's longest pattern)
    p.row = a.image + d.x;
    t.text = a.text;
    t.rel = (int64_t)(pos - a.text_off);
    t.avail = (int64_t)a.text_len;
    return 0u;
}

__device__ __forceinline__ unsigned long long apm_align_count(const ApmAlignArgs &a) {
    const unsigned long long n = *a.n_rec;
    return n < a.cap ? n : a.cap;
}

// lane form: one record per lane; the grid has exactly `rows` lanes, lane `slot` owns trace row `slot`
template <int BAND>
__global__ __launch_bounds__(APM_BLOCK) void apm_align_lane_kernel(const ApmAlignArgs a) {
    const unsigned long long n = apm_align_count(a);
    const unsigned long long rows = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long slot = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneTrace tr{reinterpret_cast<uint16_t *>(a.ws) + slot, (size_t)rows};
    for (unsigned long long idx = slot; idx < n; idx += rows) {
        AlignPat p;
        AlignTxt t;
        int size = 0;
        uint32_t v = apm_align_window(a, a.rec[idx], p, t, size);
        if (v == APM_ALIGN_UNTOUCHED) continue;
        LaneOut out{a.ops + idx * a.stride};
        if (v == 0u) v = (uint32_t)apm_align_lane<BAND>(p, t, size, a.k, tr, out);
        out.row[0] = v;
    }
}

// wave form: one record per wavefront = workgroup, the band in its LDS, workgroup b owns trace row b
__global__ __launch_bounds__(64) void apm_align_wave_kernel(const ApmAlignArgs a) {
    __shared__ int band[APM_SCORE_BAND_CELLS];
    const unsigned long long n = apm_align_count(a);
    const int lane = (int)threadIdx.x;
    uint4 *ws = reinterpret_cast<uint4 *>(a.ws) + (size_t)blockIdx.x * (size_t)a.row_entries;
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        uint4 r = a.rec[idx]; // (the same record in every lane: made wave-uniform for the compiler's sake)
        r.x = __builtin_amdgcn_readfirstlane(r.x);
        r.y = __builtin_amdgcn_readfirstlane(r.y);
        r.z = __builtin_amdgcn_readfirstlane(r.z);
        AlignPat p;
        AlignTxt t;
        int size = 0;
        uint32_t v = apm_align_window(a, r, p, t, size);
        if (v == APM_ALIGN_UNTOUCHED) continue;
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
// runtime sized from the budget and n_cu (apm_align_rows); a launch over few records costs its workgroups one load of the
// count each.
hipError_t apm_launch_align(const ApmAlignArgs &a, int n_cu, uint32_t rows, hipStream_t s) {
    (void)n_cu; // (the launcher's signature is apm_launch_score's; the geometry came in as rows)
    if (rows == 0) return hipErrorInvalidValue;
    if (a.k > APM_SCORE_LANE_MAX_K) {
        hipLaunchKernelGGL(apm_align_wave_kernel, dim3(rows), dim3(64), 0, s, a);
        return hipGetLastError();
    }
    const dim3 block(rows < APM_BLOCK ? rows : APM_BLOCK), grid(rows / block.x);
    switch (a.k / 2) {
    case 0: hipLaunchKernelGGL(apm_align_lane_kernel<0>, grid, block, 0, s, a); break;
    case 1: hipLaunchKernelGGL(apm_align_lane_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(apm_align_lane_kernel<2>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(apm_align_lane_kernel<3>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}
