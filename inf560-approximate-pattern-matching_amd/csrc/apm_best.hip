/*
 * apm_best.hip -- the best-hit pass: one launch over a finished buffer of apm_match records that keeps, of every run of
 * neighbouring starts one occurrence leaves behind, the best start (apm_best.h states the rule) and appends it, scored,
 * to a second buffer.  It stands between the find and the align pass; the records are only read.
 *
 * Per record (apm_recpass.h's triage): invalid -> dropped; the window, or the neighbourhood the decision reads
 * (apm_best_covered), not wholly inside the shard text -> skipped (several shards may share one buffer: the shard that
 * covers it decides); farther than k -> dropped; suppressed by a neighbour start -> dropped; else appended with its score.
 */
#include "apm_recpass.h"
#include "apm_best.h"

namespace {

struct ApmBestTxt : ApmRecTxt { // the record's window, and the windows o bytes further
    __device__ __forceinline__ ApmBestTxt at(int o) const {
        ApmBestTxt n = *this;
        n.rel += o;
        return n;
    }
};

__device__ __forceinline__ unsigned long long rec_pos(const uint4 r) { return (unsigned long long)r.x | ((unsigned long long)r.y << 32); }

// one lane of the wave appends the best hit: one 16-byte store, nothing at or beyond out_cap
__device__ __forceinline__ void append(const ApmBestArgs &a, const uint4 r, int s0) {
    const unsigned long long slot = atomicAdd(a.n_out, 1ull);
    if (slot < a.out_cap) a.out[slot] = make_uint4(r.x, r.y, r.z, (uint32_t)s0);
}

// lane form: one record per wavefront; lane l of round q owns the neighbour offset 64 q + l - r and walks its window
// on its own.  The round that holds offset 0 goes first, at cap k: its lanes learn the record's own score by readlane,
// the other rounds walk with the tighter caps of apm_best_cap.
template <int BAND>
__global__ __launch_bounds__(APM_BLOCK) void apm_best_lane_kernel(const ApmBestArgs a) {
    const unsigned long long n = apm_rec_count(a);
    const unsigned long long waves = (unsigned long long)gridDim.x * (APM_BLOCK / 64);
    const int lane = (int)(threadIdx.x & 63u);
    const int r = (int)a.radius, rounds = (2 * r + 1 + 63) >> 6, own_round = r >> 6, own_lane = r & 63;
    const unsigned long long w_end = apm_best_w_end(a.n_total, a.k);
    for (unsigned long long idx = (unsigned long long)blockIdx.x * (APM_BLOCK / 64) + (threadIdx.x >> 6); idx < n; idx += waves) {
        const uint4 rec = apm_rec_load_uniform(a, idx);
        ApmRecPat p;
        ApmBestTxt t;
        int size = 0;
        if (apm_rec_window(a, rec, p, t, size) != 0u) continue;
        const unsigned long long pos = rec_pos(rec);
        const int m = (int)a.table[rec.z].y;
        if (!apm_best_covered(pos, m, r, a.n_total, a.text_off, a.text_len)) continue;
        int s0 = 0;
        bool kept = true;
        for (int i = 0; i < rounds && kept; ++i) {
            const int q = i == 0 ? own_round : (i <= own_round ? i - 1 : i);
            const int o = 64 * q + lane - r;
            const int cap = i == 0 ? a.k : apm_best_cap(o, s0);
            const bool walk = o == 0 || (o <= r && cap >= 0 && apm_best_neighbour(pos, o, w_end));
            int s = APM_SCORE_INF;
            if (walk) s = apm_score_lane<BAND>(p, t.at(o), apm_best_size(m, apm_best_start(pos, o), a.n_total), cap);
            if (i == 0) {
                s0 = __builtin_amdgcn_readlane(s, own_lane);
                kept = s0 <= a.k;
            }
            if (kept && __builtin_amdgcn_ballot_w64(walk && o != 0 && apm_best_suppresses(o, s, s0)) != 0ull) kept = false;
        }
        if (kept && lane == 0) append(a, rec, s0);
    }
}

// wave form: one record per wavefront = workgroup, the band in its LDS; the record's own window first, then the
// neighbours nearest first, up to the first suppressor
__global__ __launch_bounds__(64) void apm_best_wave_kernel(const ApmBestArgs a) {
    __shared__ int band[APM_SCORE_BAND_CELLS];
    const unsigned long long n = apm_rec_count(a);
    const int lane = (int)threadIdx.x;
    const int r = (int)a.radius;
    const unsigned long long w_end = apm_best_w_end(a.n_total, a.k);
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        const uint4 rec = apm_rec_load_uniform(a, idx);
        ApmRecPat p;
        ApmBestTxt t;
        int size = 0;
        if (apm_rec_window(a, rec, p, t, size) != 0u) continue;
        const unsigned long long pos = rec_pos(rec);
        const int m = (int)a.table[rec.z].y;
        if (!apm_best_covered(pos, m, r, a.n_total, a.text_off, a.text_len)) continue;
        if (min(a.k / 2, m - 1) > APM_SCORE_MAX_BAND) continue; // (the host refuses such a set: the band would not fit)
        const int s0 = apm_score_wave(p, t, size, a.k, band, lane);
        __syncthreads(); // (the band is the next walk's)
        bool kept = s0 <= a.k;
        for (int i = 0; i < 2 * r && kept; ++i) {
            const int o = apm_best_offset(i), cap = apm_best_cap(o, s0);
            if (cap < 0 || !apm_best_neighbour(pos, o, w_end)) continue;
            const int s = apm_score_wave(p, t.at(o), apm_best_size(m, apm_best_start(pos, o), a.n_total), cap, band, lane);
            __syncthreads();
            kept = !apm_best_suppresses(o, s, s0);
        }
        if (kept && lane == 0) append(a, rec, s0);
    }
}

} // namespace

// Fixed grids sized from the CU count, as the scoring pass's: a launch over few records costs its workgroups one load of
// the count each.
hipError_t apm_launch_best(const ApmBestArgs &a, int n_cu, hipStream_t s) {
    if (a.k > APM_SCORE_LANE_MAX_K) {
        hipLaunchKernelGGL(apm_best_wave_kernel, dim3((unsigned)n_cu * 8u), dim3(64), 0, s, a);
        return hipGetLastError();
    }
    APM_REC_LAUNCH_LANE(apm_best_lane_kernel, a.k, dim3((unsigned)n_cu * 8u), dim3(APM_BLOCK), s, a);
    return hipGetLastError();
}
