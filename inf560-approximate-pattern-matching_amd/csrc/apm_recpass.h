/*
 * apm_recpass.h -- device glue of the record passes, the launches that run over a finished buffer of apm_match records:
 * the scoring pass (apm_score.hip) and the align pass (apm_align.hip).  Both read the records, the score image and the
 * shard text through ApmScoreArgs (apm_score.h) and triage a record the same way; what they compute for a window and
 * where they write it is their own.
 *
 * Per record: pattern >= n_patterns or pos >= n_total -> APM_REC_INVALID; a window [pos, pos + size) that is not wholly
 * inside the shard text -> APM_REC_UNTOUCHED, the pass leaves the record's output alone (several shards may share one
 * buffer); else 0 and the window.  The kernels read min(*n_rec, cap) themselves: no host synchronisation in front of
 * the launch.  Text bytes are fetched inside [text, text + text_len) only.
 */
#ifndef APM_RECPASS_H
#define APM_RECPASS_H

#include "apm_device.h"
#include "apm_score.h"

#define APM_REC_INVALID 0xffffffffu   /* APM_DIST_INVALID of include/apm.h */
#define APM_REC_UNTOUCHED 0xfffffffeu /* (internal: apm_rec_window's "leave the record alone") */

struct ApmRecPat {     // a pattern's row of the score image: 16-byte aligned, zero padded (apm_score_row_bytes)
    const uint8_t *row;
    __device__ __forceinline__ void load16(int off, uint32_t (&w)[4]) const {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + off);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ int byte(int i) const { return (int)row[i]; }
};

struct ApmRecTxt {     // a window of the shard text; nothing outside [0, avail) is fetched
    const uint8_t *text;
    int64_t rel, avail;
    __device__ __forceinline__ void load16(int off, uint32_t (&w)[4]) const {
        const uint4 v = apm_load16_guarded(text, rel + off, avail);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
    __device__ __forceinline__ int byte(int i) const { return (int)text[rel + i]; }
};

// what to do with record r: APM_REC_INVALID, APM_REC_UNTOUCHED, or 0 with the window's pattern row, text and size set
__device__ __forceinline__ uint32_t apm_rec_window(const ApmScoreArgs &a, const uint4 r, ApmRecPat &p, ApmRecTxt &t, int &size) {
    const unsigned long long pos = (unsigned long long)r.x | ((unsigned long long)r.y << 32);
    if (r.z >= a.n_patterns || pos >= a.n_total) return APM_REC_INVALID;
    const uint2 d = a.table[r.z];
    const unsigned long long left = a.n_total - pos;
    size = left < (unsigned long long)d.y ? (int)left : (int)d.y; // >= 1
    if (pos < a.text_off || pos - a.text_off > a.text_len || (unsigned long long)size > a.text_len - (pos - a.text_off))
        return APM_REC_UNTOUCHED;
    p.row = a.image + d.x;
    t.text = a.text;
    t.rel = (int64_t)(pos - a.text_off);
    t.avail = (int64_t)a.text_len;
    return 0u;
}

__device__ __forceinline__ unsigned long long apm_rec_count(const ApmScoreArgs &a) {
    const unsigned long long n = *a.n_rec;
    return n < a.cap ? n : a.cap;
}

// record idx for a wave that serves it as one: the same in every lane, made wave-uniform for the compiler's sake
__device__ __forceinline__ uint4 apm_rec_load_uniform(const ApmScoreArgs &a, unsigned long long idx) {
    uint4 r = a.rec[idx];
    r.x = __builtin_amdgcn_readfirstlane(r.x);
    r.y = __builtin_amdgcn_readfirstlane(r.y);
    r.z = __builtin_amdgcn_readfirstlane(r.z);
    return r;
}

// launches KERNEL<BAND> of the lane form, BAND = k/2 <= 3 (k <= APM_SCORE_LANE_MAX_K)
#define APM_REC_LAUNCH_LANE(KERNEL, k, grid, block, stream, args)                                  \
    switch ((k) / 2) {                                                                             \
    case 0: hipLaunchKernelGGL(KERNEL<0>, grid, block, 0, stream, args); break;                    \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, block, 0, stream, args); break;                    \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, block, 0, stream, args); break;                    \
    default: hipLaunchKernelGGL(KERNEL<3>, grid, block, 0, stream, args); break;                   \
    }

#endif /* APM_RECPASS_H */
