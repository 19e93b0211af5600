/*
 * apm_occ_device.h -- device glue the occurrence kernels (apm_occ.hip) and the nearest-occurrence kernels
 * (apm_nearest.hip) share: how a segment walk fetches the shard text, a pattern's Eq table in a slot of LDS, and how a span
 * walk reads the bytes in front of its end.  The walks themselves are apm_occ.h's, host and device.
 */
#ifndef APM_OCC_DEVICE_H
#define APM_OCC_DEVICE_H

#include "apm_device.h"
#include "apm_occ.h"

constexpr int kApmOccEqWords = 256 * APM_OCC_MAX_WORDS; // one slot: a pattern's Eq table at the widest column

struct ApmOccTxt { // the shard text by global position; nothing outside it is fetched
    const uint8_t *text;
    long long off, len;
    __device__ __forceinline__ void load16(long long x, uint32_t (&w)[4]) const {
        const uint4 v = apm_load16_guarded(text, (int64_t)(x - off), (int64_t)len);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    }
};

template <int W>
struct ApmOccEq { // a slot of LDS: the mask of byte c in words c * W .. c * W + W - 1
    const uint32_t *tab;
    __device__ __forceinline__ void get(int c, uint32_t (&eq)[W]) const {
#pragma unroll
        for (int w = 0; w < W; ++w) eq[w] = tab[c * W + w];
    }
};

// the Eq table of the m bytes pat[0 .. m), read forwards or backwards, into a zeroed slot; `lanes` threads share the work
__device__ __forceinline__ void apm_occ_build_eq(uint32_t *tab, const uint8_t *pat, int m, bool reversed, int lane, int lanes) {
    const int W = apm_occ_words(m);
    for (int i = lane; i < m; i += lanes) {
        const int c = (int)pat[reversed ? m - 1 - i : i];
        atomicOr(&tab[c * W + (i >> 5)], 1u << (i & 31));
    }
}

struct ApmSpanBack { // the text bytes in front of the end, last one first
    const uint8_t *bytes;
    __device__ __forceinline__ int operator()(int i) const { return (int)bytes[i]; }
};

#endif /* APM_OCC_DEVICE_H */
