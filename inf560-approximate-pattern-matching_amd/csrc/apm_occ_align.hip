/*
 * apm_occ_align.hip -- the occurrence-script pass ("oalign"): a record pass over pairs of an occurrence's end record and
 * its span record that writes the edit script of the WHOLE pattern against the text bytes [start, end] (apm_occ_align.h
 * states the rule and the arithmetic; include/apm.h: "occurrence scripts").  Compiled once; a unit of its own, beside
 * apm_occ.hip's scan and span pass.
 *
 * One pair per wavefront = workgroup, grid-stride, everything in LDS: the forward pattern's Eq table indexed by the full
 * text byte (256 x W words), the L <= m + k <= 255 text bytes of the span, and the trace -- the vertical deltas of the
 * columns 0 .. L, 2 W words each, at most 8 KB.  Every lane walks the same columns (LDS reads broadcast), lane 0 stores
 * the trace and the row; a barrier stands between the trace stores and the walk back, and in front of the next pair.
 */
#include "apm_recpass.h"
#include "apm_occ_align.h"

namespace {

constexpr int kEqWords = 256 * APM_OCC_MAX_WORDS;                 // a pattern's Eq table at the widest column
constexpr int kTraceCols = APM_OCC_ALIGN_MAX_COLS + 1;            // column 0 and one per text byte
constexpr int kTraceWords = kTraceCols * 2 * APM_OCC_MAX_WORDS;

template <int W>
struct OAlignEq { // the mask of byte c in words c * W .. c * W + W - 1 (apm_occ.hip's layout)
    const uint32_t *tab;
    __device__ __forceinline__ void get(int c, uint32_t (&eq)[W]) const {
#pragma unroll
        for (int w = 0; w < W; ++w) eq[w] = tab[c * W + w];
    }
};

struct OAlignTxt { // the span's bytes, first one first
    const uint8_t *bytes;
    __device__ __forceinline__ int operator()(int i) const { return (int)bytes[i]; }
};

template <int W>
struct OAlignTrace { // column c: pv in words c * 2 W .., mv behind them; every lane puts the same values, lane 0 stores
    uint32_t *ws;
    int lane;
    __device__ __forceinline__ void put(int col, int w, uint32_t pv, uint32_t mv) {
        if (lane == 0) {
            ws[col * 2 * W + w] = pv;
            ws[col * 2 * W + W + w] = mv;
        }
    }
    __device__ __forceinline__ void done() { __syncthreads(); } // (lane 0's stores before every lane's loads)
    __device__ __forceinline__ uint32_t pv(int col, int w) const { return ws[col * 2 * W + w]; }
    __device__ __forceinline__ uint32_t mv(int col, int w) const { return ws[col * 2 * W + W + w]; }
};

struct OAlignOut { // every lane calls store with the same arguments
    uint32_t *row;
    int lane;
    __device__ __forceinline__ void store(int word, uint32_t v) {
        if (lane == 0) row[word] = v;
    }
};

template <int W>
__device__ __forceinline__ int oalign(const uint32_t *tab, const uint8_t *bytes, uint32_t *trace, int m, int L, int k, int lane, uint32_t *row) {
    OAlignTrace<W> tr{trace, lane};
    OAlignOut out{row, lane};
    return apm_occ_align<W>(OAlignEq<W>{tab}, OAlignTxt{bytes}, m, L, k, tr, out);
}

__global__ __launch_bounds__(64) void apm_occ_align_kernel(const ApmOccAlignArgs a) {
    __shared__ uint32_t s_eq[kEqWords];
    __shared__ uint32_t s_trace[kTraceWords];
    __shared__ uint8_t s_txt[kTraceCols];
    const unsigned long long n = apm_rec_count(a);
    const int lane = (int)threadIdx.x;
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        const uint4 end = apm_rec_load_uniform(a, idx);
        uint4 span = a.span[idx]; // (the same in every lane, made wave-uniform as the end record is)
        span.x = __builtin_amdgcn_readfirstlane(span.x);
        span.y = __builtin_amdgcn_readfirstlane(span.y);
        span.z = __builtin_amdgcn_readfirstlane(span.z);
        uint32_t *row = a.ops + idx * (unsigned long long)a.stride;
        const unsigned long long e = (unsigned long long)end.x | ((unsigned long long)end.y << 32);
        const unsigned long long s = (unsigned long long)span.x | ((unsigned long long)span.y << 32);
        if (end.z >= a.n_patterns || e >= a.n_total || span.z != end.z) { // names no pair
            if (lane == 0) row[0] = APM_REC_INVALID;
            continue;
        }
        if (s == 0xffffffffffffffffull) { // APM_OCC_NO_START: the span pass found no occurrence
            if (lane == 0) row[0] = 0u;
            continue;
        }
        if (s > e) {
            if (lane == 0) row[0] = APM_REC_INVALID;
            continue;
        }
        const uint2 d = a.table[end.z];
        const int m = (int)d.y;
        if (m > APM_OCC_MAX_PATTERN_LEN || a.k >= m) continue; // (the host refuses such a set)
        const unsigned long long len = e + 1ull - s;
        if (len > (unsigned long long)(m + a.k) || len < (unsigned long long)(m - a.k)) { // the distance is at least |L - m| > k
            if (lane == 0) row[0] = 0u;
            continue;
        }
        if (s < a.text_off || e - a.text_off >= a.text_len) continue; // not covered: another shard's
        const int L = (int)len, W = apm_occ_words(m); // L <= m + k <= APM_OCC_ALIGN_MAX_COLS
        for (int i = lane; i < 256 * W; i += 64) s_eq[i] = 0u;
        for (int i = lane; i < L; i += 64) s_txt[i] = a.text[s - a.text_off + (unsigned long long)i];
        __syncthreads();
        const uint8_t *pat = a.image + d.x;
        for (int i = lane; i < m; i += 64) atomicOr(&s_eq[(int)pat[i] * W + (i >> 5)], 1u << (i & 31));
        __syncthreads();
        int n_ops = 0; // (every lane walks the same columns: LDS broadcasts)
        switch (W) {
        case 1: n_ops = oalign<1>(s_eq, s_txt, s_trace, m, L, a.k, lane, row); break;
        case 2: n_ops = oalign<2>(s_eq, s_txt, s_trace, m, L, a.k, lane, row); break;
        case 3: n_ops = oalign<3>(s_eq, s_txt, s_trace, m, L, a.k, lane, row); break;
        default: n_ops = oalign<4>(s_eq, s_txt, s_trace, m, L, a.k, lane, row); break;
        }
        if (lane == 0) row[0] = (uint32_t)n_ops; // 0: farther than k, nothing else stored
        __syncthreads(); // (the tables and the trace are the next pair's)
    }
}

} // namespace

// A fixed grid sized from the CU count, as the span pass's
hipError_t apm_launch_occ_align(const ApmOccAlignArgs &a, int n_cu, hipStream_t s) {
    hipLaunchKernelGGL(apm_occ_align_kernel, dim3((unsigned)n_cu * 16u), dim3(64), 0, s, a);
    return hipGetLastError();
}
