/*
 * apm_seqocc.hip -- the occurrence search per sequence: the occurrence scan and its span pass (apm_occ.hip) with every
 * sequence of a sequence table a text of its own (apm_seqocc.h states the semantics and the boundary-aware walk).  Compiled
 * once; neither feeds the counting kernels' sinks.
 *
 * Scan ("socc"): the geometry and the text delivery of the occurrence scan -- a workgroup is APM_OCC_SLOTS waves, wave w walks
 * pattern blockIdx.y * APM_OCC_SLOTS + w with its Eq table in its slot of LDS, lane l the segment blockIdx.x * 64 + l, text as
 * per-lane guarded 16-byte streams.  The column loop and the sink's ballot are wave-uniform; what a lane does at a sequence
 * boundary (find the next one, start its column again) is the only divergent code.  Ends are appended wave-aggregated and
 * counted per pattern as apm_occ_scan_kernel does.
 *
 * Span ("sspan"): one record per wavefront = workgroup, grid-stride; the span kernel with its columns clamped to the
 * sequence of the end, cols = min(m + k, e + 1 - t_begin[s(e)]), and s(e) stored into an optional parallel array.
 */
#include "apm_recpass.h"
#include "apm_occ_device.h"
#include "apm_seqocc.h"

namespace {

struct SeqTab { // the sequence table: only t_begin is read
    const apm_seq *seqs;
    __device__ __forceinline__ unsigned long long begin(unsigned long long s) const { return seqs[s].t_begin; }
};

struct SeqoccSink { // wave-aggregated append of the ends reported in one column
    const ApmOccArgs &a;
    uint32_t pattern;
    __device__ __forceinline__ void operator()(bool hit, long long end, int dist) const {
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(hit);
        if (mask == 0ull) return; // (wave-uniform)
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        unsigned long long base = 0ull;
        if (hit && rank == 0u) base = atomicAdd(a.n_found, (unsigned long long)__builtin_popcountll(mask));
        const int leader = __builtin_ctzll(mask);
        const uint32_t blo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, leader);
        const uint32_t bhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base >> 32), leader);
        const unsigned long long slot = (((unsigned long long)bhi << 32) | blo) + rank;
        if (hit && slot < a.cap) a.out[slot] = make_uint4((uint32_t)end, (uint32_t)((unsigned long long)end >> 32), pattern, (uint32_t)dist);
    }
};

template <int W>
__device__ __forceinline__ unsigned seqocc_walk(const ApmSeqoccArgs &a, const uint32_t *tab, uint32_t pattern, int m, long long b, long long e) {
    const ApmOccTxt t{a.text, (long long)a.text_off, (long long)a.text_len};
    const ApmOccEq<W> eq{tab};
    SeqoccSink sink{a, pattern};
    return apm_seqocc_walk<W>(t, eq, SeqTab{a.seqs}, a.n_seq, m, a.k, b, e, (long long)a.n_total, a.flags, apm_occ_steps((int)a.segment, m, a.k), sink);
}

__global__ __launch_bounds__(64 * APM_OCC_SLOTS) void apm_seqocc_scan_kernel(const ApmSeqoccArgs a) {
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
        served = m >= 1 && m <= APM_OCC_MAX_PATTERN_LEN && a.k < m;
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
    unsigned found = 0;
    switch (apm_occ_words(m)) { // (wave-uniform)
    case 1: found = seqocc_walk<1>(a, tab, pattern, m, b, e); break;
    case 2: found = seqocc_walk<2>(a, tab, pattern, m, b, e); break;
    case 3: found = seqocc_walk<3>(a, tab, pattern, m, b, e); break;
    default: found = seqocc_walk<4>(a, tab, pattern, m, b, e); break;
    }
    // the wave's ends into the pattern's count: a DPP-free butterfly over 64 lanes, one atomic
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) found += (unsigned)__shfl_xor((int)found, o, 64);
    if (lane == 0 && found) atomicAdd(&a.counts[pattern], (unsigned long long)found);
}

template <int W>
__device__ __forceinline__ void span_walk(const uint32_t *tab, const uint8_t *bytes, int m, int cols, int *d, int *l) {
    apm_occ_span_walk<W>(ApmOccEq<W>{tab}, ApmSpanBack{bytes}, m, cols, d, l);
}

__global__ __launch_bounds__(64) void apm_seqocc_span_kernel(const ApmSeqspanArgs a) {
    __shared__ uint32_t s_eq[kApmOccEqWords];
    __shared__ uint8_t s_txt[2 * APM_OCC_MAX_PATTERN_LEN]; // m + k <= 2 m - 1 bytes
    const unsigned long long n = apm_rec_count(a);
    const int lane = (int)threadIdx.x;
    for (unsigned long long idx = blockIdx.x; idx < n; idx += gridDim.x) {
        const uint4 rec = apm_rec_load_uniform(a, idx);
        const unsigned long long e = (unsigned long long)rec.x | ((unsigned long long)rec.y << 32);
        if (rec.z >= a.n_patterns || e >= a.n_total) { // names no end
            if (lane == 0) {
                a.span[idx] = make_uint4(0xffffffffu, 0xffffffffu, rec.z, APM_REC_INVALID);
                if (a.seq) a.seq[idx] = 0xffffffffu;
            }
            continue;
        }
        const uint2 d = a.table[rec.z];
        const int m = (int)d.y;
        if (m > APM_OCC_MAX_PATTERN_LEN || a.k >= m) continue; // (the host refuses such a set)
        if (e - a.text_off >= a.text_len || e < a.text_off) continue; // not covered: another shard's
        unsigned long long s = apm_seqnear_find(SeqTab{a.seqs}, a.n_seq, e), first = a.seqs[s].t_begin; // (the same in every lane)
        s = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)s);
        first = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(first >> 32)) << 32) |
                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)first);
        if (first > e) first = e; // (a table that breaks its promise)
        const int cols = apm_seqocc_span_cols(m, a.k, e, first);
        const unsigned long long lo = e + 1ull - (unsigned long long)cols;
        if (lo < a.text_off) continue; // not covered: another shard's
        const int W = apm_occ_words(m);
        for (int i = lane; i < 256 * W; i += 64) s_eq[i] = 0u;
        for (int i = lane; i < cols; i += 64) s_txt[i] = a.text[e - a.text_off - (unsigned long long)i];
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
        if (lane == 0) {
            const unsigned long long start = e + 1ull - (unsigned long long)ls;
            a.span[idx] = ds <= a.k ? make_uint4((uint32_t)start, (uint32_t)(start >> 32), rec.z, (uint32_t)ds)
                                    : make_uint4(0xffffffffu, 0xffffffffu, rec.z, (uint32_t)(a.k + 1));
            if (a.seq) a.seq[idx] = (uint32_t)s;
        }
        __syncthreads(); // (the tables are the next record's)
    }
}

} // namespace

hipError_t apm_launch_seqocc(const ApmSeqoccArgs &a, hipStream_t s) {
    const dim3 grid((a.n_segments + APM_OCC_LANES - 1) / APM_OCC_LANES, (a.n_patterns + APM_OCC_SLOTS - 1) / APM_OCC_SLOTS);
    hipLaunchKernelGGL(apm_seqocc_scan_kernel, grid, dim3(64 * APM_OCC_SLOTS), 0, s, a);
    return hipGetLastError();
}

// A fixed grid sized from the CU count, as the span pass's
hipError_t apm_launch_seqspan(const ApmSeqspanArgs &a, int n_cu, hipStream_t s) {
    hipLaunchKernelGGL(apm_seqocc_span_kernel, dim3((unsigned)n_cu * 16u), dim3(64), 0, s, a);
    return hipGetLastError();
}
