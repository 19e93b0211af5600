/*
 * apm_seqnear.hip -- the nearest-occurrence search per sequence: a scan that reduces, for every (sequence, pattern) pair of a
 * sequence table, the occurrence search's E(e) over the ends of that sequence -- the sequence a text of its own -- to ONE key
 * (apm_nearest.h's key; apm_seqnear.h's walk), and a finishing pass that turns the keys into end and start records.
 * Compiled once; neither feeds the counting kernels' sinks.
 *
 * Scan ("snear"): the geometry and the text delivery of the nearest scan (apm_nearest.hip) -- a workgroup is APM_OCC_SLOTS
 * waves, wave w walks pattern blockIdx.y * APM_OCC_SLOTS + w with its Eq table in its slot of LDS, lane l the segment
 * blockIdx.x * 64 + l, text as per-lane guarded 16-byte streams.  The column loop is wave-uniform; what a lane does at a
 * sequence boundary (flush its key, move on, start again) is the only divergent code.  A flush reads the key first and
 * issues its atomicMin only where it would lower it: the keys only ever fall, so a stale read costs an atomic, never an
 * answer.  Behind the walk, if every live lane of the wave ended in the same sequence, the wave reduces its 64 keys and
 * issues one flush -- on a text of one sequence that is the nearest scan's one atomic per wave; otherwise every lane flushes
 * for itself.
 *
 * Finish ("snspan"): one wavefront = workgroup per (sequence, pattern) PAIR, grid-stride with 64-bit indices; the nearest
 * search's finishing pass with the span walk's columns clamped to the sequence: cols = min(m + d, e + 1 - t_begin[s]).
 */
#include "apm_recpass.h"
#include "apm_occ_device.h"
#include "apm_seqnear.h"

namespace {

struct SeqTab { // the sequence table: only t_begin is read
    const apm_seq *seqs;
    __device__ __forceinline__ unsigned long long begin(unsigned long long s) const { return seqs[s].t_begin; }
};

struct SeqKeys { // the keys of one pattern: keys[s * P + pattern]
    unsigned long long *keys;
    unsigned long long n_patterns, pattern;
    __device__ __forceinline__ void operator()(unsigned long long s, unsigned long long key) const {
        unsigned long long *at = keys + (s * n_patterns + pattern);
        if (key < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(at, key);
    }
};

template <int W>
__device__ __forceinline__ void seqnear_walk(const ApmSeqnearArgs &a, const uint32_t *tab, const SeqKeys &flush, int m, long long b, long long e,
                                             unsigned long long *best, unsigned long long *seq) {
    const ApmOccTxt t{a.text, (long long)a.text_off, (long long)a.text_len};
    apm_seqnear_walk<W>(t, ApmOccEq<W>{tab}, SeqTab{a.seqs}, a.n_seq, flush, m, b, e, apm_seqnear_steps((int)a.segment, m), best, seq);
}

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(64 * APM_OCC_SLOTS) void apm_seqnear_scan_kernel(const ApmSeqnearArgs a) {
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
    const SeqKeys flush{a.keys, a.n_patterns, pattern};
    unsigned long long key = APM_NEAREST_NONE, s = 0;
    switch (apm_occ_words(m)) { // (wave-uniform)
    case 1: seqnear_walk<1>(a, tab, flush, m, b, e, &key, &s); break;
    case 2: seqnear_walk<2>(a, tab, flush, m, b, e, &key, &s); break;
    case 3: seqnear_walk<3>(a, tab, flush, m, b, e, &key, &s); break;
    default: seqnear_walk<4>(a, tab, flush, m, b, e, &key, &s); break;
    }
    // what the walks left: one sequence in every live lane -- the wave's smallest key, one flush; else a flush per lane
    const bool live = b < e;
    const unsigned long long lives = __ballot(live);
    if (!lives) return;
    const unsigned long long s0 = shfl64(s, __ffsll((long long)lives) - 1);
    if (__ballot(live && s != s0) == 0ull) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), o, 64);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            key = other < key ? other : key;
        }
        if (lane == 0 && key != APM_NEAREST_NONE) flush(s0, key);
    } else if (key != APM_NEAREST_NONE) {
        flush(s, key);
    }
}

__device__ __forceinline__ uint4 seqnear_record(unsigned long long pos, uint32_t pattern, uint32_t dist) {
    return make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), pattern, dist);
}

template <int W>
__device__ __forceinline__ void span_walk(const uint32_t *tab, const uint8_t *bytes, int m, int cols, int *d, int *l) {
    apm_occ_span_walk<W>(ApmOccEq<W>{tab}, ApmSpanBack{bytes}, m, cols, d, l);
}

__global__ __launch_bounds__(64) void apm_seqnear_span_kernel(const ApmSnspanArgs a) {
    __shared__ uint32_t s_eq[kApmOccEqWords];
    __shared__ uint8_t s_txt[2 * APM_OCC_MAX_PATTERN_LEN]; // m + d <= 2 m - 1 bytes
    const int lane = (int)threadIdx.x;
    const unsigned long long none = 0xffffffffffffffffull; // APM_OCC_NO_START
    const unsigned long long pairs = a.n_seq * (unsigned long long)a.n_patterns;
    for (unsigned long long r = blockIdx.x; r < pairs; r += gridDim.x) {
        const unsigned long long s = r / a.n_patterns;
        const uint32_t i = (uint32_t)(r - s * a.n_patterns);
        unsigned long long key = a.keys[r]; // (the same in every lane: made wave-uniform for the compiler's sake)
        key = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32)) << 32) |
              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key);
        const uint2 d = a.table[i];
        const int m = (int)d.y;
        if (m > APM_OCC_MAX_PATTERN_LEN) continue; // (the host refuses such a set)
        const int dist = (int)APM_NEAREST_DIST(key);
        const unsigned long long e = APM_NEAREST_END(key);
        const unsigned long long first = a.seqs[s].t_begin, behind = a.seqs[s + 1ull].t_begin;
        if (key == APM_NEAREST_NONE || dist >= m || e < first || e >= behind) { // no end below m; or a key no scan made
            const uint4 rec = seqnear_record(none, i, key == APM_NEAREST_NONE ? (uint32_t)m : APM_REC_INVALID);
            if (lane == 0) {
                a.end[r] = rec;
                if (a.start) a.start[r] = rec;
            }
            continue;
        }
        if (lane == 0) a.end[r] = seqnear_record(e, i, (uint32_t)dist);
        if (!a.start) continue;
        const int cols = apm_occ_span_cols(m, dist, e - first); // min(m + d, e + 1 - t_begin[s])
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
        if (lane == 0) a.start[r] = ds <= dist ? seqnear_record(e + 1ull - (unsigned long long)ls, i, (uint32_t)ds) : seqnear_record(none, i, (uint32_t)(dist + 1));
        __syncthreads(); // (the tables are the next pair's)
    }
}

} // namespace

hipError_t apm_launch_seqnear(const ApmSeqnearArgs &a, hipStream_t s) {
    const dim3 grid((a.n_segments + APM_OCC_LANES - 1) / APM_OCC_LANES, (a.n_patterns + APM_OCC_SLOTS - 1) / APM_OCC_SLOTS);
    hipLaunchKernelGGL(apm_seqnear_scan_kernel, grid, dim3(64 * APM_OCC_SLOTS), 0, s, a);
    return hipGetLastError();
}

// one workgroup per (sequence, pattern) pair, no more than the span pass's fixed grid
hipError_t apm_launch_snspan(const ApmSnspanArgs &a, int n_cu, hipStream_t s) {
    const unsigned long long most = (unsigned long long)n_cu * 16ull, pairs = a.n_seq * (unsigned long long)a.n_patterns;
    hipLaunchKernelGGL(apm_seqnear_span_kernel, dim3((unsigned)(pairs < most ? pairs : most)), dim3(64), 0, s, a);
    return hipGetLastError();
}
