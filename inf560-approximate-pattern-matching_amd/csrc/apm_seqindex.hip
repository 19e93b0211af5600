/*
 * apm_seqindex.hip -- the sequence index of a normalised source (apm_index_sequences_device) and the locate pass over match
 * records (apm_locate_records_device); the arithmetic is apm_seqindex.h's, the view of the source and the block helpers are
 * apm_textnorm.h's.
 *
 * Three launches build the table, none of which waits on another workgroup:
 *   count    one wavefront per 4 KiB block: the block's header opens ('>' at a line start; no header state is needed)
 *   scan     ONE workgroup sums the counts into 64-bit prefixes and the total
 *   emit     one wavefront per block: the masks again with the block's state and kept prefix from the normalisation's map,
 *            every open's entry at 1 + prefix + its rank; the first wavefront also writes entry 0 and the sentinel
 * The fourth kernel locates records: one wavefront per record resolves the record's block -- (pos + lead) / 4096, no search
 * -- for "is the byte kept" and its index in the kept text, then searches the table by hdr_off, 64 probes a round.
 */
#include "apm_wave.h"
#include "apm_seqindex.h"

#include <algorithm>

namespace {

// ---- 1. count ----
__global__ __launch_bounds__(APM_BLOCK) void apm_sq_count_kernel(const ApmSqIndexArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * APM_BLOCK + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * APM_BLOCK) >> 6;
    for (uint64_t b = wave; b < a.src.n_blocks; b += n_waves) {
        uint32_t w[4][4], valid[4];
        tn_load_block(a.src, b, lane, w, valid);
        uint32_t ls = tn_block_line_start(a.src, b), cnt = 0u;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const TnChunk t = tn_chunk(w[c], valid[c], a.src.flags, lane, ls);
            cnt += (uint32_t)__builtin_popcount(apm_sq_opens(t.m, a.src.flags, t.ls_in));
        }
        const uint32_t sum = apm_wave_incl_scan(cnt);
        if (lane == 63u) a.count[b] = sum;
    }
}

// ---- 2. scan: one workgroup ----
__global__ __launch_bounds__(APM_SQ_SCAN_THREADS) void apm_sq_scan_kernel(const ApmSqIndexArgs a) {
    __shared__ uint32_t s_wave[2][APM_SQ_SCAN_THREADS / 64]; // the waves' sums, two rounds' worth
    const uint64_t nb = a.src.n_blocks;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint4 *cnt4 = reinterpret_cast<const uint4 *>(a.count); // (allocated in whole scan chunks)
    unsigned long long before = 0ull; // opens in front of the chunk
    uint32_t par = 0u;
    for (uint64_t c0 = 0; c0 < nb; c0 += APM_SQ_SCAN_CHUNK, par ^= 1u) {
        const uint64_t i0 = c0 + (uint64_t)tid * 4u;
        const uint4 cur = cnt4[(c0 >> 2) + tid];
        uint32_t v[4] = {cur.x, cur.y, cur.z, cur.w}, sum = 0u;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (i0 + q >= nb) v[q] = 0u; // (behind the last block: never written)
            sum += v[q];
        }
        const uint32_t incl = apm_wave_incl_scan(sum); // (a chunk holds at most 4096 x 2048 opens)
        if (lane == 63u) s_wave[par][wave] = incl;
        __syncthreads();
        uint32_t lower = 0u, all = 0u; // the waves below this one; the whole chunk
        for (uint32_t x = 0; x < APM_SQ_SCAN_THREADS / 64; ++x) {
            if (x == wave) lower = all;
            all += s_wave[par][x];
        }
        unsigned long long ex = before + lower + incl - sum;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (i0 + q < nb) a.prefix[i0 + q] = ex;
            ex += v[q];
        }
        before += all;
    }
    if (tid == 0) {
        a.prefix[nb] = before;
        *a.total = before;
    }
}

// ---- 3. emit ----
__global__ __launch_bounds__(APM_BLOCK) void apm_sq_emit_kernel(const ApmSqIndexArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * APM_BLOCK + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * APM_BLOCK) >> 6;
    if (wave == 0 && lane < 2u) { // entry 0 and the sentinel
        apm_seq e;
        e.hdr_off = lane ? a.src_len : APM_SEQ_NO_HEADER;
        e.t_begin = lane ? a.kept : 0ull;
        a.table[lane ? a.n_seq : 0ull] = e;
    }
    for (uint64_t b = wave; b < a.src.n_blocks; b += n_waves) {
        const unsigned long long e = a.map[b];
        const unsigned long long first = 1ull + a.prefix[b];
        if (a.prefix[b + 1] == a.prefix[b]) continue; // (no open in the block)
        uint32_t w[4][4], valid[4];
        tn_load_block(a.src, b, lane, w, valid);
        uint32_t ls = tn_block_line_start(a.src, b);
        uint32_t h = (uint32_t)(e >> APM_TN_STATE_BIT), run = 0u; // run: kept bytes (low half) and opens (high half) so far
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            const TnChunk t = tn_chunk(w[c], valid[c], a.src.flags, lane, ls);
            const ApmTnLane r = apm_tn_resolve(t.m, valid[c], a.src.flags, apm_tn_state_at(t.fixed, t.value, lane, h), t.ls_in);
            const uint32_t opens = apm_sq_opens(t.m, a.src.flags, t.ls_in);
            const uint32_t mine = r.count | ((uint32_t)__builtin_popcount(opens) << 16); // (at most 1024 and 512 a chunk)
            const uint32_t incl = apm_wave_incl_scan(mine);
            const uint32_t ex = run + incl - mine;
            const unsigned long long index = first + (ex >> 16);
            // (the lane's entries end in front of the sentinel for an unchanged source; a changed one must not write beyond the table)
            const uint32_t take = index + (uint32_t)__builtin_popcount(opens) <= a.n_seq ? opens : 0u;
            apm_sq_emit(a.table, index, take, r.keep, b * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u, a.src.lead,
                        (e & APM_TN_PREFIX_MASK) + (ex & 0xffffu));
            run += tn_wave_total(incl);
            h = apm_tn_state_at(t.fixed, t.value, 64u, h);
        }
    }
}

// ---- 4. locate: one wavefront per record ----
__global__ __launch_bounds__(APM_BLOCK) void apm_sq_locate_kernel(const ApmSqLocateArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * APM_BLOCK + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * APM_BLOCK) >> 6;
    const unsigned long long have = *a.n_rec, n = have < a.cap ? have : a.cap;
    for (unsigned long long r = wave; r < n; r += n_waves) {
        const uint4 rec = a.rec[r];
        const unsigned long long pos = (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)rec.x) |
                                       ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)rec.y) << 32);
        const uint32_t pattern = (uint32_t)__builtin_amdgcn_readfirstlane((int)rec.z);
        apm_loc out = apm_sq_invalid();
        if (pattern < a.n_patterns && pos < a.src_len) {
            const ApmSqAt at = apm_sq_at(pos, a.src.lead); // (at.block < n_blocks: pos lies in the source)
            const unsigned long long e = a.map[at.block];
            uint32_t w[4][4], valid[4];
            tn_load_block(a.src, at.block, lane, w, valid);
            uint32_t ls = tn_block_line_start(a.src, at.block);
            uint32_t h = (uint32_t)(e >> APM_TN_STATE_BIT), run = 0u, in_block = 0u, kept = 0u;
#pragma unroll
            for (uint32_t c = 0; c < 4; ++c) {
                if (c > at.chunk) continue; // (wave-uniform)
                const TnChunk t = tn_chunk(w[c], valid[c], a.src.flags, lane, ls);
                const ApmTnLane res = apm_tn_resolve(t.m, valid[c], a.src.flags, apm_tn_state_at(t.fixed, t.value, lane, h), t.ls_in);
                const uint32_t incl = apm_wave_incl_scan(res.count);
                if (c == at.chunk) { // the lane that holds the byte: is it kept, and how many kept bytes of the block lie in front
                    const uint32_t mine = run + incl - res.count + (uint32_t)__builtin_popcount(res.keep & ((1u << at.bit) - 1u));
                    in_block = (uint32_t)__shfl((int)mine, (int)at.lane);
                    kept = (uint32_t)__shfl((int)((res.keep >> at.bit) & 1u), (int)at.lane);
                }
                run += tn_wave_total(incl);
                h = apm_tn_state_at(t.fixed, t.value, 64u, h);
            }
            if (kept) {
                const unsigned long long c_idx = (e & APM_TN_PREFIX_MASK) + in_block;
                uint64_t lo = 0, hi = a.n_seq;
                while (hi - lo > 1) {
                    const bool ok = apm_sq_probe(a.table, lo, hi, lane, pos);
                    apm_sq_narrow(lo, hi, (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(ok)));
                }
                out = apm_sq_location(c_idx, a.pat[pattern].y, a.kept, (uint32_t)lo, a.table[lo].t_begin, a.table[lo + 1].t_begin);
            }
        }
        if (lane == 0u)
            reinterpret_cast<uint4 *>(a.loc)[r] = make_uint4((uint32_t)out.off, (uint32_t)(out.off >> 32), out.seq, out.flags);
    }
}

} // namespace

// fixed grids sized from the CU count; every kernel strides over its blocks or records
hipError_t apm_launch_sq_count(const ApmSqIndexArgs &a, int n_cu, hipStream_t s) {
    const uint64_t want = (a.src.n_blocks + APM_BLOCK / 64 - 1) / (APM_BLOCK / 64);
    hipLaunchKernelGGL(apm_sq_count_kernel, dim3((unsigned)std::min<uint64_t>(want, (uint64_t)n_cu * 8u)), dim3(APM_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t apm_launch_sq_scan(const ApmSqIndexArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(apm_sq_scan_kernel, dim3(1), dim3(APM_SQ_SCAN_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t apm_launch_sq_emit(const ApmSqIndexArgs &a, int n_cu, hipStream_t s) {
    const uint64_t want = std::max<uint64_t>((a.src.n_blocks + APM_BLOCK / 64 - 1) / (APM_BLOCK / 64), 1); // (an empty source: the two fixed entries)
    hipLaunchKernelGGL(apm_sq_emit_kernel, dim3((unsigned)std::min<uint64_t>(want, (uint64_t)n_cu * 8u)), dim3(APM_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t apm_launch_sq_locate(const ApmSqLocateArgs &a, int n_cu, hipStream_t s) {
    hipLaunchKernelGGL(apm_sq_locate_kernel, dim3((unsigned)n_cu * 8u), dim3(APM_BLOCK), 0, s, a);
    return hipGetLastError();
}
