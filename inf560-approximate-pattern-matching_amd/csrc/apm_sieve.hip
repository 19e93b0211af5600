/*
 * apm_sieve.hip -- SIEVE: the first launch of the pipeline of the per-position key classes of the BANDED path (the
 * second, or both in one launch: apm_verify.hip).  Exact for the predicate dist <= k of the reference's window DP
 * (src/utils.c:76-99, applied at every text position by src/sequential.c:105-144; the lemmas are stated in
 * apm_banded.h).
 *
 *   apm_sieve2_kernel   one HBM pass over the text, wave-autonomous (no LDS text tile, no barrier in the loop):
 *                       1 KiB chunks, 16 bytes per lane (+ the 8 that follow), four chunks in flight per wave.
 *                       The lane's 24 bytes become a 48-bit string of 2-bit codes (v_dot4_u32_u8 packs four
 *                       codes per instruction); every EVEN position's 18-bit code word (9 bytes) is one lookup in
 *                       a 32 KiB LDS presence bitmap that answers for the position and the odd one behind it.
 *                       The hit masks of a 4 KiB block (32 bits per lane) leave with one coalesced store.
 *   apm_sieve2cf_kernel, apm_sieve2cfdp_kernel   ... with the code filter, and the window DP on codes, behind the lookups
 *                       (apm_sieve2cfdg_kernel, the diagonal form of that DP for k <= 3: apm_sieve_diag.hip; the body of
 *                       all of them: apm_sieve_body.h)
 *   apm_sieve8_kernel   the sampled form: one lookup per 8 text bytes
 *
 * They need a 16-byte aligned text pointer and a shard of < 4 GiB: the runtime scans bigger shards in pieces and falls
 * back to the LDS-tile kernels of apm_banded_tile.h for unaligned pointers.
 */
#include "apm_wave.h"
#include "apm_sieve.h"
#include "apm_launch.h"
#include "apm_sieve_body.h"


__global__ __launch_bounds__(APM_SIEVE2_BLOCK, 8) void apm_sieve2_kernel(ApmSieve2Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    apm_sieve2_body<false, false>(a, smem);
}

// the code-filter form: workgroups of up to 1024 threads share the tables (2 x 16 waves fill a CU)
__global__ __launch_bounds__(1024, 8) void apm_sieve2cf_kernel(ApmSieve2Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    apm_sieve2_body<true, false>(a, smem);
}
// ... with the window DP on codes of short patterns' units (ApmSieve2Args::cf_o_dp; launched with the candidate list only)
__global__ __launch_bounds__(1024, 8) void apm_sieve2cfdp_kernel(ApmSieve2Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    apm_sieve2_body<true, true>(a, smem);
}

// Sampled form (stride 8): every key piece is >= 15 bytes long and therefore contains an 8-byte block that starts at a
// multiple of 8 in the text; one lookup per 8 text bytes in an 8 KiB bitmap over the blocks' 16-bit code words.  No
// bytes beyond the lane's 16 are needed.  ~25 VALU instructions per KiB: the pass is bound by HBM alone.
__global__ __launch_bounds__(APM_SIEVE2_BLOCK, 8) void apm_sieve8_kernel(ApmSieve2Args a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if ((int)blockIdx.x >= a.n_main_blocks) { // extra workgroups: truncated tail windows (one pattern each)
        apm_tail_body(a.tail, (int)blockIdx.x - a.n_main_blocks, reinterpret_cast<uint4 *>(smem), tid);
        return;
    }
    apm_stage_image(reinterpret_cast<uint4 *>(smem), a.bitmap, 512, tid, APM_SIEVE2_BLOCK);
    __syncthreads();
    const int64_t W = (int64_t)a.n_main_blocks * (APM_SIEVE2_BLOCK / 64);
    const int64_t nch = a.nchunks;
    // (one resource over the shard and 32-bit offsets, as in apm_sieve2_body; chunks behind the range: no load at all)
    const __amdgpu_buffer_rsrc_t rs_all =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.text), 0, (int)(uint32_t)a.avail_pad, 0x00020000);
    const uint32_t t0_32 = (uint32_t)a.tile0, lane16 = 16u * (uint32_t)lane;
    auto load_chunk = [&](int64_t cc, u32x4 &r) __attribute__((always_inline)) {
        r = __builtin_amdgcn_raw_buffer_load_b128(rs_all, (int)(cc < nch ? t0_32 + (uint32_t)cc * 1024u + lane16 : 0xfffffff0u), 0, 0);
    };
    const uint32_t cs = (uint32_t)a.code_shift;
    auto hit_bits = [&](const u32x4 &v, int64_t cc) __attribute__((always_inline)) { // bit t = block at byte 8 t of the lane
        const uint32_t slo = apm_pack16(v.x, v.y, v.z, v.w, cs);
        const uint32_t w0 = *(const apm_lds_u32 *)(uintptr_t)((slo << 2) & 0x1ffcu), w1 = *(const apm_lds_u32 *)(uintptr_t)((slo >> 14) & 0x1ffcu);
        uint32_t hits = ((w0 >> ((slo >> 11) & 31u)) & 1u) | (((w1 >> (slo >> 27)) & 1u) << 1);
#ifdef APM_MEASURE
        if (APM_SKIP(a, 1)) hits = 0;
#endif
        return cc < nch ? hits : 0u;
    };
    int64_t c = ((int64_t)blockIdx.x * (APM_SIEVE2_BLOCK / 64) + wv) * 4; // four neighbouring chunks per wave
    u32x4 r0, r1, r2, r3;
    load_chunk(c, r0);
    load_chunk(c + 1, r1);
    load_chunk(c + 2, r2);
    load_chunk(c + 3, r3);
    for (; c < nch; c += 4 * W) {
        uint32_t h0, h1, h2, h3;
        { const u32x4 v = r0; load_chunk(c + 4 * W, r0); h0 = hit_bits(v, c); }
        { const u32x4 v = r1; load_chunk(c + 4 * W + 1, r1); h1 = hit_bits(v, c + 1); }
        { const u32x4 v = r2; load_chunk(c + 4 * W + 2, r2); h2 = hit_bits(v, c + 2); }
        { const u32x4 v = r3; load_chunk(c + 4 * W + 3, r3); h3 = hit_bits(v, c + 3); }
        // the block's hit masks (two lookups per lane and chunk): one coalesced 256-byte store per wave and 4 KiB
        a.masks[(size_t)(c >> 2) * 64 + (size_t)lane] = h0 | (h1 << 8) | (h2 << 16) | (h3 << 24);
    }
}

static size_t apm_sieve2cf_lds_bytes(int cf_len, int threads, bool dp) {
    return (size_t)32768 + (size_t)cf_len + (size_t)(threads / 64) * (APM_CF_WAVE_BYTES + (dp ? APM_CF_DP_PEND_BYTES : 0)) + 16; // (... | the candidate list's two counters)
}

// workgroup size (a multiple of 64) and workgroups per CU that put the most waves on a CU for this code-filter image
// the code-filter kernel of a window-DP form (apm_cf_dp_form)
static const void *apm_sieve2cf_fn(int dp_form) {
    return dp_form == 2 ? apm_sieve2cfdg_fn() : dp_form == 1 ? (const void *)apm_sieve2cfdp_kernel : (const void *)apm_sieve2cf_kernel;
}

int apm_sieve2cf_geometry(int cf_len, int dp_form, int *threads) {
    const bool dp = dp_form != 0;
    const void *fn = apm_sieve2cf_fn(dp_form);
    apm_ensure_max_lds(fn);
#ifdef APM_MEASURE
    static const int forced = getenv("APM_CF_THREADS") ? atoi(getenv("APM_CF_THREADS")) : 0;
#else
    constexpr int forced = 0;
#endif
    return apm_best_geometry([&](int) { return fn; }, 1024, 256, -64, [&](int t) { return apm_sieve2cf_lds_bytes(cf_len, t, dp); }, INT_MAX, forced, threads);
}

int apm_sieve2cf_blocks(const ApmSieve2Args &a, int n_cu) {
    const int wpb = a.cf_threads / 64;
    if (a.nchunks <= 0 || wpb < 1 || a.cf_blocks_per_cu < 1) return 0;
    const int64_t want = (a.nchunks + 4 * wpb - 1) / (4 * wpb), cap = (int64_t)n_cu * a.cf_blocks_per_cu;
    return (int)(want < cap ? want : cap);
}

hipError_t apm_launch_sieve2(const ApmSieve2PoolArgs &a, int n_cu, hipStream_t s, bool dp_diag, int *cf_waves, int *cf_dp_form, int *clist_pools) {
    if (cf_waves) *cf_waves = 0;
    if (cf_dp_form) *cf_dp_form = 0;
    if (clist_pools) *clist_pools = 0;
    if (a.nchunks <= 0) return hipSuccess;
    if (a.avail_pad > APM_SIEVE_MAX_BYTES || a.tile0 < 0) return hipErrorInvalidValue; // (32-bit offsets, the loads a wave issues ahead included)
    ApmSieve2PoolArgs args = a; // (the kernels of this unit take its ApmSieve2Args part: the leading bytes)
#ifdef APM_MEASURE
    if (const char *e = getenv("APM_MEASURE_SKIP")) args.skip_mask = atoi(e);
#endif
    void *kargs[] = {&args};
    if (a.stride != 8 && a.cf_image) { // the code-filter form
        const int threads = a.cf_threads;
        if (threads < 128 || threads > 1024 || (threads & 63) || a.cf_blocks_per_cu < 1) return hipErrorInvalidValue;
        const int64_t nb = apm_sieve2cf_blocks(a, n_cu);
        if (a.clist && (!a.blist || !a.clist_cnt || a.clist_cap < 1u)) return hipErrorInvalidValue; // (what does not fit a region leaves through the block list)
        args.n_main_blocks = (int)nb;
#ifdef APM_CF_NODP /* (A/B builds: the code filter without its third stage) */
        const bool dp = false;
#else
        const bool dp = a.clist && a.cf_o_dp > 0; // (the DP's survivors leave through the list only)
#endif
        if (dp && (a.cf_dp_cols < 1 || a.cf_dp_cols > APM_CF_DP_COLS || a.cf_dp_k < 0 || a.cf_o_dp + 128 > a.cf_len)) return hipErrorInvalidValue;
        const int dp_form = apm_cf_dp_form(dp, a.cf_dp_k, dp_diag);
        const void *fn = apm_sieve2cf_fn(dp_form);
        // pooled hand-over of the list (ApmSieve2PoolArgs): the diagonal kernel's only -- the others are pinned as they are
        const bool pooled = dp_form == 2 && a.cpool != nullptr;
        if (pooled) {
            if (!a.cpool_cnt || !a.cpool_cnt_next || a.cpool_n < 1 || a.cpool_next_n < 0) return hipErrorInvalidValue;
            args.cpool_n = (int)std::min<int64_t>(a.cpool_n, nb);
            const int64_t regions_per_pool = (nb + args.cpool_n - 1) / args.cpool_n;
            if ((int64_t)a.cpool_cap < regions_per_pool * (int64_t)a.clist_cap) return hipErrorInvalidValue; // (a pool takes all its regions, full)
        } else {
            args.cpool = nullptr;
        }
        const size_t lds = apm_sieve2cf_lds_bytes(a.cf_len, threads, dp);
        if (lds > (size_t)160 * 1024) return hipErrorInvalidValue;
        if (lds > 48 * 1024) apm_ensure_max_lds(fn); // (per device: the geometry query ran on one)
        if (cf_dp_form) *cf_dp_form = dp_form;
        if (clist_pools) *clist_pools = pooled ? args.cpool_n : 0;
        if (cf_waves) *cf_waves = (int)nb * (threads / 64); // (= the kernel's W: a wave's blocks are w, w + W, ...)
        return hipLaunchKernel(fn, dim3((unsigned)(nb + a.n_tail)), dim3((unsigned)threads), kargs, lds, s);
    }
    const size_t lds = 32768;
    const int64_t want = (a.nchunks + 4 * (APM_SIEVE2_BLOCK / 64) - 1) / (4 * (APM_SIEVE2_BLOCK / 64));
    const int64_t cap = (int64_t)n_cu * 4; // = the kernel's launch bound (4 x 512 threads per CU; 4 x 32 KiB of LDS)
    const int64_t nb = want < cap ? want : cap;
    args.n_main_blocks = (int)nb;
    if (a.stride == 8)
        return hipLaunchKernel((const void *)apm_sieve8_kernel, dim3((unsigned)(nb + a.n_tail)), dim3(APM_SIEVE2_BLOCK), kargs, 8192, s);
    return hipLaunchKernel((const void *)apm_sieve2_kernel, dim3((unsigned)(nb + a.n_tail)), dim3(APM_SIEVE2_BLOCK), kargs, lds, s);
}
