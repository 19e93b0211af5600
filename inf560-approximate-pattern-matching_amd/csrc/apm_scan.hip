/*
 * apm_scan.hip -- the shard scan: every launch a call makes over one device's piece of the text, in stream order and
 * without a host sync.  Reads the plan (apm_plan.h, const here) and its device mirrors (apm_state.h); the only state
 * it keeps is per device: grown buffers, cached launch geometry, the last call's statistics.
 *
 * There is no CPU fallback in this file by design.
 */
#include "apm_state.h"
#include "apm_core.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

// ---- internal kernels defined here (tiny) ----
// statistics: number of set bits in the sieve's hit masks
__global__ void apm_popcount_kernel(const uint32_t *w, unsigned long long n, unsigned long long *sum) {
    unsigned long long acc = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
        acc += (unsigned long long)__popc(w[i]);
    for (int d = 32; d; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

// the same over the rows of the listed blocks, plus the entries of the candidate list's regions (the statistics of a pass
// that ran with the list: the other rows were never written)
__global__ void apm_popcount_listed_kernel(const uint32_t *w, const uint32_t *blist, const uint32_t *n_listed, const uint32_t *clist_cnt, int regions, unsigned long long *sum) {
    unsigned long long acc = 0;
    const unsigned long long n = (unsigned long long)*n_listed * 64ull, t0 = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (unsigned long long i = t0; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
        acc += (unsigned long long)__popc(w[(unsigned long long)blist[i >> 6] * 64ull + (i & 63ull)]);
    for (unsigned long long i = t0; i < (unsigned long long)regions; i += (unsigned long long)gridDim.x * blockDim.x) acc += clist_cnt[i];
    for (int d = 32; d; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(sum, acc);
}

// k >= m: every window start matches (the DP never exceeds m); one launch adds the window count to all of them
__global__ void apm_add_const_kernel(unsigned long long *counts, const int *idx, int n, unsigned long long v) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) atomicAdd(&counts[idx[i]], v);
}

// record calls (apm_find_all_buffer, apm_find_shard_device): the patterns with k >= m match at every window start --
// one record per (pattern, window start) of the owner range [ob, oe); out / count / cap as in ApmPosSink's record form
__global__ void apm_rec_const_kernel(uint4 *out, unsigned long long *count, unsigned long long cap, const int *idx, int n,
                                     unsigned long long ob, unsigned long long oe) {
    const unsigned long long span = oe - ob, total = span * (unsigned long long)n;
    __shared__ unsigned long long s_base;
    const unsigned long long first = (unsigned long long)blockIdx.x * blockDim.x;
    for (unsigned long long b0 = first; b0 < total; b0 += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long here = total - b0 < blockDim.x ? total - b0 : blockDim.x; // one reservation per workgroup and round
        __syncthreads();
        if (threadIdx.x == 0) s_base = atomicAdd(count, here);
        __syncthreads();
        const unsigned long long i = b0 + threadIdx.x, at = s_base + threadIdx.x;
        if (i < total && at < cap) {
            const unsigned long long pos = ob + i % span;
            out[at] = make_uint4((uint32_t)pos, (uint32_t)(pos >> 32), (uint32_t)idx[i / span], 0u);
        }
    }
}

int note_launch(apm_ctx *ctx, DeviceState &ds, const char *label) {
    ds.launches++;
    if (!ctx->timing_on || ds.n_stamps >= DeviceState::MAX_STAMPS) return APM_OK;
    hipEvent_t &e = ds.ev_launch[ds.n_stamps];
    if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    HIP_TRY(ctx, hipEventRecord(e, ds.stream));
    ds.launch_label[ds.n_stamps++] = label;
    return APM_OK;
}

int ensure_text(apm_ctx *ctx, DeviceState &ds, size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes <= ds.text_cap) return APM_OK;
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    return grow_device_buffer(ctx, ds, (void **)&ds.d_text, &ds.text_cap, bytes, 1);
}

// ---- environment switches of the scan, read once per process ----
static int env_int(const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; }
static int env_1_to_64(const char *name, int unset) { return getenv(name) ? std::max(1, std::min(64, env_int(name, 0))) : unset; }
struct ScanEnv {
    // FUSED form: one kernel per verify group sieves and verifies; the text leaves HBM once, no masks.  Measured on
    // MI355X (profiles/r02/fused_ab.txt): the sampled pipeline gains 15 % (cfg4 0.268 -> 0.228 ms per GiB: its
    // sieve is a few instructions per KiB, the verification hides behind the stream), the per-position one is
    // latency bound in either form and loses occupancy to the bigger kernel (cfg3 0.50 -> 0.48 at best, cfg5
    // 0.64 -> 1.08).  So: fused when the sieve is sampled; APM_FUSED=1 / 0 forces it on / off (A/B aid, and the
    // tests run both forms).
    int fused = env_int("APM_FUSED", -1);
    int blist = env_int("APM_SIEVE_BLIST", 1); // (A/B aid: 0 = the verify launches walk every mask row)
    // candidate list of the code-filter form: 32 entries allocated per 4 KiB block (half the bytes of the mask rows).
    // APM_SIEVE_CLIST=0 turns it off (A/B aid); APM_CLIST_REGION_CAP=n (1..64) shrinks every region to n entries (the
    // tests force the overflow path with it)
    int clist = env_int("APM_SIEVE_CLIST", 1);
    int clist_region_cap = env_1_to_64("APM_CLIST_REGION_CAP", 0);
    // (8: with 1 a planted occurrence's nominations scatter over as many waves, with 64 one wave walks two
    // occurrences of its region one after the other -- 0.06 against 0.037 ms on sparse sets of long patterns,
    // profiles/r03/clist_ab.txt; APM_CLIST_MIN_BATCH overrides, A/B aid)
    int clist_min_batch = env_1_to_64("APM_CLIST_MIN_BATCH", 8);
    // POOLED hand-over of the list (ApmSieve2PoolArgs; the diagonal sieve kernel only): its scanning workgroups move their
    // regions into this many pools, clamped to the region count, and the verify launch is given the pools as its regions.
    // APM_CLIST_POOLS=0 hands the regions over as they are (A/B aid, and the tests compare the two).  8: cfg3 on one box, three
    // rounds, ms per step: regions 0.2778-0.2792, 1 pool 0.2741-0.2746 (512 workgroups on one counter), 8 pools
    // 0.2719-0.2730, 32 0.2729-0.2735, 128 0.2730-0.2738; APM_CLIST_MIN_BATCH 4 and 2 on top of any of them lose 0.005 and
    // 0.009 (profiles/r12/pools_ab.txt): 8 stays
    int clist_pools = std::max(0, env_int("APM_CLIST_POOLS", 8));
    // the sieve's window DP on codes takes its diagonal form for k <= 3 (apm_cf_dp_form); APM_CF_DP_DIAG=0 keeps the column
    // form (A/B aid, and the tests compare the two)
    int cf_dp_diag = env_int("APM_CF_DP_DIAG", 1);
    int filter_dma = env_int("APM_FILTER_DMA", 1); // 0: register-staged tiles even for aligned text (A/B aid)
    // APM_FILTER_STREAM=0 forces the tile kernel (A/B aid); default: stream kernel for the sampled classes.
    // per-position classes stream only when candidates are expected to be rare (verification then
    // reads global text, dense 64-candidate batches); APM_FILTER_STREAM=2 forces, 3 forbids (A/B aid)
    int filter_stream = env_int("APM_FILTER_STREAM", 1);
#ifdef APM_MEASURE
    int qcap_s1 = env_int("APM_QCAP_S1", 0); // overrides the per-tile candidate queue of the per-position classes
    int bpc_cap = env_int("APM_BPC_CAP", 0); // caps the tile kernel's workgroups per CU
#endif
};
static const ScanEnv &scan_env() {
    static const ScanEnv env;
    return env;
}

// ---- one shard, as every launch of the call sees it ----
struct ShardGeom {
    const uint8_t *text;          // device; every position below is relative to text[0]
    int64_t jb, je;               // window starts to decide
    int64_t nrel;                 // end of the whole text
    int64_t avail;                // valid text bytes
    int64_t avail_pad;            // ... rounded up so that text + avail_pad is 16-byte aligned (same allocation granule)
    int band;                     // k / 2
    ApmPosSink sink;
    unsigned long long *counts;
    bool rec_on;                  // record call: the SAME launches with the same geometry out of the record build of the kernel files (apm_rec.h)
    bool aligned() const { return (reinterpret_cast<uintptr_t>(text) & 15u) == 0; }
};
#define APM_PICK(g, fn) ((g).rec_on ? fn##_rec : fn)

// the fields every launch-argument structure starts from, for the window starts [g.jb, je)
template <typename Args> static void set_common(Args &a, const apm_ctx *ctx, const ShardGeom &g, int64_t je) {
    a.text = g.text;
    a.jb = g.jb;
    a.je = je;
    a.nrel = g.nrel;
    a.counts = g.counts;
    a.k = ctx->k;
    a.pos = g.sink;
}

// first window start of tile 0: the last one <= jb with text + tile0 - front 16-byte aligned (16-byte loads; the kernels skip j < jb)
static int64_t aligned_tile0(const ShardGeom &g, int front = 0) {
    return g.jb - (int64_t)((reinterpret_cast<uintptr_t>(g.text) + (uintptr_t)g.jb - (uintptr_t)front) & 15u);
}

static bool has_tail_windows(const GenericGroup &grp, const ShardGeom &g) {
    return !grp.descs.empty() && g.nrel - (int64_t)grp.m_max + 1 < g.je;
}

// truncated tail windows of the m <= 128 patterns (only the shard owning the end of the text has any): they ride as
// extra workgroups of the first launch of the call that can take them, else get their own small launch at its end
struct ShortTails {
    ApmTailArgs args;
    int n = 0;
    bool pending = false;
    template <typename Args> void ride_with(Args &a) { // a: the arguments of a launch with tail workgroups
        if (!pending) return;
        a.n_tail = n;
        a.tail = args;
        pending = false;
    }
};

// generic-kernel launch over a pattern group; mode 0 full windows, 1 tails only, 2 everything
static int launch_generic_group(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, const GenericGroup &grp, const ApmPatDesc *d_descs, int mode) {
    if (grp.descs.empty() || g.je <= g.jb) return APM_OK;
    int64_t span = g.je - g.jb;
    if (mode == 1) span = std::min<int64_t>(span, grp.m_max); // at most m-1 tail windows per pattern
    const size_t col = (size_t)grp.m_max + 1;
    const size_t budget = (size_t)1 << 30;
    const size_t per_launch = std::min<size_t>(grp.descs.size(), 65535); // grid.y limit: more patterns = more launches
    int64_t nbx = (span + APM_BLOCK - 1) / APM_BLOCK;
    const int64_t cap = std::max<int64_t>(1, (int64_t)(budget / (col * 2 * APM_BLOCK * per_launch)));
    nbx = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(nbx, cap), 4096));
    const size_t need = col * 2 * APM_BLOCK * (size_t)nbx * per_launch;
    const int rc = grow_device_buffer(ctx, ds, (void **)&ds.d_scratch, &ds.scratch_bytes, need, 1);
    if (rc) return rc;
    ApmGenericArgs a{};
    set_common(a, ctx, g, g.je);
    a.avail = g.avail;
    a.bytes = ds.d_allpat;
    a.mode = mode;
    a.col_stride = (int)col;
    a.scratch = ds.d_scratch;
    for (size_t first = 0; first < grp.descs.size(); first += per_launch) { // (same scratch: launches of one stream run in order)
        a.pats = d_descs + first;
        APM_LAUNCH(ctx, ds, "generic", APM_PICK(g, apm_launch_generic)(a, (int)nbx, (int)std::min(per_launch, grp.descs.size() - first), ds.stream));
    }
    return APM_OK;
}

// ---- step 1: the sieve pipeline ----
struct SieveRange {               // the text the sieve looks at, and what its passes hand to the verify launches
    int64_t p_lo, p_hi;           // scanned relative positions [p_lo, p_hi), p_lo a multiple of 16
    int64_t n_mask_blocks = 0;    // 4 KiB blocks with a row of hit masks
    // of the sieve pass in hand:
    const uint32_t *blist_ctr = nullptr; // its block-list counter (NULL: no list kept)
    int clist_regions = 0;        // regions of its candidate list (0: no list kept)
    uint32_t clist_region_cap = 0;
    int clist_pools = 0;          // pools it moved the regions into (0: none, the verify launch reads the regions)
    uint32_t clist_pool_cap = 0;
    const uint32_t *cpool_cnt = nullptr; // the set of pool counters it counted in
    int64_t nchunks() const { return (p_hi - p_lo + 1023) / 1024; }
};
constexpr int kClistPerBlock = 32;
constexpr int kClistMaxRegions = 4096;

// what the sieve kernels read in every form of the pipeline; bitmap: the set's, or a verify launch's own
static ApmSieve2Args sieve_args(const SievePlan &S, const ShardGeom &g, const SieveRange &r, const uint32_t *d_bitmap) {
    ApmSieve2Args sv{};
    sv.text = g.text;
    sv.avail_pad = g.avail_pad;
    sv.tile0 = r.p_lo;
    sv.nchunks = r.nchunks();
    sv.bitmap = reinterpret_cast<const uint4 *>(d_bitmap);
    sv.code_shift = S.code_shift;
    sv.stride = S.stride;
    return sv;
}

// what a verify group's kernel reads in either form of the pipeline, for the window starts [g.jb, je_v); the fused form
// and the verify launch add their own hand-over fields
static ApmVerifyArgs verify_args(const apm_ctx *ctx, const VerifyLaunch &V, const DevVerify &D, const ShardGeom &g, int64_t je_v) {
    const SievePlan &S = ctx->plan.sieve;
    ApmVerifyArgs va{};
    set_common(va, ctx, g, je_v);
    va.avail = g.avail;
    va.avail_pad = g.avail_pad;
    va.image = reinterpret_cast<const uint4 *>(D.d_image);
    va.image_len = (int)V.image.size();
    va.o_prefix = V.o_prefix;
    va.o_r2s = V.o_r2s;
    va.o_slots = V.o_slots;
    va.o_kext = V.o_kext;
    va.o_pat = V.o_pat;
    va.o_masks = V.o_masks;
    va.o_kinfo = V.o_kinfo;
    va.o_pinfo = V.o_pinfo;
    va.o_rc = V.o_rc;
    va.kinfo = D.d_kinfo;
    va.pinfo = reinterpret_cast<const uint2 *>(D.d_pinfo);
    va.kpart = D.d_kpart;
    va.pats = D.d_descs;
    va.n_pats = (int)V.descs.size();
    va.nk = (int)V.kinfo.size();
    va.band = g.band;
    va.code_shift = S.code_shift;
    va.stride = S.stride;
    return va;
}

// FUSED form: one launch per verify group.  *ran stays false, and nothing was launched, when a group does not fit a CU
// in this form or the switch says no.
static int run_fused(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, const SieveRange &r, ShortTails &tails, bool *ran) {
    const SievePlan &S = ctx->plan.sieve;
    bool fused_ok = scan_env().fused < 0 ? S.stride == 8 : scan_env().fused != 0;
    std::vector<ApmFusedArgs> fargs;
    std::vector<size_t> fa_index; // fargs[i] belongs to launches[fa_index[i]]
    for (size_t v = 0; fused_ok && v < S.launches.size(); ++v) {
        const VerifyLaunch &V = S.launches[v];
        DevVerify &D = ds.verify[v];
        ApmFusedArgs fa{};
        fa.s = sieve_args(S, g, r, ds.d_sieve_bmp);
        fa.v = verify_args(ctx, V, D, g, std::min<int64_t>(g.je, g.nrel - V.m_min + 1));
#ifdef APM_MEASURE
        if (!ds.d_stats) HIP_TRY(ctx, hipMalloc((void **)&ds.d_stats, APM_STATS_BYTES));
        fa.v.stats = ds.d_stats;
#endif
        if (!D.fused_threads) {
            D.fused_blocks_per_cu = apm_fused_geometry(fa, &D.fused_threads);
            if (D.fused_blocks_per_cu < 1) D.fused_threads = -1; // does not fit a CU
        }
        if (D.fused_threads < 64) fused_ok = false;
        if (fa.v.je > g.jb) { fargs.push_back(fa); fa_index.push_back(v); }
    }
    if (!fused_ok) return APM_OK;
    for (ApmFusedArgs &fa : fargs) {
        tails.ride_with(fa.s); // the truncated tail windows ride as extra workgroups beside the scan
        const DevVerify &D = ds.verify[fa_index[&fa - fargs.data()]];
#ifdef APM_MEASURE
        HIP_TRY(ctx, hipMemsetAsync(ds.d_stats, 0, APM_STATS_BYTES, ds.stream));
#endif
        fa.v.work = ds.d_work;
        APM_LAUNCH(ctx, ds, "fused", APM_PICK(g, apm_launch_fused)(fa, D.fused_threads, ds.n_cu * D.fused_blocks_per_cu, &ds.work_epoch, ds.stream));
    }
    *ran = true;
    return APM_OK;
}

// one sieve pass: the set's shared bitmap (v < 0), or launch v's own bitmap with its code filter
static int sieve_pass(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, SieveRange &r, ShortTails &tails, int v) {
    const SievePlan &S = ctx->plan.sieve;
    ApmSieve2PoolArgs sv{};
    static_cast<ApmSieve2Args &>(sv) = sieve_args(S, g, r, v < 0 ? ds.d_sieve_bmp : ds.verify[(size_t)v].d_bmp18);
    sv.masks = ds.d_masks;
    if (v >= 0) { // second stage of the sieve: the code filter
        const VerifyLaunch &V = S.launches[(size_t)v];
        const DevVerify &D = ds.verify[(size_t)v];
        sv.cf_image = reinterpret_cast<const uint4 *>(D.d_cf);
        sv.cf_len = (int)V.cf_image.size();
        sv.cf_o_rrec = V.cf_o_rrec;
        sv.cf_o_lrec = V.cf_o_lrec;
        sv.cf_threads = D.cf_threads;
        sv.cf_blocks_per_cu = D.cf_blocks_per_cu;
        sv.cf_o_dp = V.cf_o_dp;
        sv.cf_dp_k = ctx->k;
        sv.cf_dp_cols = V.cf_dp_cols;
    }
    // the truncated tail windows ride as extra workgroups beside the scan -- in the code-filter form only a few of
    // them: its workgroups are big (1024 threads, most of a CU's LDS) and 2000 of them, one per pattern, made the
    // pass three times as long (256 cost nothing measurable); beyond 512 they get the small launch of their own at the end of the call
    if (v < 0 || tails.n <= 512) tails.ride_with(sv);
    const bool use_blist = scan_env().blist && sv.cf_image != nullptr; // (the list is kept by the code-filter form of the sieve only)
    r.blist_ctr = nullptr;
    if (use_blist) {
        sv.blist = ds.d_blist;
        sv.blist_ctr = APM_BLIST_CTR(ds.d_work, ds.sieve_epoch & 1);
        sv.blist_ctr_next = APM_BLIST_CTR(ds.d_work, (ds.sieve_epoch + 1) & 1);
        r.blist_ctr = sv.blist_ctr;
    }
    r.clist_regions = 0;
    if (use_blist && scan_env().clist) {
        // (allocated by the first pass that keeps a list: sets without the code filter never do)
        const size_t want = (size_t)r.n_mask_blocks * (size_t)kClistPerBlock + (size_t)kClistMaxRegions * 64;
        const int grc = grow_device_buffer(ctx, ds, (void **)&ds.d_clist, &ds.clist_cap, want, 4);
        if (grc) return grc;
        if (!ds.d_clist_cnt) HIP_TRY(ctx, hipMalloc((void **)&ds.d_clist_cnt, (size_t)kClistMaxRegions * 4));
        const int regions = apm_sieve2cf_blocks(sv, ds.n_cu);
        if (regions >= 1 && regions <= kClistMaxRegions) {
            r.clist_regions = regions;
            r.clist_region_cap = scan_env().clist_region_cap ? (uint32_t)scan_env().clist_region_cap
                                                             : (uint32_t)std::max<int64_t>(64, r.n_mask_blocks * kClistPerBlock / regions);
            sv.clist = ds.d_clist;
            sv.clist_cnt = ds.d_clist_cnt;
            sv.clist_cap = r.clist_region_cap;
        }
    }
    // the pools, when the pass will run the diagonal kernel (the launcher decides by the same rule and reports what it did)
    r.clist_pools = 0;
    if (r.clist_regions && scan_env().clist_pools > 0 && apm_cf_dp_form(sv.cf_o_dp > 0, sv.cf_dp_k, scan_env().cf_dp_diag != 0) == 2) {
        const int pools = std::min(scan_env().clist_pools, r.clist_regions);
        r.clist_pool_cap = (uint32_t)((r.clist_regions + pools - 1) / pools) * r.clist_region_cap; // (all of a pool's regions, full)
        const int grc = grow_device_buffer(ctx, ds, (void **)&ds.d_cpool, &ds.cpool_cap, (size_t)pools * r.clist_pool_cap, 4);
        if (grc) return grc;
        if (!ds.d_cpool_cnt) { // two sets: launch i counts in set i & 1 and zeroes the other (as the block list's counters)
            HIP_TRY(ctx, hipMalloc((void **)&ds.d_cpool_cnt, (size_t)2 * kClistMaxRegions * 4));
            HIP_TRY(ctx, hipMemsetAsync(ds.d_cpool_cnt, 0, (size_t)2 * kClistMaxRegions * 4, ds.stream));
        }
        sv.cpool = ds.d_cpool;
        sv.cpool_cnt = ds.d_cpool_cnt + (size_t)(ds.pool_epoch & 1) * kClistMaxRegions;
        sv.cpool_cnt_next = ds.d_cpool_cnt + (size_t)((ds.pool_epoch + 1) & 1) * kClistMaxRegions;
        sv.cpool_cap = r.clist_pool_cap;
        sv.cpool_n = pools;
        sv.cpool_next_n = ds.pool_dirty[(ds.pool_epoch + 1) & 1]; // (what the last launch in that set left: it may have had more pools than this one)
        r.cpool_cnt = sv.cpool_cnt;
    }
    ds.last_clist_regions = r.clist_regions;
    ds.last_blist_ctr = r.blist_ctr;
    ds.last_clist_pools = 0;
    HIP_TRY(ctx, APM_PICK(g, apm_launch_sieve2)(sv, ds.n_cu, ds.stream, scan_env().cf_dp_diag != 0, &ds.last_sieve_waves, &ds.last_cf_dp_form, &r.clist_pools));
    ds.last_clist_pools = r.clist_pools;
    if (use_blist) ++ds.sieve_epoch; // (a launch that did not run leaves its counter set as it was: still zero)
    if (r.clist_pools) { // (likewise)
        ds.pool_dirty[ds.pool_epoch & 1] = r.clist_pools;
        ds.pool_dirty[(ds.pool_epoch + 1) & 1] = 0;
        ++ds.pool_epoch;
    }
    return note_launch(ctx, ds, "sieve");
}

// the verify launch of group v over what the sieve pass in hand left for it
static int verify_pass(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, const SieveRange &r, size_t v, int64_t je_v) {
    DevVerify &D = ds.verify[v];
    ApmVerifyArgs va = verify_args(ctx, ctx->plan.sieve.launches[v], D, g, je_v);
    va.masks = ds.d_masks;
    if (r.blist_ctr) {
        va.blist = ds.d_blist;
        va.blist_ctr = r.blist_ctr;
    }
    if (r.clist_pools) { // the sieve pass moved its regions into pools: they are the launch's regions, few and large
        va.clist = ds.d_cpool;
        va.clist_cnt = r.cpool_cnt;
        va.clist_cap = r.clist_pool_cap;
        va.clist_regions = r.clist_pools;
        va.clist_min_batch = scan_env().clist_min_batch;
    } else if (r.clist_regions) {
        va.clist = ds.d_clist;
        va.clist_cnt = ds.d_clist_cnt;
        va.clist_cap = r.clist_region_cap;
        va.clist_regions = r.clist_regions;
        va.clist_min_batch = scan_env().clist_min_batch;
    }
    va.tile0 = r.p_lo;
    va.n_mask_blocks = r.n_mask_blocks;
#ifdef APM_MEASURE
    if (!ds.d_stats) HIP_TRY(ctx, hipMalloc((void **)&ds.d_stats, APM_STATS_BYTES));
    HIP_TRY(ctx, hipMemsetAsync(ds.d_stats, 0, APM_STATS_BYTES, ds.stream));
    va.stats = ds.d_stats;
#endif
    va.work = ds.d_work;
    if (!D.blocks_per_cu) D.blocks_per_cu = apm_verify_geometry(va, &D.threads);
    APM_LAUNCH(ctx, ds, "verify", APM_PICK(g, apm_launch_verify)(va, D.threads, ds.n_cu * D.blocks_per_cu, &ds.work_epoch, ds.stream));
    return APM_OK;
}

// TWO-LAUNCH form: sieve pass(es) into the hit masks and lists, a verify launch per group
static int run_sieve_verify(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, SieveRange &r, ShortTails &tails) {
    const SievePlan &S = ctx->plan.sieve;
    // hit masks: one dword per lane and 4 KiB block; every one is written by the sieve, nothing to clear
    r.n_mask_blocks = (r.nchunks() + 3) / 4;
    int rc = grow_device_buffer(ctx, ds, (void **)&ds.d_masks, &ds.masks_cap, (size_t)r.n_mask_blocks * 64 + 64, 4);
    if (rc) return rc;
    rc = grow_device_buffer(ctx, ds, (void **)&ds.d_blist, &ds.blist_cap, (size_t)r.n_mask_blocks + 64, 4);
    if (rc) return rc;
    ds.last_mask_blocks = r.n_mask_blocks;
    // every launch group with a sieve pass of its own (code filter), when all of them fit a CU in that form ...
    bool per_launch = S.per_launch_sieve;
    for (size_t v = 0; per_launch && v < S.launches.size(); ++v) {
        const VerifyLaunch &V = S.launches[v];
        DevVerify &D = ds.verify[v];
        if (!D.cf_threads) {
            D.cf_blocks_per_cu = apm_sieve2cf_geometry((int)V.cf_image.size(), apm_cf_dp_form(V.cf_o_dp > 0, ctx->k, scan_env().cf_dp_diag != 0), &D.cf_threads);
            if (D.cf_blocks_per_cu < 1) D.cf_threads = -1; // does not fit a CU
        }
        if (D.cf_threads < 64) per_launch = false;
    }
    bool any_pass = false;
    for (size_t v = 0; v < S.launches.size(); ++v) {
        const int64_t je_v = std::min<int64_t>(g.je, g.nrel - S.launches[v].m_min + 1);
        if (je_v <= g.jb) continue;
        if (per_launch || !any_pass) { // ... else ONE pass over the set's shared bitmap, in front of the first verify launch
            rc = sieve_pass(ctx, ds, g, r, tails, per_launch ? (int)v : -1);
            if (rc) return rc;
            any_pass = true;
        }
        rc = verify_pass(ctx, ds, g, r, v, je_v);
        if (rc) return rc;
    }
    // (no launch had windows to decide: the tails get their own launch at the end of the call)
    return APM_OK;
}

// sieve + verify pipeline of the per-position classes (needs 16-byte aligned text and < 4 GiB of it: 32-bit
// buffer offsets, 32-bit list entries); otherwise the LDS-tile / stream launches of step 2 do the whole job
static int run_sieve_pipeline(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, ShortTails &tails, bool *fused_run, bool *sieve_run) {
    const SievePlan &S = ctx->plan.sieve;
    if (!S.on || !g.aligned()) return APM_OK;
    SieveRange r;
    r.p_lo = std::max<int64_t>(0, g.jb - g.band) & ~(int64_t)15;
    r.p_hi = std::min<int64_t>(g.avail, g.je + S.m_max + g.band);
    if (!(r.p_hi > r.p_lo && g.avail_pad >= 16 && g.avail_pad <= APM_SIEVE_MAX_BYTES)) return APM_OK;
    if (!ds.d_work) {
        HIP_TRY(ctx, hipMalloc((void **)&ds.d_work, APM_WORK_BYTES));
        HIP_TRY(ctx, hipMemsetAsync(ds.d_work, 0, APM_WORK_BYTES, ds.stream));
        ds.work_epoch = 0;
        ds.sieve_epoch = 0;
    }
    int rc = run_fused(ctx, ds, g, r, tails, fused_run);
    if (rc || *fused_run) return rc;
    rc = run_sieve_verify(ctx, ds, g, r, tails);
    if (rc) return rc;
    *sieve_run = true;
    return APM_OK;
}

// ---- step 2: the tiled launches ----
// BANDED launch over the window starts [g.jb, je_l): the stream kernel where it applies, else the LDS-tile kernel
static int launch_banded(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, const TiledLaunch &L, DevTiled &D, int64_t je_l, ShortTails &tails) {
    const ScanEnv &env = scan_env();
    ApmFilterArgs f{};
    set_common(f, ctx, g, je_l);
    f.avail = g.avail;
    f.avail_pad = g.avail_pad;
    f.band = g.band;
    f.front = f.band > 0 ? 16 : 0;
    f.tile0 = aligned_tile0(g, f.front);
    f.pats = D.d_descs;
    f.image = reinterpret_cast<const uint4 *>(D.d_image);
    f.image_len = (int)L.image.size();
    f.o_tab = L.o_tab;
    f.o_kid = L.o_kid;
    f.o_ovf = L.o_ovf;
    f.o_kinfo = L.o_kinfo;
    f.o_pinfo = L.o_pinfo;
    f.o_next = L.o_next;
    f.o_poff = L.o_poff;
    f.o_bmp = L.o_bmp;
    f.o_pat = L.o_pat;
    f.o_kext = L.o_kext;
    f.code_shift = L.code_shift;
    f.nk = (int)L.keys.size();
    f.nb = L.nb;
    f.lg_nb = L.lg_nb;
    f.n_ovf = (int)(L.ovf.size() / 2);
    f.qcap = L.qcap;
#ifdef APM_MEASURE
    if (L.stride == 1 && env.qcap_s1 >= 64 && env.qcap_s1 <= 8192) f.qcap = env.qcap_s1;
#endif
    f.key_len = L.key_len;
    f.stride = L.stride;
    f.n_cu = ds.n_cu;
    f.n_pats = (int)L.descs.size();
    f.tile_w = L.tile;
    f.tile_len = APM_FILTER_POS;
    f.ntiles = (je_l - f.tile0 + L.tile - 1) / L.tile;
    const bool can_load16 = g.aligned() && f.avail_pad >= 16;
    f.use_dma = (env.filter_dma && can_load16) ? 1 : 0;
    const double hit_rate = (double)L.keys.size() / (double)(1ull << (2 * std::min(L.key_len, 8)));
    const bool stream_ok = L.stride > 1 || (f.band <= 1 && (env.filter_stream == 2 || (env.filter_stream != 3 && hit_rate < 1.0 / 200.0)));
    if (env.filter_stream && stream_ok && can_load16) {
        // wave-autonomous streaming kernel over 1 KiB chunks
        const int64_t p_lo = std::max<int64_t>(0, g.jb - f.band) & ~(int64_t)15;
        const int64_t p_hi = std::min<int64_t>(g.avail, je_l + L.m_max + f.band);
        f.tile0 = p_lo;
        f.ntiles = p_hi > p_lo ? (p_hi - p_lo + 1023) / 1024 : 0;
        if (!D.blocks_per_cu[2]) D.blocks_per_cu[2] = apm_stream_blocks_per_cu(f);
        tails.ride_with(f);
        APM_LAUNCH(ctx, ds, "stream", APM_PICK(g, apm_launch_stream)(f, ds.n_cu * D.blocks_per_cu[2], ds.stream));
        return APM_OK;
    }
    if (!D.blocks_per_cu[f.use_dma])
        D.blocks_per_cu[f.use_dma] = apm_filter_blocks_per_cu(f.band, f.key_len, f.stride, f.use_dma, apm_filter_lds_bytes(f));
    tails.ride_with(f);
    int bpc = D.blocks_per_cu[f.use_dma];
#ifdef APM_MEASURE
    if (env.bpc_cap > 0) bpc = std::min(env.bpc_cap, bpc);
#endif
    APM_LAUNCH(ctx, ds, "tile", APM_PICK(g, apm_launch_filter)(f, ds.n_cu * bpc, ds.stream));
    return APM_OK;
}

static int launch_nfa(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, const TiledLaunch &L, const DevTiled &D, int64_t je_l) {
    ApmNfaArgs na{};
    set_common(na, ctx, g, je_l);
    na.avail = g.avail;
    na.tile0 = aligned_tile0(g);
    na.pats = D.d_descs;
    na.classes = D.d_bytes;
    na.cls_len = (int)L.bytes.size();
    memcpy(na.class_bytes, L.lut, 16);
    na.n_classes = L.nb;
    na.n_pats = (int)L.descs.size();
    APM_LAUNCH(ctx, ds, "nfa", APM_PICK(g, apm_launch_nfa)(na, ds.stream));
    return APM_OK;
}

// full-DP launches: BITPAR (one window per lane; beyond 1024 bytes one window per wave, one pattern per launch, full and
// truncated windows alike) and WAVEFRONT
static int launch_full_dp(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, const TiledLaunch &L, const DevTiled &D, int64_t je_l) {
    const bool per_wave = L.kind == APM_KERNEL_BITPAR && L.m_max > 1024;
    ApmScanArgs a{};
    set_common(a, ctx, g, per_wave ? g.je : je_l);
    a.avail = g.avail;
    a.tile0 = aligned_tile0(g);
    a.pats = D.d_descs;
    a.tables = D.d_tables;
    a.lut = D.d_lut;
    a.n_pats = per_wave ? 1 : (int)L.descs.size();
    a.table_words = (int)L.tables.size();
    if (per_wave) {
        APM_LAUNCH(ctx, ds, "bitpar", APM_PICK(g, apm_launch_bitlong)(a, L.m_max, ds.stream));
        return APM_OK;
    }
    a.bytes = D.d_bytes;
    a.tile = L.tile;
    a.halo = L.m_max - 1;
    a.bytes_len = (int)L.bytes.size();
    if (L.kind == APM_KERNEL_BITPAR) APM_LAUNCH(ctx, ds, "bitpar", APM_PICK(g, apm_launch_bitpar)(a, ds.stream));
    else APM_LAUNCH(ctx, ds, "wavefront", APM_PICK(g, apm_launch_wavefront)(a, ds.stream));
    return APM_OK;
}

// every tiled launch of the plan; sieved: the sieve pipeline ran, and has decided the BANDED launches it feeds (it
// cannot overflow: no fallback)
static int run_tiled_launches(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, ShortTails &tails, bool sieved) {
    for (size_t t = 0; t < ctx->plan.tiled.size(); ++t) {
        const TiledLaunch &L = ctx->plan.tiled[t];
        const bool per_wave = L.kind == APM_KERNEL_BITPAR && L.m_max > 1024;
        const int64_t je_l = std::min<int64_t>(g.je, g.nrel - L.m_min + 1); // full windows only (the per-wave kernel takes all)
        if (!per_wave && je_l <= g.jb) continue;
        int rc;
        if (L.kind == APM_KERNEL_BANDED) {
            if (sieved && L.sieved) continue;
            rc = launch_banded(ctx, ds, g, L, ds.tiled[t], je_l, tails);
        } else if (L.kind == APM_KERNEL_NFA) {
            rc = launch_nfa(ctx, ds, g, L, ds.tiled[t], je_l);
        } else {
            rc = launch_full_dp(ctx, ds, g, L, ds.tiled[t], je_l);
        }
        if (rc) return rc;
    }
    return APM_OK;
}

// ---- step 4: tails and trivial patterns ----
static int run_tails_and_trivial(apm_ctx *ctx, DeviceState &ds, const ShardGeom &g, ShortTails &tails, uint64_t ob, uint64_t oe) {
    const ApmPlan &plan = ctx->plan;
    // truncated windows of the tiled-kernel patterns by length class: the short ones unless a launch above took them
    // along, then those of the 128 < m <= 512 and of the 512 < m <= 1024 patterns
    typedef hipError_t (*TailLauncher)(const ApmTailArgs &, int, hipStream_t);
    const struct { bool due; const GenericGroup &grp; const ApmPatDesc *d_descs; TailLauncher count, rec; } classes[3] = {
        {tails.pending, plan.stails, ds.d_stail_descs, apm_launch_tail, apm_launch_tail_rec},
        {has_tail_windows(plan.wtails, g), plan.wtails, ds.d_wtail_descs, apm_launch_tail_wide, apm_launch_tail_wide_rec},
        {has_tail_windows(plan.xtails, g), plan.xtails, ds.d_xtail_descs, apm_launch_tail_xwide, apm_launch_tail_xwide_rec},
    };
    for (const auto &c : classes) {
        if (!c.due) continue;
        ApmTailArgs ta = tails.args;
        ta.pats = c.d_descs;
        APM_LAUNCH(ctx, ds, "tail", (g.rec_on ? c.rec : c.count)(ta, (int)c.grp.descs.size(), ds.stream));
    }
    if (!plan.trivial.empty()) {
        const int nt = (int)plan.trivial.size();
        hipLaunchKernelGGL(apm_add_const_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, ds.stream, g.counts,
                           ds.d_trivial, nt, (unsigned long long)(oe - ob));
        if (g.rec_on) {
            const unsigned long long total = (unsigned long long)(oe - ob) * (unsigned long long)nt;
            const unsigned nb = (unsigned)std::min<unsigned long long>((total + 255) / 256, 4096);
            hipLaunchKernelGGL(apm_rec_const_kernel, dim3(nb), dim3(256), 0, ds.stream, reinterpret_cast<uint4 *>(g.sink.out), g.sink.count,
                               g.sink.cap, ds.d_trivial, nt, (unsigned long long)ob, (unsigned long long)oe);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    return APM_OK;
}

// ---- the shard scan proper, all on ds.stream, no host sync ----
static int scan_shard_one(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end,
                          unsigned long long *d_counts, const ApmPosSink *rec) {
    const uint8_t *d_text = sh.text;
    const uint64_t text_off = sh.text_off, text_len = sh.text_len, n_total = sh.n_total;
    const ApmPlan &plan = ctx->plan;
    const uint64_t k = (uint64_t)ctx->k;
    const uint64_t limit = n_total > k ? n_total - k : 0;
    const uint64_t ob = own_begin, oe = std::min(own_end, limit);
    if (oe <= ob) return APM_OK;
    if (text_off > ob) return fail(ctx, APM_ERR_INVALID, "shard text starts after own_begin");
    const uint64_t m_max = (uint64_t)std::max(plan.m_max, 1);
    const uint64_t need_end = std::min<uint64_t>(n_total, oe + m_max - 1);
    if (text_off + text_len < need_end)
        return fail(ctx, APM_ERR_INVALID, "shard text too short: halo of m_max-1 = %llu bytes required",
                    (unsigned long long)(m_max - 1));
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    ds.text_bytes += need_end - ob;

    ShardGeom g{};
    g.text = d_text;
    g.jb = (int64_t)(ob - text_off);
    g.je = (int64_t)(oe - text_off);
    g.nrel = (int64_t)(n_total - text_off);
    g.avail = (int64_t)text_len;
    g.avail_pad = g.avail + (int64_t)((16u - ((reinterpret_cast<uintptr_t>(d_text) + (uintptr_t)g.avail) & 15u)) & 15u);
    g.band = ctx->k / 2;
    g.counts = d_counts;
    g.rec_on = rec != nullptr;
    if (rec) {
        g.sink = *rec;
        g.sink.text_off = text_off;
    } else if (ctx->find_active) {
        g.sink.out = ds.d_pos_out;
        g.sink.count = ds.d_pos_count;
        g.sink.cap = ds.pos_cap;
        g.sink.text_off = text_off;
    }
    ShortTails tails;
    set_common(tails.args, ctx, g, g.je);
    tails.args.pats = ds.d_stail_descs;
    tails.args.bytes = ds.d_allpat;
    tails.n = (int)plan.stails.descs.size();
    tails.pending = has_tail_windows(plan.stails, g);

    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
    // 1. the sieve pipeline (fused, or sieve + verify) when it applies
    bool fused_run = false, sieve_run = false;
    int rc = run_sieve_pipeline(ctx, ds, g, tails, &fused_run, &sieve_run);
    if (rc) return rc;
    // 2. the tiled launches it did not cover
    rc = run_tiled_launches(ctx, ds, g, tails, fused_run || sieve_run);
    if (rc) return rc;
    ds.last_fused = fused_run;
    if (!sieve_run) { ds.last_mask_blocks = 0; ds.last_clist_regions = 0; ds.last_clist_pools = 0; ds.last_sieve_waves = 0; ds.last_cf_dp_form = 0; }
    // 3. the generic groups: full scans, then the truncated windows of tiled-kernel patterns beyond the tail kernels' reach
    rc = launch_generic_group(ctx, ds, g, plan.longs, ds.d_long_descs, 2);
    if (rc) return rc;
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
    if (has_tail_windows(plan.tails, g)) {
        rc = launch_generic_group(ctx, ds, g, plan.tails, ds.d_tail_descs, 1);
        if (rc) return rc;
    }
    // 4. tails and trivial patterns
    return run_tails_and_trivial(ctx, ds, g, tails, ob, oe);
}

// The sieve pipeline addresses its shard with 32 bits.  A bigger shard (a 288 GB device holds a lot of text) is scanned
// in pieces of 3 GiB of window starts, each with its own text window [piece begin rounded down so that the pointer
// keeps its 16-byte alignment, piece end + m_max + 31) -- the same cut a caller sharding the text would make (every
// window lies in exactly one piece; what a piece reads in front of its first window start never decides a match).
int scan_shard(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, unsigned long long *d_counts,
               const ApmPosSink *rec) {
    const uint8_t *d_text = sh.text;
    uint64_t text_off = sh.text_off, text_len = sh.text_len;
    const uint64_t n_total = sh.n_total;
    const bool sieve_on = ctx->plan.sieve.on;
    const uint64_t lim32 = (uint64_t)APM_SIEVE_MAX_BYTES - 4096;
    // an unaligned text pointer into a bigger buffer: start the shard's text at the 16-byte boundary in front of it (those
    // bytes are readable -- apm.h -- and lie in front of every window start of the shard, where nothing decides a match)
    const uint64_t mis = (uint64_t)(reinterpret_cast<uintptr_t>(d_text) & 15u);
    if (sieve_on && mis != 0 && text_off >= mis && text_len > 0) {
        d_text -= mis;
        text_off -= mis;
        text_len += mis;
    }
    if (!sieve_on || text_len < lim32 || (reinterpret_cast<uintptr_t>(d_text) & 15u) != 0 || own_begin < text_off)
        return scan_shard_one(ctx, ds, ShardText{d_text, text_off, text_len, n_total}, own_begin, own_end, d_counts, rec);
    const uint64_t k = (uint64_t)ctx->k;
    const uint64_t oe = std::min(own_end, n_total > k ? n_total - k : 0);
    const uint64_t m_max = (uint64_t)std::max(ctx->plan.m_max, 1), step = (uint64_t)3 << 30;
    for (uint64_t b = own_begin; b < oe;) {
        const uint64_t e = std::min(oe, b + step);
        const uint64_t sb = text_off + ((b - text_off) & ~(uint64_t)15);
        const uint64_t se = std::min(text_off + text_len, e + m_max + 31);
        const int rc = scan_shard_one(ctx, ds, ShardText{d_text + (sb - text_off), sb, se - sb, n_total}, b, e, d_counts, rec);
        if (rc) return rc;
        b = e;
    }
    return APM_OK;
}

// hits of the last call's sieve: popcount over its masks (synchronises with the stream)
int sieve_candidates(apm_ctx *ctx, DeviceState &ds, double *value) {
    *value = 0;
    if (!ds.d_masks || ds.last_mask_blocks <= 0) return APM_OK;
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    if (!ds.d_stats) HIP_TRY(ctx, hipMalloc((void **)&ds.d_stats, APM_STATS_BYTES));
    unsigned long long *d_sum = ds.d_stats + 7;
    HIP_TRY(ctx, hipMemsetAsync(d_sum, 0, 8, ds.stream));
    if (ds.last_clist_regions)
        hipLaunchKernelGGL(apm_popcount_listed_kernel, dim3(1024), dim3(256), 0, ds.stream, ds.d_masks, ds.d_blist, ds.last_blist_ctr, ds.d_clist_cnt, ds.last_clist_regions, d_sum);
    else
        hipLaunchKernelGGL(apm_popcount_kernel, dim3(1024), dim3(256), 0, ds.stream, ds.d_masks, (unsigned long long)ds.last_mask_blocks * 64ull, d_sum);
    unsigned long long h = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&h, d_sum, 8, hipMemcpyDeviceToHost, ds.stream));
    HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    *value = (double)h;
    return APM_OK;
}
