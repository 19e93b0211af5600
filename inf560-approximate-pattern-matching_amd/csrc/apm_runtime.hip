/*
 * apm_runtime.hip -- the context behind the C ABI in include/apm.h: its life cycle, the plan of its pattern set on every
 * device, the setters, the children of the pattern partition, and the device-level calls.  The host-level count calls
 * are in apm_ingest.hip, the host-level find calls in apm_find.hip, the record passes with their device-level calls in
 * apm_records.hip, timing and statistics in apm_stats.hip.
 *
 * Host-side replacement for the reference's dispatch layer around its GPU shim:
 *   MPI master/worker + shard bounds   /root/reference/src/database_over_ranks.c:141-195
 *   GPU shims                          /root/reference/src/*.cu (see include/apm.h)
 *
 * There is no CPU fallback in this file by design.
 */
#include "apm_runtime.h"
#include "apm_core.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

static thread_local std::string g_create_error;

int fail(apm_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    static std::mutex mu; // (the per-device staging threads of count_sharded may fail side by side)
    std::lock_guard<std::mutex> lock(mu);
    if (ctx) ctx->err = buf;
    else g_create_error = buf;
    return code;
}

int grow_device_buffer(apm_ctx *ctx, DeviceState &ds, void **ptr, size_t *cap, size_t want, size_t elem_bytes, int status, const char *noun_fmt, ...) {
    if (*cap >= want) return APM_OK;
    if (*ptr) {
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
        HIP_TRY(ctx, hipFree(*ptr));
    }
    *ptr = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc(ptr, want * elem_bytes);
    if (e != hipSuccess) {
        *ptr = nullptr;
        if (!noun_fmt) return fail(ctx, APM_ERR_HIP, "hipMalloc(ptr, want * elem_bytes) failed: %s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        (void)hipGetLastError();
        char noun[256];
        va_list ap;
        va_start(ap, noun_fmt);
        vsnprintf(noun, sizeof noun, noun_fmt, ap);
        va_end(ap);
        return fail(ctx, status, "cannot allocate %s", noun);
    }
    *cap = want;
    return APM_OK;
}

namespace {

void free_device_plan(DeviceState &ds) {
    hipSetDevice(ds.dev);
    auto drop = [](auto *&p) { if (p) hipFree(p); p = nullptr; };
    for (auto &t : ds.tiled) { drop(t.d_descs); drop(t.d_bytes); drop(t.d_tables); drop(t.d_lut); drop(t.d_image); }
    ds.tiled.clear();
    for (auto &v : ds.verify) { drop(v.d_bmp18); drop(v.d_cf); drop(v.d_descs); drop(v.d_image); drop(v.d_kinfo); drop(v.d_pinfo); drop(v.d_kpart); }
    ds.verify.clear();
    drop(ds.d_allpat);
    drop(ds.d_tail_descs);
    drop(ds.d_stail_descs);
    drop(ds.d_wtail_descs);
    drop(ds.d_xtail_descs);
    drop(ds.d_long_descs);
    drop(ds.d_trivial);
    drop(ds.d_counts);
    drop(ds.d_sieve_bmp);
    drop(ds.d_score_img); // (not part of the plan: the next scoring call builds it anew)
    drop(ds.d_score_tab);
    drop(ds.d_align_ws); // (the align pass's trace workspace goes where the score image goes)
    ds.align_rows = ds.last_align_rows = 0;
}

// a device's mirror of ctx->plan; what it held of an earlier plan is released first, behind the stream: a scan still in
// flight there may read those buffers, and nothing but an implicit synchronisation inside hipFree stood in its way
int upload_plan(apm_ctx *ctx, DeviceState &ds) {
    const ApmPlan &plan = ctx->plan;
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    free_device_plan(ds);
    int rc = APM_OK; // (of the first upload that failed; nothing is uploaded behind it)
    auto up = [&](auto **dptr, const auto &v) { if (!rc) rc = upload_vec(ctx, dptr, v); };
    up(&ds.d_allpat, plan.allpat);
    up(&ds.d_tail_descs, plan.tails.descs);
    up(&ds.d_stail_descs, plan.stails.descs);
    up(&ds.d_wtail_descs, plan.wtails.descs);
    up(&ds.d_xtail_descs, plan.xtails.descs);
    up(&ds.d_long_descs, plan.longs.descs);
    up(&ds.d_trivial, plan.trivial);
    if (rc) return rc;
    HIP_TRY(ctx, hipMalloc((void **)&ds.d_counts, std::max<size_t>(ctx->pats.size() * 8, 16)));
    if (plan.sieve.on) {
        up(&ds.d_sieve_bmp, plan.sieve.bitmap);
        ds.verify.resize(plan.sieve.launches.size());
        for (size_t v = 0; v < plan.sieve.launches.size(); ++v) {
            const VerifyLaunch &V = plan.sieve.launches[v];
            DevVerify &D = ds.verify[v];
            if (plan.sieve.per_launch_sieve) { up(&D.d_bmp18, V.bitmap18); up(&D.d_cf, V.cf_image); }
            up(&D.d_descs, V.descs); up(&D.d_image, V.image); up(&D.d_kinfo, V.kinfo); up(&D.d_pinfo, V.pinfo); up(&D.d_kpart, V.kpart);
        }
    }
    ds.tiled.resize(plan.tiled.size());
    for (size_t t = 0; t < plan.tiled.size(); ++t) {
        const TiledLaunch &L = plan.tiled[t];
        DevTiled &D = ds.tiled[t];
        up(&D.d_descs, L.descs); up(&D.d_bytes, L.bytes); up(&D.d_tables, L.tables);
        up(&D.d_lut, std::vector<uint8_t>(L.lut, L.lut + 256));
        up(&D.d_image, L.image);
    }
    return rc;
}

int init_device(apm_ctx *ctx, DeviceState &ds, int dev) {
    ds.dev = dev;
    HIP_TRY(ctx, hipSetDevice(dev));
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) ds.n_cu = ncu;
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ds.own_stream, hipStreamNonBlocking));
    ds.stream = ds.own_stream;
    HIP_TRY(ctx, hipEventCreate(&ds.ev_start));
    HIP_TRY(ctx, hipEventCreate(&ds.ev_kstart));
    HIP_TRY(ctx, hipEventCreate(&ds.ev_mstart));
    HIP_TRY(ctx, hipEventCreate(&ds.ev_mstop));
    HIP_TRY(ctx, hipEventCreate(&ds.ev_stop));
    return APM_OK;
}

} // namespace

// plan ctx->pats at ctx->k under ctx->kernel (apm_plan.cpp) and hand the plan to every device
int build_plan(apm_ctx *ctx) {
    std::string err;
    const int prc = apm_build_plan(ctx->pats, ctx->k, ctx->kernel, &ctx->plan, &err);
    if (prc) return fail(ctx, prc, "%s", err.c_str());
    for (auto &ds : ctx->devs) {
        const int rc = upload_plan(ctx, ds);
        if (rc) return rc;
    }
    return APM_OK;
}

static int create_common(apm_ctx **out, const std::vector<int> &devs, bool multi);

// (re)build the children of a pattern-sharded context from ctx->pats / ctx->k / ctx->kernel: contiguous slices of the
// pattern list, as even as they come (the replacement of /root/reference/src/patterns_over_ranks.c:160-182, where the
// master dealt patterns to the ranks by a cost model and every rank read the whole file)
static int build_children(apm_ctx *ctx) {
    const int G = (int)ctx->devs.size(), P = (int)ctx->pats.size();
    if (ctx->children.empty()) {
        ctx->children.assign((size_t)G, nullptr);
        for (int g = 0; g < G; ++g) {
            const int rc = create_common(&ctx->children[(size_t)g], std::vector<int>{ctx->devs[(size_t)g].dev}, false);
            if (rc) return fail(ctx, rc, "pattern-sharded context: device %d: %s", ctx->devs[(size_t)g].dev, g_create_error.c_str());
        }
    }
    ctx->pat_first.assign((size_t)G + 1, 0);
    for (int g = 0; g <= G; ++g) ctx->pat_first[(size_t)g] = (int)((long long)P * g / G);
    for (int g = 0; g < G; ++g) {
        apm_ctx *ch = ctx->children[(size_t)g];
        const int a = ctx->pat_first[(size_t)g], b = ctx->pat_first[(size_t)g + 1];
        ch->timing_on = ctx->timing_on;
        ch->patterns_set = false;
        if (b <= a) continue; // (fewer patterns than devices)
        std::vector<const char *> pp;
        std::vector<int> ll;
        for (int i = a; i < b; ++i) { pp.push_back(ctx->pats[(size_t)i].bytes.data()); ll.push_back(ctx->pats[(size_t)i].m); }
        ch->kernel = ctx->kernel;
        const int rc = apm_set_patterns(ch, b - a, pp.data(), ll.data(), ctx->k);
        if (rc) return fail(ctx, rc, "%s", ch->err.c_str());
        for (int i = a; i < b; ++i) ctx->pats[(size_t)i].kernel = ch->pats[(size_t)(i - a)].kernel;
    }
    return APM_OK;
}

// run fn(child, counts of its slice) on every child at once, one host thread per device
int for_children(apm_ctx *ctx, uint64_t *counts, const std::function<int(apm_ctx *, uint64_t *)> &fn) {
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!counts) return fail(ctx, APM_ERR_INVALID, "counts is NULL");
    const auto t0 = clk::now();
    const int G = (int)ctx->children.size();
    std::vector<int> rcs((size_t)G, APM_OK);
    auto work = [&](int g) {
        const int a = ctx->pat_first[(size_t)g], b = ctx->pat_first[(size_t)g + 1];
        if (b > a) rcs[(size_t)g] = fn(ctx->children[(size_t)g], counts + a);
    };
    std::vector<std::thread> th;
    for (int g = 1; g < G; ++g) th.emplace_back(work, g);
    work(0);
    for (auto &t : th) t.join();
    ctx->timing = apm_timing{};
    ctx->timing.n_devices = G;
    for (int g = 0; g < G; ++g) {
        if (rcs[(size_t)g]) return fail(ctx, rcs[(size_t)g], "%s", ctx->children[(size_t)g]->err.c_str());
        if (ctx->pat_first[(size_t)g + 1] <= ctx->pat_first[(size_t)g]) continue;
        const apm_timing &t = ctx->children[(size_t)g]->timing;
        ctx->timing.h2d_ms = std::max(ctx->timing.h2d_ms, t.h2d_ms);
        ctx->timing.kernel_ms = std::max(ctx->timing.kernel_ms, t.kernel_ms);
        ctx->timing.main_kernel_ms = std::max(ctx->timing.main_kernel_ms, t.main_kernel_ms);
        ctx->timing.text_bytes += t.text_bytes;
        ctx->timing.windows += t.windows;
        ctx->timing.cells_algorithmic += t.cells_algorithmic;
        ctx->timing.cells_evaluated += t.cells_evaluated;
        ctx->timing.n_launches += t.n_launches;
    }
    ctx->timing.total_ms = ms_since(t0);
    return APM_OK;
}

// the plan, or the children of a pattern-sharded context, anew from ctx->pats / k / kernel; patterns_set: it stands
static int rebuild(apm_ctx *ctx) {
    ctx->patterns_set = false;
    const int rc = pattern_sharded(ctx) ? build_children(ctx) : build_plan(ctx);
    ctx->patterns_set = rc == APM_OK;
    return rc;
}

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int apm_abi_version(void) { return APM_ABI_VERSION; }

int apm_device_count(void) {
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) {
        g_create_error = std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e);
        return APM_ERR_HIP;
    }
    return n;
}

const char *apm_last_error(const apm_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

static int create_common(apm_ctx **out, const std::vector<int> &devs, bool multi) {
    apm_ctx *ctx = new (std::nothrow) apm_ctx();
    if (!ctx) return fail(nullptr, APM_ERR_NOMEM, "out of memory");
    ctx->multi = multi;
    ctx->devs.resize(devs.size());
    for (size_t i = 0; i < devs.size(); ++i) {
        const int rc = init_device(ctx, ctx->devs[i], devs[i]);
        if (rc) {
            g_create_error = ctx->err;
            apm_destroy(ctx);
            return rc;
        }
    }
    *out = ctx;
    return APM_OK;
}

int apm_create(apm_ctx **ctx, int n_devices) {
    if (!ctx) return fail(nullptr, APM_ERR_INVALID, "ctx is NULL");
    *ctx = nullptr;
    const int have = apm_device_count();
    if (have < 0) return have;
    if (have == 0) return fail(nullptr, APM_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
    std::vector<int> devs;
    // APM_DEVICES=a,b,...: the device ids of the context, in shard order, instead of 0 .. n_devices-1.  An id may repeat
    // ("0,0"): several shards then share one GPU, each with its own stream, text buffer and count vector -- the rehearsal of
    // the multi-device path on a one-GPU box (tests); the partial counts are then summed on the host (RCCL wants one rank
    // per device).
    if (const char *e = getenv("APM_DEVICES")) {
        for (const char *p = e; *p;) {
            char *end = nullptr;
            const long id = strtol(p, &end, 10);
            if (end == p || id < 0 || id >= have) return fail(nullptr, APM_ERR_NO_DEVICE, "APM_DEVICES: bad device list <%s> (%d visible)", e, have);
            devs.push_back((int)id);
            p = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') return fail(nullptr, APM_ERR_NO_DEVICE, "APM_DEVICES: bad device list <%s>", e);
        }
        if (devs.empty() || (int)devs.size() > apm_ctx::N_STAGE / 2) return fail(nullptr, APM_ERR_NO_DEVICE, "APM_DEVICES: bad device list <%s>", e);
        if (n_devices > 0 && n_devices != (int)devs.size())
            return fail(nullptr, APM_ERR_NO_DEVICE, "%d devices requested, APM_DEVICES lists %d", n_devices, (int)devs.size());
        return create_common(ctx, devs, true);
    }
    if (n_devices <= 0) n_devices = have;
    if (n_devices > have) return fail(nullptr, APM_ERR_NO_DEVICE, "%d devices requested, %d visible", n_devices, have);
    if (n_devices > apm_ctx::N_STAGE / 2) return fail(nullptr, APM_ERR_NO_DEVICE, "at most %d devices per context", apm_ctx::N_STAGE / 2);
    for (int i = 0; i < n_devices; ++i) devs.push_back(i);
    return create_common(ctx, devs, true);
}

int apm_create_on_device(apm_ctx **ctx, int device_id) {
    if (!ctx) return fail(nullptr, APM_ERR_INVALID, "ctx is NULL");
    *ctx = nullptr;
    const int have = apm_device_count();
    if (have < 0) return have;
    if (have == 0) return fail(nullptr, APM_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
    if (device_id < 0 || device_id >= have)
        return fail(nullptr, APM_ERR_NO_DEVICE, "device %d out of range (%d visible)", device_id, have);
    return create_common(ctx, std::vector<int>{device_id}, false);
}

void apm_destroy(apm_ctx *ctx) {
    if (!ctx) return;
    for (apm_ctx *ch : ctx->children) apm_destroy(ch);
    ctx->children.clear();
    if (ctx->rccl.ready)
        for (void *c : ctx->rccl.comms) if (c) ctx->rccl.CommDestroy(c);
    for (auto &ds : ctx->devs) {
        if (ds.dev < 0) continue;
        hipSetDevice(ds.dev);
        if (ds.own_stream) hipStreamSynchronize(ds.own_stream);
        free_device_plan(ds);
        for (void *p : {(void *)ds.d_scratch, (void *)ds.d_text, (void *)ds.d_rec, (void *)ds.d_rec2, (void *)ds.d_rec_n, (void *)ds.d_ops, (void *)ds.d_masks, (void *)ds.d_stats,
                        (void *)ds.d_work, (void *)ds.d_blist, (void *)ds.d_clist, (void *)ds.d_clist_cnt, (void *)ds.d_cpool, (void *)ds.d_cpool_cnt, (void *)ds.d_raw, (void *)ds.d_tn_summary,
                        (void *)ds.d_tn_map, (void *)ds.d_tn_total, (void *)ds.d_sq_count, (void *)ds.d_sq_prefix, (void *)ds.d_sq_total,
                        (void *)ds.d_seq_table, (void *)ds.d_loc_buf, (void *)ds.d_nearest_keys, (void *)ds.d_seqnear_keys, (void *)ds.d_seqocc_seq})
            if (p) hipFree(p);
        for (hipEvent_t e : ds.ev_best) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ds.ev_stage) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ds.ev_launch) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ds.ev_tn) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ds.ev_sq) if (e) hipEventDestroy(e);
        for (hipEvent_t e : {ds.ev_start, ds.ev_kstart, ds.ev_mstart, ds.ev_mstop, ds.ev_stop}) if (e) hipEventDestroy(e);
        if (ds.own_stream) hipStreamDestroy(ds.own_stream);
    }
    for (int b = 0; b < apm_ctx::N_STAGE; ++b)
        if (ctx->stage[b]) hipHostFree(ctx->stage[b]);
    delete ctx;
}

int apm_set_stream(apm_ctx *ctx, void *hip_stream) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_set_stream needs a single-device context");
    ctx->devs[0].stream = hip_stream == APM_STREAM_OWN ? ctx->devs[0].own_stream : (hipStream_t)hip_stream;
    return APM_OK;
}

int apm_set_partition(apm_ctx *ctx, int partition) {
    if (!ctx) return APM_ERR_INVALID;
    if (partition != APM_PARTITION_TEXT && partition != APM_PARTITION_PATTERNS) return fail(ctx, APM_ERR_INVALID, "unknown partition %d", partition);
    if (partition == ctx->partition) return APM_OK;
    ctx->partition = partition;
    return ctx->pats.empty() ? (int)APM_OK : rebuild(ctx);
}

int apm_set_patterns(apm_ctx *ctx, int n_patterns, const char *const *pat, const int *len, int k) {
    if (!ctx) return APM_ERR_INVALID;
    if (n_patterns <= 0 || n_patterns > APM_MAX_PATTERNS || !pat || !len)
        return fail(ctx, APM_ERR_INVALID, "need 1..%d patterns", APM_MAX_PATTERNS);
    if (k < 0) return fail(ctx, APM_ERR_INVALID, "distance must be >= 0 (the reference reads out of bounds for k<0)");
    std::vector<PatternInfo> v((size_t)n_patterns);
    for (int i = 0; i < n_patterns; ++i) {
        if (!pat[i] || len[i] <= 0) return fail(ctx, APM_ERR_INVALID, "pattern %d is empty", i);
        if (len[i] > APM_MAX_PATTERN_LEN)
            return fail(ctx, APM_ERR_UNSUPPORTED, "pattern %d longer than %d bytes", i, APM_MAX_PATTERN_LEN);
        v[i].bytes.assign(pat[i], pat[i] + len[i]);
        v[i].m = len[i];
    }
    ctx->pats.swap(v);
    ctx->k = k;
    return rebuild(ctx);
}

int apm_set_timing(apm_ctx *ctx, int enabled) {
    if (!ctx) return APM_ERR_INVALID;
    ctx->timing_on = enabled != 0;
    for (apm_ctx *ch : ctx->children) if (ch) ch->timing_on = ctx->timing_on;
    return APM_OK;
}

int apm_set_kernel(apm_ctx *ctx, int kernel) {
    if (!ctx) return APM_ERR_INVALID;
    if (kernel < APM_KERNEL_AUTO || kernel > APM_KERNEL_NFA) return fail(ctx, APM_ERR_INVALID, "unknown kernel variant %d", kernel);
    const int old = ctx->kernel;
    ctx->kernel = kernel;
    if (ctx->patterns_set || !ctx->pats.empty()) {
        const int rc = rebuild(ctx);
        if (rc) { // back to the variant that stood, under the error of the one that did not
            const std::string msg = ctx->err;
            ctx->kernel = old;
            rebuild(ctx);
            ctx->err = msg;
            return rc;
        }
    }
    return APM_OK;
}

int apm_pattern_kernel(const apm_ctx *ctx, int i) {
    if (!ctx || i < 0 || i >= (int)ctx->pats.size()) return APM_ERR_INVALID;
    return ctx->pats[i].kernel == KERNEL_TRIVIAL ? APM_KERNEL_AUTO : ctx->pats[i].kernel;
}

int apm_shard_range(uint64_t n_total, int k, int shard, int n_shards, uint64_t *own_begin, uint64_t *own_end) {
    if (!own_begin || !own_end || n_shards <= 0 || shard < 0 || shard >= n_shards || k < 0) return APM_ERR_INVALID;
    const uint64_t limit = n_total > (uint64_t)k ? n_total - (uint64_t)k : 0;
    auto cut = [&](int s) -> uint64_t {
        if (s <= 0) return 0;
        if (s >= n_shards) return limit;
        const uint64_t c = (uint64_t)((unsigned __int128)limit * (unsigned)s / (unsigned)n_shards);
        return std::min<uint64_t>(limit, c & ~(uint64_t)15);
    };
    *own_begin = cut(shard);
    *own_end = cut(shard + 1);
    return APM_OK;
}

int apm_count_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len,
                           uint64_t n_total, uint64_t own_begin, uint64_t own_end, uint64_t *d_counts) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<false>(
        ctx, "apm_count_shard_device", sh, !d_counts, nullptr, "",
        [&]() { return own_begin > own_end ? fail(ctx, APM_ERR_INVALID, "inconsistent shard description") : (int)APM_OK; },
        [&](DeviceState &ds) {
            const int rc = scan_shard(ctx, ds, sh, own_begin, own_end, (unsigned long long *)d_counts);
            if (!rc) account(ctx, n_total, own_begin, own_end);
            return rc;
        });
}

int apm_synth_fill_device(apm_ctx *ctx, void *d_dst, uint64_t global_off, uint64_t len, uint64_t seed) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_synth_fill_device needs a single-device context");
    if (!d_dst && len) return fail(ctx, APM_ERR_INVALID, "NULL device pointer");
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
    HIP_TRY(ctx, apm_launch_synth((uint8_t *)d_dst, global_off, len, seed, ctx->devs[0].stream));
    return APM_OK;
}

void apm_synth_fill_host(uint8_t *dst, uint64_t global_off, uint64_t len, uint64_t seed) {
    for (uint64_t i = 0; i < len; ++i) dst[i] = apm_synth_byte(global_off + i, seed);
}

int apm_device_alloc(apm_ctx *ctx, void **d_ptr, uint64_t bytes) {
    if (!ctx || !d_ptr) return APM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
    HIP_TRY(ctx, hipMalloc(d_ptr, (size_t)std::max<uint64_t>(bytes, 16)));
    return APM_OK;
}
int apm_device_free(apm_ctx *ctx, void *d_ptr) {
    if (!ctx) return APM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->devs[0].stream));
    HIP_TRY(ctx, hipFree(d_ptr));
    return APM_OK;
}
int apm_device_upload(apm_ctx *ctx, void *d_dst, const void *src, uint64_t bytes) {
    if (!ctx) return APM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->devs[0].stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->devs[0].stream));
    return APM_OK;
}
int apm_device_download(apm_ctx *ctx, void *dst, const void *d_src, uint64_t bytes) {
    if (!ctx) return APM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->devs[0].stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->devs[0].stream));
    return APM_OK;
}
int apm_device_memset(apm_ctx *ctx, void *d_dst, int value, uint64_t bytes) {
    if (!ctx) return APM_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
    HIP_TRY(ctx, hipMemsetAsync(d_dst, value, (size_t)bytes, ctx->devs[0].stream));
    return APM_OK;
}
int apm_synchronize(apm_ctx *ctx) {
    if (!ctx) return APM_ERR_INVALID;
    for (auto &ds : ctx->devs) {
        HIP_TRY(ctx, hipSetDevice(ds.dev));
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    }
    return APM_OK;
}

} // extern "C"
