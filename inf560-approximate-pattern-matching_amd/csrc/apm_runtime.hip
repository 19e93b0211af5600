/*
 * apm_runtime.hip -- implementation of the C ABI in include/apm.h.
 *
 * Host-side replacement for the reference's dispatch layer around its GPU shim:
 *   MPI master/worker + shard bounds   /root/reference/src/database_over_ranks.c:141-195
 *   GPU shims                          /root/reference/src/*.cu (see include/apm.h)
 * Design: owner-computes text sharding with an (m_max-1)-byte halo, truncation
 * only at the end of the WHOLE text, counts summed with one RCCL
 * all-reduce (single-process mode) or by the caller's collective
 * (one-process-per-GPU mode: apm_count_shard_device + torch.distributed).
 *
 * There is no CPU fallback in this file by design.
 */
#include "apm_state.h"
#include "apm_core.h"
#include "apm_score.h"
#include "apm_align.h"
#include "apm_textnorm.h"

#include <algorithm>
#include <atomic>
#include <functional>
#include <mutex>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

thread_local std::string g_create_error;

using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t0) {
    return std::chrono::duration<double, std::milli>(clk::now() - t0).count();
}

} // namespace

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

template <typename T>
int upload_vec(apm_ctx *ctx, T **dptr, const std::vector<T> &v) {
    *dptr = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIP_TRY(ctx, hipMalloc((void **)dptr, bytes));
    if (!v.empty()) HIP_TRY(ctx, hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return APM_OK;
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

void account(apm_ctx *ctx, uint64_t n_total, uint64_t ob, uint64_t oe) {
    // algorithmic / evaluated cells for window starts [ob, oe) (already clipped to n-k)
    const uint64_t k = (uint64_t)ctx->k;
    const uint64_t limit = n_total > k ? n_total - k : 0;
    oe = std::min(oe, limit);
    if (oe <= ob) return;
    for (const auto &p : ctx->pats) {
        const uint64_t m = (uint64_t)p.m;
        const uint64_t full_end = n_total >= m ? std::min<uint64_t>(oe, n_total - m + 1) : 0;
        const uint64_t nfull = full_end > ob ? full_end - ob : 0;
        double cells = double(nfull) * double(m) * double(m);
        for (uint64_t j = std::max(ob, full_end); j < oe; ++j) { // <= m-1 truncated windows
            const double s = double(n_total - j);
            cells += s * s;
        }
        ctx->timing.windows += oe - ob;
        ctx->timing.cells_algorithmic += cells;
        if (p.kernel == APM_KERNEL_BANDED || p.kernel == APM_KERNEL_NFA)
            ctx->timing.cells_evaluated += double(oe - ob) * double(m) * double(2 * (ctx->k / 2) + 1); // upper bound
        else if (p.kernel != KERNEL_TRIVIAL)
            ctx->timing.cells_evaluated += cells;
    }
}

void begin_call(apm_ctx *ctx) {
    ctx->timing = apm_timing{};
    ctx->timing.n_devices = (int)ctx->devs.size();
    for (auto &ds : ctx->devs) {
        ds.text_bytes = 0;
        ds.launches = 0;
        ds.n_stamps = 0;
        ds.events_recorded = false;
    }
}

int load_rccl(apm_ctx *ctx) {
    RcclApi &r = ctx->rccl;
    if (r.ready) return APM_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names) {
        r.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (r.handle) break;
    }
    if (!r.handle) return fail(ctx, APM_ERR_COMM, "cannot load librccl: %s", dlerror());
    r.CommInitAll = (int (*)(void **, int, const int *))dlsym(r.handle, "ncclCommInitAll");
    r.CommDestroy = (int (*)(void *))dlsym(r.handle, "ncclCommDestroy");
    r.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(r.handle, "ncclAllReduce");
    r.GroupStart = (int (*)())dlsym(r.handle, "ncclGroupStart");
    r.GroupEnd = (int (*)())dlsym(r.handle, "ncclGroupEnd");
    if (!r.CommInitAll || !r.CommDestroy || !r.AllReduce || !r.GroupStart || !r.GroupEnd)
        return fail(ctx, APM_ERR_COMM, "librccl lacks a required symbol");
    std::vector<int> devlist;
    for (auto &ds : ctx->devs) devlist.push_back(ds.dev);
    r.comms.assign(ctx->devs.size(), nullptr);
    const int rc = r.CommInitAll(r.comms.data(), (int)devlist.size(), devlist.data());
    if (rc != 0) return fail(ctx, APM_ERR_COMM, "ncclCommInitAll failed (%d)", rc);
    r.ready = true;
    return APM_OK;
}

// sum the per-device partial count vectors into counts[] (host)
int reduce_counts(apm_ctx *ctx, uint64_t *counts) {
    const int P = (int)ctx->pats.size();
    const auto t0 = clk::now();
    const size_t G = ctx->devs.size();
    bool done = false;
    // APM_FORCE_RCCL=1 runs the collective even on one device (test hook for the RCCL path)
    bool distinct = true; // (APM_DEVICES rehearsal: shards sharing a GPU are summed on the host)
    for (size_t a = 0; a < G; ++a)
        for (size_t b = a + 1; b < G; ++b)
            if (ctx->devs[a].dev == ctx->devs[b].dev) distinct = false;
    if (distinct && (G > 1 || getenv("APM_FORCE_RCCL")) && !getenv("APM_NO_RCCL")) {
        if (load_rccl(ctx) == APM_OK) {
            // one ncclAllReduce(sum, uint64 x P) per device, grouped (RCCL over xGMI);
            // replaces the MPI_Send/Recv + manual sum of database_over_ranks.c:174-195
            RcclApi &r = ctx->rccl;
            int rc = r.GroupStart();
            for (size_t g = 0; g < G && rc == 0; ++g) {
                hipSetDevice(ctx->devs[g].dev);
                rc = r.AllReduce(ctx->devs[g].d_counts, ctx->devs[g].d_counts, (size_t)P, /*ncclUint64*/ 5,
                                 /*ncclSum*/ 0, r.comms[g], ctx->devs[g].stream);
            }
            if (rc == 0) rc = r.GroupEnd();
            if (rc != 0) return fail(ctx, APM_ERR_COMM, "ncclAllReduce failed (%d)", rc);
            HIP_TRY(ctx, hipSetDevice(ctx->devs[0].dev));
            HIP_TRY(ctx, hipMemcpyAsync(counts, ctx->devs[0].d_counts, (size_t)P * 8, hipMemcpyDeviceToHost,
                                        ctx->devs[0].stream));
            for (auto &ds : ctx->devs) {
                HIP_TRY(ctx, hipSetDevice(ds.dev));
                HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
            }
            done = true;
        }
    }
    if (!done) {
        std::vector<uint64_t> tmp((size_t)P);
        for (int i = 0; i < P; ++i) counts[i] = 0;
        for (auto &ds : ctx->devs) {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ds.d_counts, (size_t)P * 8, hipMemcpyDeviceToHost, ds.stream));
            HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
            for (int i = 0; i < P; ++i) counts[i] += tmp[i];
        }
    }
    ctx->timing.reduce_ms = ms_since(t0);
    return APM_OK;
}

int collect_event_times(apm_ctx *ctx) {
    double kmax = 0, mmax = 0, hmax = 0;
    uint64_t bytes = 0;
    int launches = 0;
    for (auto &ds : ctx->devs) {
        bytes += ds.text_bytes;
        launches += ds.launches;
        if (!ds.events_recorded) continue;
        HIP_TRY(ctx, hipSetDevice(ds.dev));
        HIP_TRY(ctx, hipEventSynchronize(ds.ev_stop));
        float h = 0, kk = 0, mm = 0;
        hipEventElapsedTime(&h, ds.ev_start, ds.ev_kstart);
        hipEventElapsedTime(&kk, ds.ev_kstart, ds.ev_stop);
        if (hipEventElapsedTime(&mm, ds.ev_mstart, ds.ev_mstop) != hipSuccess) mm = 0;
        hmax = std::max<double>(hmax, h);
        kmax = std::max<double>(kmax, kk);
        mmax = std::max<double>(mmax, mm);
    }
    ctx->timing.h2d_ms = hmax;
    ctx->timing.kernel_ms = kmax;
    ctx->timing.main_kernel_ms = mmax;
    ctx->timing.text_bytes = bytes;
    ctx->timing.n_launches = launches;
    return APM_OK;
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

// the longest pattern of the set, those with k >= m included (the plan's m_max leaves them out: the scan needs no text for
// them, the scoring pass does)
int longest_pattern(const apm_ctx *ctx) {
    int m = 1;
    for (const auto &p : ctx->pats) m = std::max(m, p.m);
    return m;
}

// the half-band the scoring pass needs for ctx->pats at ctx->k, refused beyond what the wave form's LDS band holds
int check_score_band(apm_ctx *ctx) {
    const int band = std::min(ctx->k / 2, longest_pattern(ctx) - 1);
    if (ctx->k > APM_SCORE_LANE_MAX_K && band > APM_SCORE_MAX_BAND)
        return fail(ctx, APM_ERR_UNSUPPORTED, "scoring serves a half-band min(k/2, m_max-1) of at most %d diagonals, this pattern set needs %d",
                    APM_SCORE_MAX_BAND, band);
    return APM_OK;
}

// the scoring and align passes' image of ctx->pats on the device: built by the first such call with a pattern set
// (allocates, copies synchronously), dropped with the plan
int ensure_score_image(apm_ctx *ctx, DeviceState &ds) {
    if (ds.d_score_img) return APM_OK;
    std::vector<uint2> tab(ctx->pats.size());
    size_t bytes = 0;
    for (size_t i = 0; i < ctx->pats.size(); ++i) {
        tab[i] = make_uint2((uint32_t)bytes, (uint32_t)ctx->pats[i].m);
        bytes += apm_score_row_bytes((size_t)ctx->pats[i].m);
    }
    if (bytes > 0xffffffffull) return fail(ctx, APM_ERR_UNSUPPORTED, "the pattern set is too large for the score image");
    std::vector<uint8_t> img(bytes, 0);
    for (size_t i = 0; i < ctx->pats.size(); ++i) memcpy(img.data() + tab[i].x, ctx->pats[i].bytes.data(), (size_t)ctx->pats[i].m);
    int urc = upload_vec(ctx, &ds.d_score_tab, tab);
    if (!urc) urc = upload_vec(ctx, &ds.d_score_img, img);
    return urc;
}

// The record passes' common arguments (ApmScoreArgs) for the records d_rec[0 .. min(*d_n_rec, capacity)) against the shard
// text: refuses a band the scoring pass does not serve and makes sure the score image is on the device.
int record_args(apm_ctx *ctx, DeviceState &ds, const uint8_t *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, ApmScoreArgs &a) {
    int rc = check_score_band(ctx);
    if (!rc) rc = ensure_score_image(ctx, ds);
    if (rc) return rc;
    a.text = d_text;
    a.text_off = text_off;
    a.text_len = text_len;
    a.n_total = n_total;
    a.rec = reinterpret_cast<uint4 *>(const_cast<apm_match *>(d_rec)); // (the align pass only reads them)
    a.cap = capacity;
    a.n_rec = reinterpret_cast<const unsigned long long *>(d_n_rec);
    a.image = ds.d_score_img;
    a.table = ds.d_score_tab;
    a.n_patterns = (uint32_t)ctx->pats.size();
    a.k = ctx->k;
    return APM_OK;
}

// The scoring pass over those records, enqueued on ds.stream behind whatever filled the buffer (apm_score.hip).  Later
// calls with the same pattern set only launch.
int score_records(apm_ctx *ctx, DeviceState &ds, const uint8_t *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                  apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec) {
    ApmScoreArgs a{};
    const int rc = record_args(ctx, ds, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    APM_LAUNCH(ctx, ds, "score", apm_launch_score(a, ds.n_cu, ds.stream));
    return APM_OK;
}

// dwords of one record's row of ops for ctx->pats at ctx->k: the count and the most ops a script of the set has
uint32_t align_row_words(const apm_ctx *ctx) { return (uint32_t)apm_align_words(apm_align_max_ops(longest_pattern(ctx), ctx->k)); }

// The align pass over the same records (apm_align.hip): row r of d_ops (stride dwords apart) gets record r's edit script.
// It refuses what the scoring pass refuses and shares its image; the first call with a pattern set also allocates the
// trace workspace (apm_align.h: sized from APM_ALIGN_WS_BUDGET), later calls only launch.
int align_records(apm_ctx *ctx, DeviceState &ds, const uint8_t *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                  const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, uint32_t *d_ops, uint32_t stride) {
    ApmAlignArgs a{};
    const int rc = record_args(ctx, ds, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    const int m_max = longest_pattern(ctx);
    if (!ds.align_rows) {
        size_t bytes = 0;
        const uint32_t rows = apm_align_rows(m_max, ctx->k, ds.n_cu, APM_BLOCK, &bytes);
        if (bytes && hipMalloc(&ds.d_align_ws, bytes) != hipSuccess) {
            (void)hipGetLastError();
            ds.d_align_ws = nullptr;
            return fail(ctx, APM_ERR_NOMEM, "cannot allocate the align pass's trace workspace (%zu bytes)", bytes);
        }
        ds.align_rows = rows;
    }
    a.ops = d_ops;
    a.stride = stride;
    a.ws = ds.d_align_ws;
    a.m_max = (uint32_t)m_max;
    a.row_entries = apm_align_wave_row_entries(m_max, ctx->k);
    APM_LAUNCH(ctx, ds, "align", apm_launch_align(a, ds.align_rows, ds.stream));
    ds.last_align_rows = ds.align_rows;
    return APM_OK;
}

// apm_score_shard_device and apm_align_shard_device: the checks both make, in `name`'s words, then `extra()` (the caller's
// own checks, 0: pass), then `pass(ds)` between the call's events -- the one launch is the whole call, all of its event
// pairs bracket it.  extra_null: a pointer of the caller's own that is NULL where it may not be.
template <class Extra, class Pass>
int record_pass_shard_device(apm_ctx *ctx, const char *name, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, bool extra_null, Extra extra, Pass pass) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "%s needs a single-device context", name);
    if (!d_n_rec || ((!d_rec || extra_null) && capacity) || (!d_text && text_len)) return fail(ctx, APM_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_rec) & 15u) return fail(ctx, APM_ERR_INVALID, "d_rec must be 16-byte aligned");
    if (text_off + text_len > n_total) return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
    int rc = extra();
    if (rc) return rc;
    begin_call(ctx);
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    if (ctx->timing_on) {
        for (hipEvent_t e : {ds.ev_start, ds.ev_kstart, ds.ev_mstart}) HIP_TRY(ctx, hipEventRecord(e, ds.stream));
    }
    rc = pass(ds);
    if (rc) return rc;
    if (ctx->timing_on) {
        for (hipEvent_t e : {ds.ev_mstop, ds.ev_stop}) HIP_TRY(ctx, hipEventRecord(e, ds.stream));
        ds.events_recorded = true;
    }
    return APM_OK;
}

// the three host-level entry points share this: `stage(g, ds, lo, len)` must enqueue the
// bytes of global positions [lo, lo+len) into ds.d_text on ds.stream.
// Staging runs CONCURRENTLY, one host thread per device (the replacement of the reference's per-rank reads,
// /root/reference/src/database_over_ranks.c:141-166: there every MPI rank read its own piece at the same time; round 2
// staged device g's whole shard before touching device g + 1).  The scan launches follow from the calling thread as
// each device's staging thread returns: they are microseconds of host time.
// find_cap != NULL (apm_find_all_buffer): every device also appends the (pattern, position) records of its owner range,
// up to *find_cap of them, to its own buffer ds.d_rec / ds.d_rec_n (global positions: nothing to fix up at the merge);
// mode FIND_DIST (apm_find_all_dist_buffer): and scores them there against its resident text -- the halo covers every owned
// window; FIND_ALIGN (apm_find_all_align_buffer): and then aligns them into its own rows ds.d_ops, `stride` dwords each
enum FindMode { FIND_PLAIN = 0, FIND_DIST = 1, FIND_ALIGN = 2 };
template <typename Stage>
int count_sharded(apm_ctx *ctx, uint64_t n, uint64_t *counts, Stage stage, const uint64_t *find_cap = nullptr, int mode = FIND_PLAIN,
                  uint32_t stride = 0) {
    const bool score = mode != FIND_PLAIN;
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!counts) return fail(ctx, APM_ERR_INVALID, "counts is NULL");
    const auto t0 = clk::now();
    begin_call(ctx);
    const bool timing_saved = ctx->timing_on;
    ctx->timing_on = true; // the host-level calls synchronise anyway; keep their event times
    struct Restore { apm_ctx *c; bool v; ~Restore() { c->timing_on = v; } } restore{ctx, timing_saved};
    const int G = (int)ctx->devs.size();
    const int P = (int)ctx->pats.size();
    // (scoring: the windows of patterns with k >= m need their text too)
    const uint64_t halo = (uint64_t)(score ? longest_pattern(ctx) : std::max(ctx->plan.m_max, 1)) - 1;
    struct Shard { uint64_t ob = 0, oe = 0, lo = 0, len = 0; int rc = APM_OK; };
    std::vector<Shard> sh((size_t)G);
    auto stage_device = [&](int g) {
        DeviceState &ds = ctx->devs[g];
        Shard &S = sh[(size_t)g];
        apm_shard_range(n, ctx->k, g, G, &S.ob, &S.oe);
        S.lo = S.ob;
        const uint64_t hi = std::min<uint64_t>(n, S.oe + halo);
        S.len = hi > S.lo ? hi - S.lo : 0;
        S.rc = [&]() -> int {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            HIP_TRY(ctx, hipEventRecord(ds.ev_start, ds.stream));
            HIP_TRY(ctx, hipMemsetAsync(ds.d_counts, 0, std::max<size_t>((size_t)P * 8, 16), ds.stream));
            if (find_cap) {
                if (!ds.d_rec_n) HIP_TRY(ctx, hipMalloc((void **)&ds.d_rec_n, 16));
                if (ds.rec_cap < *find_cap || !ds.d_rec) { // (reused while it is large enough)
                    if (ds.d_rec) {
                        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
                        HIP_TRY(ctx, hipFree(ds.d_rec));
                    }
                    ds.d_rec = nullptr;
                    ds.rec_cap = 0;
                    if (hipMalloc((void **)&ds.d_rec, (size_t)std::max<uint64_t>(*find_cap, 1) * 16) != hipSuccess) {
                        (void)hipGetLastError();
                        return fail(ctx, APM_ERR_NOMEM, "cannot allocate the record buffer (%llu records)", (unsigned long long)*find_cap);
                    }
                    ds.rec_cap = std::max<uint64_t>(*find_cap, 1);
                }
                HIP_TRY(ctx, hipMemsetAsync(ds.d_rec_n, 0, 16, ds.stream));
                const unsigned long long ops_words = std::max<uint64_t>(*find_cap, 1) * stride;
                if (mode == FIND_ALIGN && (ds.ops_cap < ops_words || !ds.d_ops)) { // (reused while it is large enough)
                    if (ds.d_ops) {
                        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
                        HIP_TRY(ctx, hipFree(ds.d_ops));
                    }
                    ds.d_ops = nullptr;
                    ds.ops_cap = 0;
                    if (hipMalloc((void **)&ds.d_ops, (size_t)ops_words * 4) != hipSuccess) {
                        (void)hipGetLastError();
                        return fail(ctx, APM_ERR_NOMEM, "cannot allocate the rows of ops (%llu records of %u dwords)", (unsigned long long)*find_cap, stride);
                    }
                    ds.ops_cap = ops_words;
                }
            }
            if (S.oe > S.ob) {
                int rc = ensure_text(ctx, ds, (size_t)S.len + 16);
                if (rc) return rc;
                rc = stage(g, ds, S.lo, S.len);
                if (rc) return rc;
            }
            HIP_TRY(ctx, hipEventRecord(ds.ev_kstart, ds.stream));
            return APM_OK;
        }();
    };
    std::vector<std::thread> th;
    for (int g = 1; g < G; ++g) th.emplace_back(stage_device, g);
    stage_device(0);
    int first_rc = APM_OK;
    for (int g = 0; g < G; ++g) {
        if (g > 0) th[(size_t)g - 1].join();
        DeviceState &ds = ctx->devs[g];
        const Shard &S = sh[(size_t)g];
        if (S.rc && !first_rc) first_rc = S.rc;
        if (first_rc) continue; // (keep joining)
        int rc = [&]() -> int {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            if (S.oe > S.ob) {
                ApmPosSink rs{};
                if (find_cap) {
                    rs.out = ds.d_rec;
                    rs.count = ds.d_rec_n;
                    rs.cap = *find_cap;
                }
                const int r2 = scan_shard(ctx, ds, ds.d_text, S.lo, S.len, n, S.ob, S.oe, ds.d_counts, find_cap ? &rs : nullptr);
                if (r2) return r2;
                if (find_cap && score) {
                    const int r3 = score_records(ctx, ds, ds.d_text, S.lo, S.len, n, reinterpret_cast<apm_match *>(ds.d_rec), *find_cap,
                                                 reinterpret_cast<const uint64_t *>(ds.d_rec_n));
                    if (r3) return r3;
                }
                if (find_cap && mode == FIND_ALIGN) {
                    const int r4 = align_records(ctx, ds, ds.d_text, S.lo, S.len, n, reinterpret_cast<const apm_match *>(ds.d_rec), *find_cap,
                                                 reinterpret_cast<const uint64_t *>(ds.d_rec_n), ds.d_ops, stride);
                    if (r4) return r4;
                }
                account(ctx, n, S.ob, S.oe);
            } else {
                HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
                HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
            }
            HIP_TRY(ctx, hipEventRecord(ds.ev_stop, ds.stream));
            ds.events_recorded = true;
            return APM_OK;
        }();
        if (rc && !first_rc) first_rc = rc;
    }
    if (first_rc) return first_rc;
    int rc = reduce_counts(ctx, counts);
    if (rc) return rc;
    rc = collect_event_times(ctx);
    if (rc) return rc;
    ctx->timing.total_ms = ms_since(t0);
    return APM_OK;
}

// Host bytes -> d_dst (the device text, or the raw buffer of a text mode) through the context's ring of pinned staging
// buffers (apm_count_buffer, apm_count_file).
// `read(off, dst, len)` must put bytes [off, off+len) of the source into dst (false: I/O error).  Device g of G owns the
// buffers [g * per, (g + 1) * per) of the ring, two per reader thread: a reader takes the next 8 MiB chunk of the
// device's shard, reads it into one of its two buffers, enqueues the copy on the device's stream and reads the next
// chunk into the other while that one travels (a buffer is reused once its copy's event has fired).  A single reader
// runs at a fraction of the PCIe link; several side by side keep it busy (2 -> 35, 4 -> 44, 8 -> 40 GB/s on one
// device), and no pages of the caller's buffer are pinned per call.
int stage_through_ring(apm_ctx *ctx, int g, int G, DeviceState &ds, uint8_t *d_dst, uint64_t lo, uint64_t len,
                       const std::function<bool(uint64_t, uint8_t *, size_t)> &read) {
    const size_t CH = apm_ctx::STAGE_BYTES;
    static const int n_readers = [] {
        const char *e = getenv("APM_INGEST_THREADS");
        const int hw = (int)std::thread::hardware_concurrency();
        int t = e ? atoi(e) : std::min(4, hw > 1 ? hw / 2 : 1);
        return t < 1 ? 1 : t;
    }();
    const int per = std::max(2, (apm_ctx::N_STAGE / std::max(G, 1)) & ~1); // buffers of this device (G <= N_STAGE / 2)
    if ((g + 1) * per > apm_ctx::N_STAGE) return fail(ctx, APM_ERR_UNSUPPORTED, "more devices than staging buffers");
    const int b0 = g * per;
    const uint64_t n_chunks = (len + CH - 1) / CH;
    const int nt = (int)std::min<uint64_t>((uint64_t)std::min(n_readers, per / 2), n_chunks);
    for (int b = b0; b < b0 + 2 * nt; ++b) { // (current device = ds.dev; these buffers are this device's alone)
        if (!ctx->stage[b] && hipHostMalloc((void **)&ctx->stage[b], CH, hipHostMallocDefault) != hipSuccess)
            return fail(ctx, APM_ERR_NOMEM, "cannot allocate pinned staging buffers");
        if (!ds.ev_stage[b]) HIP_TRY(ctx, hipEventCreateWithFlags(&ds.ev_stage[b], hipEventDisableTiming));
    }
    std::atomic<uint64_t> next{0};
    std::atomic<int> bad{0};
    auto reader = [&](int t) {
        if (hipSetDevice(ds.dev) != hipSuccess) { bad = 2; return; }
        int flip = 0;
        bool used[2] = {false, false};
        for (;;) {
            const uint64_t c = next.fetch_add(1);
            if (c >= n_chunks || bad.load()) break;
            const int b = b0 + 2 * t + flip;
            if (used[flip] && hipEventSynchronize(ds.ev_stage[b]) != hipSuccess) { bad = 2; break; }
            const uint64_t off = c * CH;
            const size_t want = (size_t)std::min<uint64_t>(CH, len - off);
            if (!read(lo + off, ctx->stage[b], want)) { bad = 1; break; }
            if (hipMemcpyAsync(d_dst + off, ctx->stage[b], want, hipMemcpyHostToDevice, ds.stream) != hipSuccess ||
                hipEventRecord(ds.ev_stage[b], ds.stream) != hipSuccess) { bad = 2; break; }
            used[flip] = true;
            flip ^= 1;
        }
        for (int f = 0; f < 2; ++f) // the buffers are free again when this call returns (the next call may be another device's)
            if (used[f] && hipEventSynchronize(ds.ev_stage[b0 + 2 * t + f]) != hipSuccess) bad = 2;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(reader, t);
    if (nt > 0) reader(0);
    for (auto &t : th) t.join();
    if (bad.load() == 1) return fail(ctx, APM_ERR_IO, "Unable to copy %llu byte(s) from text file", (unsigned long long)len);
    if (bad.load()) return fail(ctx, APM_ERR_HIP, "staging copy failed: %s", hipGetErrorString(hipGetLastError()));
    return APM_OK;
}


// ---- text normalisation (apm_textnorm.hip) ----
int ensure_tn_event(apm_ctx *ctx, hipEvent_t &e) {
    if (!e) HIP_TRY(ctx, hipEventCreate(&e));
    return APM_OK;
}

// the pass's summaries and map for a source of n_blocks blocks: grown on demand (behind the stream: a map launch of an
// earlier call may still read them), kept by the context
int ensure_tn_map(apm_ctx *ctx, DeviceState &ds, uint64_t n_blocks) {
    if (!ds.d_tn_total) HIP_TRY(ctx, hipMalloc((void **)&ds.d_tn_total, 16));
    if (n_blocks <= ds.tn_cap) return APM_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    if (ds.d_tn_summary) hipFree(ds.d_tn_summary);
    if (ds.d_tn_map) hipFree(ds.d_tn_map);
    ds.d_tn_summary = nullptr;
    ds.d_tn_map = nullptr;
    ds.tn_cap = 0;
    const size_t cap = (size_t)((n_blocks + 4095) & ~(uint64_t)4095); // (the scan reads the summaries in whole chunks)
    if (hipMalloc((void **)&ds.d_tn_summary, cap * 4) != hipSuccess || hipMalloc((void **)&ds.d_tn_map, (cap + 1) * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, APM_ERR_NOMEM, "cannot allocate the normalisation map (%llu blocks)", (unsigned long long)n_blocks);
    }
    ds.tn_cap = cap;
    return APM_OK;
}

// apm_normalize_device on ds.stream: summary and scan, ONE synchronisation for the total, the scatter
int normalize_on_stream(apm_ctx *ctx, DeviceState &ds, const uint8_t *d_src, uint64_t src_len, unsigned flags, uint8_t *d_dst,
                        uint64_t dst_capacity, uint64_t *out_len) {
    ds.tn_valid = ds.tn_timed = false;
    ds.tn_src_bytes = src_len;
    ds.tn_kept_bytes = 0;
    ApmTnSrc src{};
    src.lead = (uint32_t)(reinterpret_cast<uintptr_t>(d_src) & 15u);
    src.base = d_src - src.lead;
    src.end = (uint64_t)src.lead + src_len;
    src.n_blocks = src_len ? (src.end + APM_TN_BLOCK - 1) / APM_TN_BLOCK : 0;
    src.flags = flags;
    *out_len = 0;
    if (src_len) {
        int rc = ensure_tn_map(ctx, ds, src.n_blocks);
        for (int i = 0; i < 2 && !rc && ctx->timing_on; ++i) rc = ensure_tn_event(ctx, ds.ev_tn[i]);
        if (rc) return rc;
        ApmTnArgs a{};
        a.src = src;
        a.summary = ds.d_tn_summary;
        a.map = ds.d_tn_map;
        a.total = ds.d_tn_total;
        a.dst = d_dst;
        if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_tn[0], ds.stream));
        HIP_TRY(ctx, apm_launch_tn_summary(a, ds.n_cu, ds.stream));
        HIP_TRY(ctx, apm_launch_tn_scan(a, ds.stream));
        unsigned long long total = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&total, ds.d_tn_total, 8, hipMemcpyDeviceToHost, ds.stream));
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
        if (total > dst_capacity)
            return fail(ctx, APM_ERR_INVALID, "the normalised text has %llu bytes, the destination holds %llu", total, (unsigned long long)dst_capacity);
        HIP_TRY(ctx, apm_launch_tn_scatter(a, ds.n_cu, ds.stream));
        if (ctx->timing_on) {
            HIP_TRY(ctx, hipEventRecord(ds.ev_tn[1], ds.stream));
            ds.tn_timed = true;
        }
        ds.tn_kept_bytes = *out_len = total;
    }
    ds.tn_src = src;
    ds.tn_valid = true;
    return APM_OK;
}

// apm_map_positions_device on ds.stream, behind whatever filled the records
int map_positions_on_stream(apm_ctx *ctx, DeviceState &ds, apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec) {
    if (!ds.tn_valid) return fail(ctx, APM_ERR_STATE, "no text has been normalised on this context");
    ds.map_timed = false;
    if (!ds.tn_src.n_blocks || !capacity) return APM_OK; // (no record names a byte of an empty text)
    ApmTnMapArgs a{};
    a.src = ds.tn_src;
    a.map = ds.d_tn_map;
    a.rec = reinterpret_cast<uint4 *>(d_rec);
    a.cap = capacity;
    a.n_rec = reinterpret_cast<const unsigned long long *>(d_n_rec);
    if (ctx->timing_on) {
        for (int i = 2; i < 4; ++i) { const int rc = ensure_tn_event(ctx, ds.ev_tn[i]); if (rc) return rc; }
        HIP_TRY(ctx, hipEventRecord(ds.ev_tn[2], ds.stream));
    }
    HIP_TRY(ctx, apm_launch_tn_map(a, ds.n_cu, ds.stream));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_tn[3], ds.stream));
        ds.map_timed = true;
    }
    return APM_OK;
}

// A text mode's ingest on the (single) device: `stage_raw(ds, d_raw)` enqueues the n source bytes into the raw buffer,
// the pass normalises them into ds.d_text -- sized for the raw length first, so that count_sharded finds it large enough
// and leaves it alone -- and *n_text is the length count_sharded then scans, with a stage step that has nothing to copy.
template <typename StageRaw>
int stage_normalized(apm_ctx *ctx, uint64_t n, StageRaw stage_raw, uint64_t *n_text) {
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    const size_t want = ((size_t)n + 16 + 255) & ~(size_t)255;
    if (want > ds.raw_cap) {
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream)); // (a map launch of an earlier call may still read it)
        if (ds.d_raw) hipFree(ds.d_raw);
        ds.d_raw = nullptr;
        ds.raw_cap = 0;
        ds.tn_valid = false;
        if (hipMalloc((void **)&ds.d_raw, want) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, APM_ERR_NOMEM, "cannot allocate the raw text buffer (%zu bytes)", want);
        }
        ds.raw_cap = want;
    }
    int rc = ensure_text(ctx, ds, (size_t)n + 16);
    if (!rc && n) rc = stage_raw(ds, ds.d_raw);
    if (rc) return rc;
    return normalize_on_stream(ctx, ds, ds.d_raw, n, ctx->text_mode, ds.d_text, n, n_text);
}

// count_sharded's stage step behind stage_normalized
int stage_nothing(int, DeviceState &, uint64_t, uint64_t) { return APM_OK; }

} // namespace

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
        for (void *p : {(void *)ds.d_scratch, (void *)ds.d_text, (void *)ds.d_rec, (void *)ds.d_rec_n, (void *)ds.d_ops, (void *)ds.d_masks, (void *)ds.d_stats,
                        (void *)ds.d_work, (void *)ds.d_blist, (void *)ds.d_clist, (void *)ds.d_clist_cnt, (void *)ds.d_raw, (void *)ds.d_tn_summary,
                        (void *)ds.d_tn_map, (void *)ds.d_tn_total})
            if (p) hipFree(p);
        for (hipEvent_t e : ds.ev_stage) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ds.ev_launch) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ds.ev_tn) if (e) hipEventDestroy(e);
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

static bool pattern_sharded(const apm_ctx *ctx) { return ctx->partition == APM_PARTITION_PATTERNS && ctx->devs.size() > 1; }

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
static int for_children(apm_ctx *ctx, uint64_t *counts, const std::function<int(apm_ctx *, uint64_t *)> &fn) {
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

int apm_set_partition(apm_ctx *ctx, int partition) {
    if (!ctx) return APM_ERR_INVALID;
    if (partition != APM_PARTITION_TEXT && partition != APM_PARTITION_PATTERNS) return fail(ctx, APM_ERR_INVALID, "unknown partition %d", partition);
    if (partition == ctx->partition) return APM_OK;
    ctx->partition = partition;
    if (ctx->pats.empty()) return APM_OK;
    ctx->patterns_set = false;
    const int rc = pattern_sharded(ctx) ? build_children(ctx) : build_plan(ctx);
    if (rc) return rc;
    ctx->patterns_set = true;
    return APM_OK;
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
    ctx->patterns_set = false;
    const int rc = pattern_sharded(ctx) ? build_children(ctx) : build_plan(ctx);
    if (rc) return rc;
    ctx->patterns_set = true;
    return APM_OK;
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
        ctx->patterns_set = false;
        auto rebuild = [&]() { return pattern_sharded(ctx) ? build_children(ctx) : build_plan(ctx); };
        const int rc = rebuild();
        if (rc) {
            const std::string msg = ctx->err;
            ctx->kernel = old;
            if (rebuild() == APM_OK) ctx->patterns_set = true;
            ctx->err = msg;
            return rc;
        }
        ctx->patterns_set = true;
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
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_count_shard_device needs a single-device context");
    if (!d_counts || (!d_text && text_len)) return fail(ctx, APM_ERR_INVALID, "NULL device pointer");
    if (text_off + text_len > n_total || own_begin > own_end)
        return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
    begin_call(ctx);
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_start, ds.stream));
        HIP_TRY(ctx, hipEventRecord(ds.ev_kstart, ds.stream));
    }
    const int rc = scan_shard(ctx, ds, (const uint8_t *)d_text, text_off, text_len, n_total, own_begin, own_end,
                              (unsigned long long *)d_counts);
    if (rc) return rc;
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_stop, ds.stream));
        ds.events_recorded = true;
    }
    account(ctx, n_total, own_begin, own_end);
    return APM_OK;
}

// host text -> the devices' shards -> scan; find_cap, mode, stride: see count_sharded
static int count_host_text(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t *counts, const uint64_t *find_cap, int mode = FIND_PLAIN,
                           uint32_t stride = 0) {
    const int G = (int)ctx->devs.size();
    // the bytes [lo, lo + len) of the host text -> d_dst on device g
    auto stage = [&](int g, DeviceState &ds, uint8_t *d_dst, uint64_t lo, uint64_t len) -> int {
        if (len < (1u << 20)) { // small: one pageable copy (the runtime stages it itself)
            HIP_TRY(ctx, hipMemcpyAsync(d_dst, text + lo, (size_t)len, hipMemcpyHostToDevice, ds.stream));
            return APM_OK;
        }
        // through the pinned ring: round 2 pinned the caller's whole buffer with hipHostRegister on every call
        return stage_through_ring(ctx, g, G, ds, d_dst, lo, len, [&](uint64_t off, uint8_t *dst, size_t want) {
            memcpy(dst, text + off, want);
            return true;
        });
    };
    if (ctx->text_mode) { // (single device: apm_set_text_mode)
        if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
        if (!counts) return fail(ctx, APM_ERR_INVALID, "counts is NULL");
        const auto t0 = clk::now();
        uint64_t n_text = 0;
        int rc = stage_normalized(ctx, n, [&](DeviceState &ds, uint8_t *d_raw) { return stage(0, ds, d_raw, 0, n); }, &n_text);
        if (!rc) rc = count_sharded(ctx, n_text, counts, stage_nothing, find_cap, mode, stride);
        if (!rc) ctx->timing.total_ms = ms_since(t0);
        return rc;
    }
    return count_sharded(ctx, n, counts, [&](int g, DeviceState &ds, uint64_t lo, uint64_t len) { return stage(g, ds, ds.d_text, lo, len); },
                         find_cap, mode, stride);
}

int apm_count_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t *counts) {
    if (!ctx) return APM_ERR_INVALID;
    if (!text && n) return fail(ctx, APM_ERR_INVALID, "text is NULL");
    if (pattern_sharded(ctx)) return for_children(ctx, counts, [&](apm_ctx *ch, uint64_t *c) { return apm_count_buffer(ch, text, n, c); });
    return count_host_text(ctx, text, n, counts, nullptr);
}

int apm_count_file(apm_ctx *ctx, const char *path, uint64_t *counts) {
    if (!ctx) return APM_ERR_INVALID;
    if (!path) return fail(ctx, APM_ERR_INVALID, "path is NULL");
    if (pattern_sharded(ctx)) { // every device reads the whole file (as every rank of the reference's PATTERNS_OVER_RANKS did)
        const int fdt = open(path, O_RDONLY);
        if (fdt < 0) return fail(ctx, APM_ERR_IO, "Unable to open the text file <%s>", path);
        close(fdt);
        return for_children(ctx, counts, [&](apm_ctx *ch, uint64_t *c) { return apm_count_file(ch, path, c); });
    }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(ctx, APM_ERR_IO, "Unable to open the text file <%s>", path);
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
        close(fd);
        return fail(ctx, APM_ERR_IO, "Unable to stat the text file <%s>", path);
    }
    const uint64_t n = (uint64_t)st.st_size;
    const int G = (int)ctx->devs.size();
    // chunked ingest, all devices at once (stage_through_ring): pread out of the page cache into pinned buffers
    auto stage = [&](int g, DeviceState &ds, uint8_t *d_dst, uint64_t lo, uint64_t len) -> int {
        return stage_through_ring(ctx, g, G, ds, d_dst, lo, len, [&](uint64_t off, uint8_t *dst, size_t want) {
            size_t got = 0;
            while (got < want) {
                const ssize_t r = pread(fd, dst + got, want - got, (off_t)(off + got));
                if (r <= 0) return false;
                got += (size_t)r;
            }
            return true;
        });
    };
    int rc = APM_OK;
    if (ctx->text_mode) { // (single device: apm_set_text_mode) the whole file into the raw buffer, the pass, the scan of what it kept
        const auto t0 = clk::now();
        uint64_t n_text = 0;
        if (!ctx->patterns_set) rc = fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
        else if (!counts) rc = fail(ctx, APM_ERR_INVALID, "counts is NULL");
        if (!rc) rc = stage_normalized(ctx, n, [&](DeviceState &ds, uint8_t *d_raw) { return stage(0, ds, d_raw, 0, n); }, &n_text);
        if (!rc) rc = count_sharded(ctx, n_text, counts, stage_nothing);
        if (!rc) ctx->timing.total_ms = ms_since(t0);
    } else {
        rc = count_sharded(ctx, n, counts, [&](int g, DeviceState &ds, uint64_t lo, uint64_t len) { return stage(g, ds, ds.d_text, lo, len); });
    }
    close(fd);
    return rc;
}

int apm_find_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, int pattern_index, uint64_t *positions,
                    uint64_t capacity, uint64_t *n_found) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (pattern_index < 0 || pattern_index >= (int)ctx->pats.size() || !n_found || (!positions && capacity) || (!text && n))
        return fail(ctx, APM_ERR_INVALID, "bad argument to apm_find_buffer");
    if (ctx->text_mode) return fail(ctx, APM_ERR_UNSUPPORTED, "apm_find_buffer does not serve a text mode (apm_set_text_mode): use apm_find_all_buffer");
    if (pattern_sharded(ctx)) { // the device that holds the pattern
        size_t g = 0;
        while (g + 1 < ctx->children.size() && pattern_index >= ctx->pat_first[g + 1]) ++g;
        const int rc = apm_find_buffer(ctx->children[g], text, n, pattern_index - ctx->pat_first[g], positions, capacity, n_found);
        if (rc) return fail(ctx, rc, "%s", ctx->children[g]->err.c_str());
        return APM_OK;
    }
    // run the one pattern through the full-DP kernels with a position sink, then restore the plan
    const std::vector<PatternInfo> saved = ctx->pats;
    const int saved_kernel = ctx->kernel;
    const PatternInfo one = saved[(size_t)pattern_index];
    auto restore = [&]() {
        ctx->pats = saved;
        ctx->kernel = saved_kernel;
        ctx->find_active = false;
        for (auto &ds : ctx->devs) {
            hipSetDevice(ds.dev);
            if (ds.d_pos_out) hipFree(ds.d_pos_out), ds.d_pos_out = nullptr;
            if (ds.d_pos_count) hipFree(ds.d_pos_count), ds.d_pos_count = nullptr;
        }
        const std::string keep = ctx->err;
        ctx->patterns_set = (build_plan(ctx) == APM_OK);
        if (!keep.empty()) ctx->err = keep;
    };
    ctx->pats.assign(1, one);
    // the full-DP kernel AUTO's long-pattern rule picks: BITPAR up to 1024 bytes or while the Eq rows fit LDS, else GENERIC
    ctx->kernel = one.m <= 1024 || (one.m <= APM_BITPAR_MAX_M && bitlong_rows_fit(one)) ? APM_KERNEL_BITPAR : APM_KERNEL_GENERIC;
    int rc = build_plan(ctx);
    if (rc) { restore(); return rc; }
    for (auto &ds : ctx->devs) {
        if (hipSetDevice(ds.dev) != hipSuccess ||
            hipMalloc((void **)&ds.d_pos_out, (size_t)std::max<uint64_t>(capacity, 1) * 8) != hipSuccess ||
            hipMalloc((void **)&ds.d_pos_count, 16) != hipSuccess || hipMemset(ds.d_pos_count, 0, 16) != hipSuccess) {
            restore();
            return fail(ctx, APM_ERR_NOMEM, "cannot allocate the position buffer (%llu entries)", (unsigned long long)capacity);
        }
        ds.pos_cap = capacity;
    }
    ctx->find_active = true;
    ctx->err.clear();
    uint64_t cnt1 = 0;
    rc = apm_count_buffer(ctx, text, n, &cnt1);
    std::vector<uint64_t> all;
    uint64_t total = 0;
    if (rc == APM_OK) {
        for (auto &ds : ctx->devs) {
            unsigned long long c = 0;
            if (hipSetDevice(ds.dev) != hipSuccess || hipMemcpy(&c, ds.d_pos_count, 8, hipMemcpyDeviceToHost) != hipSuccess) {
                rc = fail(ctx, APM_ERR_HIP, "cannot read back the match positions");
                break;
            }
            total += c;
            const size_t take = (size_t)std::min<uint64_t>(c, capacity);
            const size_t at = all.size();
            all.resize(at + take);
            if (take && hipMemcpy(all.data() + at, ds.d_pos_out, take * 8, hipMemcpyDeviceToHost) != hipSuccess) {
                rc = fail(ctx, APM_ERR_HIP, "cannot read back the match positions");
                break;
            }
        }
    }
    if (rc == APM_OK) {
        std::sort(all.begin(), all.end());
        for (size_t i = 0; i < all.size() && i < capacity; ++i) positions[i] = all[i];
        *n_found = total;
        if (total != cnt1) rc = fail(ctx, APM_ERR_STATE, "position sink count %llu != match count %llu", (unsigned long long)total, (unsigned long long)cnt1);
    }
    restore();
    return rc;
}

static bool match_less(const apm_match &a, const apm_match &b) { return a.pattern != b.pattern ? a.pattern < b.pattern : a.pos < b.pos; }

// apm_find_all_buffer; mode FIND_DIST: apm_find_all_dist_buffer, every device (every child) scores its records before they
// leave it; FIND_ALIGN: apm_find_all_align_buffer, and aligns them into rows of `stride` dwords, which travel with their
// records through the (pattern, pos) sort as an index permutation
static int find_all(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found, int mode,
                    uint32_t *ops = nullptr, uint32_t stride = 0) {
    static const char *const names[] = {"apm_find_all_buffer", "apm_find_all_dist_buffer", "apm_find_all_align_buffer"};
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!n_found || (!out && capacity) || (!text && n) || (mode == FIND_ALIGN && !ops && capacity))
        return fail(ctx, APM_ERR_INVALID, "bad argument to %s", names[mode]);
    if (mode == FIND_ALIGN && stride < align_row_words(ctx))
        return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than apm_align_row_words() = %u", stride, align_row_words(ctx));
    std::vector<apm_match> all;
    std::vector<uint32_t> rows; // FIND_ALIGN: row i of `stride` dwords belongs to all[i]
    uint64_t total = 0;
    if (pattern_sharded(ctx)) { // every child finds its slice in the whole text; the indices are shifted by the slice's first pattern
        const size_t G = ctx->children.size();
        std::vector<std::vector<apm_match>> part(G);
        std::vector<std::vector<uint32_t>> part_ops(G);
        std::vector<uint64_t> found(G, 0);
        std::vector<uint64_t> dummy(ctx->pats.size(), 0);
        const int rc = for_children(ctx, dummy.data(), [&](apm_ctx *ch, uint64_t *) {
            const size_t g = (size_t)(std::find(ctx->children.begin(), ctx->children.end(), ch) - ctx->children.begin());
            part[g].resize((size_t)capacity);
            if (mode == FIND_ALIGN) part_ops[g].assign((size_t)capacity * stride, 0u);
            // (scored and aligned with the child's own slice, at the parent's stride)
            return find_all(ch, text, n, part[g].data(), capacity, &found[g], mode, part_ops[g].data(), stride);
        });
        if (rc) return rc;
        for (size_t g = 0; g < G; ++g) {
            total += found[g];
            const size_t take = (size_t)std::min<uint64_t>(found[g], capacity);
            for (size_t i = 0; i < take; ++i) {
                apm_match r = part[g][i];
                r.pattern += (uint32_t)ctx->pat_first[g];
                all.push_back(r);
            }
            if (mode == FIND_ALIGN) rows.insert(rows.end(), part_ops[g].begin(), part_ops[g].begin() + (ptrdiff_t)(take * stride));
        }
    } else {
        std::vector<uint64_t> counts(ctx->pats.size(), 0);
        int rc = mode != FIND_PLAIN ? check_score_band(ctx) : APM_OK; // (refused before anything is scanned)
        if (!rc) rc = count_host_text(ctx, text, n, counts.data(), &capacity, mode, stride);
        if (rc) return rc;
        uint64_t csum = 0;
        for (uint64_t c : counts) csum += c;
        if (ctx->text_mode) { // positions in the normalised text -> source offsets, behind scan, score and align
            DeviceState &ds = ctx->devs[0];
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            rc = map_positions_on_stream(ctx, ds, reinterpret_cast<apm_match *>(ds.d_rec), capacity, reinterpret_cast<const uint64_t *>(ds.d_rec_n));
            if (rc) return rc;
            HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
        }
        for (auto &ds : ctx->devs) { // TEXT partition: every device holds the records of its owner range, global positions
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            unsigned long long c = 0;
            HIP_TRY(ctx, hipMemcpy(&c, ds.d_rec_n, 8, hipMemcpyDeviceToHost));
            total += c;
            const size_t take = (size_t)std::min<uint64_t>(c, capacity), at = all.size();
            all.resize(at + take);
            if (take) HIP_TRY(ctx, hipMemcpy(all.data() + at, ds.d_rec, take * sizeof(apm_match), hipMemcpyDeviceToHost));
            if (mode == FIND_ALIGN) {
                rows.resize((at + take) * stride);
                if (take) HIP_TRY(ctx, hipMemcpy(rows.data() + at * stride, ds.d_ops, take * stride * 4, hipMemcpyDeviceToHost));
            }
        }
        if (total != csum)
            return fail(ctx, APM_ERR_STATE, "record sink count %llu != match count %llu", (unsigned long long)total, (unsigned long long)csum);
    }
    if (mode != FIND_ALIGN) {
        std::sort(all.begin(), all.end(), match_less);
        for (size_t i = 0; i < all.size() && i < capacity; ++i) out[i] = all[i];
    } else {
        std::vector<size_t> perm(all.size());
        for (size_t i = 0; i < perm.size(); ++i) perm[i] = i;
        std::sort(perm.begin(), perm.end(), [&](size_t a, size_t b) { return match_less(all[a], all[b]); });
        for (size_t i = 0; i < perm.size() && i < capacity; ++i) {
            out[i] = all[perm[i]];
            const uint32_t *row = rows.data() + perm[i] * stride;
            // the words the row format defines: the count, and the ops behind it (every match is within k: n_ops >= 1)
            const size_t used = row[0] == APM_DIST_INVALID ? 1 : std::min<size_t>((size_t)apm_align_words((int)row[0]), stride);
            memcpy(ops + i * stride, row, used * 4);
        }
    }
    *n_found = total;
    return APM_OK;
}

int apm_find_all_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found) {
    return find_all(ctx, text, n, out, capacity, n_found, FIND_PLAIN);
}

int apm_find_all_dist_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found) {
    return find_all(ctx, text, n, out, capacity, n_found, FIND_DIST);
}

int apm_find_all_align_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found,
                              uint32_t *ops, uint32_t stride_words) {
    return find_all(ctx, text, n, out, capacity, n_found, FIND_ALIGN, ops, stride_words);
}

int apm_align_row_words(const apm_ctx *ctx) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->pats.empty()) return fail(const_cast<apm_ctx *>(ctx), APM_ERR_STATE, "apm_set_patterns has not been called");
    return (int)align_row_words(ctx);
}

int apm_align_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                           const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, uint32_t *d_ops, uint32_t stride_words) {
    return record_pass_shard_device(
        ctx, "apm_align_shard_device", d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, !d_ops,
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_ops) & 3u) return fail(ctx, APM_ERR_INVALID, "d_ops must be 4-byte aligned");
            if (stride_words < align_row_words(ctx))
                return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than apm_align_row_words() = %u", stride_words, align_row_words(ctx));
            return (int)APM_OK;
        },
        [&](DeviceState &ds) {
            return align_records(ctx, ds, (const uint8_t *)d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, d_ops, stride_words);
        });
}

int apm_score_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                           apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec) {
    return record_pass_shard_device(
        ctx, "apm_score_shard_device", d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, false, []() { return (int)APM_OK; },
        [&](DeviceState &ds) { return score_records(ctx, ds, (const uint8_t *)d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec); });
}

int apm_find_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                          uint64_t own_begin, uint64_t own_end, apm_match *d_out, uint64_t capacity, uint64_t *d_n_found,
                          uint64_t *d_counts) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_find_shard_device needs a single-device context");
    if (!d_n_found || (!d_out && capacity) || (!d_text && text_len)) return fail(ctx, APM_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(ctx, APM_ERR_INVALID, "d_out must be 16-byte aligned");
    if (text_off + text_len > n_total || own_begin > own_end)
        return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
    begin_call(ctx);
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_start, ds.stream));
        HIP_TRY(ctx, hipEventRecord(ds.ev_kstart, ds.stream));
    }
    ApmPosSink rs{};
    rs.out = reinterpret_cast<unsigned long long *>(d_out);
    rs.count = reinterpret_cast<unsigned long long *>(d_n_found);
    rs.cap = capacity;
    // without d_counts the kernels add into the context's own count vector (what apm_count_buffer zeroes per call)
    const int rc = scan_shard(ctx, ds, (const uint8_t *)d_text, text_off, text_len, n_total, own_begin, own_end,
                              d_counts ? (unsigned long long *)d_counts : ds.d_counts, &rs);
    if (rc) return rc;
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_stop, ds.stream));
        ds.events_recorded = true;
    }
    account(ctx, n_total, own_begin, own_end);
    return APM_OK;
}

int apm_set_text_mode(apm_ctx *ctx, unsigned flags) {
    if (!ctx) return APM_ERR_INVALID;
    if (flags & ~(APM_TEXT_FASTA | APM_TEXT_UPPER)) return fail(ctx, APM_ERR_INVALID, "unknown text mode flags 0x%x", flags);
    if (flags && ctx->devs.size() != 1)
        return fail(ctx, APM_ERR_UNSUPPORTED, "text modes need a single-device context: the shards of a multi-device one depend on the normalised length");
    ctx->text_mode = flags;
    return APM_OK;
}

int apm_normalize_device(apm_ctx *ctx, const void *d_src, uint64_t src_len, unsigned flags, void *d_dst, uint64_t dst_capacity,
                         uint64_t *out_len) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_normalize_device needs a single-device context");
    if (!flags || (flags & ~(APM_TEXT_FASTA | APM_TEXT_UPPER))) return fail(ctx, APM_ERR_INVALID, "text mode flags 0x%x: need APM_TEXT_FASTA and / or APM_TEXT_UPPER", flags);
    if (!out_len || (!d_src && src_len) || (!d_dst && dst_capacity)) return fail(ctx, APM_ERR_INVALID, "NULL pointer");
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    return normalize_on_stream(ctx, ds, (const uint8_t *)d_src, src_len, flags, (uint8_t *)d_dst, dst_capacity, out_len);
}

int apm_map_positions_device(apm_ctx *ctx, apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_map_positions_device needs a single-device context");
    if (!d_n_rec || (!d_rec && capacity)) return fail(ctx, APM_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_rec) & 15u) return fail(ctx, APM_ERR_INVALID, "d_rec must be 16-byte aligned");
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    return map_positions_on_stream(ctx, ds, d_rec, capacity, d_n_rec);
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

int apm_count_synthetic(apm_ctx *ctx, uint64_t n, uint64_t seed, uint64_t *counts) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->text_mode) return fail(ctx, APM_ERR_UNSUPPORTED, "apm_count_synthetic does not serve a text mode (apm_set_text_mode)");
    if (pattern_sharded(ctx)) return for_children(ctx, counts, [&](apm_ctx *ch, uint64_t *c) { return apm_count_synthetic(ch, n, seed, c); });
    return count_sharded(ctx, n, counts, [&](int, DeviceState &ds, uint64_t lo, uint64_t len) -> int {
        HIP_TRY(ctx, apm_launch_synth(ds.d_text, lo, len, seed, ds.stream));
        return APM_OK;
    });
}

int apm_get_timing(const apm_ctx *cctx, apm_timing *out) {
    apm_ctx *ctx = const_cast<apm_ctx *>(cctx);
    if (!ctx || !out) return APM_ERR_INVALID;
    if (pattern_sharded(ctx)) { *out = ctx->timing; return APM_OK; } // (aggregated by the call itself)
    const int rc = collect_event_times(ctx);
    if (rc) return rc;
    *out = ctx->timing;
    return APM_OK;
}

int apm_get_launch_times(const apm_ctx *cctx, int max, double *ms, const char **labels) {
    apm_ctx *ctx = const_cast<apm_ctx *>(cctx);
    if (!ctx || max < 0 || (max > 0 && !ms)) return APM_ERR_INVALID;
    if (ctx->devs.empty()) return 0;
    DeviceState &ds = ctx->devs[0];
    if (!ds.events_recorded || ds.n_stamps == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    HIP_TRY(ctx, hipEventSynchronize(ds.ev_launch[ds.n_stamps - 1]));
    const int n = std::min(max, ds.n_stamps);
    for (int i = 0; i < n; ++i) {
        float t = 0;
        if (hipEventElapsedTime(&t, i ? ds.ev_launch[i - 1] : ds.ev_mstart, ds.ev_launch[i]) != hipSuccess) t = 0;
        ms[i] = t;
        if (labels) labels[i] = ds.launch_label[i];
    }
    return n;
}

int apm_get_stat(const apm_ctx *cctx, const char *name, double *value) {
    apm_ctx *ctx = const_cast<apm_ctx *>(cctx);
    if (!ctx || !name || !value || ctx->devs.empty()) return APM_ERR_INVALID;
    DeviceState &ds = ctx->devs[0];
    const std::string n = name;
    const SievePlan &S = ctx->plan.sieve;
    // launch geometry of the first verify group as this device answered it (none uploaded: as before the first call)
    static const DevVerify no_verify;
    const DevVerify &G0 = ds.verify.empty() ? no_verify : ds.verify[0];
    if (n == "sieve_on") { *value = S.on ? 1 : 0; return APM_OK; }
    if (n == "sieve_rate") { *value = S.rate; return APM_OK; }
    if (n == "sieve_fused") { *value = ds.last_fused ? 1 : 0; return APM_OK; }
    if (n == "sieve_cf") { *value = (S.on && S.per_launch_sieve && G0.cf_threads >= 64) ? (double)G0.cf_threads : 0.0; return APM_OK; } // (after a call: workgroup size of the code-filter form, 0 = plain sieve)
    if (n == "sieve_weak_frac") { *value = S.weak_frac; return APM_OK; }
    if (n == "sieve_cf_dp_slots") { *value = S.per_launch_sieve ? (double)S.launches[0].cf_dp_slots : 0.0; return APM_OK; } // (units with the window DP on codes, first launch)
    if (n == "sieve_cf_waves_per_cu") { *value = (S.per_launch_sieve && G0.cf_threads >= 64) ? (double)(G0.cf_threads / 64 * G0.cf_blocks_per_cu) : 0.0; return APM_OK; }
    if (n == "sieve_cf_bytes") { *value = S.per_launch_sieve ? (double)S.launches[0].cf_image.size() : 0.0; return APM_OK; }
    if (n == "sieve_stride") { *value = S.on ? (double)S.stride : 0.0; return APM_OK; }
    if (n == "sieve_clist") { *value = ds.last_clist_regions ? 1.0 : 0.0; return APM_OK; }
    if (n == "sieve_waves") { *value = (double)ds.last_sieve_waves; return APM_OK; } // (as launched: wave w scans blocks w, w + sieve_waves, ...)
    if (n == "sieve_mask_bytes") { // what the last sieve pass handed over: mask rows, or list entries + the rows of the overflow blocks
        *value = (double)ds.last_mask_blocks * 256.0;
        if (ds.last_clist_regions && ds.last_mask_blocks > 0) {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            std::vector<uint32_t> cnt((size_t)ds.last_clist_regions);
            uint32_t listed = 0;
            HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), ds.d_clist_cnt, cnt.size() * 4, hipMemcpyDeviceToHost, ds.stream));
            HIP_TRY(ctx, hipMemcpyAsync(&listed, ds.last_blist_ctr, 4, hipMemcpyDeviceToHost, ds.stream));
            HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
            double entries = 0;
            for (uint32_t c : cnt) entries += (double)c;
            *value = 4.0 * entries + 256.0 * (double)listed;
        }
        return APM_OK;
    }
    if (n == "verify_launches") { *value = (double)S.launches.size(); return APM_OK; }
    if (n == "verify_image_bytes") { *value = S.launches.empty() ? 0.0 : (double)S.launches[0].image.size(); return APM_OK; }
    if (n == "verify_blocks_per_cu") { // (of the form the last call ran)
        *value = S.launches.empty() ? 0.0 : (double)(ds.last_fused ? G0.fused_blocks_per_cu : G0.blocks_per_cu);
        return APM_OK;
    }
    if (n == "verify_threads") {
        *value = S.launches.empty() ? 0.0 : (double)(ds.last_fused ? G0.fused_threads : G0.threads);
        return APM_OK;
    }
    if (n == "sieve_candidates") return sieve_candidates(ctx, ds, value);
    if (n == "align_rows") { *value = (double)ds.last_align_rows; return APM_OK; } // (trace rows of the last align launch; 0: none since the patterns were set)
    if (n == "norm_src_bytes") { *value = (double)ds.tn_src_bytes; return APM_OK; }
    if (n == "norm_kept_bytes") { *value = (double)ds.tn_kept_bytes; return APM_OK; }
    if (n == "norm_ms" || n == "map_ms") { // (HIP events around the pass's three launches / the map launch; 0: not timed)
        const int at = n == "norm_ms" ? 0 : 2;
        *value = 0.0;
        if (at == 0 ? ds.tn_timed : ds.map_timed) {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            HIP_TRY(ctx, hipEventSynchronize(ds.ev_tn[at + 1]));
            float t = 0;
            HIP_TRY(ctx, hipEventElapsedTime(&t, ds.ev_tn[at], ds.ev_tn[at + 1]));
            *value = t;
        }
        return APM_OK;
    }
#ifdef APM_MEASURE
    if (n.rfind("verify_", 0) == 0 && ds.d_stats) {
        HIP_TRY(ctx, hipSetDevice(ds.dev));
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
        unsigned long long h[8] = {};
        HIP_TRY(ctx, hipMemcpy(h, ds.d_stats, 64, hipMemcpyDeviceToHost));
        if (n == "verify_survivors") { *value = (double)h[1]; return APM_OK; }
        if (n == "verify_dp_items") { *value = (double)h[2]; return APM_OK; }
        if (n == "verify_counted") { *value = (double)h[3]; return APM_OK; }
        if (n.rfind("verify_wave_", 0) == 0) { // per-wave start / end stamps (APM_MEASURE_SKIP bit 9), in us from the first start
            std::vector<unsigned long long> t(2 * APM_STATS_WAVES);
            HIP_TRY(ctx, hipMemcpy(t.data(), ds.d_stats + 8, t.size() * 8, hipMemcpyDeviceToHost));
            std::vector<double> st, en;
            unsigned long long t0 = ~0ull;
            for (size_t w = 0; w < APM_STATS_WAVES; ++w) if (t[2 * w + 1]) t0 = std::min(t0, t[2 * w]);
            for (size_t w = 0; w < APM_STATS_WAVES; ++w) if (t[2 * w + 1]) { st.push_back((double)(t[2 * w] - t0) * 0.01); en.push_back((double)(t[2 * w + 1] - t0) * 0.01); }
            if (n.rfind("verify_wave_grp", 0) == 0 || n.rfind("verify_wave_xcd", 0) == 0) { // verify_wave_grpmax<g> / grpmin<g> / xcdavg<x>: end stamps by group / by blockIdx % 8
                const bool by_xcd = n[12] == 'x';
                const int want = atoi(n.c_str() + 18);
                double lo = 1e30, hi = 0, sum = 0; long cnt = 0;
                for (size_t w = 0; w < APM_STATS_WAVES; ++w) {
                    if (!t[2 * w + 1]) continue;
                    const int key = by_xcd ? (int)((w / 4) % 8) : (int)((w ^ (w >> 5)) % APM_WORK_GROUPS);
                    if (key != want) continue;
                    const double e = (double)(t[2 * w + 1] - t0) * 0.01;
                    lo = std::min(lo, e); hi = std::max(hi, e); sum += e; ++cnt;
                }
                *value = n[15] == 'm' && n[16] == 'a' ? hi : (n[15] == 'm' && n[16] == 'i' ? lo : (cnt ? sum / cnt : 0));
                return APM_OK;
            }
            if (n.rfind("verify_wave_slow", 0) == 0) { // verify_wave_slow<i>: the wave with the i-th latest end stamp; verify_wave_slowend<i>: that stamp
                const bool end = n.rfind("verify_wave_slowend", 0) == 0;
                const size_t want = (size_t)atoi(n.c_str() + (end ? 19 : 16));
                std::vector<std::pair<unsigned long long, size_t>> by_end;
                for (size_t w = 0; w < APM_STATS_WAVES; ++w) if (t[2 * w + 1]) by_end.push_back({t[2 * w + 1], w});
                std::sort(by_end.rbegin(), by_end.rend());
                if (want >= by_end.size()) { *value = -1; return APM_OK; }
                *value = end ? (double)(by_end[want].first - t0) * 0.01 : (double)by_end[want].second;
                return APM_OK;
            }
            if (en.empty()) { *value = 0; return APM_OK; }
            std::sort(st.begin(), st.end());
            std::sort(en.begin(), en.end());
            if (n == "verify_wave_count") { *value = (double)en.size(); return APM_OK; }
            if (n == "verify_wave_start_max") { *value = st.back(); return APM_OK; }
            if (n == "verify_wave_end_min") { *value = en.front(); return APM_OK; }
            if (n == "verify_wave_end_p10") { *value = en[en.size() / 10]; return APM_OK; }
            if (n == "verify_wave_end_p50") { *value = en[en.size() / 2]; return APM_OK; }
            if (n == "verify_wave_end_p90") { *value = en[en.size() * 9 / 10]; return APM_OK; }
            if (n == "verify_wave_end_max") { *value = en.back(); return APM_OK; }
        }
    }
#endif
    return fail(ctx, APM_ERR_INVALID, "unknown statistic '%s'", name);
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