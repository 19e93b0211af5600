/*
 * apm_ingest.hip -- the host-level count calls (apm_count_buffer, apm_count_file, apm_count_synthetic) and what they are
 * made of: owner-computes text sharding with an (m_max-1)-byte halo, truncation only at the end of the WHOLE text
 * (SURVEY 8e), staging through the pinned ring, the text modes' normalisation pass (apm_textnorm.hip) with the sequence index and the
 * locate pass behind it (apm_seqindex.hip), and the counts
 * summed with one RCCL all-reduce (one-process-per-GPU mode sums with the caller's collective instead:
 * apm_count_shard_device + torch.distributed).
 *
 * There is no CPU fallback in this file by design.
 */
#include "apm_runtime.h"
#include "apm_core.h"
#include "apm_textnorm.h"
#include "apm_seqindex.h"

#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

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

// the record buffers of a find request on one device: its two counters, zeroed on ds.stream, its records and, where the
// request needs them, the second record buffer and the rows of ops -- each kept while it is large enough
int prepare_records(apm_ctx *ctx, DeviceState &ds, const FindRequest &f) {
    const size_t recs = (size_t)std::max<uint64_t>(f.cap, 1);
    if (!ds.d_rec_n) HIP_TRY(ctx, hipMalloc((void **)&ds.d_rec_n, 16));
    int rc = grow_device_buffer(ctx, ds, (void **)&ds.d_rec, &ds.rec_cap, recs, 16, APM_ERR_NOMEM, "the record buffer (%llu records)",
                                (unsigned long long)f.cap);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ds.d_rec_n, 0, 16, ds.stream));
    if (f.second_buffer())
        rc = grow_device_buffer(ctx, ds, (void **)&ds.d_rec2, &ds.rec2_cap, recs, 16, APM_ERR_NOMEM, "the best-hit buffer (%llu records)",
                                (unsigned long long)f.cap);
    if (rc) return rc;
    if (f.rows != FindRequest::NO_ROWS)
        rc = grow_device_buffer(ctx, ds, (void **)&ds.d_ops, &ds.ops_cap, recs * f.row_stride, 4, APM_ERR_NOMEM,
                                "the rows of ops (%llu records of %u dwords)", (unsigned long long)f.cap, f.row_stride);
    if (!rc && f.seq_ids)
        rc = grow_device_buffer(ctx, ds, (void **)&ds.d_seqocc_seq, &ds.seqocc_seq_cap, recs, 4, APM_ERR_NOMEM,
                                "the records' sequences (%llu records)", (unsigned long long)f.cap);
    if (rc || f.counted()) return rc;
    // one key per pattern -- NEAREST_SEQ: per (sequence, pattern) pair --, all NONE; the finishing pass leaves a record per key:
    // the count is known in advance
    const bool per_seq = f.scan == FindRequest::NEAREST_SEQ;
    rc = per_seq ? grow_device_buffer(ctx, ds, (void **)&ds.d_seqnear_keys, &ds.seqnear_keys_cap, recs, 8, APM_ERR_NOMEM,
                                      "the per-sequence nearest keys (%llu pairs)", (unsigned long long)f.cap)
                 : grow_device_buffer(ctx, ds, (void **)&ds.d_nearest_keys, &ds.nearest_keys_cap, recs, 8, APM_ERR_NOMEM, "the nearest keys (%llu patterns)",
                                      (unsigned long long)f.cap);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(per_seq ? ds.d_seqnear_keys : ds.d_nearest_keys, 0xff, recs * 8, ds.stream));
    HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ds.d_rec_n, (int)f.cap, 1, ds.stream));
    if (f.cap >> 32) // (pairs beyond 2^32: the counter's upper half, zeroed above)
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)((uint32_t *)ds.d_rec_n + 1), (int)(uint32_t)(f.cap >> 32), 1, ds.stream));
    return APM_OK;
}

// the host-level entry points share this: `stage(g, ds, lo, len)` must enqueue the
// bytes of global positions [lo, lo+len) into ds.d_text on ds.stream.
// Staging runs CONCURRENTLY, one host thread per device (the replacement of the reference's per-rank reads,
// /root/reference/src/database_over_ranks.c:141-166: there every MPI rank read its own piece at the same time; round 2
// staged device g's whole shard before touching device g + 1).  The scan launches follow from the calling thread as
// each device's staging thread returns: they are microseconds of host time.
// find != NULL (the find calls): the request (apm_runtime.h) is run as scan -> the passes it names, on every device's stream
template <typename Stage>
int count_sharded(apm_ctx *ctx, uint64_t n, uint64_t *counts, Stage stage, const FindRequest *find = nullptr) {
    const FindRequest f = find ? *find : FindRequest{}; // (count only: a window scan, no sink, no pass)
    const bool occ = f.scan == FindRequest::OCCURRENCES, per_seq = f.scan == FindRequest::NEAREST_SEQ, nearest = f.scan == FindRequest::NEAREST || per_seq;
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
    const uint64_t halo = f.whole_text() ? n : (uint64_t)(f.score ? longest_pattern(ctx) : std::max(ctx->plan.m_max, 1)) - 1;
    struct Shard { uint64_t ob = 0, oe = 0; ShardText text{}; int rc = APM_OK; };
    std::vector<Shard> sh((size_t)G);
    auto stage_device = [&](int g) {
        DeviceState &ds = ctx->devs[g];
        Shard &S = sh[(size_t)g];
        apm_shard_range(n, ctx->k, g, G, &S.ob, &S.oe);
        if (occ || nearest) S.ob = 0, S.oe = n; // (every byte of the text is an end)
        const uint64_t hi = std::min<uint64_t>(n, S.oe + halo);
        S.text = ShardText{nullptr, S.ob, hi > S.ob ? hi - S.ob : 0, n};
        S.rc = [&]() -> int {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            HIP_TRY(ctx, hipEventRecord(ds.ev_start, ds.stream));
            HIP_TRY(ctx, hipMemsetAsync(ds.d_counts, 0, std::max<size_t>((size_t)P * 8, 16), ds.stream));
            int rc = find ? prepare_records(ctx, ds, *find) : APM_OK;
            if (rc) return rc;
            if (S.oe > S.ob) {
                rc = ensure_text(ctx, ds, (size_t)S.text.text_len + 16);
                if (rc) return rc;
                S.text.text = ds.d_text;
                rc = stage(g, ds, S.text.text_off, S.text.text_len);
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
            if (nearest) { // (an empty text too: every pattern gets its "none" records)
                apm_match *rec = reinterpret_cast<apm_match *>(ds.d_rec), *rec2 = reinterpret_cast<apm_match *>(ds.d_rec2);
                int rc = per_seq ? seqnear_scan(ctx, ds, S.text, S.ob, S.oe, ds.d_seq_table, ds.seq_table_n, ds.d_seqnear_keys)
                                 : nearest_scan(ctx, ds, S.text, S.ob, S.oe, ds.d_nearest_keys);
                if (!rc)
                    rc = per_seq ? seqnear_records(ctx, ds, S.text, ds.d_seq_table, ds.seq_table_n, ds.d_seqnear_keys, rec, f.spans ? rec2 : nullptr)
                                 : nearest_records(ctx, ds, S.text, ds.d_nearest_keys, rec, f.spans ? rec2 : nullptr);
                if (rc) return rc;
            } else if (S.oe > S.ob) {
                apm_match *rec = reinterpret_cast<apm_match *>(ds.d_rec), *rec2 = reinterpret_cast<apm_match *>(ds.d_rec2);
                uint64_t *n_rec = reinterpret_cast<uint64_t *>(ds.d_rec_n), *n_rec2 = n_rec + 1;
                const ApmPosSink sink{ds.d_rec, ds.d_rec_n, f.cap, 0};
                // the scan; then the passes over its records; then the rows: of the records, of the best hits alone, or of the (end, span) pairs
                int rc = occ && f.per_seq ? seqocc_scan(ctx, ds, S.text, S.ob, S.oe, ds.d_seq_table, ds.seq_table_n, f.occ_flags, rec, f.cap, n_rec, ds.d_counts)
                         : occ ? occ_scan(ctx, ds, S.text, S.ob, S.oe, f.occ_flags, rec, f.cap, n_rec, ds.d_counts)
                             : scan_shard(ctx, ds, S.text, S.ob, S.oe, ds.d_counts, find ? &sink : nullptr);
                if (!rc && f.score) rc = score_records(ctx, ds, S.text, rec, f.cap, n_rec);
                if (!rc && f.best) rc = best_records(ctx, ds, S.text, rec, f.cap, n_rec, f.radius, rec2, f.cap, n_rec2);
                if (!rc && f.spans)
                    rc = f.per_seq ? seqocc_span_records(ctx, ds, S.text, ds.d_seq_table, ds.seq_table_n, rec, f.cap, n_rec, rec2, f.seq_ids ? ds.d_seqocc_seq : nullptr)
                                   : span_records(ctx, ds, S.text, rec, f.cap, n_rec, rec2);
                if (!rc && f.rows == FindRequest::WINDOW_ROWS)
                    rc = f.best ? align_records(ctx, ds, S.text, rec2, f.cap, n_rec2, ds.d_ops, f.row_stride)
                                : align_records(ctx, ds, S.text, rec, f.cap, n_rec, ds.d_ops, f.row_stride);
                if (!rc && f.rows == FindRequest::OCC_ROWS) rc = occ_align_records(ctx, ds, S.text, rec, rec2, f.cap, n_rec, ds.d_ops, f.row_stride);
                if (rc) return rc;
                // (cells and windows are the window scan's: the occurrence scan leaves them 0, as include/apm.h says)
                if (!occ) account(ctx, n, S.ob, S.oe);
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
    const size_t cap = (size_t)((n_blocks + 4095) & ~(uint64_t)4095); // (the scan reads the summaries in whole chunks)
    size_t have_summary = 0, have_map = 0; // (both too small: tn_cap stays 0 until both stand)
    ds.tn_cap = 0;
    int rc = grow_device_buffer(ctx, ds, (void **)&ds.d_tn_summary, &have_summary, cap, 4, APM_ERR_NOMEM, "the normalisation map (%llu blocks)",
                                (unsigned long long)n_blocks);
    if (!rc) rc = grow_device_buffer(ctx, ds, (void **)&ds.d_tn_map, &have_map, cap + 1, 8, APM_ERR_NOMEM, "the normalisation map (%llu blocks)",
                                     (unsigned long long)n_blocks);
    if (!rc) ds.tn_cap = cap;
    return rc;
}

// apm_normalize_device on ds.stream: summary and scan, ONE synchronisation for the total, the scatter
int normalize_on_stream(apm_ctx *ctx, DeviceState &ds, const uint8_t *d_src, uint64_t src_len, unsigned flags, uint8_t *d_dst,
                        uint64_t dst_capacity, uint64_t *out_len) {
    ds.tn_valid = ds.tn_timed = false;
    ds.tn_host = false; // (the context's own sequence table goes with the text it was made from)
    ds.seq_table_n = 0;
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

// ---- the sequence index (apm_seqindex.hip) ----
// the index pass's counts and prefixes for a source of n_blocks blocks: grown on demand and kept, like the map
int ensure_sq_scratch(apm_ctx *ctx, DeviceState &ds, uint64_t n_blocks) {
    if (n_blocks <= ds.sq_cap) return APM_OK;
    const size_t cap = (size_t)((n_blocks + APM_SQ_SCAN_CHUNK - 1) & ~(uint64_t)(APM_SQ_SCAN_CHUNK - 1)); // (the scan reads the counts in whole chunks)
    size_t have_count = 0, have_prefix = 0; // (both too small: sq_cap stays 0 until both stand)
    ds.sq_cap = 0;
    int rc = grow_device_buffer(ctx, ds, (void **)&ds.d_sq_count, &have_count, cap, 4, APM_ERR_NOMEM, "the sequence index's counts (%llu blocks)",
                                (unsigned long long)n_blocks);
    if (!rc) rc = grow_device_buffer(ctx, ds, (void **)&ds.d_sq_prefix, &have_prefix, cap + 1, 8, APM_ERR_NOMEM, "the sequence index's counts (%llu blocks)",
                                     (unsigned long long)n_blocks);
    if (!rc) ds.sq_cap = cap;
    return rc;
}

// apm_index_sequences_device on ds.stream: count and scan, ONE synchronisation for the total, the emit into the table that
// `table_for(entries, &d_table)` hands out for n_seq + 1 entries (not 0: nothing is emitted).  *n_seq is set before it is asked.
template <class TableFor>
int index_sequences_on_stream(apm_ctx *ctx, DeviceState &ds, uint64_t *n_seq, TableFor table_for) {
    if (!ds.tn_valid) return fail(ctx, APM_ERR_STATE, "no text has been normalised on this context");
    ds.sq_timed = false;
    ApmSqIndexArgs a{};
    a.src = ds.tn_src;
    a.map = ds.d_tn_map;
    a.src_len = ds.tn_src_bytes;
    a.kept = ds.tn_kept_bytes;
    for (int i = 0; i < 2 && ctx->timing_on; ++i) { const int rc = ensure_tn_event(ctx, ds.ev_sq[i]); if (rc) return rc; }
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_sq[0], ds.stream));
    unsigned long long opens = 0;
    if (a.src.n_blocks) {
        if (!ds.d_sq_total) HIP_TRY(ctx, hipMalloc((void **)&ds.d_sq_total, 16));
        const int rc = ensure_sq_scratch(ctx, ds, a.src.n_blocks);
        if (rc) return rc;
        a.count = ds.d_sq_count;
        a.prefix = ds.d_sq_prefix;
        a.total = ds.d_sq_total;
        HIP_TRY(ctx, apm_launch_sq_count(a, ds.n_cu, ds.stream));
        HIP_TRY(ctx, apm_launch_sq_scan(a, ds.stream));
        HIP_TRY(ctx, hipMemcpyAsync(&opens, ds.d_sq_total, 8, hipMemcpyDeviceToHost, ds.stream));
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    }
    *n_seq = ds.sq_n_seq = 1 + opens;
    a.n_seq = *n_seq;
    const int rc = table_for(a.n_seq + 1, &a.table);
    if (rc) return rc;
    HIP_TRY(ctx, apm_launch_sq_emit(a, ds.n_cu, ds.stream));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_sq[1], ds.stream));
        ds.sq_timed = true;
    }
    return APM_OK;
}

// apm_locate_records_device on ds.stream, behind whatever filled the records
int locate_on_stream(apm_ctx *ctx, DeviceState &ds, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, const apm_seq *d_table,
                     uint64_t n_seq, apm_loc *d_loc) {
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!ds.tn_valid) return fail(ctx, APM_ERR_STATE, "no text has been normalised on this context");
    ds.locate_timed = false;
    if (!capacity) return APM_OK;
    int rc = ensure_score_image(ctx, ds); // (the pattern lengths: the record passes' {row, m} table)
    if (rc) return rc;
    ApmSqLocateArgs a{};
    a.src = ds.tn_src;
    a.map = ds.d_tn_map;
    a.rec = reinterpret_cast<const uint4 *>(d_rec);
    a.cap = capacity;
    a.n_rec = reinterpret_cast<const unsigned long long *>(d_n_rec);
    a.table = d_table;
    a.n_seq = n_seq;
    a.pat = ds.d_score_tab;
    a.n_patterns = (uint32_t)ctx->pats.size();
    a.src_len = ds.tn_src_bytes;
    a.kept = ds.tn_kept_bytes;
    a.loc = d_loc;
    if (ctx->timing_on) {
        for (int i = 2; i < 4; ++i) { rc = ensure_tn_event(ctx, ds.ev_sq[i]); if (rc) return rc; }
        HIP_TRY(ctx, hipEventRecord(ds.ev_sq[2], ds.stream));
    }
    HIP_TRY(ctx, apm_launch_sq_locate(a, ds.n_cu, ds.stream));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_sq[3], ds.stream));
        ds.locate_timed = true;
    }
    return APM_OK;
}

// apm_locate_buffer, apm_get_sequences: the single device of a context whose last host-level call ran in a text mode, with
// the context's own table of that text built (once per normalisation)
int host_sequence_table(apm_ctx *ctx, const char *name, DeviceState **out) {
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_UNSUPPORTED, "%s needs a single-device context: text modes are single-device", name);
    DeviceState &ds = ctx->devs[0];
    if (!ds.tn_valid || !ds.tn_host) return fail(ctx, APM_ERR_STATE, "%s: no text normalised by a host-level call in a text mode is resident", name);
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    *out = &ds;
    if (ds.seq_table_n) return APM_OK;
    uint64_t n_seq = 0;
    const int rc = index_sequences_on_stream(ctx, ds, &n_seq, [&](uint64_t entries, apm_seq **d_table) {
        const int grc = grow_device_buffer(ctx, ds, (void **)&ds.d_seq_table, &ds.seq_table_cap, (size_t)entries, sizeof(apm_seq), APM_ERR_NOMEM,
                                           "the sequence table (%llu entries)", (unsigned long long)entries);
        *d_table = ds.d_seq_table;
        return grc;
    });
    if (!rc) ds.seq_table_n = n_seq;
    return rc;
}

// A text mode's ingest on the (single) device: `stage_into(0, ds, d_raw, 0, n)` enqueues the n source bytes into the raw
// buffer, the pass normalises them into ds.d_text -- sized for the raw length first, so that count_sharded finds it large
// enough and leaves it alone -- and *n_text is the length count_sharded then scans, with a stage step that has nothing to copy.
template <typename StageInto>
int stage_normalized(apm_ctx *ctx, uint64_t n, StageInto stage_into, uint64_t *n_text) {
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    const size_t want = ((size_t)n + 16 + 255) & ~(size_t)255;
    if (want > ds.raw_cap) ds.tn_valid = false; // (the map of an earlier pass goes with the bytes it was made from)
    int rc = grow_device_buffer(ctx, ds, (void **)&ds.d_raw, &ds.raw_cap, want, 1, APM_ERR_NOMEM, "the raw text buffer (%zu bytes)", want);
    if (!rc) rc = ensure_text(ctx, ds, (size_t)n + 16);
    if (!rc && n) rc = stage_into(0, ds, ds.d_raw, 0, n);
    if (rc) return rc;
    rc = normalize_on_stream(ctx, ds, ds.d_raw, n, ctx->text_mode, ds.d_text, n, n_text);
    ds.tn_host = !rc; // (apm_locate_buffer, apm_get_sequences: the source is the context's own raw buffer)
    return rc;
}

// count_sharded's stage step behind stage_normalized
int stage_nothing(int, DeviceState &, uint64_t, uint64_t) { return APM_OK; }

// The host-level ingest of an n-byte source, written once for apm_count_buffer and apm_count_file:
// `stage_into(g, ds, d_dst, lo, len)` enqueues the source bytes [lo, lo + len) into d_dst on device g.  Verbatim: shard by
// shard into ds.d_text.  In a text mode (single device: apm_set_text_mode): the whole source into the raw buffer, the
// pass, the scan of what it kept.
template <typename StageInto>
int count_staged(apm_ctx *ctx, uint64_t n, uint64_t *counts, StageInto stage_into, const FindRequest *find) {
    ctx->devs[0].tn_host = false; // (a new host-level scan: apm_locate_buffer serves the last one in a text mode only)
    if (!ctx->text_mode)
        return count_sharded(ctx, n, counts, [&](int g, DeviceState &ds, uint64_t lo, uint64_t len) { return stage_into(g, ds, ds.d_text, lo, len); }, find);
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!counts) return fail(ctx, APM_ERR_INVALID, "counts is NULL");
    const auto t0 = clk::now();
    uint64_t n_text = 0;
    int rc = stage_normalized(ctx, n, stage_into, &n_text);
    FindRequest sized; // (NEAREST_SEQ: the request with its cap, once the sequences are counted)
    if (!rc && find && find->scan == FindRequest::NEAREST_SEQ) {
        // the context's own sequence table of this text: apm_locate_buffer and apm_get_sequences find it built
        DeviceState *dsp = nullptr;
        rc = host_sequence_table(ctx, "apm_find_nearest_seq_buffer", &dsp);
        if (rc) return rc;
        *find->n_seq = dsp->seq_table_n;
        if (dsp->seq_table_n > find->cap_seq)
            return fail(ctx, APM_ERR_INVALID, "the text has %llu sequences, the arrays hold %llu", (unsigned long long)dsp->seq_table_n,
                        (unsigned long long)find->cap_seq);
        if (dsp->seq_table_n >= (1ull << 32)) return fail(ctx, APM_ERR_UNSUPPORTED, "apm_find_nearest_seq_buffer serves fewer than 2^32 sequences");
        sized = *find;
        sized.cap = dsp->seq_table_n * (uint64_t)ctx->pats.size();
        find = &sized;
    }
    if (!rc && find && find->per_seq) {
        // the same table under the occurrence scan: it cuts the normalised text, so an empty text has no scan to read it
        DeviceState *dsp = nullptr;
        rc = host_sequence_table(ctx, "apm_find_occ_seq_buffer", &dsp);
        if (rc) return rc;
        if (dsp->seq_table_n >= (1ull << 32)) return fail(ctx, APM_ERR_UNSUPPORTED, "apm_find_occ_seq_buffer serves fewer than 2^32 sequences");
    }
    if (!rc) rc = count_sharded(ctx, n_text, counts, stage_nothing, find);
    if (!rc) ctx->timing.total_ms = ms_since(t0);
    return rc;
}

} // namespace

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

int count_host_text(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t *counts, const FindRequest *find) {
    const int G = (int)ctx->devs.size();
    // the bytes [lo, lo + len) of the host text -> d_dst on device g
    return count_staged(ctx, n, counts, [&](int g, DeviceState &ds, uint8_t *d_dst, uint64_t lo, uint64_t len) -> int {
        if (len < (1u << 20)) { // small: one pageable copy (the runtime stages it itself)
            HIP_TRY(ctx, hipMemcpyAsync(d_dst, text + lo, (size_t)len, hipMemcpyHostToDevice, ds.stream));
            return APM_OK;
        }
        // through the pinned ring: round 2 pinned the caller's whole buffer with hipHostRegister on every call
        return stage_through_ring(ctx, g, G, ds, d_dst, lo, len, [&](uint64_t off, uint8_t *dst, size_t want) {
            memcpy(dst, text + off, want);
            return true;
        });
    }, find);
}

extern "C" {

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
    const int rc = count_staged(ctx, n, counts, [&](int g, DeviceState &ds, uint8_t *d_dst, uint64_t lo, uint64_t len) -> int {
        return stage_through_ring(ctx, g, G, ds, d_dst, lo, len, [&](uint64_t off, uint8_t *dst, size_t want) {
            size_t got = 0;
            while (got < want) {
                const ssize_t r = pread(fd, dst + got, want - got, (off_t)(off + got));
                if (r <= 0) return false;
                got += (size_t)r;
            }
            return true;
        });
    }, nullptr);
    close(fd);
    return rc;
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

int apm_index_sequences_device(apm_ctx *ctx, apm_seq *d_table, uint64_t capacity, uint64_t *n_seq) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_index_sequences_device needs a single-device context");
    if (!n_seq || (!d_table && capacity)) return fail(ctx, APM_ERR_INVALID, "NULL pointer");
    if (reinterpret_cast<uintptr_t>(d_table) & 7u) return fail(ctx, APM_ERR_INVALID, "d_table must be 8-byte aligned");
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    return index_sequences_on_stream(ctx, ds, n_seq, [&](uint64_t entries, apm_seq **out) {
        if (entries > capacity)
            return fail(ctx, APM_ERR_INVALID, "the sequence table has %llu entries, d_table holds %llu", (unsigned long long)entries, (unsigned long long)capacity);
        *out = d_table;
        return (int)APM_OK;
    });
}

int apm_locate_records_device(apm_ctx *ctx, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, const apm_seq *d_table,
                              uint64_t n_seq, apm_loc *d_loc) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "apm_locate_records_device needs a single-device context");
    if (!d_n_rec || !d_table || !n_seq || ((!d_rec || !d_loc) && capacity)) return fail(ctx, APM_ERR_INVALID, "NULL device pointer or an empty table");
    if ((reinterpret_cast<uintptr_t>(d_rec) | reinterpret_cast<uintptr_t>(d_loc)) & 15u) return fail(ctx, APM_ERR_INVALID, "d_rec and d_loc must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_table) & 7u) return fail(ctx, APM_ERR_INVALID, "d_table must be 8-byte aligned");
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    return locate_on_stream(ctx, ds, d_rec, capacity, d_n_rec, d_table, n_seq, d_loc);
}

int apm_locate_buffer(apm_ctx *ctx, const apm_match *rec, uint64_t n, apm_loc *loc) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_UNSUPPORTED, "apm_locate_buffer needs a single-device context: text modes are single-device");
    if (!n) return APM_OK;
    if (!rec || !loc) return fail(ctx, APM_ERR_INVALID, "NULL pointer");
    DeviceState *dsp = nullptr;
    int rc = host_sequence_table(ctx, "apm_locate_buffer", &dsp);
    if (rc) return rc;
    DeviceState &ds = *dsp;
    // one buffer of 16-byte units: the counter, the records, the locations
    rc = grow_device_buffer(ctx, ds, (void **)&ds.d_loc_buf, &ds.loc_buf_cap, (size_t)(1 + 2 * n), 16, APM_ERR_NOMEM, "the locate buffer (%llu records)",
                            (unsigned long long)n);
    if (rc) return rc;
    const unsigned long long counter[2] = {n, 0};
    uint8_t *d_n = ds.d_loc_buf, *d_rec = d_n + 16, *d_loc = d_rec + 16 * n;
    HIP_TRY(ctx, hipMemcpyAsync(d_n, counter, 16, hipMemcpyHostToDevice, ds.stream));
    HIP_TRY(ctx, hipMemcpyAsync(d_rec, rec, (size_t)n * 16, hipMemcpyHostToDevice, ds.stream));
    const bool timing_saved = ctx->timing_on;
    ctx->timing_on = true; // (the call synchronises anyway; keep its event times)
    rc = locate_on_stream(ctx, ds, reinterpret_cast<const apm_match *>(d_rec), n, reinterpret_cast<const uint64_t *>(d_n), ds.d_seq_table, ds.seq_table_n,
                          reinterpret_cast<apm_loc *>(d_loc));
    ctx->timing_on = timing_saved;
    if (rc) {
        hipStreamSynchronize(ds.stream); // (the copies above read the caller's memory)
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(loc, d_loc, (size_t)n * 16, hipMemcpyDeviceToHost, ds.stream));
    HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    return APM_OK;
}

int apm_get_sequences(apm_ctx *ctx, apm_seq *out, uint64_t capacity, uint64_t *n_seq) {
    if (!ctx) return APM_ERR_INVALID;
    if (!n_seq || (!out && capacity)) return fail(ctx, APM_ERR_INVALID, "NULL pointer");
    DeviceState *dsp = nullptr;
    const int rc = host_sequence_table(ctx, "apm_get_sequences", &dsp);
    if (rc) return rc;
    *n_seq = dsp->seq_table_n;
    const uint64_t take = std::min<uint64_t>(capacity, dsp->seq_table_n + 1);
    if (take) HIP_TRY(ctx, hipMemcpyAsync(out, dsp->d_seq_table, (size_t)take * sizeof(apm_seq), hipMemcpyDeviceToHost, dsp->stream));
    HIP_TRY(ctx, hipStreamSynchronize(dsp->stream));
    return APM_OK;
}

} // extern "C"
