/*
 * apm_runtime.h -- what the runtime units call of one another (apm_runtime.hip, apm_ingest.hip, apm_find.hip,
 * apm_records.hip, apm_stats.hip), each function declared once and named with the unit that defines it, and the frame every device-level
 * shard call runs in.  Not part of the ABI, and not exported by the library.
 */
#ifndef APM_RUNTIME_H
#define APM_RUNTIME_H

#include "apm_state.h"

#include <algorithm>
#include <chrono>
#include <functional>

#pragma GCC visibility push(hidden)

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

inline bool pattern_sharded(const apm_ctx *ctx) { return ctx->partition == APM_PARTITION_PATTERNS && ctx->devs.size() > 1; }

// the longest pattern of the set, those with k >= m included (the plan's m_max leaves them out: the scan needs no text for
// them, the scoring pass does)
inline int longest_pattern(const apm_ctx *ctx) {
    int m = 1;
    for (const auto &p : ctx->pats) m = std::max(m, p.m);
    return m;
}

// v on the device at *dptr (allocates; an empty vector gets 16 bytes), copied synchronously
template <typename T>
int upload_vec(apm_ctx *ctx, T **dptr, const std::vector<T> &v) {
    *dptr = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIP_TRY(ctx, hipMalloc((void **)dptr, bytes));
    if (!v.empty()) HIP_TRY(ctx, hipMemcpy(*dptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return APM_OK;
}

// ---- apm_runtime.hip ----
// plan ctx->pats at ctx->k under ctx->kernel (apm_plan.cpp) and hand the plan to every device
int build_plan(apm_ctx *ctx);
// run fn(child, counts of its slice) on every child of a pattern-sharded context at once, one host thread per device
int for_children(apm_ctx *ctx, uint64_t *counts, const std::function<int(apm_ctx *, uint64_t *)> &fn);

// ---- apm_stats.hip ----
// algorithmic / evaluated cells of the window starts [ob, oe) into ctx->timing
void account(apm_ctx *ctx, uint64_t n_total, uint64_t ob, uint64_t oe);
// a call starts: its timing record and every device's per-call accounting are reset
void begin_call(apm_ctx *ctx);
// the event times and per-device sums of the last call into ctx->timing (synchronises with the devices' last events)
int collect_event_times(apm_ctx *ctx);

// ---- what a host-level find call asks (apm_find.hip builds it, count_sharded in apm_ingest.hip runs it) ----
// Beside the counts, every device appends up to `cap` records of its owner range to its own buffer ds.d_rec, counted in
// ds.d_rec_n[0] (global positions: nothing to fix up at the merge); the passes the request names then run behind the scan on
// the device's stream, in the order of the fields.  Each field means one thing, whichever call set it.
struct FindRequest {
    enum Scan { WINDOWS, OCCURRENCES, NEAREST, NEAREST_SEQ };
    enum Rows { NO_ROWS, WINDOW_ROWS, OCC_ROWS };
    uint64_t cap = 0;
    Scan scan = WINDOWS;     // what fills ds.d_rec: the window scan's record sink, or the occurrence scan's ends (it adds into the counts),
                             // or NEAREST: the nearest-occurrence scan into ds.d_nearest_keys and its finishing pass -- one end record
                             // per pattern (cap = n_patterns = the count it leaves in ds.d_rec_n[0]; it adds nothing into the counts),
                             // or NEAREST_SEQ: the per-sequence nearest scan into ds.d_seqnear_keys and its finishing pass -- one end
                             // record per (sequence, pattern) pair of the context's sequence table, which the request builds behind the
                             // normalisation (a text mode only).  The request says how many sequences the caller has room for
                             // (cap_seq); the run sets *n_seq and, if they fit, cap = n_seq * n_patterns before anything is sized
    uint64_t cap_seq = 0;    // NEAREST_SEQ: the sequences the caller's arrays hold
    uint64_t *n_seq = nullptr; //           where the run leaves the number of sequences (never NULL there)
    unsigned occ_flags = 0;  // OCCURRENCES: the scan's APM_OCC_* flags
    bool per_seq = false;    // OCCURRENCES: the per-sequence scan and span pass (apm_seqocc.hip) under the context's sequence table,
                             // which the request builds behind the normalisation (a text mode only)
    bool seq_ids = false;    //   and the span pass leaves every record's sequence in ds.d_seqocc_seq (needs `spans`)
    bool score = false;      // score ds.d_rec in place against the resident text -- the halo covers every owned window
    bool best = false;       // thin ds.d_rec to its best hits at `radius` into ds.d_rec2, counted in ds.d_rec_n[1]
    uint32_t radius = 0;
    bool spans = false;      // the span records of the ends in ds.d_rec into ds.d_rec2 (NEAREST: by its finishing pass)
    Rows rows = NO_ROWS;     // rows of ops into ds.d_ops: WINDOW_ROWS, the scripts of ds.d_rec -- of the best hits when `best`;
    uint32_t row_stride = 0; // OCC_ROWS, those of the (end, span) pairs (needs `spans`); dwords from one row to the next
    // the device must hold the WHOLE text (single device): the best-hit pass reads `radius` bytes around every window, and every
    // byte of the text is an end of the occurrence scans
    bool whole_text() const { return best || scan != WINDOWS; }
    // the records the request leaves are as many as the counts it adds up
    bool counted() const { return scan != NEAREST && scan != NEAREST_SEQ; }
    // the second record buffer ds.d_rec2 is needed
    bool second_buffer() const { return best || spans; }
};

// ---- apm_records.hip ----
// what the record passes refuse, asked by the host-level calls before anything is scanned: a half-band the scoring pass does
// not serve; a set the occurrence search does not serve; a row stride below apm_align_row_words() or, `occ`,
// apm_occ_align_row_words()
int check_score_band(apm_ctx *ctx);
int check_occ_set(apm_ctx *ctx);
int check_row_stride(apm_ctx *ctx, uint32_t stride, bool occ);
// The scoring pass over the records d_rec[0 .. min(*d_n_rec, capacity)) against the shard text, enqueued on ds.stream
// behind whatever filled the buffer (apm_score.hip).  Later calls with the same pattern set only launch.
int score_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec);
// The align pass over the same records (apm_align.hip): row r of d_ops (stride dwords apart) gets record r's edit script.
int align_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                  uint32_t *d_ops, uint32_t stride);

// The best-hit pass over the same records (apm_best.hip): the best hits at `radius`, scored, are appended to d_out at *d_n_out.
int best_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                 uint32_t radius, apm_match *d_out, uint64_t out_capacity, uint64_t *d_n_out);

// The occurrence scan (apm_occ.hip) of the ends [own_begin, own_end) of the shard text under `flags` (APM_OCC_*): ends are
// appended to d_out at *d_n_found, counts added into d_counts; it refuses a set the scan does not serve and a shard
// without the left halo m_max + k.
int occ_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, unsigned flags, apm_match *d_out,
             uint64_t capacity, uint64_t *d_n_found, unsigned long long *d_counts);
// The span pass over such ends (apm_occ.hip): d_span[r] = the span record of d_rec[r].
int span_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                 apm_match *d_span);
// The per-sequence occurrence scan (apm_seqocc.hip): occ_scan under the sequence table d_table (n_seq + 1 entries).
int seqocc_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, const apm_seq *d_table, uint64_t n_seq,
                unsigned flags, apm_match *d_out, uint64_t capacity, uint64_t *d_n_found, unsigned long long *d_counts);
// The per-sequence span pass over such ends (apm_seqocc.hip): span_records clamped to the sequence; d_seq (may be NULL) gets s(e).
int seqocc_span_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_seq *d_table, uint64_t n_seq, const apm_match *d_rec,
                        uint64_t capacity, const uint64_t *d_n_rec, apm_match *d_span, uint32_t *d_seq);
// The occurrence-script pass over such (end, span) pairs (apm_occ_align.hip): row r of d_ops (stride dwords apart) gets the
// script of d_end[r]'s pattern against the text bytes [d_span[r].pos, d_end[r].pos].
int occ_align_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_end, const apm_match *d_span, uint64_t capacity,
                      const uint64_t *d_n_rec, uint32_t *d_ops, uint32_t stride);

// what the nearest-occurrence search refuses, in `name`'s words: a multi-device context, a pattern beyond
// APM_OCC_MAX_PATTERN_LEN bytes, a text beyond 2^56 bytes -- and nothing for the sake of k
int check_nearest_set(apm_ctx *ctx, const char *name, uint64_t n_total);
// The nearest-occurrence scan (apm_nearest.hip) of the ends [own_begin, own_end) of the shard text: every pattern's best key is
// merged into d_keys[pattern]; it refuses a shard without the left halo 2 m_max - 1.
int nearest_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, unsigned long long *d_keys);
// The finishing pass over such keys (apm_nearest.hip): d_end[i], and with d_start the span record d_start[i], of every pattern.
int nearest_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const unsigned long long *d_keys, apm_match *d_end, apm_match *d_start);
// The per-sequence nearest scan (apm_seqnear.hip) of the ends [own_begin, own_end) of the shard text under the sequence table
// d_table (n_seq + 1 entries): the best key of every (sequence, pattern) pair is merged into d_keys[s * n_patterns + pattern];
// it refuses a shard without the left halo 2 m_max - 1.  check_nearest_set's limits are its own, and n_seq < 2^32.
int seqnear_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, const apm_seq *d_table, uint64_t n_seq,
                 unsigned long long *d_keys);
// The finishing pass over such keys (apm_seqnear.hip): d_end[r], and with d_start the span record d_start[r], of every pair r.
int seqnear_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_seq *d_table, uint64_t n_seq, const unsigned long long *d_keys,
                    apm_match *d_end, apm_match *d_start);

// The record passes' image of ctx->pats and its {row offset, m} table (ds.d_score_img, ds.d_score_tab) on the device, built by
// the first call that needs them with a pattern set
int ensure_score_image(apm_ctx *ctx, DeviceState &ds);

// ---- apm_ingest.hip ----
// host text -> the devices' shards (or, in a text mode, the raw buffer and the normalisation pass) -> scan; find: the
// record request of a find call, NULL: count only
int count_host_text(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t *counts, const FindRequest *find);
// apm_map_positions_device on ds.stream, behind whatever filled the records
int map_positions_on_stream(apm_ctx *ctx, DeviceState &ds, apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec);

// ---- the frame of a device-level shard call ----
// apm_count_shard_device, apm_find_shard_device, apm_occ_shard_device, apm_nearest_shard_device (kRecordPass false) and
// apm_score_shard_device, apm_align_shard_device, apm_best_shard_device, apm_occ_spans_device, apm_occ_align_device,
// apm_nearest_records_device, apm_nearest_seq_records_device, apm_occ_seq_spans_device (true; apm_nearest_seq_shard_device, apm_occ_seq_shard_device: false) run in it.  The checks all of them make, in `name`'s words -- null_arg: a pointer of the caller's own is NULL
// where it may not be; d_rec / rec_name: the caller's record buffer and what its header calls it (NULL: the call has none)
// -- then `checks()` (the caller's further checks, 0: pass), then `body(ds)` between the call's events.  A scan opens the
// bracket for its launches, which record ev_mstart / ev_mstop themselves; a record pass is one launch and the whole call:
// all of its event pairs bracket it.  Templates and lambdas only: apm_count_shard_device is called once per step.
template <bool kRecordPass, class Checks, class Body>
int shard_call(apm_ctx *ctx, const char *name, const ShardText &sh, bool null_arg, const void *d_rec, const char *rec_name, Checks checks, Body body) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_STATE, "%s needs a single-device context", name);
    if (null_arg || (!sh.text && sh.text_len)) return fail(ctx, APM_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_rec) & 15u) return fail(ctx, APM_ERR_INVALID, "%s must be 16-byte aligned", rec_name);
    if (sh.text_off + sh.text_len > sh.n_total) return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
    int rc = checks();
    if (rc) return rc;
    begin_call(ctx);
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_start, ds.stream));
        HIP_TRY(ctx, hipEventRecord(ds.ev_kstart, ds.stream));
        if (kRecordPass) HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
    }
    rc = body(ds);
    if (rc) return rc;
    if (ctx->timing_on) {
        if (kRecordPass) HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
        HIP_TRY(ctx, hipEventRecord(ds.ev_stop, ds.stream));
        ds.events_recorded = true;
    }
    return APM_OK;
}

#pragma GCC visibility pop

#endif /* APM_RUNTIME_H */
