/*
 * apm_find.hip -- the host-level find calls: each says what it wants as a FindRequest (apm_runtime.h), count_sharded
 * (apm_ingest.hip) runs the scan and the record passes (apm_records.hip) on every device, and what the devices -- or the
 * child contexts of a pattern-sharded one -- found is downloaded and merged here, by one rule for every call.
 * apm_find_buffer, the one-pattern call, runs the counting kernels with a position sink instead.
 *
 * There is no CPU fallback in this file by design.
 */
#include "apm_runtime.h"
#include "apm_core.h"
#include "apm_align.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

// how every host-level find call begins; `bad`: the call's own test of its arguments (it must not look into ctx)
int begin_find(apm_ctx *ctx, const char *name, bool bad) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (bad) return fail(ctx, APM_ERR_INVALID, "bad argument to %s", name);
    return APM_OK;
}

// what a call gathered on the host, device by device (or child by child)
struct Found {
    std::vector<apm_match> rec, rec2; // rec2[i] (where asked for): the companion of rec[i], the span record of an end
    std::vector<uint32_t> rows;       // (where asked for) row i of `stride` dwords belongs to rec[i]
    std::vector<uint32_t> seq;        // (where asked for) seq[i]: the sequence of rec[i]
};

// Appends the first `take` records of d_rec to f -- with d_rec2, their companions there; with a stride, their rows of ds.d_ops;
// with d_seq, their sequences.  The stream's work on them is done.
int gather(apm_ctx *ctx, DeviceState &ds, const void *d_rec, const void *d_rec2, size_t take, uint32_t stride, Found &f, const uint32_t *d_seq = nullptr) {
    const size_t at = f.rec.size();
    f.rec.resize(at + take);
    if (d_rec2) f.rec2.resize(at + take);
    if (d_seq) f.seq.resize(at + take);
    f.rows.resize((at + take) * stride);
    if (!take) return APM_OK;
    HIP_TRY(ctx, hipMemcpy(f.rec.data() + at, d_rec, take * sizeof(apm_match), hipMemcpyDeviceToHost));
    if (d_rec2) HIP_TRY(ctx, hipMemcpy(f.rec2.data() + at, d_rec2, take * sizeof(apm_match), hipMemcpyDeviceToHost));
    if (stride) HIP_TRY(ctx, hipMemcpy(f.rows.data() + at * stride, ds.d_ops, take * stride * 4, hipMemcpyDeviceToHost));
    if (d_seq) HIP_TRY(ctx, hipMemcpy(f.seq.data() + at, d_seq, take * 4, hipMemcpyDeviceToHost));
    return APM_OK;
}

// One request on the context's own devices, up to the merge: scan and passes (count_host_text), in a text mode the position
// map over what will be downloaded (normalised text -> source offsets, behind every pass), the counters, the download of
// min(found, cap) records per device -- the best hits where the request thins to them -- with their spans and rows.
// *n_sunk: the records the sink counted, checked against the counts in `what`'s words where the request counts them; *n_have: the records there were to
// download (the best hits; else *n_sunk).  TEXT partition: every device holds the records of its owner range.
int run_request(apm_ctx *ctx, const uint8_t *text, uint64_t n, const FindRequest &req, const char *what, std::vector<uint64_t> &counts, Found &f,
                uint64_t *n_sunk, uint64_t *n_have) {
    counts.assign(ctx->pats.size(), 0);
    int rc = count_host_text(ctx, text, n, counts.data(), &req);
    if (rc) return rc;
    uint64_t csum = 0;
    for (uint64_t c : counts) csum += c;
    *n_sunk = *n_have = 0;
    // (NEAREST_SEQ: the run counted the sequences and sized the record buffers for n_seq * n_patterns pairs)
    const uint64_t cap = req.scan == FindRequest::NEAREST_SEQ ? *req.n_seq * (uint64_t)ctx->pats.size() : req.cap;
    for (auto &ds : ctx->devs) {
        HIP_TRY(ctx, hipSetDevice(ds.dev));
        apm_match *d_rec = reinterpret_cast<apm_match *>(req.best ? ds.d_rec2 : ds.d_rec), *d_span = reinterpret_cast<apm_match *>(req.spans ? ds.d_rec2 : nullptr);
        const uint64_t *d_n = reinterpret_cast<const uint64_t *>(ds.d_rec_n) + (req.best ? 1 : 0);
        if (ctx->text_mode) rc = map_positions_on_stream(ctx, ds, d_rec, cap, d_n);
        if (ctx->text_mode && !rc && d_span) rc = map_positions_on_stream(ctx, ds, d_span, cap, d_n);
        if (rc) return rc;
        unsigned long long c[2] = {0, 0}; // {records, best hits}
        HIP_TRY(ctx, hipMemcpyAsync(c, ds.d_rec_n, 16, hipMemcpyDeviceToHost, ds.stream));
        HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
        const uint64_t have = c[req.best ? 1 : 0];
        *n_sunk += c[0];
        *n_have += have;
        rc = gather(ctx, ds, d_rec, d_span, (size_t)std::min<uint64_t>(have, cap), req.row_stride, f, req.seq_ids ? ds.d_seqocc_seq : nullptr);
        if (rc) return rc;
    }
    if (req.counted() && *n_sunk != csum)
        return fail(ctx, APM_ERR_STATE, "record sink count %llu != %s count %llu", (unsigned long long)*n_sunk, what, (unsigned long long)csum);
    return APM_OK;
}

// THE merge of every find call: what was gathered, sorted by (pattern, pos) through a permutation, the first `capacity` of it
// written out -- the records, their companions (out2 != NULL), their sequences (out_seq != NULL) and, with a stride, of each record's row exactly the words
// the row format defines: 1 for APM_DIST_INVALID, else the count and the ops behind it (every match is within k: n_ops >= 1).
// The caller's words behind those, and its rows behind the last record, stay untouched.  Records are unique by (pattern,
// pos) in every call -- window records after the scan's dedup, one end per (pattern, end), thinned best hits -- so the
// result does not depend on the sort being stable, nor on the order the devices appended in.
void merge_out(const Found &f, uint32_t stride, uint64_t capacity, apm_match *out, apm_match *out2, uint32_t *ops, uint32_t *out_seq = nullptr) {
    std::vector<size_t> perm(f.rec.size());
    for (size_t i = 0; i < perm.size(); ++i) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](size_t x, size_t y) {
        const apm_match &a = f.rec[x], &b = f.rec[y];
        return a.pattern != b.pattern ? a.pattern < b.pattern : a.pos < b.pos;
    });
    for (size_t i = 0; i < perm.size() && i < capacity; ++i) {
        out[i] = f.rec[perm[i]];
        if (out2) out2[i] = f.rec2[perm[i]];
        if (out_seq) out_seq[i] = f.seq[perm[i]];
        if (!stride) continue;
        const uint32_t *row = f.rows.data() + perm[i] * stride;
        const size_t used = row[0] == APM_DIST_INVALID ? 1 : std::min<size_t>((size_t)apm_align_words((int)row[0]), stride);
        memcpy(ops + i * stride, row, used * 4);
    }
}

// apm_find_all_buffer; `score` (apm_find_all_dist_buffer): every device (every child) scores its records before they leave
// it; `ops` (apm_find_all_align_buffer, which also scores): and aligns them into rows of `stride` dwords.  `name`: the entry
// point, for its messages; `want_ops`: it is the align call.
int find_all(apm_ctx *ctx, const char *name, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found, bool score,
             bool want_ops, uint32_t *ops, uint32_t stride) {
    int rc = begin_find(ctx, name, !n_found || (!out && capacity) || (!text && n) || (want_ops && !ops && capacity));
    if (!rc && want_ops) rc = check_row_stride(ctx, stride, false);
    if (rc) return rc;
    Found f;
    uint64_t total = 0;
    if (pattern_sharded(ctx)) { // every child finds its slice in the whole text; the indices are shifted by the slice's first pattern
        const size_t G = ctx->children.size();
        std::vector<std::vector<apm_match>> part(G);
        std::vector<std::vector<uint32_t>> part_ops(G);
        std::vector<uint64_t> found(G, 0);
        std::vector<uint64_t> dummy(ctx->pats.size(), 0);
        rc = for_children(ctx, dummy.data(), [&](apm_ctx *ch, uint64_t *) {
            const size_t g = (size_t)(std::find(ctx->children.begin(), ctx->children.end(), ch) - ctx->children.begin());
            part[g].resize((size_t)capacity);
            if (want_ops) part_ops[g].assign((size_t)capacity * stride, 0u);
            // (scored and aligned with the child's own slice, at the parent's stride)
            return find_all(ch, name, text, n, part[g].data(), capacity, &found[g], score, want_ops, part_ops[g].data(), stride);
        });
        if (rc) return rc;
        for (size_t g = 0; g < G; ++g) {
            total += found[g];
            const size_t take = (size_t)std::min<uint64_t>(found[g], capacity);
            for (size_t i = 0; i < take; ++i) {
                apm_match r = part[g][i];
                r.pattern += (uint32_t)ctx->pat_first[g];
                f.rec.push_back(r);
            }
            if (want_ops) f.rows.insert(f.rows.end(), part_ops[g].begin(), part_ops[g].begin() + (ptrdiff_t)(take * stride));
        }
    } else {
        FindRequest req;
        req.cap = capacity;
        req.score = score;
        req.rows = want_ops ? FindRequest::WINDOW_ROWS : FindRequest::NO_ROWS;
        req.row_stride = want_ops ? stride : 0;
        std::vector<uint64_t> counts;
        uint64_t have = 0;
        rc = score ? check_score_band(ctx) : APM_OK; // (refused before anything is scanned)
        if (!rc) rc = run_request(ctx, text, n, req, "match", counts, f, &total, &have);
        if (rc) return rc;
    }
    merge_out(f, want_ops ? stride : 0, capacity, out, nullptr, ops);
    *n_found = total;
    return APM_OK;
}

// One occurrence scan of the whole text on the single device; with out_start the span pass over its ends; `scripts`
// (apm_find_occ_align_buffer, `name` says which call this is) the occurrence-script pass over both into rows of `stride`
// dwords.  capacity == 0 counts only.
int find_occ(apm_ctx *ctx, const char *name, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end, apm_match *out_start,
             uint64_t capacity, uint64_t *n_found, uint64_t *counts, bool scripts, uint32_t *ops, uint32_t stride) {
    // (the script call needs starts and rows)
    int rc = begin_find(ctx, name, !n_found || (!out_end && capacity) || (!text && n) || (scripts && capacity && (!out_start || !ops)));
    if (rc) return rc;
    if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
    if (ctx->devs.size() != 1)
        return fail(ctx, APM_ERR_UNSUPPORTED, "%s needs a single-device context: the resident shards bring a right halo, the "
                                              "occurrence scan needs a left one", name);
    rc = check_occ_set(ctx); // (refused before anything is staged)
    if (!rc && scripts) rc = check_row_stride(ctx, stride, true);
    if (rc) return rc;
    if (scripts && !capacity) out_start = nullptr; // (a count only: neither spans nor scripts)
    FindRequest req;
    req.cap = capacity;
    req.scan = FindRequest::OCCURRENCES;
    req.occ_flags = flags;
    req.spans = out_start != nullptr;
    req.rows = scripts && out_start ? FindRequest::OCC_ROWS : FindRequest::NO_ROWS;
    req.row_stride = scripts && out_start ? stride : 0;
    std::vector<uint64_t> cnt;
    Found f;
    uint64_t total = 0, have = 0;
    rc = run_request(ctx, text, n, req, "occurrence", cnt, f, &total, &have);
    if (rc) return rc;
    merge_out(f, req.row_stride, capacity, out_end, out_start, ops);
    *n_found = total;
    if (counts) memcpy(counts, cnt.data(), cnt.size() * sizeof(uint64_t));
    return APM_OK;
}

} // namespace

extern "C" {

int apm_find_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, int pattern_index, uint64_t *positions,
                    uint64_t capacity, uint64_t *n_found) {
    const bool bad_index = ctx && (pattern_index < 0 || pattern_index >= (int)ctx->pats.size());
    const int brc = begin_find(ctx, "apm_find_buffer", bad_index || !n_found || (!positions && capacity) || (!text && n));
    if (brc) return brc;
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

int apm_find_all_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found) {
    return find_all(ctx, "apm_find_all_buffer", text, n, out, capacity, n_found, false, false, nullptr, 0);
}

int apm_find_all_dist_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found) {
    return find_all(ctx, "apm_find_all_dist_buffer", text, n, out, capacity, n_found, true, false, nullptr, 0);
}

int apm_find_all_align_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found,
                              uint32_t *ops, uint32_t stride_words) {
    return find_all(ctx, "apm_find_all_align_buffer", text, n, out, capacity, n_found, true, true, ops, stride_words);
}

// The window scan on the single device, behind it on the same stream the best-hit pass from the context's record buffer into
// its second one and, with ops, the align pass over the best hits.  Only the best hits are downloaded.
int apm_find_best_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t radius, apm_match *out, uint64_t capacity,
                         uint64_t *n_best, uint64_t *n_matches, uint32_t *ops, uint32_t stride_words) {
    int rc = begin_find(ctx, "apm_find_best_buffer", !n_best || !n_matches || (!out && capacity) || (!text && n));
    if (rc) return rc;
    if (radius > APM_BEST_MAX_RADIUS) return fail(ctx, APM_ERR_INVALID, "radius %u is beyond APM_BEST_MAX_RADIUS = %d", radius, APM_BEST_MAX_RADIUS);
    if (ctx->devs.size() != 1)
        return fail(ctx, APM_ERR_UNSUPPORTED, "apm_find_best_buffer needs a single-device context: the resident shards' halo is m_max - 1, the pass needs "
                                              "the radius more on both sides");
    if (ops) rc = check_row_stride(ctx, stride_words, false);
    if (!rc) rc = check_score_band(ctx); // (refused before anything is scanned)
    if (rc) return rc;
    FindRequest req;
    req.cap = capacity;
    req.best = true;
    req.radius = radius;
    req.rows = ops ? FindRequest::WINDOW_ROWS : FindRequest::NO_ROWS;
    req.row_stride = ops ? stride_words : 0;
    std::vector<uint64_t> counts;
    Found f;
    uint64_t total = 0, best = 0;
    rc = run_request(ctx, text, n, req, "match", counts, f, &total, &best);
    if (rc) return rc;
    merge_out(f, req.row_stride, capacity, out, nullptr, ops);
    *n_matches = total;
    *n_best = best;
    return APM_OK;
}

int apm_find_occ_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end, apm_match *out_start,
                        uint64_t capacity, uint64_t *n_found, uint64_t *counts) {
    return find_occ(ctx, "apm_find_occ_buffer", text, n, flags, out_end, out_start, capacity, n_found, counts, false, nullptr, 0);
}

int apm_find_occ_align_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end, apm_match *out_start,
                              uint64_t capacity, uint64_t *n_found, uint64_t *counts, uint32_t *ops, uint32_t stride_words) {
    return find_occ(ctx, "apm_find_occ_align_buffer", text, n, flags, out_end, out_start, capacity, n_found, counts, true, ops, stride_words);
}

// One per-sequence occurrence scan of the whole text on the single device under the context's sequence table, which the
// request builds behind the normalisation; with out_start the per-sequence span pass over its ends (and out_seq from it), with
// ops the occurrence-script pass over both.  capacity == 0 counts only.
int apm_find_occ_seq_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end, apm_match *out_start,
                            uint32_t *out_seq, uint64_t capacity, uint64_t *n_found, uint64_t *counts, uint32_t *ops, uint32_t stride_words) {
    const char *name = "apm_find_occ_seq_buffer";
    int rc = begin_find(ctx, name, !n_found || (!out_end && capacity) || (!text && n) || ((out_seq || ops) && !out_start));
    if (rc) return rc;
    if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_UNSUPPORTED, "%s needs a single-device context", name);
    rc = check_occ_set(ctx); // (refused before anything is staged)
    if (!rc && n > (1ull << 56)) rc = fail(ctx, APM_ERR_UNSUPPORTED, "%s serves texts of at most 2^56 bytes", name);
    if (!rc && ops) rc = check_row_stride(ctx, stride_words, true);
    if (!rc && !ctx->text_mode) rc = fail(ctx, APM_ERR_STATE, "%s needs a text mode (apm_set_text_mode): that is where sequences come from", name);
    if (rc) return rc;
    if (!capacity) out_start = nullptr, out_seq = nullptr, ops = nullptr; // (a count only: neither spans nor scripts)
    FindRequest req;
    req.cap = capacity;
    req.scan = FindRequest::OCCURRENCES;
    req.occ_flags = flags;
    req.per_seq = true;
    req.spans = out_start != nullptr;
    req.seq_ids = out_seq != nullptr;
    req.rows = ops ? FindRequest::OCC_ROWS : FindRequest::NO_ROWS;
    req.row_stride = ops ? stride_words : 0;
    std::vector<uint64_t> cnt;
    Found f;
    uint64_t total = 0, have = 0;
    rc = run_request(ctx, text, n, req, "occurrence", cnt, f, &total, &have);
    if (rc) return rc;
    merge_out(f, req.row_stride, capacity, out_end, out_start, ops, out_seq);
    *n_found = total;
    if (counts) memcpy(counts, cnt.data(), cnt.size() * sizeof(uint64_t));
    return APM_OK;
}

// One nearest-occurrence scan of the whole text on the single device and its finishing pass: a record per pattern, with
// out_start the span records too.
int apm_find_nearest_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out_end, apm_match *out_start) {
    int rc = begin_find(ctx, "apm_find_nearest_buffer", !out_end || (!text && n));
    if (!rc) rc = check_nearest_set(ctx, "apm_find_nearest_buffer", n); // (refused before anything is staged)
    if (rc) return rc;
    FindRequest req;
    req.cap = ctx->pats.size();
    req.scan = FindRequest::NEAREST;
    req.spans = out_start != nullptr;
    std::vector<uint64_t> cnt;
    Found f;
    uint64_t total = 0, have = 0;
    rc = run_request(ctx, text, n, req, "nearest", cnt, f, &total, &have);
    if (rc) return rc;
    merge_out(f, 0, req.cap, out_end, out_start, nullptr); // (one record per pattern: pattern order)
    return APM_OK;
}

// One per-sequence nearest scan of the whole text on the single device and its finishing pass: a record per (sequence,
// pattern) pair in row order s * n_patterns + i -- the order the device left them in, no merge --, with out_start the span
// records too.
int apm_find_nearest_seq_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out_end, apm_match *out_start, uint64_t capacity_seq,
                                uint64_t *n_seq) {
    int rc = begin_find(ctx, "apm_find_nearest_seq_buffer", !n_seq || (!out_end && capacity_seq) || (!text && n));
    if (!rc) rc = check_nearest_set(ctx, "apm_find_nearest_seq_buffer", n); // (refused before anything is staged)
    if (!rc && !ctx->text_mode) rc = fail(ctx, APM_ERR_STATE, "apm_find_nearest_seq_buffer needs a text mode (apm_set_text_mode): that is where sequences come from");
    if (rc) return rc;
    *n_seq = 0;
    FindRequest req;
    req.scan = FindRequest::NEAREST_SEQ;
    req.cap_seq = capacity_seq;
    req.n_seq = n_seq;
    req.spans = out_start != nullptr;
    std::vector<uint64_t> cnt;
    Found f;
    uint64_t total = 0, have = 0;
    rc = run_request(ctx, text, n, req, "nearest per sequence", cnt, f, &total, &have);
    if (rc) return rc;
    std::copy(f.rec.begin(), f.rec.end(), out_end);
    if (out_start) std::copy(f.rec2.begin(), f.rec2.end(), out_start);
    return APM_OK;
}

} // extern "C"
