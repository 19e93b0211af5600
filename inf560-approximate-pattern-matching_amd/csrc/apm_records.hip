/*
 * apm_records.hip -- the record passes over finished match records (scoring, apm_score.hip; align, apm_align.hip; best
 * hits, apm_best.hip; spans, apm_occ.hip; occurrence scripts, apm_occ_align.hip), the occurrence scan (apm_occ.hip) and the
 * nearest-occurrence scan and its finishing pass (apm_nearest.hip; per sequence: apm_seqnear.hip), the per-sequence occurrence scan and span pass (apm_seqocc.hip), with what they refuse, and the device-level entry points of all of them and of the find call.  The host-level find calls, which
 * run these behind a scan and merge what every device found, are in apm_find.hip.
 *
 * There is no CPU fallback in this file by design.
 */
#include "apm_runtime.h"
#include "apm_core.h"
#include "apm_score.h"
#include "apm_align.h"
#include "apm_best.h"
#include "apm_occ.h"
#include "apm_occ_align.h"
#include "apm_nearest.h"
#include "apm_seqnear.h"
#include "apm_seqocc.h"

#include <cstring>
#include <string>
#include <vector>

// the half-band the scoring pass needs for ctx->pats at ctx->k, refused beyond what the wave form's LDS band holds
int check_score_band(apm_ctx *ctx) {
    const int band = std::min(ctx->k / 2, longest_pattern(ctx) - 1);
    if (ctx->k > APM_SCORE_LANE_MAX_K && band > APM_SCORE_MAX_BAND)
        return fail(ctx, APM_ERR_UNSUPPORTED, "scoring serves a half-band min(k/2, m_max-1) of at most %d diagonals, this pattern set needs %d",
                    APM_SCORE_MAX_BAND, band);
    return APM_OK;
}

namespace {

// The record passes' common arguments (ApmScoreArgs) for the records d_rec[0 .. min(*d_n_rec, capacity)) against the shard
// text: refuses a band the scoring pass does not serve and makes sure the score image is on the device.
int record_args(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                ApmScoreArgs &a) {
    int rc = check_score_band(ctx);
    if (!rc) rc = ensure_score_image(ctx, ds);
    if (rc) return rc;
    a.text = sh.text;
    a.text_off = sh.text_off;
    a.text_len = sh.text_len;
    a.n_total = sh.n_total;
    a.rec = reinterpret_cast<uint4 *>(const_cast<apm_match *>(d_rec)); // (the align pass only reads them)
    a.cap = capacity;
    a.n_rec = reinterpret_cast<const unsigned long long *>(d_n_rec);
    a.image = ds.d_score_img;
    a.table = ds.d_score_tab;
    a.n_patterns = (uint32_t)ctx->pats.size();
    a.k = ctx->k;
    return APM_OK;
}

// dwords of one record's row of ops for ctx->pats at ctx->k: the count and the most ops a script of the set has
uint32_t align_row_words(const apm_ctx *ctx) { return (uint32_t)apm_align_words(apm_align_max_ops(longest_pattern(ctx), ctx->k)); }

// dwords of one pair's row of ops for ctx->pats at ctx->k (a set check_occ_set accepts): the count and m_max + k ops
uint32_t occ_align_row_words(const apm_ctx *ctx) { return (uint32_t)apm_occ_align_row_words_of(longest_pattern(ctx), ctx->k); }

} // namespace

int check_row_stride(apm_ctx *ctx, uint32_t stride, bool occ) {
    const uint32_t words = occ ? occ_align_row_words(ctx) : align_row_words(ctx);
    if (stride < words)
        return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than %s() = %u", stride, occ ? "apm_occ_align_row_words" : "apm_align_row_words", words);
    return APM_OK;
}

// the scoring, align and locate passes' image of ctx->pats on the device: built by the first such call with a pattern set
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

int score_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec) {
    ApmScoreArgs a{};
    const int rc = record_args(ctx, ds, sh, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    APM_LAUNCH(ctx, ds, "score", apm_launch_score(a, ds.n_cu, ds.stream));
    return APM_OK;
}

// It refuses what the scoring pass refuses and shares its image; the first call with a pattern set also allocates the
// trace workspace (apm_align.h: sized from APM_ALIGN_WS_BUDGET), later calls only launch.
int align_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                  uint32_t *d_ops, uint32_t stride) {
    ApmAlignArgs a{};
    int rc = record_args(ctx, ds, sh, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    const int m_max = longest_pattern(ctx);
    if (!ds.align_rows) {
        size_t bytes = 0, have = 0; // (d_align_ws went with the plan: nothing to free)
        const uint32_t rows = apm_align_rows(m_max, ctx->k, ds.n_cu, APM_BLOCK, &bytes);
        if (bytes) rc = grow_device_buffer(ctx, ds, &ds.d_align_ws, &have, bytes, 1, APM_ERR_NOMEM, "the align pass's trace workspace (%zu bytes)", bytes);
        if (rc) return rc;
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

// It refuses what the scoring pass refuses and shares its image; later calls with the same pattern set only launch.  The
// launch is bracketed by events of its own (apm_get_stat "best_ms").
int best_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                 uint32_t radius, apm_match *d_out, uint64_t out_capacity, uint64_t *d_n_out) {
    ApmBestArgs a{};
    const int rc = record_args(ctx, ds, sh, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    a.radius = radius;
    a.out = reinterpret_cast<uint4 *>(d_out);
    a.out_cap = out_capacity;
    a.n_out = reinterpret_cast<unsigned long long *>(d_n_out);
    ds.best_timed = false;
    if (ctx->timing_on) {
        for (hipEvent_t &e : ds.ev_best)
            if (!e) HIP_TRY(ctx, hipEventCreate(&e));
        HIP_TRY(ctx, hipEventRecord(ds.ev_best[0], ds.stream));
    }
    APM_LAUNCH(ctx, ds, "best", apm_launch_best(a, ds.n_cu, ds.stream));
    if (ctx->timing_on) {
        HIP_TRY(ctx, hipEventRecord(ds.ev_best[1], ds.stream));
        ds.best_timed = true;
    }
    return APM_OK;
}

// what the occurrence search serves: every pattern of at most APM_OCC_MAX_PATTERN_LEN bytes and k < m (with k >= m every
// position matches the empty substring)
int check_occ_set(apm_ctx *ctx) {
    for (const auto &p : ctx->pats) {
        if (p.m > APM_OCC_MAX_PATTERN_LEN)
            return fail(ctx, APM_ERR_UNSUPPORTED, "the occurrence search serves patterns of at most %d bytes, this set has one of %d", APM_OCC_MAX_PATTERN_LEN, p.m);
        if (ctx->k >= p.m)
            return fail(ctx, APM_ERR_UNSUPPORTED, "the occurrence search needs k < m: with k = %d a pattern of %d bytes matches the empty substring everywhere", ctx->k, p.m);
    }
    return APM_OK;
}

// The occurrence scan of the ends [own_begin, own_end) n [0, n_total) on ds.stream: one launch, "occ", between the main
// events.  The shard text must bring the LEFT halo m_max + k and the look-ahead byte.  Later calls with the same pattern
// set only launch.
int occ_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, unsigned flags, apm_match *d_out,
             uint64_t capacity, uint64_t *d_n_found, unsigned long long *d_counts) {
    int rc = check_occ_set(ctx);
    if (rc) return rc;
    if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
    const int m_max = longest_pattern(ctx);
    const uint64_t eb = std::min(own_begin, sh.n_total), ee = std::min(own_end, sh.n_total);
    const uint64_t halo = (uint64_t)(m_max + ctx->k);
    const uint64_t need_lo = eb > halo ? eb - halo : 0, need_hi = std::min(sh.n_total, ee + 1);
    if (ee > eb && (sh.text_off > need_lo || sh.text_off + sh.text_len < need_hi))
        return fail(ctx, APM_ERR_INVALID, "shard text too short: the ends [%llu, %llu) need the bytes [%llu, %llu), a left halo of m_max + k = %llu",
                    (unsigned long long)eb, (unsigned long long)ee, (unsigned long long)need_lo, (unsigned long long)need_hi, (unsigned long long)halo);
    if (ee > eb) rc = ensure_score_image(ctx, ds);
    if (rc) return rc;
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
    if (ee > eb) {
        ApmOccArgs a{};
        a.text = sh.text;
        a.text_off = sh.text_off;
        a.text_len = sh.text_len;
        a.n_total = sh.n_total;
        a.e_begin = eb;
        a.e_end = ee;
        uint64_t S = (uint64_t)apm_occ_segment(m_max, ctx->k, ee - eb, ds.n_cu, (int)ctx->pats.size());
        while ((ee - eb + S - 1) / S > (1ull << 30)) S *= 2; // (the grid's x dimension)
        a.segment = (uint32_t)S;
        a.n_segments = (uint32_t)((ee - eb + S - 1) / S);
        a.image = ds.d_score_img;
        a.table = ds.d_score_tab;
        a.n_patterns = (uint32_t)ctx->pats.size();
        a.k = ctx->k;
        a.m_max = m_max;
        a.flags = flags;
        a.out = reinterpret_cast<uint4 *>(d_out);
        a.cap = capacity;
        a.n_found = reinterpret_cast<unsigned long long *>(d_n_found);
        a.counts = d_counts;
        APM_LAUNCH(ctx, ds, "occ", apm_launch_occ(a, ds.stream));
        ds.occ_segment = a.segment;
        ds.occ_lanes = (uint64_t)a.n_segments * a.n_patterns;
        ds.text_bytes += need_hi - need_lo;
    }
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
    return APM_OK;
}

// The span pass over the ends d_rec[0 .. min(*d_n_rec, capacity)) (apm_occ.hip): d_span[r] = the span record of d_rec[r].
int span_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                 apm_match *d_span) {
    int rc = check_occ_set(ctx);
    if (rc) return rc;
    ApmSpanArgs a{};
    rc = record_args(ctx, ds, sh, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    a.span = reinterpret_cast<uint4 *>(d_span);
    APM_LAUNCH(ctx, ds, "span", apm_launch_span(a, ds.n_cu, ds.stream));
    return APM_OK;
}

// what the nearest-occurrence search serves: a single device, every pattern of at most APM_OCC_MAX_PATTERN_LEN bytes (k is
// not looked at), ends below 2^56 (the key's end field)
int check_nearest_set(apm_ctx *ctx, const char *name, uint64_t n_total) {
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_UNSUPPORTED, "%s needs a single-device context", name);
    for (const auto &p : ctx->pats)
        if (p.m > APM_OCC_MAX_PATTERN_LEN)
            return fail(ctx, APM_ERR_UNSUPPORTED, "the nearest-occurrence search serves patterns of at most %d bytes, this set has one of %d", APM_OCC_MAX_PATTERN_LEN, p.m);
    if (n_total > APM_NEAREST_MAX_TEXT) return fail(ctx, APM_ERR_UNSUPPORTED, "the nearest-occurrence search serves texts of at most 2^56 bytes");
    return APM_OK;
}

// The nearest-occurrence scan of the ends [own_begin, own_end) n [0, n_total) on ds.stream: one launch, "nearest", between the
// main events, merging into d_keys.  The shard text must bring the LEFT halo 2 m_max - 1 and the look-ahead byte.  Later
// calls with the same pattern set only launch.
int nearest_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, unsigned long long *d_keys) {
    const int m_max = longest_pattern(ctx);
    const uint64_t eb = std::min(own_begin, sh.n_total), ee = std::min(own_end, sh.n_total);
    const uint64_t halo = (uint64_t)(2 * m_max - 1);
    const uint64_t need_lo = eb > halo ? eb - halo : 0, need_hi = std::min(sh.n_total, ee + 1);
    if (ee > eb && (sh.text_off > need_lo || sh.text_off + sh.text_len < need_hi))
        return fail(ctx, APM_ERR_INVALID, "shard text too short: the ends [%llu, %llu) need the bytes [%llu, %llu), a left halo of 2 m_max - 1 = %llu",
                    (unsigned long long)eb, (unsigned long long)ee, (unsigned long long)need_lo, (unsigned long long)need_hi, (unsigned long long)halo);
    int rc = ee > eb ? ensure_score_image(ctx, ds) : APM_OK;
    if (rc) return rc;
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
    if (ee > eb) {
        ApmNearestArgs a{};
        a.text = sh.text;
        a.text_off = sh.text_off;
        a.text_len = sh.text_len;
        a.n_total = sh.n_total;
        a.e_begin = eb;
        a.e_end = ee;
        uint64_t S = (uint64_t)apm_nearest_segment(m_max, ee - eb, ds.n_cu, (int)ctx->pats.size());
        while ((ee - eb + S - 1) / S > (1ull << 30)) S *= 2; // (the grid's x dimension)
        a.segment = (uint32_t)S;
        a.n_segments = (uint32_t)((ee - eb + S - 1) / S);
        a.image = ds.d_score_img;
        a.table = ds.d_score_tab;
        a.n_patterns = (uint32_t)ctx->pats.size();
        a.keys = d_keys;
        APM_LAUNCH(ctx, ds, "nearest", apm_launch_nearest(a, ds.stream));
        ds.nearest_segment = a.segment;
        ds.nearest_lanes = (uint64_t)a.n_segments * a.n_patterns;
        ds.text_bytes += need_hi - need_lo;
    }
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
    return APM_OK;
}

// The finishing pass over the keys (apm_nearest.hip): one launch, "nspan"; d_end[i] and, with d_start, d_start[i] of every pattern.
int nearest_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const unsigned long long *d_keys, apm_match *d_end, apm_match *d_start) {
    const int rc = ensure_score_image(ctx, ds);
    if (rc) return rc;
    ApmNspanArgs a{};
    a.text = sh.text;
    a.text_off = sh.text_off;
    a.text_len = sh.text_len;
    a.n_total = sh.n_total;
    a.image = ds.d_score_img;
    a.table = ds.d_score_tab;
    a.n_patterns = (uint32_t)ctx->pats.size();
    a.keys = d_keys;
    a.end = reinterpret_cast<uint4 *>(d_end);
    a.start = reinterpret_cast<uint4 *>(d_start);
    APM_LAUNCH(ctx, ds, "nspan", apm_launch_nspan(a, ds.n_cu, ds.stream));
    return APM_OK;
}

// The per-sequence nearest scan of the ends [own_begin, own_end) n [0, n_total) on ds.stream: one launch, "snear", between the
// main events, merging into d_keys[s * n_patterns + pattern].  The shard text must bring the LEFT halo 2 m_max - 1 (a walk may
// start that far in front of its first end, where no sequence begins in between) and, the nearest scan's cover rule kept as
// it is, the byte behind the last end, which this walk never reads.
int seqnear_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, const apm_seq *d_table, uint64_t n_seq,
                 unsigned long long *d_keys) {
    const int m_max = longest_pattern(ctx);
    const uint64_t eb = std::min(own_begin, sh.n_total), ee = std::min(own_end, sh.n_total);
    const uint64_t halo = (uint64_t)(2 * m_max - 1);
    const uint64_t need_lo = eb > halo ? eb - halo : 0, need_hi = std::min(sh.n_total, ee + 1);
    if (ee > eb && (sh.text_off > need_lo || sh.text_off + sh.text_len < need_hi))
        return fail(ctx, APM_ERR_INVALID, "shard text too short: the ends [%llu, %llu) need the bytes [%llu, %llu), a left halo of 2 m_max - 1 = %llu",
                    (unsigned long long)eb, (unsigned long long)ee, (unsigned long long)need_lo, (unsigned long long)need_hi, (unsigned long long)halo);
    int rc = ee > eb ? ensure_score_image(ctx, ds) : APM_OK;
    if (rc) return rc;
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
    if (ee > eb) {
        ApmSeqnearArgs a{};
        a.text = sh.text;
        a.text_off = sh.text_off;
        a.text_len = sh.text_len;
        a.n_total = sh.n_total;
        a.e_begin = eb;
        a.e_end = ee;
        uint64_t S = (uint64_t)apm_nearest_segment(m_max, ee - eb, ds.n_cu, (int)ctx->pats.size());
        while ((ee - eb + S - 1) / S > (1ull << 30)) S *= 2; // (the grid's x dimension)
        a.segment = (uint32_t)S;
        a.n_segments = (uint32_t)((ee - eb + S - 1) / S);
        a.image = ds.d_score_img;
        a.table = ds.d_score_tab;
        a.n_patterns = (uint32_t)ctx->pats.size();
        a.seqs = d_table;
        a.n_seq = n_seq;
        a.keys = d_keys;
        APM_LAUNCH(ctx, ds, "snear", apm_launch_seqnear(a, ds.stream));
        ds.seqnear_segment = a.segment;
        ds.seqnear_lanes = (uint64_t)a.n_segments * a.n_patterns;
        ds.text_bytes += need_hi - need_lo;
    }
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
    return APM_OK;
}

// The finishing pass over the keys (apm_seqnear.hip): one launch, "snspan"; d_end[r] and, with d_start, d_start[r] of every pair.
int seqnear_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_seq *d_table, uint64_t n_seq, const unsigned long long *d_keys,
                    apm_match *d_end, apm_match *d_start) {
    const int rc = ensure_score_image(ctx, ds);
    if (rc) return rc;
    ApmSnspanArgs a{};
    a.text = sh.text;
    a.text_off = sh.text_off;
    a.text_len = sh.text_len;
    a.n_total = sh.n_total;
    a.image = ds.d_score_img;
    a.table = ds.d_score_tab;
    a.n_patterns = (uint32_t)ctx->pats.size();
    a.seqs = d_table;
    a.n_seq = n_seq;
    a.keys = d_keys;
    a.end = reinterpret_cast<uint4 *>(d_end);
    a.start = reinterpret_cast<uint4 *>(d_start);
    APM_LAUNCH(ctx, ds, "snspan", apm_launch_snspan(a, ds.n_cu, ds.stream));
    return APM_OK;
}

// The per-sequence occurrence scan of the ends [own_begin, own_end) n [0, n_total) on ds.stream: one launch, "socc", between the
// main events.  The shard text must bring the occurrence scan's LEFT halo m_max + k and the look-ahead byte: a walk never
// starts farther in front of its first end, and starts later where a sequence begins in between.
int seqocc_scan(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, const apm_seq *d_table, uint64_t n_seq,
                unsigned flags, apm_match *d_out, uint64_t capacity, uint64_t *d_n_found, unsigned long long *d_counts) {
    int rc = check_occ_set(ctx);
    if (rc) return rc;
    if (!n_seq || !d_table) return fail(ctx, APM_ERR_INVALID, "the per-sequence occurrence scan needs a sequence table of at least one sequence");
    if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
    const int m_max = longest_pattern(ctx);
    const uint64_t eb = std::min(own_begin, sh.n_total), ee = std::min(own_end, sh.n_total);
    const uint64_t halo = (uint64_t)(m_max + ctx->k);
    const uint64_t need_lo = eb > halo ? eb - halo : 0, need_hi = std::min(sh.n_total, ee + 1);
    if (ee > eb && (sh.text_off > need_lo || sh.text_off + sh.text_len < need_hi))
        return fail(ctx, APM_ERR_INVALID, "shard text too short: the ends [%llu, %llu) need the bytes [%llu, %llu), a left halo of m_max + k = %llu",
                    (unsigned long long)eb, (unsigned long long)ee, (unsigned long long)need_lo, (unsigned long long)need_hi, (unsigned long long)halo);
    if (ee > eb) rc = ensure_score_image(ctx, ds);
    if (rc) return rc;
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstart, ds.stream));
    if (ee > eb) {
        ApmSeqoccArgs a{};
        a.text = sh.text;
        a.text_off = sh.text_off;
        a.text_len = sh.text_len;
        a.n_total = sh.n_total;
        a.e_begin = eb;
        a.e_end = ee;
        uint64_t S = (uint64_t)apm_occ_segment(m_max, ctx->k, ee - eb, ds.n_cu, (int)ctx->pats.size());
        while ((ee - eb + S - 1) / S > (1ull << 30)) S *= 2; // (the grid's x dimension)
        a.segment = (uint32_t)S;
        a.n_segments = (uint32_t)((ee - eb + S - 1) / S);
        a.image = ds.d_score_img;
        a.table = ds.d_score_tab;
        a.n_patterns = (uint32_t)ctx->pats.size();
        a.k = ctx->k;
        a.m_max = m_max;
        a.flags = flags;
        a.out = reinterpret_cast<uint4 *>(d_out);
        a.cap = capacity;
        a.n_found = reinterpret_cast<unsigned long long *>(d_n_found);
        a.counts = d_counts;
        a.seqs = d_table;
        a.n_seq = n_seq;
        APM_LAUNCH(ctx, ds, "socc", apm_launch_seqocc(a, ds.stream));
        ds.seqocc_segment = a.segment;
        ds.seqocc_lanes = (uint64_t)a.n_segments * a.n_patterns;
        ds.text_bytes += need_hi - need_lo;
    }
    if (ctx->timing_on) HIP_TRY(ctx, hipEventRecord(ds.ev_mstop, ds.stream));
    return APM_OK;
}

// The per-sequence span pass over the ends d_rec[0 .. min(*d_n_rec, capacity)) (apm_seqocc.hip): one launch, "sspan".
int seqocc_span_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_seq *d_table, uint64_t n_seq, const apm_match *d_rec,
                        uint64_t capacity, const uint64_t *d_n_rec, apm_match *d_span, uint32_t *d_seq) {
    int rc = check_occ_set(ctx);
    if (rc) return rc;
    if (!n_seq || !d_table) return fail(ctx, APM_ERR_INVALID, "the per-sequence span pass needs a sequence table of at least one sequence");
    ApmSeqspanArgs a{};
    rc = record_args(ctx, ds, sh, d_rec, capacity, d_n_rec, a);
    if (rc) return rc;
    a.span = reinterpret_cast<uint4 *>(d_span);
    a.seqs = d_table;
    a.n_seq = n_seq;
    a.seq = d_seq;
    APM_LAUNCH(ctx, ds, "sspan", apm_launch_seqspan(a, ds.n_cu, ds.stream));
    return APM_OK;
}

// The occurrence-script pass over the pairs (d_end[r], d_span[r]), r < min(*d_n_rec, capacity) (apm_occ_align.hip).  Its
// trace lives in LDS: there is no workspace, later calls with the same pattern set only launch.
int occ_align_records(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, const apm_match *d_end, const apm_match *d_span, uint64_t capacity,
                      const uint64_t *d_n_rec, uint32_t *d_ops, uint32_t stride) {
    int rc = check_occ_set(ctx);
    if (rc) return rc;
    ApmOccAlignArgs a{};
    rc = record_args(ctx, ds, sh, d_end, capacity, d_n_rec, a);
    if (rc) return rc;
    a.span = reinterpret_cast<const uint4 *>(d_span);
    a.ops = d_ops;
    a.stride = stride;
    APM_LAUNCH(ctx, ds, "oalign", apm_launch_occ_align(a, ds.n_cu, ds.stream));
    return APM_OK;
}

extern "C" {

int apm_align_row_words(const apm_ctx *ctx) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->pats.empty()) return fail(const_cast<apm_ctx *>(ctx), APM_ERR_STATE, "apm_set_patterns has not been called");
    return (int)align_row_words(ctx);
}

int apm_align_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                           const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, uint32_t *d_ops, uint32_t stride_words) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<true>(
        ctx, "apm_align_shard_device", sh, !d_n_rec || ((!d_rec || !d_ops) && capacity), d_rec, "d_rec",
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_ops) & 3u) return fail(ctx, APM_ERR_INVALID, "d_ops must be 4-byte aligned");
            return check_row_stride(ctx, stride_words, false);
        },
        [&](DeviceState &ds) { return align_records(ctx, ds, sh, d_rec, capacity, d_n_rec, d_ops, stride_words); });
}

int apm_score_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                           apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<true>(
        ctx, "apm_score_shard_device", sh, !d_n_rec || (!d_rec && capacity), d_rec, "d_rec", []() { return (int)APM_OK; },
        [&](DeviceState &ds) { return score_records(ctx, ds, sh, d_rec, capacity, d_n_rec); });
}

int apm_best_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                          const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, uint32_t radius,
                          apm_match *d_out, uint64_t out_capacity, uint64_t *d_n_out) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<true>(
        ctx, "apm_best_shard_device", sh, !d_n_rec || !d_n_out || (!d_rec && capacity) || (!d_out && out_capacity), d_rec, "d_rec",
        [&]() {
            if (radius > APM_BEST_MAX_RADIUS) return fail(ctx, APM_ERR_INVALID, "radius %u is beyond APM_BEST_MAX_RADIUS = %d", radius, APM_BEST_MAX_RADIUS);
            if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(ctx, APM_ERR_INVALID, "d_out must be 16-byte aligned");
            const uintptr_t r0 = reinterpret_cast<uintptr_t>(d_rec), o0 = reinterpret_cast<uintptr_t>(d_out);
            if (capacity && out_capacity && r0 < o0 + 16 * out_capacity && o0 < r0 + 16 * capacity)
                return fail(ctx, APM_ERR_INVALID, "d_out overlaps d_rec");
            return (int)APM_OK;
        },
        [&](DeviceState &ds) { return best_records(ctx, ds, sh, d_rec, capacity, d_n_rec, radius, d_out, out_capacity, d_n_out); });
}

int apm_find_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                          uint64_t own_begin, uint64_t own_end, apm_match *d_out, uint64_t capacity, uint64_t *d_n_found,
                          uint64_t *d_counts) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<false>(
        ctx, "apm_find_shard_device", sh, !d_n_found || (!d_out && capacity), d_out, "d_out",
        [&]() { return own_begin > own_end ? fail(ctx, APM_ERR_INVALID, "inconsistent shard description") : (int)APM_OK; },
        [&](DeviceState &ds) {
            ApmPosSink rs{};
            rs.out = reinterpret_cast<unsigned long long *>(d_out);
            rs.count = reinterpret_cast<unsigned long long *>(d_n_found);
            rs.cap = capacity;
            // without d_counts the kernels add into the context's own count vector (what apm_count_buffer zeroes per call)
            const int rc = scan_shard(ctx, ds, sh, own_begin, own_end, d_counts ? (unsigned long long *)d_counts : ds.d_counts, &rs);
            if (!rc) account(ctx, n_total, own_begin, own_end);
            return rc;
        });
}

int apm_occ_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                         uint64_t own_begin, uint64_t own_end, unsigned flags, apm_match *d_out, uint64_t capacity,
                         uint64_t *d_n_found, uint64_t *d_counts) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<false>(
        ctx, "apm_occ_shard_device", sh, !d_n_found || (!d_out && capacity), d_out, "d_out",
        [&]() {
            if (own_begin > own_end) return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
            if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
            return check_occ_set(ctx);
        },
        [&](DeviceState &ds) {
            // without d_counts the kernel adds into the context's own count vector, as the find call's do
            return occ_scan(ctx, ds, sh, own_begin, own_end, flags, d_out, capacity, d_n_found, d_counts ? (unsigned long long *)d_counts : ds.d_counts);
        });
}

int apm_occ_spans_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                         const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, apm_match *d_span) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<true>(
        ctx, "apm_occ_spans_device", sh, !d_n_rec || ((!d_rec || !d_span) && capacity), d_rec, "d_rec",
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_span) & 15u) return fail(ctx, APM_ERR_INVALID, "d_span must be 16-byte aligned");
            return check_occ_set(ctx);
        },
        [&](DeviceState &ds) { return span_records(ctx, ds, sh, d_rec, capacity, d_n_rec, d_span); });
}

int apm_occ_align_row_words(const apm_ctx *ctx) {
    if (!ctx) return APM_ERR_INVALID;
    if (ctx->pats.empty()) return fail(const_cast<apm_ctx *>(ctx), APM_ERR_STATE, "apm_set_patterns has not been called");
    const int rc = check_occ_set(const_cast<apm_ctx *>(ctx));
    return rc ? rc : (int)occ_align_row_words(ctx);
}

int apm_occ_align_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                         const apm_match *d_end, const apm_match *d_span, uint64_t capacity, const uint64_t *d_n_rec, uint32_t *d_ops,
                         uint32_t stride_words) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    return shard_call<true>(
        ctx, "apm_occ_align_device", sh, !d_n_rec || ((!d_end || !d_span || !d_ops) && capacity), d_end, "d_end",
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_span) & 15u) return fail(ctx, APM_ERR_INVALID, "d_span must be 16-byte aligned");
            if (reinterpret_cast<uintptr_t>(d_ops) & 3u) return fail(ctx, APM_ERR_INVALID, "d_ops must be 4-byte aligned");
            const int rc = check_occ_set(ctx);
            return rc ? rc : check_row_stride(ctx, stride_words, true);
        },
        [&](DeviceState &ds) { return occ_align_records(ctx, ds, sh, d_end, d_span, capacity, d_n_rec, d_ops, stride_words); });
}

int apm_nearest_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             uint64_t own_begin, uint64_t own_end, uint64_t *d_keys) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    // (a multi-device context is a limit of the search, APM_ERR_UNSUPPORTED, in all three calls: asked in front of the frame)
    if (ctx && ctx->patterns_set && ctx->devs.size() != 1) return check_nearest_set(ctx, "apm_nearest_shard_device", n_total);
    return shard_call<false>(
        ctx, "apm_nearest_shard_device", sh, !d_keys, nullptr, "",
        [&]() {
            if (own_begin > own_end) return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
            if (reinterpret_cast<uintptr_t>(d_keys) & 7u) return fail(ctx, APM_ERR_INVALID, "d_keys must be 8-byte aligned");
            return check_nearest_set(ctx, "apm_nearest_shard_device", n_total);
        },
        [&](DeviceState &ds) { return nearest_scan(ctx, ds, sh, own_begin, own_end, reinterpret_cast<unsigned long long *>(d_keys)); });
}

int apm_nearest_records_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                               const uint64_t *d_keys, apm_match *d_end, apm_match *d_start) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    if (ctx && ctx->patterns_set && ctx->devs.size() != 1) return check_nearest_set(ctx, "apm_nearest_records_device", n_total);
    return shard_call<true>(
        ctx, "apm_nearest_records_device", sh, !d_keys || !d_end, d_end, "d_end",
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_keys) & 7u) return fail(ctx, APM_ERR_INVALID, "d_keys must be 8-byte aligned");
            if (reinterpret_cast<uintptr_t>(d_start) & 15u) return fail(ctx, APM_ERR_INVALID, "d_start must be 16-byte aligned");
            return check_nearest_set(ctx, "apm_nearest_records_device", n_total);
        },
        [&](DeviceState &ds) { return nearest_records(ctx, ds, sh, reinterpret_cast<const unsigned long long *>(d_keys), d_end, d_start); });
}

// what both per-sequence calls check of their table beyond the nearest search's own limits
static int check_seq_table(apm_ctx *ctx, const char *name, const apm_seq *d_table, uint64_t n_seq, uint64_t n_total) {
    if (!n_seq) return fail(ctx, APM_ERR_INVALID, "%s: n_seq is 0", name);
    if (reinterpret_cast<uintptr_t>(d_table) & 7u) return fail(ctx, APM_ERR_INVALID, "d_table must be 8-byte aligned");
    if (n_seq >= (1ull << 32)) return fail(ctx, APM_ERR_UNSUPPORTED, "%s serves fewer than 2^32 sequences", name);
    return check_nearest_set(ctx, name, n_total);
}

int apm_nearest_seq_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                                 uint64_t own_begin, uint64_t own_end, const apm_seq *d_table, uint64_t n_seq, uint64_t *d_keys) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    if (ctx && ctx->patterns_set && ctx->devs.size() != 1) return check_nearest_set(ctx, "apm_nearest_seq_shard_device", n_total);
    return shard_call<false>(
        ctx, "apm_nearest_seq_shard_device", sh, !d_keys || !d_table, nullptr, "",
        [&]() {
            if (own_begin > own_end) return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
            if (reinterpret_cast<uintptr_t>(d_keys) & 7u) return fail(ctx, APM_ERR_INVALID, "d_keys must be 8-byte aligned");
            return check_seq_table(ctx, "apm_nearest_seq_shard_device", d_table, n_seq, n_total);
        },
        [&](DeviceState &ds) { return seqnear_scan(ctx, ds, sh, own_begin, own_end, d_table, n_seq, reinterpret_cast<unsigned long long *>(d_keys)); });
}

int apm_nearest_seq_records_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                                   const apm_seq *d_table, uint64_t n_seq, const uint64_t *d_keys, apm_match *d_end, apm_match *d_start) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    if (ctx && ctx->patterns_set && ctx->devs.size() != 1) return check_nearest_set(ctx, "apm_nearest_seq_records_device", n_total);
    return shard_call<true>(
        ctx, "apm_nearest_seq_records_device", sh, !d_keys || !d_end || !d_table, d_end, "d_end",
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_keys) & 7u) return fail(ctx, APM_ERR_INVALID, "d_keys must be 8-byte aligned");
            if (reinterpret_cast<uintptr_t>(d_start) & 15u) return fail(ctx, APM_ERR_INVALID, "d_start must be 16-byte aligned");
            return check_seq_table(ctx, "apm_nearest_seq_records_device", d_table, n_seq, n_total);
        },
        [&](DeviceState &ds) {
            return seqnear_records(ctx, ds, sh, d_table, n_seq, reinterpret_cast<const unsigned long long *>(d_keys), d_end, d_start);
        });
}

// what the per-sequence occurrence calls refuse beyond the occurrence search's own set, in `name`'s words
static int check_seqocc(apm_ctx *ctx, const char *name, uint64_t n_total) {
    if (ctx->devs.size() != 1) return fail(ctx, APM_ERR_UNSUPPORTED, "%s needs a single-device context", name);
    if (n_total > APM_NEAREST_MAX_TEXT) return fail(ctx, APM_ERR_UNSUPPORTED, "%s serves texts of at most 2^56 bytes", name);
    return check_occ_set(ctx);
}

static int check_seqocc_table(apm_ctx *ctx, const char *name, const apm_seq *d_table, uint64_t n_seq, uint64_t n_total) {
    if (!n_seq) return fail(ctx, APM_ERR_INVALID, "%s: n_seq is 0", name);
    if (reinterpret_cast<uintptr_t>(d_table) & 7u) return fail(ctx, APM_ERR_INVALID, "d_table must be 8-byte aligned");
    if (n_seq >= (1ull << 32)) return fail(ctx, APM_ERR_UNSUPPORTED, "%s serves fewer than 2^32 sequences", name);
    return check_seqocc(ctx, name, n_total);
}

int apm_occ_seq_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             uint64_t own_begin, uint64_t own_end, const apm_seq *d_table, uint64_t n_seq, unsigned flags,
                             apm_match *d_out, uint64_t capacity, uint64_t *d_n_found, uint64_t *d_counts) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    // (a multi-device context is a limit of the search, APM_ERR_UNSUPPORTED: asked in front of the frame)
    if (ctx && ctx->patterns_set && ctx->devs.size() != 1) return check_seqocc(ctx, "apm_occ_seq_shard_device", n_total);
    return shard_call<false>(
        ctx, "apm_occ_seq_shard_device", sh, !d_n_found || !d_table || (!d_out && capacity), d_out, "d_out",
        [&]() {
            if (own_begin > own_end) return fail(ctx, APM_ERR_INVALID, "inconsistent shard description");
            if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
            return check_seqocc_table(ctx, "apm_occ_seq_shard_device", d_table, n_seq, n_total);
        },
        [&](DeviceState &ds) {
            // without d_counts the kernel adds into the context's own count vector, as the find call's do
            return seqocc_scan(ctx, ds, sh, own_begin, own_end, d_table, n_seq, flags, d_out, capacity, d_n_found,
                               d_counts ? (unsigned long long *)d_counts : ds.d_counts);
        });
}

int apm_occ_seq_spans_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             const apm_seq *d_table, uint64_t n_seq, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                             apm_match *d_span, uint32_t *d_seq) {
    const ShardText sh{(const uint8_t *)d_text, text_off, text_len, n_total};
    if (ctx && ctx->patterns_set && ctx->devs.size() != 1) return check_seqocc(ctx, "apm_occ_seq_spans_device", n_total);
    return shard_call<true>(
        ctx, "apm_occ_seq_spans_device", sh, !d_n_rec || !d_table || ((!d_rec || !d_span) && capacity), d_rec, "d_rec",
        [&]() {
            if (reinterpret_cast<uintptr_t>(d_span) & 15u) return fail(ctx, APM_ERR_INVALID, "d_span must be 16-byte aligned");
            if (reinterpret_cast<uintptr_t>(d_seq) & 3u) return fail(ctx, APM_ERR_INVALID, "d_seq must be 4-byte aligned");
            return check_seqocc_table(ctx, "apm_occ_seq_spans_device", d_table, n_seq, n_total);
        },
        [&](DeviceState &ds) { return seqocc_span_records(ctx, ds, sh, d_table, n_seq, d_rec, capacity, d_n_rec, d_span, d_seq); });
}

} // extern "C"
