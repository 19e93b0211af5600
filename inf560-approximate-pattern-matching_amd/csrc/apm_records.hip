/*
 * apm_records.hip -- the calls that report matches instead of counting them: the record passes over finished match
 * records (scoring, apm_score.hip; align, apm_align.hip; best hits, apm_best.hip; spans, apm_occ.hip; occurrence scripts, apm_occ_align.hip) with their device-level
 * entry points, the device-level find call, the occurrence scan (apm_occ.hip), and the host-level find calls, which download and merge what every device (or child context) found.
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

#include <cstring>
#include <string>
#include <vector>

namespace {

// the half-band the scoring pass needs for ctx->pats at ctx->k, refused beyond what the wave form's LDS band holds
int check_score_band(apm_ctx *ctx) {
    const int band = std::min(ctx->k / 2, longest_pattern(ctx) - 1);
    if (ctx->k > APM_SCORE_LANE_MAX_K && band > APM_SCORE_MAX_BAND)
        return fail(ctx, APM_ERR_UNSUPPORTED, "scoring serves a half-band min(k/2, m_max-1) of at most %d diagonals, this pattern set needs %d",
                    APM_SCORE_MAX_BAND, band);
    return APM_OK;
}

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

} // namespace

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

// dwords of one pair's row of ops for ctx->pats at ctx->k (a set check_occ_set accepts): the count and m_max + k ops
static uint32_t occ_align_row_words(const apm_ctx *ctx) { return (uint32_t)apm_occ_align_row_words_of(longest_pattern(ctx), ctx->k); }

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

static bool match_less(const apm_match &a, const apm_match &b) { return a.pattern != b.pattern ? a.pattern < b.pattern : a.pos < b.pos; }

// apm_find_all_buffer; mode FIND_DIST: apm_find_all_dist_buffer, every device (every child) scores its records before they
// leave it; FIND_ALIGN: apm_find_all_align_buffer, and aligns them into rows of `stride` dwords, which travel with their
// records through the (pattern, pos) sort as an index permutation
static int find_all(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity, uint64_t *n_found, FindMode mode,
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
        const FindRequest find{capacity, mode, stride};
        int rc = mode != FIND_PLAIN ? check_score_band(ctx) : APM_OK; // (refused before anything is scanned)
        if (!rc) rc = count_host_text(ctx, text, n, counts.data(), &find);
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

extern "C" {

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

// The scan is find_all's FIND_PLAIN on the single device; behind it, on the same stream, the best-hit pass from the
// context's record buffer into its best-hit buffer, the align pass over the best hits (ops != NULL) and, in a text mode, the
// position map over them.  Only the best hits are downloaded.
int apm_find_best_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t radius, apm_match *out, uint64_t capacity,
                         uint64_t *n_best, uint64_t *n_matches, uint32_t *ops, uint32_t stride_words) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!n_best || !n_matches || (!out && capacity) || (!text && n)) return fail(ctx, APM_ERR_INVALID, "bad argument to apm_find_best_buffer");
    if (radius > APM_BEST_MAX_RADIUS) return fail(ctx, APM_ERR_INVALID, "radius %u is beyond APM_BEST_MAX_RADIUS = %d", radius, APM_BEST_MAX_RADIUS);
    if (ctx->devs.size() != 1)
        return fail(ctx, APM_ERR_UNSUPPORTED, "apm_find_best_buffer needs a single-device context: the resident shards' halo is m_max - 1, the pass needs "
                                              "the radius more on both sides");
    if (ops && stride_words < align_row_words(ctx))
        return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than apm_align_row_words() = %u", stride_words, align_row_words(ctx));
    const uint32_t stride = ops ? stride_words : 0;
    std::vector<uint64_t> counts(ctx->pats.size(), 0);
    FindRequest find{capacity, FIND_BEST, stride};
    find.radius = radius;
    int rc = check_score_band(ctx); // (refused before anything is scanned)
    if (!rc) rc = count_host_text(ctx, text, n, counts.data(), &find);
    if (rc) return rc;
    uint64_t csum = 0;
    for (uint64_t c : counts) csum += c;
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    apm_match *d_kept = reinterpret_cast<apm_match *>(ds.d_best);
    const uint64_t *d_n_kept = reinterpret_cast<const uint64_t *>(ds.d_rec_n + 1);
    if (ctx->text_mode) { // positions in the normalised text -> source offsets, behind scan, best and align
        rc = map_positions_on_stream(ctx, ds, d_kept, capacity, d_n_kept);
        if (rc) return rc;
    }
    unsigned long long c[2] = {0, 0}; // {records, best hits}
    HIP_TRY(ctx, hipMemcpyAsync(c, ds.d_rec_n, 16, hipMemcpyDeviceToHost, ds.stream));
    HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    if (c[0] != csum) return fail(ctx, APM_ERR_STATE, "record sink count %llu != match count %llu", c[0], (unsigned long long)csum);
    const size_t take = (size_t)std::min<uint64_t>(c[1], capacity);
    std::vector<apm_match> all(take);
    std::vector<uint32_t> rows((size_t)take * stride);
    if (take) HIP_TRY(ctx, hipMemcpy(all.data(), ds.d_best, take * sizeof(apm_match), hipMemcpyDeviceToHost));
    if (take && stride) HIP_TRY(ctx, hipMemcpy(rows.data(), ds.d_ops, take * stride * 4, hipMemcpyDeviceToHost));
    std::vector<size_t> perm(take);
    for (size_t i = 0; i < take; ++i) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](size_t x, size_t y) { return match_less(all[x], all[y]); });
    for (size_t i = 0; i < take; ++i) {
        out[i] = all[perm[i]];
        if (!stride) continue;
        const uint32_t *row = rows.data() + perm[i] * stride; // (the words the row format defines, as find_all copies them)
        const size_t used = row[0] == APM_DIST_INVALID ? 1 : std::min<size_t>((size_t)apm_align_words((int)row[0]), stride);
        memcpy(ops + i * stride, row, used * 4);
    }
    *n_matches = c[0];
    *n_best = c[1];
    return APM_OK;
}

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
            if (stride_words < align_row_words(ctx))
                return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than apm_align_row_words() = %u", stride_words, align_row_words(ctx));
            return (int)APM_OK;
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

// One occurrence scan of the whole text on the single device into the context's record buffer; with out_start the span
// pass from there into its second record buffer (the best-hit call's); with ops (apm_find_occ_align_buffer, `name` says
// which call this is) the occurrence-script pass over both into the context's rows of ops; in a text mode the position
// map over both record buffers, behind all three.  capacity == 0 counts only.
static int find_occ(apm_ctx *ctx, const char *name, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end, apm_match *out_start,
                    uint64_t capacity, uint64_t *n_found, uint64_t *counts, bool scripts, uint32_t *ops, uint32_t stride) {
    if (!ctx) return APM_ERR_INVALID;
    if (!ctx->patterns_set) return fail(ctx, APM_ERR_STATE, "apm_set_patterns has not been called");
    if (!n_found || (!out_end && capacity) || (!text && n) || (scripts && capacity && (!out_start || !ops))) // (the script call needs starts and rows)
        return fail(ctx, APM_ERR_INVALID, "bad argument to %s", name);
    if (flags & ~APM_OCC_LOCAL_MIN) return fail(ctx, APM_ERR_INVALID, "unknown occurrence flags 0x%x", flags);
    if (ctx->devs.size() != 1)
        return fail(ctx, APM_ERR_UNSUPPORTED, "%s needs a single-device context: the resident shards bring a right halo, the "
                                              "occurrence scan needs a left one", name);
    int rc = check_occ_set(ctx); // (refused before anything is staged)
    if (rc) return rc;
    if (scripts && stride < occ_align_row_words(ctx))
        return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than apm_occ_align_row_words() = %u", stride, occ_align_row_words(ctx));
    if (scripts && !capacity) out_start = nullptr; // (a count only: neither spans nor scripts)
    std::vector<uint64_t> cnt(ctx->pats.size(), 0);
    FindRequest find{capacity, FIND_OCC, out_start ? 1u : 0u};
    find.radius = flags;
    find.occ_stride = scripts && out_start ? stride : 0u;
    rc = count_host_text(ctx, text, n, cnt.data(), &find);
    if (rc) return rc;
    DeviceState &ds = ctx->devs[0];
    HIP_TRY(ctx, hipSetDevice(ds.dev));
    apm_match *d_end = reinterpret_cast<apm_match *>(ds.d_rec), *d_start = reinterpret_cast<apm_match *>(ds.d_best);
    const uint64_t *d_n = reinterpret_cast<const uint64_t *>(ds.d_rec_n);
    if (ctx->text_mode) { // positions in the normalised text -> source offsets, behind scan and span
        rc = map_positions_on_stream(ctx, ds, d_end, capacity, d_n);
        if (!rc && out_start) rc = map_positions_on_stream(ctx, ds, d_start, capacity, d_n);
        if (rc) return rc;
    }
    unsigned long long c = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&c, ds.d_rec_n, 8, hipMemcpyDeviceToHost, ds.stream));
    HIP_TRY(ctx, hipStreamSynchronize(ds.stream));
    uint64_t csum = 0;
    for (uint64_t v : cnt) csum += v;
    if (c != csum) return fail(ctx, APM_ERR_STATE, "record sink count %llu != occurrence count %llu", c, (unsigned long long)csum);
    const size_t take = (size_t)std::min<uint64_t>(c, capacity);
    std::vector<apm_match> ends(take), starts(out_start ? take : 0);
    if (take) HIP_TRY(ctx, hipMemcpy(ends.data(), ds.d_rec, take * sizeof(apm_match), hipMemcpyDeviceToHost));
    if (take && out_start) HIP_TRY(ctx, hipMemcpy(starts.data(), ds.d_best, take * sizeof(apm_match), hipMemcpyDeviceToHost));
    std::vector<uint32_t> rows(find.occ_stride ? take * stride : 0);
    if (!rows.empty()) HIP_TRY(ctx, hipMemcpy(rows.data(), ds.d_ops, rows.size() * 4, hipMemcpyDeviceToHost));
    std::vector<size_t> perm(take);
    for (size_t i = 0; i < take; ++i) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](size_t x, size_t y) { return match_less(ends[x], ends[y]); });
    for (size_t i = 0; i < take; ++i) {
        out_end[i] = ends[perm[i]];
        if (out_start) out_start[i] = starts[perm[i]];
        if (rows.empty()) continue;
        const uint32_t *row = rows.data() + perm[i] * stride; // (the words the row format defines, as find_all copies them)
        const size_t used = row[0] == APM_DIST_INVALID ? 1 : std::min<size_t>((size_t)apm_align_words((int)row[0]), stride);
        memcpy(ops + i * stride, row, used * 4);
    }
    *n_found = c;
    if (counts) memcpy(counts, cnt.data(), cnt.size() * sizeof(uint64_t));
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
            if (rc) return rc;
            if (stride_words < occ_align_row_words(ctx))
                return fail(ctx, APM_ERR_INVALID, "stride_words %u is less than apm_occ_align_row_words() = %u", stride_words, occ_align_row_words(ctx));
            return (int)APM_OK;
        },
        [&](DeviceState &ds) { return occ_align_records(ctx, ds, sh, d_end, d_span, capacity, d_n_rec, d_ops, stride_words); });
}

} // extern "C"
