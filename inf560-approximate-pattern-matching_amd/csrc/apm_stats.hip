/*
 * apm_stats.hip -- what a call leaves behind for its caller to read: the per-call accounting (begin_call, account), the
 * event times (apm_get_timing, apm_get_launch_times) and the named statistics (apm_get_stat).
 */
#include "apm_runtime.h"
#include "apm_core.h"

#include <cstdlib>
#include <string>
#include <vector>

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

extern "C" {

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
    if (n == "sieve_cf_dp_form") { *value = (double)ds.last_cf_dp_form; return APM_OK; } // (as the last sieve pass launched it: 0 no window DP on codes, 1 column form, 2 diagonal form)
    if (n == "sieve_cf_waves_per_cu") { *value = (S.per_launch_sieve && G0.cf_threads >= 64) ? (double)(G0.cf_threads / 64 * G0.cf_blocks_per_cu) : 0.0; return APM_OK; }
    if (n == "sieve_cf_bytes") { *value = S.per_launch_sieve ? (double)S.launches[0].cf_image.size() : 0.0; return APM_OK; }
    if (n == "sieve_stride") { *value = S.on ? (double)S.stride : 0.0; return APM_OK; }
    if (n == "sieve_clist") { *value = ds.last_clist_regions ? 1.0 : 0.0; return APM_OK; }
    if (n == "sieve_clist_pools") { *value = (double)ds.last_clist_pools; return APM_OK; } // (pools the last sieve pass moved its list regions into; 0: the regions as they are -- switched off, or not the diagonal kernel)
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
    if (n == "seq_count") { *value = (double)ds.sq_n_seq; return APM_OK; }
    if (n == "seq_index_ms" || n == "locate_ms") { // (HIP events around the index pass's three launches / the locate launch; 0: not timed)
        const int at = n == "seq_index_ms" ? 0 : 2;
        *value = 0.0;
        if (at == 0 ? ds.sq_timed : ds.locate_timed) {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            HIP_TRY(ctx, hipEventSynchronize(ds.ev_sq[at + 1]));
            float t = 0;
            HIP_TRY(ctx, hipEventElapsedTime(&t, ds.ev_sq[at], ds.ev_sq[at + 1]));
            *value = t;
        }
        return APM_OK;
    }
    if (n == "occ_segment") { *value = (double)ds.occ_segment; return APM_OK; } // (S of the last occurrence scan; 0: there was none)
    if (n == "occ_lanes") { *value = (double)ds.occ_lanes; return APM_OK; }     // (the (segment, pattern) walks it launched)
    if (n == "nearest_segment") { *value = (double)ds.nearest_segment; return APM_OK; } // (the same of the last nearest-occurrence scan)
    if (n == "nearest_lanes") { *value = (double)ds.nearest_lanes; return APM_OK; }
    if (n == "seqnear_segment") { *value = (double)ds.seqnear_segment; return APM_OK; } // (the same of the last per-sequence nearest scan)
    if (n == "seqnear_lanes") { *value = (double)ds.seqnear_lanes; return APM_OK; }
    if (n == "seqocc_segment") { *value = (double)ds.seqocc_segment; return APM_OK; } // (the same of the last per-sequence occurrence scan)
    if (n == "seqocc_lanes") { *value = (double)ds.seqocc_lanes; return APM_OK; }
    if (n == "best_ms") { // (HIP events around the last best-hit launch; 0: not timed)
        *value = 0.0;
        if (ds.best_timed) {
            HIP_TRY(ctx, hipSetDevice(ds.dev));
            HIP_TRY(ctx, hipEventSynchronize(ds.ev_best[1]));
            float t = 0;
            HIP_TRY(ctx, hipEventElapsedTime(&t, ds.ev_best[0], ds.ev_best[1]));
            *value = t;
        }
        return APM_OK;
    }
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

} // extern "C"
