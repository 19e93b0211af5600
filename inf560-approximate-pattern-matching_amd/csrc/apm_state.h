/*
 * apm_state.h -- the context behind the C ABI and its per-device state, shared by the runtime units (apm_runtime.hip:
 * life cycle, plan upload, setters, the device-level frame; apm_ingest.hip: the host-level count calls, staging, reduce,
 * text modes; apm_find.hip: the host-level find calls; apm_records.hip: the record passes and their device-level calls;
 * apm_stats.hip: timing and statistics -- what they call of one another is declared in apm_runtime.h) and the shard scan
 * (apm_scan.hip).  Not part of the ABI.
 */
#ifndef APM_STATE_H
#define APM_STATE_H

#include "../../include/apm.h"
#include "apm_plan.h"
#include "apm_sieve.h"
#include "apm_textnorm.h"
#include "apm_seqindex.h"

#include <string>
#include <vector>

struct DevVerify {         // device mirror of one VerifyLaunch
    uint32_t *d_bmp18 = nullptr;   // VerifyLaunch::bitmap18
    uint8_t *d_cf = nullptr;       // VerifyLaunch::cf_image
    ApmPatDesc *d_descs = nullptr;
    uint8_t *d_image = nullptr;
    uint32_t *d_kinfo = nullptr;
    uint32_t *d_pinfo = nullptr;
    uint32_t *d_kpart = nullptr;
    // launch geometry: this device's occupancy answers, asked once per uploaded plan
    int blocks_per_cu = 0, threads = 256;
    int fused_blocks_per_cu = 0, fused_threads = 0; // the same for the fused form (threads < 0: it does not fit a CU)
    int cf_threads = 0, cf_blocks_per_cu = 0;       // ... for the launch's own code-filter sieve pass (threads < 0: does not fit a CU)
};

struct DevTiled {          // device mirror of one TiledLaunch
    ApmPatDesc *d_descs = nullptr;
    uint8_t *d_bytes = nullptr;
    uint32_t *d_tables = nullptr;
    uint8_t *d_lut = nullptr;
    uint8_t *d_image = nullptr;
    int blocks_per_cu[3] = {0, 0, 0}; // BANDED: resident workgroups per CU (occupancy query, asked once per uploaded plan) [tile, tile+dma, stream]
};

struct DeviceState {
    int dev = -1;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    uint8_t *d_allpat = nullptr;              // every pattern's raw bytes, concatenated
    ApmPatDesc *d_tail_descs = nullptr;       // tails of tiled-kernel patterns with m > 128 (generic kernel)
    ApmPatDesc *d_stail_descs = nullptr;      // tails of tiled-kernel patterns with m <= 128 (tail kernel)
    ApmPatDesc *d_wtail_descs = nullptr;      // ... with 128 < m <= 512 (wide tail kernel)
    ApmPatDesc *d_xtail_descs = nullptr;      // ... with 512 < m <= 1024 (32-word tail kernel)
    ApmPatDesc *d_long_descs = nullptr;       // generic full-scan patterns
    int *d_trivial = nullptr;                 // indices of the patterns with k >= m
    std::vector<DevTiled> tiled;
    unsigned long long *d_counts = nullptr;   // P
    uint16_t *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    unsigned long long *d_pos_out = nullptr;   // apm_find_buffer: match positions (cap entries) + 1 counter
    unsigned long long *d_pos_count = nullptr;
    unsigned long long pos_cap = 0;
    unsigned long long *d_rec = nullptr;       // apm_find_all_buffer: this device's (pattern, position) records, kept while large enough
    size_t rec_cap = 0;                        // records allocated
    unsigned long long *d_rec_n = nullptr;     // ... and their counter
    uint8_t *d_score_img = nullptr;            // the scoring pass's image of the patterns (apm_score.h), built by the first scoring
    uint2 *d_score_tab = nullptr;              // call with a pattern set and freed with the plan; {row offset, m} per pattern
    void *d_align_ws = nullptr;                // the align pass's trace workspace (apm_align.h), built by the first align call with a
    uint32_t align_rows = 0;                   // pattern set and freed with the score image; its trace rows (0: not sized yet)
    uint32_t last_align_rows = 0;              // trace rows of the last align launch (statistics; 0: there was none)
    uint32_t *d_ops = nullptr;                 // apm_find_all_align_buffer: this device's rows of ops, kept while large enough
    size_t ops_cap = 0;                        // dwords allocated
    unsigned long long *d_rec2 = nullptr;      // the second record buffer, kept while large enough: best hits, counted in d_rec_n[1]; or
    size_t rec2_cap = 0;                       // the span records of d_rec, counted by d_rec_n[0] (both words are zeroed together)
    hipEvent_t ev_best[2] = {};                // around the last best-hit launch (apm_get_stat "best_ms")
    bool best_timed = false;
    uint32_t occ_segment = 0;                  // the last occurrence scan (apm_occ.h): its segment S and the (segment, pattern)
    uint64_t occ_lanes = 0;                    // walks it launched (statistics; 0: there was none)
    uint32_t nearest_segment = 0;              // the same of the last nearest-occurrence scan (apm_nearest.h)
    uint64_t nearest_lanes = 0;
    unsigned long long *d_nearest_keys = nullptr; // apm_find_nearest_buffer: one key per pattern, kept while large enough
    size_t nearest_keys_cap = 0;
    uint32_t seqnear_segment = 0;              // the same of the last per-sequence nearest scan (apm_seqnear.h)
    uint64_t seqnear_lanes = 0;
    unsigned long long *d_seqnear_keys = nullptr; // apm_find_nearest_seq_buffer: one key per (sequence, pattern), kept while large enough
    size_t seqnear_keys_cap = 0;
    uint32_t seqocc_segment = 0;               // the same of the last per-sequence occurrence scan (apm_seqocc.h)
    uint64_t seqocc_lanes = 0;
    uint32_t *d_seqocc_seq = nullptr;          // apm_find_occ_seq_buffer: every record's sequence, kept while large enough
    size_t seqocc_seq_cap = 0;
    uint8_t *d_text = nullptr;
    size_t text_cap = 0;
    uint8_t *d_raw = nullptr;                  // text modes (apm_set_text_mode): the staged source bytes, normalised into d_text
    size_t raw_cap = 0;
    // the text-normalisation pass (apm_textnorm.h): its map, kept for apm_map_positions_device, and what the last pass saw
    uint32_t *d_tn_summary = nullptr;          // one dword per 4 KiB source block, allocated in whole chunks of the scan
    unsigned long long *d_tn_map = nullptr;    // tn_cap + 1 entries
    unsigned long long *d_tn_total = nullptr;  // the kept total, for the host
    size_t tn_cap = 0;                         // source blocks allocated
    ApmTnSrc tn_src{};                         // the last normalisation's source (tn_valid: there was one and it went through)
    bool tn_valid = false;
    uint64_t tn_src_bytes = 0, tn_kept_bytes = 0;
    hipEvent_t ev_tn[4] = {};                  // around the pass's three launches [0, 1], around the map launch [2, 3]
    bool tn_timed = false, map_timed = false;  // ... recorded by the last pass / the last map launch
    // the sequence index (apm_seqindex.h) of the last normalisation: scratch of its passes, the context's own table
    uint32_t *d_sq_count = nullptr;            // header opens per source block, allocated in whole chunks of the scan
    unsigned long long *d_sq_prefix = nullptr; // sq_cap + 1 entries
    unsigned long long *d_sq_total = nullptr;  // the opens' total, for the host
    size_t sq_cap = 0;                         // source blocks allocated
    uint64_t sq_n_seq = 0;                     // n_seq of the last index pass (statistics)
    bool tn_host = false;                      // the last normalisation was a host-level call's: its source is d_raw
    apm_seq *d_seq_table = nullptr;            // apm_locate_buffer, apm_get_sequences: the table of that source, seq_table_cap entries,
    size_t seq_table_cap = 0;                  // built once per normalisation (seq_table_n: its n_seq; 0: not built)
    uint64_t seq_table_n = 0;
    uint8_t *d_loc_buf = nullptr;              // apm_locate_buffer: a counter, the uploaded records and their locations
    size_t loc_buf_cap = 0;                    // 16-byte units allocated
    hipEvent_t ev_sq[4] = {};                  // around the index pass's three launches [0, 1], around the locate launch [2, 3]
    bool sq_timed = false, locate_timed = false;
    hipEvent_t ev_stage[32] = {};             // apm_count_buffer, apm_count_file: staging buffer b copied out (this device's stream)
    uint32_t *d_sieve_bmp = nullptr;           // sieve bitmap of the whole set (32 KiB)
    std::vector<DevVerify> verify;
    uint32_t *d_masks = nullptr;               // the sieve's hit masks: one dword per lane and 4 KiB block (n / 16 bytes)
    size_t masks_cap = 0;                      // dwords
    int64_t last_mask_blocks = 0;              // blocks the last call's sieve wrote (statistics)
    uint32_t *d_work = nullptr;                // block-distribution counters of the verify / fused launches (ApmVerifyArgs::work)
    int work_epoch = 0;
    uint32_t *d_blist = nullptr;               // the sieve's list of non-empty blocks (one dword per 4 KiB block at most)
    size_t blist_cap = 0;
    int sieve_epoch = 0;                       // which of the two list counters the next sieve launch counts in
    uint32_t *d_clist = nullptr;               // the sieve's candidate list (ApmSieve2Args::clist) and its per-region counts
    uint32_t *d_clist_cnt = nullptr;
    size_t clist_cap = 0;                      // entries allocated
    int last_clist_regions = 0;                // the last sieve pass ran with the list: its regions and block-list counter (statistics)
    const uint32_t *last_blist_ctr = nullptr;
    uint32_t *d_cpool = nullptr;               // the list's pooled hand-over (ApmSieve2PoolArgs::cpool) and its two sets of kClistMaxRegions counters
    uint32_t *d_cpool_cnt = nullptr;
    size_t cpool_cap = 0;                      // entries allocated
    int pool_epoch = 0;                        // which set of pool counters the next pooled sieve launch counts in
    int pool_dirty[2] = {0, 0};                // counters of each set that may be non-zero (the pools of the last launch that counted in it)
    int last_clist_pools = 0;                  // pools of the last sieve pass (statistics; 0: it handed its regions over as they were)
    unsigned long long *d_stats = nullptr;     // 8 counters (statistics kernel; measurement build: verify counters)
    int last_sieve_waves = 0;                  // scanning waves of the last code-filter sieve pass (statistics; 0: the last pass was none)
    int last_cf_dp_form = 0;                   // ... and the form of its window DP on codes (apm_cf_dp_form)
    bool last_fused = false;                  // the last call used the fused form of the pipeline
    hipEvent_t ev_start = nullptr, ev_kstart = nullptr, ev_mstart = nullptr, ev_mstop = nullptr, ev_stop = nullptr;
    bool events_recorded = false;
    // per-launch event stamps (apm_get_launch_times): stamp i is recorded right behind scan launch i, so the time
    // between two stamps is one launch as the stream saw it (the first one is measured from ev_mstart)
    static constexpr int MAX_STAMPS = 32;
    hipEvent_t ev_launch[MAX_STAMPS] = {};
    const char *launch_label[MAX_STAMPS] = {};
    int n_stamps = 0;
    // per-call accounting
    uint64_t text_bytes = 0;
    int launches = 0;
};

struct RcclApi {
    void *handle = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    std::vector<void *> comms;
    bool ready = false;
};

struct apm_ctx {
    std::vector<DeviceState> devs;
    std::vector<PatternInfo> pats;
    ApmPlan plan;            // of pats at distance k under `kernel` (apm_build_plan), uploaded to every device
    int k = 0;
    int kernel = APM_KERNEL_AUTO;
    bool patterns_set = false;
    bool timing_on = true;   // hipEvent bracketing of every call (apm_set_timing)
    bool find_active = false; // apm_find_buffer in progress: kernels also push match positions
    unsigned text_mode = 0;   // apm_set_text_mode: APM_TEXT_* flags the host-level calls normalise their text with (0: verbatim)
    std::string err;
    apm_timing timing{};
    RcclApi rccl;
    bool multi = false; // created by apm_create (single process, >=1 devices)
    // PATTERN-SHARDED partition (apm_set_partition): one single-device child context per device, child g holds the patterns
    // [pat_first[g], pat_first[g + 1]) and scans the WHOLE text; the count vectors are disjoint, nothing is reduced
    int partition = APM_PARTITION_TEXT;
    std::vector<apm_ctx *> children;
    std::vector<int> pat_first; // children.size() + 1 entries
    // apm_count_buffer, apm_count_file: pinned staging ring (kept for the life of the context) and its "copied out" events
    static constexpr int N_STAGE = 32;                 // two per reader thread, allocated on first use
    static constexpr size_t STAGE_BYTES = (size_t)8 << 20;
    uint8_t *stage[N_STAGE] = {};
};

// records the message in the context (ctx == NULL: as the creating thread's error) and returns code (apm_runtime.hip)
int fail(apm_ctx *ctx, int code, const char *fmt, ...);

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail(ctx, APM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

// bookkeeping behind every scan-kernel launch: count it and, with timing on, stamp the stream (apm_scan.hip)
int note_launch(apm_ctx *ctx, DeviceState &ds, const char *label);

// one scan-kernel launch: the launcher call under HIP_TRY, then its bookkeeping under `label`
#define APM_LAUNCH(ctx, ds, label, expr)                 \
    do {                                                 \
        HIP_TRY(ctx, expr);                              \
        const int _nrc = note_launch(ctx, ds, label);    \
        if (_nrc) return _nrc;                           \
    } while (0)

// One shard's text as every device-level call describes it: text[0 .. text_len) holds the bytes [text_off, text_off +
// text_len) of a whole text of n_total bytes
struct ShardText {
    const uint8_t *text;
    uint64_t text_off, text_len, n_total;
};

// Scans the window starts [own_begin, own_end) of the shard text on ds.stream, no host sync (apm_scan.hip); rec: the
// record sink of the find calls (its text_off is set per piece), NULL: count only
int scan_shard(apm_ctx *ctx, DeviceState &ds, const ShardText &sh, uint64_t own_begin, uint64_t own_end, unsigned long long *d_counts,
               const ApmPosSink *rec = nullptr);
// statistics: hits of the last call's sieve on this device (apm_scan.hip; synchronises with the stream)
int sieve_candidates(apm_ctx *ctx, DeviceState &ds, double *value);
// makes ds.d_text hold at least `bytes` (apm_scan.hip)
int ensure_text(apm_ctx *ctx, DeviceState &ds, size_t bytes);

// THE way a device buffer grows with the calls (apm_runtime.hip): *ptr holds *cap elements of elem_bytes, make that at
// least `want`; the contents are not kept.  The current device is ds.dev.
//  - a buffer that is large enough is not touched;
//  - one that is too small is freed only behind hipStreamSynchronize(ds.stream): a launch of an earlier call may still read it;
//  - *ptr and *cap are zeroed before the new allocation, so a failed call leaves a consistent state.
// A failed allocation returns `status` with "cannot allocate <noun>", noun_fmt being the noun's printf format; without a
// noun it is reported like any failed HIP call (APM_ERR_HIP).  Two callers add a rule of their own: stage_normalized
// clears tn_valid when d_raw is replaced, ensure_tn_map rounds to whole 4096-block chunks and grows its two buffers together.
__attribute__((visibility("hidden"))) int grow_device_buffer(apm_ctx *ctx, DeviceState &ds, void **ptr, size_t *cap, size_t want, size_t elem_bytes,
                                                             int status = APM_ERR_HIP, const char *noun_fmt = nullptr, ...);

#endif /* APM_STATE_H */
