/*
 * include/apm.h -- C ABI of the MI355X approximate-pattern-matching engine.
 *
 * This is the drop-in boundary for ONE path of
 * linomp/INF560-approximate-pattern-matching: the Levenshtein sliding-window
 * DP + per-pattern match count
 *     levenshtein()                    /root/reference/src/utils.c:76-99
 *     per-pattern scan loop            /root/reference/src/sequential.c:105-144
 * and it replaces the reference's hand-declared extern "C" GPU shim
 *     getDeviceCount / setDevice       src/cuda_utils.cu:10-35
 *     invoke_kernel / write_kernel_result   src/patterns_over_ranks.cu:75-134
 *     initializeGPU / getGPUResult     src/database_over_ranks.cu:137-205
 * (prototypes re-declared at src/main.c:18-19, src/patterns_over_ranks.c:33-36,
 *  src/database_over_ranks.c:18-22).
 *
 * Conventions
 *   - plain C linkage, pointers + sizes only, no C++/torch types;
 *   - every function returns APM_OK (0) or a negative apm_status and NEVER
 *     calls exit(); apm_last_error() gives the message;
 *   - the library owns all device memory it allocates; caller buffers are
 *     borrowed for the duration of the call;
 *   - counts are uint64 (the reference uses int, src/sequential.c:32); values
 *     are identical whenever they fit in int;
 *   - one apm_ctx per host thread (thread-compatible, not thread-safe);
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with APM_ERR_NO_DEVICE.
 *
 * Semantics (pinned by tests/golden/golden.json, produced by the reference):
 *   counts[i] = #{ j in [0, n-k) : dist(pattern_i[0:size], text[j:j+size]) <= k },
 *   size = min(m_i, n-j), dist = square global unit-cost Levenshtein distance,
 *   bytes compared verbatim (newlines are ordinary bytes).  That is the default; apm_set_text_mode opts into a
 *   normalised text (FASTA headers and line breaks dropped, case folded) with positions reported as source offsets.
 */
#ifndef APM_H
#define APM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APM_ABI_VERSION 1

typedef enum apm_status {
    APM_OK = 0,
    APM_ERR_INVALID = -1,     /* bad argument (NULL, negative k, empty pattern ...) */
    APM_ERR_NO_DEVICE = -2,   /* no HIP device / device index out of range */
    APM_ERR_HIP = -3,         /* a HIP runtime call failed */
    APM_ERR_IO = -4,          /* open/read failed (apm_count_file) */
    APM_ERR_NOMEM = -5,
    APM_ERR_UNSUPPORTED = -6, /* e.g. pattern longer than APM_MAX_PATTERN_LEN,
                                 or a kernel variant that cannot run this (m,k) */
    APM_ERR_COMM = -7,        /* RCCL failure in single-process multi-GPU mode */
    APM_ERR_STATE = -8        /* call order (patterns not set, ...) */
} apm_status;

/* Kernel variants.  Every variant returns the SAME exact counts; they differ
 * in how many DP cells they really evaluate.
 *   WAVEFRONT  full m x m DP, lanes own pattern rows, anti-diagonal sweep with
 *              DPP/__shfl column passing (the kernel BASELINE.json names)
 *   BITPAR     full m x m DP, Myers/Hyyro bit-vector columns (32 DP cells per
 *              integer op), exact distance: one window per lane with columns of
 *              up to 32 words (m <= 1024), one window per wavefront beyond
 *              (m <= 4096; the pattern's distinct bytes x 64 or 128 words of Eq
 *              rows must fit 60 KiB of LDS, else GENERIC)
 *   BANDED     exact for the predicate dist<=k: only diagonals |x-y|<=k/2,
 *              early exit, candidates pre-filtered by pigeonhole sub-keys looked up
 *              in LDS tables (needs m<=512, k<=7, m/(k+1)>=4)
 *   NFA        exact for the predicate dist<=k, no filter: the k-error automaton over
 *              the diagonals |x-y|<=k/2, 32 consecutive window starts per lane as
 *              the bits of a word (needs m + k/2 <= 32, k <= 7, <= 16 distinct
 *              pattern bytes); AUTO's choice for short patterns with many errors,
 *              whose pieces are too short for BANDED's filter
 *   GENERIC    literal one-column DP per lane, any m, handles truncated tails
 *   AUTO       fastest applicable exact variant per pattern (default)        */
typedef enum apm_kernel {
    APM_KERNEL_AUTO = 0,
    APM_KERNEL_GENERIC = 1,
    APM_KERNEL_WAVEFRONT = 2,
    APM_KERNEL_BITPAR = 3,
    APM_KERNEL_BANDED = 4,
    APM_KERNEL_NFA = 5
} apm_kernel;

#define APM_MAX_PATTERN_LEN 65535
#define APM_MAX_PATTERNS 65536

typedef struct apm_ctx apm_ctx;

/* Filled by the counting calls (host wall-clock + HIP-event times). */
typedef struct apm_timing {
    double total_ms;        /* host wall clock of the call */
    double h2d_ms;          /* host->device copies (0 for device-resident text) */
    double kernel_ms;       /* HIP events around all kernels of the call, max over devices */
    double reduce_ms;       /* cross-device count reduction */
    double main_kernel_ms;  /* HIP events around the dominant scan kernel(s) only */
    uint64_t text_bytes;    /* bytes of text scanned (sum over devices, halos included) */
    uint64_t windows;       /* (position, pattern) pairs decided */
    double cells_algorithmic; /* sum over windows of size^2 (the BASELINE metric's numerator) */
    double cells_evaluated;   /* DP cells the chosen kernels really computed (estimate for
                                 data-dependent early exit: upper bound) */
    int n_devices;
    int n_launches;         /* scan-kernel launches in the call */
} apm_timing;

/* ---- device probe: replaces getDeviceCount/setDevice (src/cuda_utils.cu:10-35) ---- */
int apm_device_count(void);                  /* >=0, or negative apm_status */
int apm_abi_version(void);

/* ---- context ---- */
/* Single process driving devices 0..n_devices-1 (the CLI's mode): text is
 * sharded over the devices with an (m_max-1)-byte halo and partial counts are
 * summed with one RCCL all-reduce (falls back to a host sum of the P-vectors
 * if librccl cannot be loaded).  n_devices<=0: all visible devices. */
int apm_create(apm_ctx **ctx, int n_devices);
/* One device only (the one-process-per-GPU mode used under torchrun). */
int apm_create_on_device(apm_ctx **ctx, int device_id);
void apm_destroy(apm_ctx *ctx);
const char *apm_last_error(const apm_ctx *ctx); /* ctx may be NULL: last create error */

/* Use an existing HIP stream (hipStream_t passed as void*) for all work of a
 * single-device context, e.g. torch's current stream.  NULL is HIP's null
 * (legacy default) stream; APM_STREAM_OWN restores the context's own stream.
 * The context owns device scratch (candidate list, hit masks, block-distribution counters, staging) that consecutive calls reuse in
 * stream order: when the stream is changed while earlier calls may still run, the caller orders the two streams
 * (event or synchronisation) first. */
#define APM_STREAM_OWN ((void *)(intptr_t)-1)
int apm_set_stream(apm_ctx *ctx, void *hip_stream);

/* ---- patterns: replaces the pattern/size uploads of initializeGPU
 *      (src/database_over_ranks.cu:157-169) and invoke_kernel (:79-94) ---- */
/* pat[i] need not be NUL terminated; len[i] >= 1; k >= 0. */
int apm_set_patterns(apm_ctx *ctx, int n_patterns, const char *const *pat,
                     const int *len, int k);
int apm_set_kernel(apm_ctx *ctx, int kernel /* apm_kernel */);
/* How a multi-device context (apm_create, more than one device) divides the work.
 *   APM_PARTITION_TEXT      (default) the text is cut into owner ranges with a halo, every device scans its range for
 *                           all patterns, the partial counts are summed (RCCL all-reduce): the replacement of the
 *                           reference's DB_OVER_RANKS (src/database_over_ranks.c:141-195), without its seam over-count
 *   APM_PARTITION_PATTERNS  the pattern list is cut into contiguous slices, every device scans the WHOLE text for its
 *                           slice, nothing is reduced: the replacement of PATTERNS_OVER_RANKS
 *                           (src/patterns_over_ranks.c:160-182); pays when the text is short and the patterns are many
 * Counts are the same either way.  No effect on single-device contexts.  The device-pointer entry points
 * (apm_count_shard_device, apm_set_stream) remain single-device calls. */
#define APM_PARTITION_TEXT 0
#define APM_PARTITION_PATTERNS 1
int apm_set_partition(apm_ctx *ctx, int partition);

/* ---- text modes: search the sequence, not the file layout ----
 * The default compares the bytes of the text verbatim (the reference's contract).  A text mode normalises the text ON THE
 * DEVICE first and searches what is kept; flags, OR-able:
 *   APM_TEXT_FASTA  a line start is offset 0 and every offset right behind a '\n'; a '>' AT A LINE START opens a header that
 *                   runs up to and including the next '\n' (or to the end of the source) and is dropped; outside headers
 *                   '\n' and '\r' are dropped; a '>' elsewhere is an ordinary byte.  The records of a multi-record file are
 *                   simply concatenated: no separator is put between them, so a window may span two records --
 *                   apm_locate_buffer / apm_locate_records_device (below: "sequences") flag such a window.
 *   APM_TEXT_UPPER  kept bytes 'a'..'z' become 'A'..'Z'; every other byte value is unchanged.
 * With T = the kept bytes in order and src_of(c) = the source offset of T[c]: counts, records, distances and scripts in a
 * text mode are exactly what the calls give on T (the truncated tail windows at the end of T included), except that
 * apm_match.pos = src_of(position in T).  src_of is strictly increasing, so the (pattern, pos) order is that of T. */
#define APM_TEXT_FASTA 1u
#define APM_TEXT_UPPER 2u
/* The mode of apm_count_buffer, apm_count_file, apm_find_all_buffer, apm_find_all_dist_buffer and
 * apm_find_all_align_buffer on a single-device context; 0 (the default): off.  The raw bytes are staged as before, into a
 * second device buffer, normalised into the text buffer (apm_normalize_device: three launches and one stream
 * synchronisation), scanned as a text of the normalised length, and the find calls map their records' positions with one
 * more launch before they are downloaded.  apm_timing describes the scan of the normalised text (text_bytes, windows,
 * kernel_ms, n_launches as without a mode; the staging and the pass precede h2d_ms, total_ms covers them); the pass's
 * own figures are apm_get_stat's "norm_*" and "map_ms".  With a mode set, apm_find_buffer and apm_count_synthetic
 * return APM_ERR_UNSUPPORTED; the shard-level device calls ignore the mode: they take the text they are given.
 * Unknown bits: APM_ERR_INVALID.  A multi-device context (apm_create with more than one device, either partition)
 * refuses a non-zero mode with APM_ERR_UNSUPPORTED: its owner ranges depend on a length that is known only after the pass.
 * Multi-device text modes are deliberately out of scope. */
int apm_set_text_mode(apm_ctx *ctx, unsigned flags);

/* ---- whole-text counting: replaces invoke_kernel+write_kernel_result and
 *      initializeGPU+getGPUResult.  counts[n_patterns], host, overwritten. ---- */
int apm_count_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint64_t *counts);
/* 64-bit chunked file ingest (replaces read_input_file, src/utils.c:12-68). */
int apm_count_file(apm_ctx *ctx, const char *path, uint64_t *counts);

/* Match positions (no reference equivalent: the reference only counts, src/sequential.c:138-140).
 * Start offsets j of the windows of pattern `pattern_index` (of the current pattern set) with
 * dist <= k, ascending, for the whole text.  *n_found = total number of matches; at most `capacity`
 * positions are written (if *n_found > capacity they are an arbitrary subset: retry with a larger
 * buffer).  Runs the one pattern through the full-DP kernels; the pattern set is left unchanged. */
int apm_find_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, int pattern_index, uint64_t *positions,
                    uint64_t capacity, uint64_t *n_found);

/* ---- all patterns' match positions in ONE pass of the kernels the counting calls run ----
 * One record per (pattern, window start j) pair, for every j the counting calls count: the truncated tail windows at
 * the end of the whole text included, duplicate patterns of the set with records of their own.  `pos` is the global
 * 64-bit offset of the window start, `pattern` the index in the caller's list, `reserved` is 0. */
typedef struct apm_match {
    uint64_t pos;
    uint32_t pattern;
    uint32_t reserved; /* 0 from the find calls; the capped distance after a scoring call */
} apm_match; /* 16 bytes */
/* what a scoring call writes into `reserved` of a record that names no window: pattern >= n_patterns or pos >= n_total */
#define APM_DIST_INVALID 0xFFFFFFFFu

/* Whole text (host), all patterns of the current set, the kernels AUTO (or the forced variant) picks, one pass: the
 * launches, the text bytes and the plan are those of apm_count_buffer on the same input -- no plan is built, no pattern
 * swapped, a counting call before and after gives the same counts and apm_get_stat / apm_pattern_kernel the same
 * answers.  *n_found is always the exact total (= the sum of apm_count_buffer's counts).  At most `capacity` records are
 * written, sorted by (pattern, pos); if *n_found > capacity they are an arbitrary subset of the true set (retry with a
 * larger buffer).  out == NULL with capacity == 0 is legal: a total count.  Multi-device contexts: TEXT partition --
 * every device records its owner range with global positions, the host merges; PATTERNS partition -- the children's
 * indices are shifted by their slice's first pattern.  Allocates a device record buffer of `capacity` records per
 * device, kept by the context while it is large enough. */
int apm_find_all_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity,
                        uint64_t *n_found);

/* apm_find_all_buffer with every match's edit distance: everything that call promises, and `reserved` of every record =
 * dist(pattern[0:size], text[pos:pos+size]), size = min(m, n - pos) -- the distance the counting calls compare with k, so
 * every value is <= k.  The scan is apm_find_all_buffer's; ONE more launch per device (labelled "score" by
 * apm_get_launch_times, counted in n_launches and kernel_ms) recomputes the distances of the records on the device before
 * they are downloaded: TEXT partition -- every device scores its own records against its resident shard; PATTERNS
 * partition -- every child scores with its slice of the patterns before the indices are shifted.  The plan and the
 * counting calls are untouched (the shards' halo is that of the longest pattern, those with k >= m included: their windows
 * match without a look at the text, their distances do not); limits and errors of the scoring pass: apm_score_shard_device. */
int apm_find_all_dist_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity,
                             uint64_t *n_found);

/* ---- edit scripts ----
 * For a record (pattern i, pos): size = min(m_i, n_total - pos), p = pattern_i[0:size], t = text[pos:pos+size] -- the pair the
 * scoring pass measures.  The script turns p into t, one op per alignment column, listed from the window's first byte to
 * its last:
 *   code 0, letter '=': bytes equal; consumes one byte of each
 *   code 1, letter 'X': substitution; consumes one byte of each
 *   code 2, letter 'I': the text has a byte the pattern has not; consumes text only
 *   code 3, letter 'D': the pattern has a byte the text has not; consumes pattern only
 * It is the pattern-to-text edit, not SAM's query/reference roles.  Both strings have `size` bytes, so #I == #D and
 * n_ops = size + #I <= m_max + min(k/2, m_max-1), m_max the longest pattern of the set (those with k >= m included).
 * Optimal scripts are not unique; the one reported is pinned: with cell(x, y) the distance of the first x text bytes and
 * the first y pattern bytes, walk back from (size, size) and take the diagonal ('=' or 'X') if cell(x-1, y-1) + (p[y-1] !=
 * t[x-1]) == cell(x, y), else D if cell(x, y-1) + 1 == cell(x, y), else I; at y == 0 emit I until x == 0, at x == 0 emit D
 * until y == 0.  The number of ops that are not '=' is the record's distance. */
#define APM_OP_EQ 0
#define APM_OP_SUB 1
#define APM_OP_INS 2
#define APM_OP_DEL 3
/* dwords of one record's row for the current pattern set and k: 1 + ceil((m_max + min(k/2, m_max-1)) / 16) */
int apm_align_row_words(const apm_ctx *ctx);              /* >= 2, or a negative apm_status */

/* apm_find_all_dist_buffer with every match's edit script: everything that call promises (distances in `reserved`
 * included), and row i of `ops` (host, capacity * stride_words dwords; row i at ops + i * stride_words) belongs to out[i]
 * after the (pattern, pos) sort: word 0 = n_ops, words 1 .. ceil(n_ops/16) = the ops, op j in bits 2 (j % 16) of word
 * 1 + j / 16, the last word's unused high bits zero; the words beyond are not written.  stride_words <
 * apm_align_row_words(ctx): APM_ERR_INVALID.  TWO more launches per device behind the scan, labelled "score" then "align"
 * by apm_get_launch_times, both counted in n_launches and kernel_ms.  TEXT partition -- every device aligns its own records
 * against its resident shard (the halo is that of the longest pattern, as for scoring); PATTERNS partition -- every child
 * aligns with its slice, at the caller's stride, before the indices are shifted.  Allocates a device buffer of
 * capacity * stride_words dwords per device, kept by the context while it is large enough (it cannot be had:
 * APM_ERR_NOMEM); limits and errors of the align pass: apm_align_shard_device. */
int apm_find_all_align_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out, uint64_t capacity,
                              uint64_t *n_found, uint32_t *ops, uint32_t stride_words);

/* ---- best hits: one record per occurrence ----
 * The find calls report every window start j with dist <= k.  With k >= 2 one real occurrence leaves a run of records: if j
 * matches at distance d, j +- s matches at up to d + 2 s, and the scripts show it (11=1X4=1D7=1I is an occurrence seen one
 * column off, with a compensating I at the end).  The best-hit pass thins a record buffer to the best start of every run.
 * THE RULE.  Fix the pattern set, k, a text of n_total bytes and a radius r, 0 <= r <= APM_BEST_MAX_RADIUS.
 *   W       = [0, max(0, n_total - k)): the window starts the counting calls count
 *   s(i, j) = min(dist(p_i[0:size], text[j:j+size]), k + 1), size = min(m_i, n_total - j): exactly the scoring pass's score
 * Record (i, pos) is a BEST HIT iff
 *   1. s(i, pos) <= k,
 *   2. every j in W with pos - r <= j < pos has s(i, j) >  s(i, pos),
 *   3. every j in W with pos < j <= pos + r has s(i, j) >= s(i, pos).
 * Consequences:
 *   - the decision is a function of text and pattern only, not of which other records are in the buffer: records may come
 *     unordered, as a subset, duplicated (a duplicate is kept as often as it comes), or made up by the caller (seeds);
 *   - r = 0 keeps exactly the records within k: a score plus a filter for seeds;
 *   - two kept records of one pattern are never within r of each other;
 *   - a plateau of equal distances keeps its first start, and a chain of equal distances whose links are closer than r keeps
 *     only its first: on ACG x 80 with the pattern ACG x 6 at k = 3 there are 237 matches; 79 are kept at r = 1 or 2 (the
 *     exact starts, 3 apart), 1 at r >= 3;
 *   - a start outside W never suppresses: that includes the truncated tail beyond n_total - k. */
#define APM_BEST_MAX_RADIUS 64
/* apm_find_all_dist_buffer thinned to its best hits at `radius`, on the device, before anything is downloaded.  The scan is
 * apm_find_all_buffer's: same launches, same plan, a counting call before and after gives the same counts.  Behind it ONE
 * launch, labelled "best" by apm_get_launch_times (counted in n_launches and kernel_ms; apm_get_stat "best_ms"), runs from
 * the context's record buffer into a second device buffer of `capacity` records, which the context keeps as it keeps the
 * first; there is no separate "score" launch.  ops != NULL: one "align" launch follows, over the best hits only; row format
 * and stride rule are apm_find_all_align_buffer's (ops: capacity * stride_words dwords).  In a text mode the position map
 * follows, over the best hits; the pass itself runs on the normalised text.  out: the best hits sorted by (pattern, pos),
 * their distances in `reserved`, their rows following them through the sort.  *n_matches: the scan's exact total (= the sum
 * of the counts); *n_best: the number of best hits among the records examined.  If *n_matches > capacity the call still
 * returns APM_OK: the records examined were an arbitrary subset, so out is a subset of the true best hits (the rule does not
 * depend on the set) -- retry with capacity >= *n_matches.  radius > APM_BEST_MAX_RADIUS: APM_ERR_INVALID.  A multi-device
 * context (either partition): APM_ERR_UNSUPPORTED -- the resident shards' halo is m_max - 1 and the pass needs `radius` more
 * on both sides; multi-device best hits are deliberately out of scope (the device-level call below serves shards that bring
 * the halo).  Limits of the pass: apm_best_shard_device. */
int apm_find_best_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, uint32_t radius, apm_match *out,
                         uint64_t capacity, uint64_t *n_best, uint64_t *n_matches,
                         uint32_t *ops, uint32_t stride_words);

/* ---- occurrence search: free-end matches, their distances and spans ----
 * Every find call above answers the reference's question: is the fixed window text[j : j+m) within k edits of the pattern?
 * An occurrence with a net insertion or deletion has length m +- e; the window form sees it at a distance inflated by the
 * length difference, or not at all, and one occurrence leaves a run of records.  The occurrence search answers the textbook
 * question (Sellers 1980; Myers 1999, search form): for every text position e, what is the smallest edit distance between
 * the WHOLE pattern and some substring that ends at e?
 * SEMANTICS.  Use the current pattern set and the context's k.  Pattern p has m bytes and the whole text T has n_total bytes.
 *   C[0][x] = 0, C[y][0] = y, C[y][x] = min(C[y-1][x-1] + (p[y-1] != T[x-1]), C[y-1][x] + 1, C[y][x-1] + 1).
 *   E(e) = C[m][e+1] = min over s <= e+1 of dist(p, T[s : e+1)), for e in [0, n_total).
 * ENDS.  With flags = APM_OCC_ALL, end e is reported iff E(e) <= k.
 * With flags = APM_OCC_LOCAL_MIN, end e is reported iff all three hold:
 *   - E(e) <= k;
 *   - E(e-1) > E(e), taking E(-1) = m;
 *   - E(e+1) >= E(e), where this condition holds by definition at e = n_total - 1.
 * A plateau keeps its first end.  The LOCAL_MIN rule is the best-hit rule at radius 1 in end coordinates, decided inside
 * the scan.
 * A reported end is a record apm_match {pos = e (the occurrence's LAST byte), pattern = i, reserved = E(e)}.  counts[i] is
 * the number of records reported for pattern i under the flags.
 * SPAN of a record (i, e).
 *   - d* = min over L in [1, min(m + k, e + 1)] of dist(p, T[e+1-L : e+1)).  This equals E(e) whenever E(e) <= k.
 *   - If d* <= k, the span record is {pos = e + 1 - L*, pattern, reserved = d*}, where L* is the SMALLEST L that attains d*
 *     (the shortest occurrence).
 *   - If d* > k, the span record is {APM_OCC_NO_START (UINT64_MAX), pattern, k + 1}.
 * The span pass computes d* itself.  It ignores the record's fourth dword, as the best-hit pass does, so made-up records
 * (seeds) are served.
 * LIMITS.  Every pattern needs m <= APM_OCC_MAX_PATTERN_LEN = 128 (columns of 1..4 words) and k < m: with k >= m every
 * position matches the empty substring.  A set that breaks either limit gets APM_ERR_UNSUPPORTED, and nothing is written.
 * Out of scope: wider columns, multi-device contexts, and a pigeonhole filter in front of the scan.
 * RELATION TO THE WINDOW FORM.  If window j of pattern i is a full window (j + m <= n_total) and matches at distance d, then
 * ALL mode reports (i, j + m - 1) with E <= d.
 * HOW IT RUNS.  A walk started at byte x0 > 0 with the column C[y] = y, as if the text began there, gives the exact
 * min(score, k + 1) at e once it has consumed the m + k bytes [e - m - k + 1, e]: an alignment of cost <= k spans at most
 * m + k text bytes, and a later start can only raise the score.  So the ends are cut into segments of S bytes
 * (apm_get_stat "occ_segment"), one lane walks one (segment, pattern) pair with m + k bytes of warm-up, one bit-vector
 * column per text byte and pattern. */
#define APM_OCC_ALL 0u
#define APM_OCC_LOCAL_MIN 1u
#define APM_OCC_MAX_PATTERN_LEN 128
#define APM_OCC_NO_START UINT64_MAX
/* Whole text (host), all patterns of the current set, ONE occurrence scan (a launch labelled "occ" by
 * apm_get_launch_times) over the context's text buffer and record buffers, single device.  out_end: the reported ends
 * sorted by (pattern, end); out_start (may be NULL): out_start[i] is the span record of out_end[i], carried through the
 * sort; it adds one launch, "span".  *n_found is always exact; if it exceeds `capacity` the records returned are an
 * arbitrary subset (retry with a larger buffer); out_end == NULL with capacity == 0 is legal.  counts (may be NULL):
 * n_patterns values, the records per pattern under the flags.  In a text mode the call searches the normalised text T;
 * both arrays then go through the position-map launch, so ends and starts are source offsets (APM_OCC_NO_START is left as
 * it is by the map's "pos >= length" rule) and the counts are those of T.  The plan is not touched: a counting call before
 * and after gives the same counts and apm_pattern_kernel the same answers.  apm_timing is filled as for a find call
 * (text_bytes, kernel_ms, n_launches; windows and cells stay 0).  Unknown flag bits: APM_ERR_INVALID.  Multi-device
 * context: APM_ERR_UNSUPPORTED. */
int apm_find_occ_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end,
                        apm_match *out_start /* may be NULL */, uint64_t capacity, uint64_t *n_found,
                        uint64_t *counts /* may be NULL */);

/* ---- occurrence scripts: each occurrence's edit script ----
 * The pair is an end record (i, e) of the occurrence search and its span record with pos = s: p = pattern_i, all m bytes;
 * t = T[s : e + 1), so L = e + 1 - s.  The script turns p into t.  Ops, letters and packing are those of "edit scripts" above
 * without change: APM_OP_EQ / SUB / INS / DEL, 16 ops per dword, word 0 = n_ops, op j in bits 2 (j % 16) of word 1 + j / 16,
 * the last word's unused high bits zero, the words beyond not written.
 * THE RULE is the one pinned under "edit scripts", on a rectangular matrix: cell(x, y) is the distance of the first x bytes
 * of t and the first y bytes of p, cell(x, 0) = x, cell(0, y) = y.  Walk back from (L, m): take the diagonal ('=' or 'X') if
 * cell(x-1, y-1) + (p[y-1] != t[x-1]) == cell(x, y), else D if cell(x, y-1) + 1 == cell(x, y), else I; at y == 0 emit I until
 * x == 0, at x == 0 emit D until y == 0.
 * Consequences:
 *   - #D - #I = m - L;
 *   - n_ops = m + #I <= m + k;
 *   - the number of ops that are not '=' is the span record's distance;
 *   - for a span the span pass produced the first op is never I: L* is the shortest length at d*, and a leading I would
 *     leave a shorter substring at d* - 1.
 * The pass computes the distance of the pair itself and ignores both records' fourth dword, so made-up pairs (seeds) are
 * served: a pair farther than k gets n_ops = 0.  Limits: the occurrence search's (m <= 128, k < m) -- the whole trace, at
 * most 256 columns of 8 words, stays in the workgroup's local memory. */
/* dwords of one pair's row for the current pattern set and k: 1 + ceil((m_max + k) / 16).  A set the occurrence search
 * refuses: APM_ERR_UNSUPPORTED; no pattern set: what apm_align_row_words returns then. */
int apm_occ_align_row_words(const apm_ctx *ctx);          /* >= 2, or a negative apm_status */
/* apm_find_occ_buffer with out_start given, and every occurrence's script: everything that call promises, and row i of `ops`
 * (host, capacity * stride_words dwords; row i at ops + i * stride_words) belongs to out_end[i] after the (pattern, end)
 * sort -- the rows follow the records' permutation.  A record whose span record is APM_OCC_NO_START has word 0 = 0.  Three
 * launches, "occ", "span", "oalign" by apm_get_launch_times; in a text mode all three run on the normalised text, in front
 * of the two position-map launches.  out_start and ops are required when capacity > 0; capacity == 0 gives a count only,
 * with neither a span nor an oalign launch.  stride_words < apm_occ_align_row_words(ctx): APM_ERR_INVALID.  The device
 * buffer of capacity * stride_words dwords is the align call's: kept by the context while it is large enough.
 * Multi-device context: APM_ERR_UNSUPPORTED. */
int apm_find_occ_align_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end,
                              apm_match *out_start, uint64_t capacity, uint64_t *n_found,
                              uint64_t *counts /* may be NULL */, uint32_t *ops, uint32_t stride_words);

/* ---- nearest occurrences: each pattern's best match in the text, with no k ----
 * "Where is this pattern closest to matching, and how far off is it?" -- the occurrence search's E_i(e) (above: C[0][x] = 0,
 * C[y][0] = y, E(e) = C[m][e+1]) reduced over the whole text, one answer per pattern.
 * SEMANTICS.  For pattern i with m_i bytes over a text of n_total bytes:
 *   d_i = min over e in [0, n_total) of E_i(e);  e_i = the SMALLEST e with E_i(e) = d_i.
 *   - If d_i < m_i, the end record is {pos = e_i, pattern = i, reserved = d_i}, and its start record is
 *     {e_i + 1 - L*, i, d_i}: L* is the smallest L in [1, min(m_i + d_i, e_i + 1)] with dist(p, T[e_i+1-L : e_i+1)) = d_i -- the
 *     span rule of the occurrence search with k := d_i.
 *   - If no end has E < m_i, both records are {APM_OCC_NO_START, i, m_i}: "none".  This covers n_total = 0 and a pattern that
 *     shares no byte with the text (E = m_i is the empty substring, no occurrence).
 * The context's k is NOT used: a set with k >= m, which the occurrence search refuses, is served, and the results are
 * identical for every k.
 * LIMITS.  m <= APM_OCC_MAX_PATTERN_LEN (128) for every pattern, else APM_ERR_UNSUPPORTED and nothing is written;
 * n_total > 2^56: APM_ERR_UNSUPPORTED; multi-device context: APM_ERR_UNSUPPORTED.
 * Out of scope: edit scripts of nearest occurrences (the occurrence-script pass takes one launch-wide k); per-sequence
 * minima (a search of their own: "nearest occurrences per sequence" below); the number of ends that attain d_i (apm_find_occ_buffer at k = d_i gives them); multi-device contexts; m > 128.
 * HOW IT RUNS.  A walk of pattern i is the occurrence search's segment walk with the bound m_i - 1: the warm-up is 2 m_i - 1
 * bytes, behind it min(score, m_i) is exact by the warm-up lemma, and values of m_i or more are never reported.  Every lane
 * keeps the best (distance, first end) of its segment (apm_get_stat "nearest_segment"), a wave reduces its 64 lanes, and
 * the device result is ONE 64-bit key per pattern, merged with an unsigned 64-bit atomic minimum:
 *   key = (d << 56) | e;  APM_NEAREST_NONE = UINT64_MAX.
 * The smaller key is the smaller distance and, at equal distance, the smaller end, so shards, segments and waves merge in
 * any order to the pinned answer.  d <= 127, so a real key never equals APM_NEAREST_NONE. */
#define APM_NEAREST_NONE UINT64_MAX
#define APM_NEAREST_DIST(key) ((unsigned)((uint64_t)(key) >> 56))
#define APM_NEAREST_END(key) ((uint64_t)(key) & 0x00ffffffffffffffull)
/* Whole text (host), all patterns of the current set, single device: ONE nearest scan (a launch labelled "nearest" by
 * apm_get_launch_times) and its finishing launch ("nspan") over the context's text buffer and record buffers.  out_end and
 * out_start (may be NULL) get n_patterns records each, in pattern order.  In a text mode both launches run on the normalised
 * text T and both arrays then go through the position-map launch, so ends and starts are source offsets (APM_OCC_NO_START
 * is left as it is by the map's "pos >= length" rule).  The plan is not touched: a counting call before and after gives
 * the same counts and apm_pattern_kernel the same answers.  apm_timing is filled as for apm_find_occ_buffer. */
int apm_find_nearest_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out_end,
                            apm_match *out_start /* may be NULL */);

/* ---- nearest occurrences per sequence: every pattern's best match in each sequence ----
 * The matrix a multi-FASTA asks for: for EACH sequence, how close does EACH pattern (primer, adapter, barcode, probe) come,
 * and where?  The answer of "nearest occurrences" above is one record per pattern for the whole text, and may lie on an
 * occurrence that spans two sequences (a text mode concatenates them with no separator); here no occurrence crosses a
 * sequence boundary.
 * SEMANTICS.  A text T of n_total bytes and a SEQUENCE TABLE of n_seq + 1 apm_seq entries ("sequences" below) of which only
 * t_begin is read: t_begin[0] = 0, t_begin non-decreasing, t_begin[n_seq] = n_total (the sentinel).  Sequence s is
 * T_s = T[t_begin[s], t_begin[s+1]); empty sequences are legal.  For sequence s and pattern i (m_i bytes) let E be the
 * occurrence search's recurrence run ON T_s AS A TEXT OF ITS OWN: C[y][0] = y at the sequence's first byte; nothing in front
 * of t_begin[s] or at or behind t_begin[s+1] is part of any substring.
 *   d = min E(e) over the ends of T_s;  e = the SMALLEST end that attains it, reported as an index in T.
 *   - key[s * n_patterns + i] = (d << 56) | e if d < m_i, else APM_NEAREST_NONE (an empty sequence; a pattern that shares no
 *     byte with T_s).  The macros are those of the nearest search.
 *   - the end record is {e, i, d}; the start record {e + 1 - L*, i, d}: L* is the smallest L in
 *     [1, min(m_i + d, e + 1 - t_begin[s])] with dist(p, T[e+1-L : e+1)) = d -- the span rule at the bound d, clamped to the
 *     sequence.  "None" is {APM_OCC_NO_START, i, m_i} in both records.
 * Row s * n_patterns + i of the keys and of both record arrays is the pair (s, i).  The context's k is not looked at.  With
 * n_seq = 1 keys and records equal those of apm_nearest_shard_device / apm_nearest_records_device.
 * LIMITS.  m <= APM_OCC_MAX_PATTERN_LEN for every pattern, else APM_ERR_UNSUPPORTED and nothing is written; n_total <= 2^56;
 * n_seq < 2^32 (both APM_ERR_UNSUPPORTED); single-device context only, a multi-device context gets APM_ERR_UNSUPPORTED.
 * Out of scope: edit scripts; multi-device contexts; m > 128; a k-bounded early exit.
 * HOW IT RUNS.  The nearest scan's geometry with a walk that knows where sequences begin.  The lane that decides the ends
 * [b, b + S) (apm_get_stat "seqnear_segment") finds s_b, the largest s with t_begin[s] <= b, by a bounded binary search and
 * starts at max(b - (2 m - 1), t_begin[s_b]): at the sequence's first byte it is exact from its first column, otherwise the
 * warm-up lemma holds with its 2 m - 1 bytes, all inside the sequence.  At every column that is the next t_begin the lane
 * merges its best key into the pair's key with a 64-bit atomic minimum, moves past any empty sequences and starts again.  What
 * is left at the end of a walk a wave reduces to one atomic where all its lanes ended in the same sequence. */
/* Whole text (host), all patterns of the current set, single device, in a TEXT MODE (that is where sequences come from: with
 * mode 0 APM_ERR_STATE; without APM_TEXT_FASTA in the mode n_seq = 1): stage, normalise, build the context's sequence table
 * -- the one apm_locate_buffer and apm_get_sequences use, so both work after this call --, preset the keys, ONE scan (a
 * launch labelled "snear") and its finishing launch ("snspan"), then both arrays through the position-map launch: `pos` is
 * a SOURCE offset, APM_OCC_NO_START is left as it is.  out_end and out_start (may be NULL) get *n_seq * n_patterns records
 * each, row s * n_patterns + i the pair (s, i).  *n_seq is always set.  n_seq > capacity_seq: APM_ERR_INVALID, nothing is
 * written to the arrays (size a retry from *n_seq) -- so capacity_seq == 0 with NULL arrays is a count of sequences.  The
 * plan is not touched: a counting call before and after gives the same counts.  apm_timing is filled as for
 * apm_find_nearest_buffer. */
int apm_find_nearest_seq_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, apm_match *out_end,
                                apm_match *out_start /* may be NULL */, uint64_t capacity_seq, uint64_t *n_seq);

/* ---- occurrence search per sequence: no match crosses a FASTA record ----
 * The k-bounded occurrence search for a multi-FASTA (reads, contigs, amplicons against adapters, primers, barcodes, probes).
 * A text mode concatenates the sequences with no separator and E(e) of "occurrence search" above is a minimum over ALL
 * starts, so that search reports occurrences that begin in one record and end in the next -- and such a crossing occurrence
 * HIDES the true one inside the record: its E(e) is never computed, no filter afterwards brings it back.  Here every
 * sequence is a text of its own.
 * SEMANTICS.  A text T of n_total bytes and a sequence table of n_seq + 1 apm_seq entries of which only t_begin is read, with
 * the promises of "nearest occurrences per sequence": t_begin[0] = 0, non-decreasing, t_begin[n_seq] = n_total, empty
 * sequences legal; T_s = T[t_begin[s], t_begin[s+1]).  For sequence s and pattern i, E_s is the occurrence search's
 * recurrence run ON T_s AS A TEXT OF ITS OWN: C[y][0] = y at the sequence's first byte; nothing outside T_s is part of any
 * substring.  s(e) is the largest s with t_begin[s] <= e; it never names an empty sequence.
 *   ENDS.  APM_OCC_ALL reports end e -- an index in T, s = s(e) -- iff E_s(e) <= k.  APM_OCC_LOCAL_MIN iff also
 *     E_s(e-1) > E_s(e), with E_s = m in front of the sequence's first byte, and E_s(e+1) >= E_s(e), true by definition at the
 *     sequence's LAST byte.  The record is {e, i, E_s(e)}; counts[i] is the number of records of pattern i over all sequences.
 *   SPAN.  d* = the smallest dist(p, T[e+1-L : e+1)) over L in [1, min(m + k, e + 1 - t_begin[s(e)])], L* the smallest L that
 *     attains it; the span record is {e + 1 - L*, i, d*} if d* <= k, else {APM_OCC_NO_START, i, k + 1}.  The pass ignores the
 *     record's fourth dword (seeds are served) and writes s(e) into an optional parallel uint32_t array.
 *   SCRIPTS.  The occurrence-script pass runs unchanged over the (end, span) pairs: a clamped span still has
 *     m - k <= L <= m + k whenever d* <= k.
 * LIMITS are the occurrence search's, with the same errors: m <= APM_OCC_MAX_PATTERN_LEN and k < m; single device;
 * n_seq < 2^32; n_total <= 2^56 (all APM_ERR_UNSUPPORTED).  With n_seq = 1 every result equals that of the whole-text calls.
 * HOW IT RUNS.  The occurrence scan's geometry with a walk that knows where sequences begin: the lane that decides the ends
 * [b, b + S) (apm_get_stat "seqocc_segment") starts at max(b - (m + k), t_begin[s_b]); at a column that is the next t_begin
 * it decides the pending end as its sequence's last byte, starts its column again and goes on in the next sequence. */
/* Whole text (host), all patterns of the current set, single device, in a TEXT MODE (mode 0: APM_ERR_STATE; without
 * APM_TEXT_FASTA in the mode the table has one sequence).  In order: stage and normalise; build the context's sequence table
 * (apm_locate_buffer and apm_get_sequences work afterwards); the scan (a launch labelled "socc"); with out_start the span pass
 * ("sspan"); with ops the occurrence-script pass ("oalign") into rows of stride_words dwords (apm_find_occ_align_buffer's row
 * format); the position maps, so every `pos` is a SOURCE offset (APM_OCC_NO_START stays); the sort by (pattern, end), starts,
 * out_seq and rows following the permutation.  out_seq[r] (may be NULL; needs out_start) is the sequence of record r.
 * *n_found is the number of ends, of which min(*n_found, capacity) records are written; counts (may be NULL) the ends per
 * pattern; capacity == 0 counts only.  out_seq or ops without out_start, unknown flag bits, ops with
 * stride_words < apm_occ_align_row_words(ctx): APM_ERR_INVALID.  The plan is not touched: a counting call before and after
 * gives the same counts. */
int apm_find_occ_seq_buffer(apm_ctx *ctx, const uint8_t *text, uint64_t n, unsigned flags, apm_match *out_end,
                            apm_match *out_start /* may be NULL */, uint32_t *out_seq /* may be NULL; needs out_start */,
                            uint64_t capacity, uint64_t *n_found, uint64_t *counts /* may be NULL */,
                            uint32_t *ops /* may be NULL; needs out_start */, uint32_t stride_words);

/* ---- shard-level API (device-resident text, asynchronous) ----
 * d_text holds the bytes of global positions [text_off, text_off+text_len) on
 * the context's device.  Counts every window whose START j lies in
 * [own_begin, own_end) ∩ [0, n_total-k); windows running past n_total are
 * truncated exactly as the reference does at the END OF THE WHOLE TEXT only
 * (src/sequential.c:131-134) -- never at a shard end (that is the
 * reference's DB_OVER_RANKS over-count, src/database_over_ranks.c:339-343).
 * Requires text_off <= own_begin and
 *          text_off+text_len >= min(n_total, own_end + m_max - 1).
 * d_counts: device array of n_patterns uint64, ADDED into (caller zeroes it).
 * Work is enqueued on the context's stream.  In the steady state the call does not synchronise with the host; the
 * FIRST call with a pattern set, and a call that needs larger scratch than any before it (the sieve's candidate
 * list grows with text_len; the GENERIC kernel's columns), allocate device memory and may synchronise the stream.
 * Readable padding: the scan kernels fetch 16 bytes at a time, so the memory behind d_text must be readable up to
 * the next 16-byte boundary past d_text + text_len, and (for a d_text that is not 16-byte aligned) back to the
 * 16-byte boundary in front of it -- both lie inside any hipMalloc'ed block if the block is 16 bytes larger than
 * the text.  Those bytes are never part of a counted window. */
int apm_count_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off,
                           uint64_t text_len, uint64_t n_total,
                           uint64_t own_begin, uint64_t own_end,
                           uint64_t *d_counts);
/* The record form of apm_count_shard_device: same contract (ranges, halo, readable padding, single-device context,
 * work enqueued on the context's stream).  The records of the windows it counts are APPENDED to d_out at *d_n_found
 * (device uint64, the caller zeroes it; several shards may share one buffer), unordered; *d_n_found ends as the exact
 * number of matches even beyond `capacity`, records that do not fit are dropped.  d_out: device, 16-byte aligned,
 * `capacity` records; may be NULL when capacity is 0.  d_counts: may be NULL; else added into, as in the counting call.
 * In the steady state no host synchronisation and no allocation: the caller owns the buffer, the context's scratch is
 * the counting call's. */
int apm_find_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                          uint64_t own_begin, uint64_t own_end, apm_match *d_out, uint64_t capacity,
                          uint64_t *d_n_found, uint64_t *d_counts);
/* The scoring pass: one launch over the records d_rec[0 .. min(*d_n_rec, capacity)) -- found by apm_find_shard_device,
 * or made up by the caller (seeds of another tool) -- that writes each record's exact distance into its fourth dword.
 * Score = min(dist(pattern[0:size], text[pos:pos+size]), k + 1), size = min(m, n_total - pos), with the current pattern set
 * and k: the distance itself for every window within k, k + 1 for every other.  Per record:
 *   pattern >= n_patterns or pos >= n_total                         reserved = APM_DIST_INVALID
 *   window [pos, pos+size) not wholly inside [text_off, text_off+text_len)   left untouched (several shards may share one
 *                                                                   buffer, as with apm_find_shard_device: score it once per shard)
 *   otherwise                                                       reserved = the score
 * pos and pattern are never modified; nothing is written at or beyond index `capacity` (*d_n_rec may exceed it, as
 * apm_find_shard_device leaves it).  d_text / text_off / text_len / n_total and the readable padding are those of
 * apm_find_shard_device (whose halo rule leaves out the patterns with k >= m: a window of theirs is scored where the text
 * given covers it); d_rec: device, 16-byte aligned; d_n_rec: device uint64, read by the kernel.  Single-device
 * context; enqueued on the context's stream, so it may directly follow apm_find_shard_device with no synchronisation in
 * between.  In the steady state the call neither synchronises with the host nor allocates; the FIRST scoring call after
 * apm_set_patterns builds the pass's image of the patterns: it allocates device memory and may synchronise.
 * k <= 7: one record per lane; beyond, one record per wavefront with the band of diagonals in LDS, which serves a
 * half-band min(k/2, m_max-1) of at most 2048 diagonals (m_max: the longest pattern of the set): a set beyond that
 * fails with APM_ERR_UNSUPPORTED (both scoring calls), nothing is written. */
int apm_score_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                           apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec);
/* The align pass: one launch over the records d_rec[0 .. min(*d_n_rec, capacity)) that writes each record's edit script
 * (see "edit scripts" above) into its row d_ops[r * stride_words ..] (device, 4-byte aligned, capacity * stride_words
 * dwords).  The records themselves are only read.  Per record:
 *   pattern >= n_patterns or pos >= n_total                         word 0 = APM_DIST_INVALID, rest untouched
 *   window [pos, pos+size) not wholly inside [text_off, text_off+text_len)   row untouched (several shards may share one
 *                                                                   buffer: align once per shard)
 *   window farther than k                                           word 0 = 0, rest untouched
 *   otherwise                                                       word 0 = n_ops; words 1 .. ceil(n_ops/16) = the ops, op j in
 *                                                                   bits 2 (j % 16) of word 1 + j / 16 (unused high bits of the
 *                                                                   last word zero); words beyond untouched
 * stride_words < apm_align_row_words(ctx) or a d_ops that is not 4-byte aligned: APM_ERR_INVALID.  No row at or beyond
 * `capacity` is written (*d_n_rec may exceed it).  Otherwise the contract is apm_score_shard_device's: single-device
 * context; enqueued on the context's stream, so it may directly follow apm_find_shard_device and apm_score_shard_device
 * with no synchronisation in between; the same text arguments and readable padding; a window of a pattern with k >= m is
 * aligned where the text given covers it.  In the steady state the call neither synchronises with the host nor allocates;
 * the FIRST align call after apm_set_patterns allocates the pass's trace workspace (at most 80 MiB; it bounds the records
 * in flight, not what is served -- apm_get_stat "align_rows") and, if no scoring call did, the image of the patterns.  It
 * refuses exactly what the scoring pass refuses: a half-band min(k/2, m_max-1) beyond 2048 fails with APM_ERR_UNSUPPORTED
 * (both align calls), nothing is written. */
int apm_align_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                           const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                           uint32_t *d_ops, uint32_t stride_words);
/* The best-hit pass (the rule: "best hits" above): one launch over the records d_rec[0 .. min(*d_n_rec, capacity)) that
 * APPENDS every best hit at `radius`, as {pos, pattern, reserved = its score}, to d_out at *d_n_out (device uint64, the
 * caller zeroes it; several shards may share one buffer).  *d_n_out ends as the exact number of best hits among the records
 * decided, even beyond out_capacity; those that do not fit are dropped, nothing is written at or beyond out_capacity.  The
 * records are only read and their fourth dword is ignored: the pass scores for itself, so it may directly follow
 * apm_find_shard_device, and apm_align_shard_device may directly follow it on d_out.  Per record:
 *   pattern >= n_patterns, or pos >= n_total, or a score above k     dropped
 *   the shard text does not cover [max(pos, r) - r, min(n_total, pos + r + m)), m the pattern's length
 *                                                                   skipped: decide it with the shard that covers it (a
 *                                                                   caller with several shards gives r more bytes of halo
 *                                                                   on both sides)
 *   a best hit                                                      appended
 * Otherwise the contract is apm_score_shard_device's: single-device context; enqueued on the context's stream; the same
 * text arguments and readable padding; in the steady state neither a host synchronisation nor an allocation (the FIRST
 * record pass after apm_set_patterns builds the image of the patterns); a half-band min(k/2, m_max-1) beyond 2048 fails
 * with APM_ERR_UNSUPPORTED.  d_out: device, 16-byte aligned, no overlap with d_rec, may be NULL when out_capacity is 0.
 * radius > APM_BEST_MAX_RADIUS, a misaligned d_out, an overlap, or NULL pointers with non-zero capacities: APM_ERR_INVALID.
 * k <= 7: one record per wavefront, its up to 2 r + 1 starts dealt to the lanes, 64 per round; beyond: one record per
 * wavefront with the band in LDS, its own window first, then the neighbours nearest first up to the first suppressor. */
int apm_best_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                          const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, uint32_t radius,
                          apm_match *d_out, uint64_t out_capacity, uint64_t *d_n_out);
/* The occurrence scan ("occurrence search" above) of a shard: reports the ENDS e in [own_begin, own_end) n [0, n_total) under
 * `flags` (APM_OCC_ALL / APM_OCC_LOCAL_MIN), as records {e, pattern, E(e)} APPENDED to d_out at *d_n_found.  The shard
 * text must cover [max(0, own_begin - m_max - k), min(n_total, own_end + 1)): a LEFT halo of m_max + k bytes (m_max: the
 * longest pattern), the mirror of the find call's right halo, and the one look-ahead byte behind the last end; if it does
 * not: APM_ERR_INVALID, nothing is written.  d_text may have any alignment; the readable-padding rule is that of
 * apm_count_shard_device.  Appending to d_out (16-byte aligned, may be NULL when capacity is 0), *d_n_found exact beyond
 * `capacity`, the optional d_counts (added into), the single-device context, stream order and the steady state without
 * synchronisation or allocation are exactly apm_find_shard_device's; the FIRST call after apm_set_patterns builds the
 * record passes' image of the patterns, as the scoring pass does.  One launch, "occ".  Unknown flag bits, own_begin >
 * own_end: APM_ERR_INVALID; a pattern beyond APM_OCC_MAX_PATTERN_LEN bytes or k >= m: APM_ERR_UNSUPPORTED. */
int apm_occ_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                         uint64_t own_begin, uint64_t own_end, unsigned flags, apm_match *d_out, uint64_t capacity,
                         uint64_t *d_n_found, uint64_t *d_counts);
/* The span pass: one launch, "span", over the records d_rec[0 .. min(*d_n_rec, capacity)), pos = an end e: d_span[r] is the
 * span record of d_rec[r] ("occurrence search" above).  The records are only read, and nothing is written at or beyond
 * `capacity`.  Per record:
 *   pattern >= n_patterns or pos >= n_total                          {APM_OCC_NO_START, pattern, APM_DIST_INVALID}
 *   [max(0, e - m - k + 1), e] not inside [text_off, text_off+text_len)   entry untouched (several shards may share one buffer)
 *   otherwise                                                        the span record
 * One record per wavefront: the reversed pattern's bit masks in LDS, at most m + k columns read backwards from e, one
 * 16-byte store.  d_rec, d_span: device, 16-byte aligned; d_n_rec: device uint64, read by the kernel.  Otherwise the
 * contract is apm_score_shard_device's; it may directly follow apm_occ_shard_device on the stream.  Limits and their
 * errors: apm_occ_shard_device's. */
int apm_occ_spans_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                         const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec, apm_match *d_span);
/* The occurrence-script pass ("occurrence scripts" above): one launch, "oalign", over the pairs (d_end[r], d_span[r]),
 * r in [0, min(*d_n_rec, capacity)), that writes pair r's script into its row d_ops[r * stride_words ..] (device, 4-byte
 * aligned, capacity * stride_words dwords).  Both record arrays are only read; nothing is written at or beyond `capacity`.
 * Per pair, with e = d_end[r].pos, s = d_span[r].pos, L = e + 1 - s, the first line that applies:
 *   d_end[r].pattern >= n_patterns, or e >= n_total, or d_span[r].pattern != d_end[r].pattern
 *                                                                    word 0 = APM_DIST_INVALID, rest untouched
 *   s == APM_OCC_NO_START                                            word 0 = 0, rest untouched
 *   s > e                                                            word 0 = APM_DIST_INVALID, rest untouched
 *   L > m + k or L < m - k                                           word 0 = 0, rest untouched, with no look at the text
 *                                                                    (the distance is at least |L - m|)
 *   [s, e] not wholly inside [text_off, text_off+text_len)           row untouched (several shards may share one buffer)
 *   distance above k                                                 word 0 = 0, rest untouched
 *   otherwise                                                        word 0 = n_ops, then the ops; words beyond untouched
 * One pair per wavefront: the pattern's bit masks, the span's bytes and every column of the matrix (as vertical deltas) in
 * local memory, no global workspace.  d_end, d_span: device, 16-byte aligned; d_n_rec: device uint64, read by the kernel.
 * stride_words < apm_occ_align_row_words(ctx), a misaligned d_ops, d_end or d_span, or NULL pointers with a non-zero
 * capacity: APM_ERR_INVALID.  Otherwise the contract is apm_occ_spans_device's -- single-device context, stream order, in the
 * steady state neither a host synchronisation nor an allocation (the FIRST record pass after apm_set_patterns builds the
 * image of the patterns) -- and it may directly follow apm_occ_spans_device on the stream.  Limits and their errors:
 * apm_occ_shard_device's. */
int apm_occ_align_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                         const apm_match *d_end, const apm_match *d_span, uint64_t capacity,
                         const uint64_t *d_n_rec, uint32_t *d_ops, uint32_t stride_words);
/* The nearest scan ("nearest occurrences" above) of a shard: decides the ENDS e in [own_begin, own_end) n [0, n_total) and
 * merges every pattern's best key into d_keys[pattern] with an atomic minimum.  d_keys: device, 8-byte aligned, n_patterns
 * entries, preset by the caller to APM_NEAREST_NONE; several shards may share it, in any order.  The shard text must cover
 * [max(0, own_begin - (2 m_max - 1)), min(n_total, own_end + 1)): a LEFT halo of 2 m_max - 1 bytes (m_max: the longest
 * pattern) and the one look-ahead byte behind the last end; if it does not: APM_ERR_INVALID, the keys are untouched.
 * d_text may have any alignment; the readable-padding rule is that of apm_count_shard_device.  Asynchronous on the
 * context's stream; in the steady state neither an allocation nor a synchronisation -- the FIRST call after
 * apm_set_patterns builds the record passes' image of the patterns, as apm_occ_shard_device does.  One launch, "nearest";
 * apm_get_stat "nearest_segment" and "nearest_lanes" describe it.  own_begin > own_end, NULL or misaligned d_keys:
 * APM_ERR_INVALID; limits and their errors: "nearest occurrences" above. */
int apm_nearest_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             uint64_t own_begin, uint64_t own_end, uint64_t *d_keys);
/* The finishing pass: one launch, "nspan", one wavefront per pattern, that reads d_keys[i] and writes d_end[i] and, if
 * d_start is not NULL, d_start[i] (device, 16-byte aligned, n_patterns records each).  Per pattern, with d =
 * APM_NEAREST_DIST(key), e = APM_NEAREST_END(key), the first line that applies:
 *   key == APM_NEAREST_NONE                       d_end[i] = d_start[i] = {APM_OCC_NO_START, i, m_i}
 *   d >= m_i or e >= n_total (a made-up key)      d_end[i] = d_start[i] = {APM_OCC_NO_START, i, APM_DIST_INVALID}
 *   [e + 1 - min(m_i + d, e + 1), e] inside [text_off, text_off+text_len)
 *                                                 d_end[i] = {e, i, d}; d_start[i] = the span record at the bound d
 *                                                 ({APM_OCC_NO_START, i, d + 1} if a made-up key's d* exceeds d)
 *   otherwise (bytes not covered)                 d_end[i] = {e, i, d}; d_start[i] untouched (another shard's)
 * The keys are only read.  Otherwise the contract is apm_occ_spans_device's; it may directly follow
 * apm_nearest_shard_device on the stream. */
int apm_nearest_records_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                               const uint64_t *d_keys, apm_match *d_end, apm_match *d_start /* may be NULL */);
struct apm_seq;
/* The per-sequence nearest scan ("nearest occurrences per sequence" above) of a shard: decides the ENDS e in
 * [own_begin, own_end) n [0, n_total) and merges the best key of every (sequence, pattern) pair into
 * d_keys[s * n_patterns + pattern] with an atomic minimum.  d_table: device, 8-byte aligned, n_seq + 1 entries in GLOBAL
 * positions, only t_begin is read.  d_keys: device, 8-byte aligned, n_seq * n_patterns entries, preset by the caller to
 * APM_NEAREST_NONE; any number of shards may share it, in any order.  The shard text must cover
 * [max(0, own_begin - (2 m_max - 1)), min(n_total, own_end + 1)): the cover rule of apm_nearest_shard_device, so that one
 * shard description serves both scans (this walk has no look-ahead column and never reads that last byte); if it does
 * not: APM_ERR_INVALID, the keys are untouched.  d_text may have any alignment; the readable-padding rule is that
 * of apm_count_shard_device.  Asynchronous on the context's stream; in the steady state neither an allocation nor a
 * synchronisation -- the FIRST call after apm_set_patterns builds the record passes' image of the patterns.  One launch,
 * "snear"; apm_get_stat "seqnear_segment" and "seqnear_lanes" describe it.  The table is the caller's promise: for a table
 * that breaks the order the keys are unspecified, but nothing outside d_keys[0 .. n_seq * n_patterns) is ever written.
 * NULL or misaligned pointers, n_seq == 0, own_begin > own_end: APM_ERR_INVALID, nothing is written; limits, call order and
 * their errors: those of apm_nearest_shard_device, and n_seq >= 2^32: APM_ERR_UNSUPPORTED. */
int apm_nearest_seq_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                                 uint64_t own_begin, uint64_t own_end, const struct apm_seq *d_table, uint64_t n_seq,
                                 uint64_t *d_keys);
/* The finishing pass: one launch, "snspan", one wavefront per (sequence, pattern) pair over a fixed grid, that reads
 * d_keys[r] and writes d_end[r] and, if d_start is not NULL, d_start[r], r = s * n_patterns + i (device, 16-byte aligned,
 * n_seq * n_patterns records each).  Per pair, with d = APM_NEAREST_DIST(key), e = APM_NEAREST_END(key),
 * cols = min(m_i + d, e + 1 - t_begin[s]), the first line that applies:
 *   key == APM_NEAREST_NONE                       d_end[r] = d_start[r] = {APM_OCC_NO_START, i, m_i}
 *   d >= m_i, or e outside [t_begin[s], t_begin[s+1]) (a made-up key)
 *                                                 d_end[r] = d_start[r] = {APM_OCC_NO_START, i, APM_DIST_INVALID}
 *   [e + 1 - cols, e] inside [text_off, text_off+text_len)
 *                                                 d_end[r] = {e, i, d}; d_start[r] = the span record at the bound d
 *                                                 ({APM_OCC_NO_START, i, d + 1} if a made-up key's d* exceeds d)
 *   otherwise (bytes not covered)                 d_end[r] = {e, i, d}; d_start[r] untouched (another shard's)
 * The keys and the table are only read.  Otherwise the contract is apm_nearest_records_device's; it may directly follow
 * apm_nearest_seq_shard_device on the stream. */
int apm_nearest_seq_records_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                                   const struct apm_seq *d_table, uint64_t n_seq, const uint64_t *d_keys,
                                   apm_match *d_end, apm_match *d_start /* may be NULL */);
/* The per-sequence occurrence scan ("occurrence search per sequence" above) of a shard: apm_occ_shard_device's contract --
 * the ENDS e in [own_begin, own_end) n [0, n_total), a shard text that covers [max(0, own_begin - (m_max + k)),
 * min(n_total, own_end + 1)) (the left halo and the look-ahead byte), records {e, pattern, E_s(e)} appended at *d_n_found,
 * nothing written at or beyond `capacity`, the counter exact, d_counts (NULL: the context's own vector) added into -- under
 * the sequence table d_table: device, 8-byte aligned, n_seq + 1 entries in GLOBAL positions, only t_begin is read.  One
 * launch, "socc"; apm_get_stat "seqocc_segment" and "seqocc_lanes" describe it.  The table is the caller's promise: for a
 * table that breaks the order the records are unspecified, but nothing outside the buffers is ever written.  NULL or
 * misaligned pointers, n_seq == 0, unknown flags, own_begin > own_end: APM_ERR_INVALID; the occurrence search's limits, a
 * multi-device context, n_seq >= 2^32, n_total > 2^56: APM_ERR_UNSUPPORTED. */
int apm_occ_seq_shard_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             uint64_t own_begin, uint64_t own_end, const struct apm_seq *d_table, uint64_t n_seq, unsigned flags,
                             apm_match *d_out, uint64_t capacity, uint64_t *d_n_found, uint64_t *d_counts);
/* The per-sequence span pass: apm_occ_spans_device's contract with the span clamped to the sequence of the end.  One launch,
 * "sspan", one record per wavefront over a fixed grid; for r < min(*d_n_rec, capacity), e = d_rec[r].pos, the first line
 * that applies:
 *   pattern >= n_patterns, or e >= n_total           d_span[r] = {APM_OCC_NO_START, pattern, APM_DIST_INVALID}; d_seq[r] = APM_SEQ_INVALID
 *   [e + 1 - cols, e] inside the shard text, cols = min(m + k, e + 1 - t_begin[s(e)])
 *                                                    d_span[r] = the span record; d_seq[r] = s(e)
 *   otherwise (bytes not covered)                    d_span[r] and d_seq[r] untouched (another shard's)
 * d_seq (device, 4-byte aligned, may be NULL) is parallel to d_span.  d_rec[r].dist is not read.  The records and the table
 * are only read. */
int apm_occ_seq_spans_device(apm_ctx *ctx, const void *d_text, uint64_t text_off, uint64_t text_len, uint64_t n_total,
                             const struct apm_seq *d_table, uint64_t n_seq, const apm_match *d_rec, uint64_t capacity,
                             const uint64_t *d_n_rec, apm_match *d_span, uint32_t *d_seq /* may be NULL */);
/* ---- text normalisation on the device (single-device context, asynchronous but for one synchronisation) ----
 * Normalises d_src[0 .. src_len) under `flags` (APM_TEXT_*, not 0) into d_dst and sets *out_len (host) to the kept length.
 * Three launches on the context's stream: per 4 KiB block a summary, ONE workgroup's scan of the summaries into a map of
 * the kept bytes in front of every block, a scatter of the kept bytes.  Between scan and scatter the call synchronises
 * the stream ONCE and reads the total: the length must be known on the host before any scan of the text can be planned
 * (shard ranges, scratch).  A total beyond dst_capacity: APM_ERR_INVALID, d_dst untouched.  Otherwise the scatter is
 * enqueued and the call returns; d_dst may be handed to apm_count_shard_device, apm_find_shard_device,
 * apm_score_shard_device or apm_align_shard_device with no further synchronisation (for that it needs the 16 bytes of
 * readable slack those calls ask for).  Nothing is written at or beyond d_dst[*out_len].
 * d_src need not be 16-byte aligned: the kernels fetch 16 bytes at a time, so the memory around the source must be
 * readable to the enclosing 16-byte boundaries (the readable-padding rule of apm_count_shard_device).  d_dst: any
 * alignment, no overlap with the source.  src_len == 0: *out_len = 0, nothing is launched.  flags == 0, unknown bits, a
 * NULL out_len, or a NULL pointer with a non-zero length: APM_ERR_INVALID.  Every offset is 64-bit: sources beyond 4 GiB
 * are served.  The context owns the map (8 bytes per 4 KiB of source, grown on demand, reused) and remembers d_src: the
 * caller keeps d_src alive and unchanged until the last apm_map_positions_device that refers to it. */
int apm_normalize_device(apm_ctx *ctx, const void *d_src, uint64_t src_len, unsigned flags,
                         void *d_dst, uint64_t dst_capacity, uint64_t *out_len /* host */);
/* One launch over the records d_rec[0 .. min(*d_n_rec, capacity)): `pos` of each goes from an offset in the text of the
 * LAST apm_normalize_device to the offset of that byte in its source (a 64-way search of the map for the block, then a
 * select inside the block's 4 KiB, re-read from d_src: one wavefront per record).  A record with pos >= that text's
 * length is left as it is; pattern and reserved are never touched; nothing at or beyond `capacity` is touched.  d_rec:
 * device, 16-byte aligned; d_n_rec: device uint64, read by the kernel.  Enqueued on the context's stream: it may directly
 * follow the find, score and align calls.  Without a preceding normalisation (or after one that failed): APM_ERR_STATE. */
int apm_map_positions_device(apm_ctx *ctx, apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec);
/* ---- sequences: which FASTA sequence a match lies in, and where inside it ----
 * An apm_match is a "record"; a FASTA record is a SEQUENCE throughout.  src = the source of the last apm_normalize_device
 * (or of the last host-level call in a text mode), src_len its length, T its kept bytes.  A HEADER OPEN is a '>' at a line
 * start -- exactly what opens a header in the normalisation pass; whether a byte opens a header does not depend on the
 * header state it is reached in (the '\n' that makes the line start has closed any header).
 * The SEQUENCE TABLE has n_seq + 1 entries, n_seq = 1 + the number of header opens:
 *   entry 0                  { APM_SEQ_NO_HEADER, 0 }: the bytes in front of the first header (usually none)
 *   entry i, 1 <= i < n_seq  { source offset of the i-th opening '>', number of kept bytes in front of it }
 *   entry n_seq              the sentinel { src_len, |T| }
 * Sequence i is T[t_begin[i], t_begin[i+1]); empty sequences are legal (two headers in a row).  Without APM_TEXT_FASTA in
 * the normalisation no header opens: n_seq = 1. */
typedef struct apm_seq {
    uint64_t hdr_off;  /* source offset of the sequence's opening '>' */
    uint64_t t_begin;  /* kept bytes in front of it = index in T of the sequence's first byte */
} apm_seq; /* 16 bytes */
#define APM_SEQ_NO_HEADER UINT64_MAX
/* The LOCATION of a record whose `pos` is a SOURCE offset (after apm_map_positions_device, or as the host-level find calls
 * return it in a text mode), c = the index in T of the source byte at pos, m = the length of the record's pattern:
 *   seq    the largest i with hdr_off[i] < pos, 0 if there is none (searched in source coordinates: empty sequences make
 *          the same search in T ambiguous)
 *   off    c - t_begin[seq]: the residue offset inside the sequence, line breaks not counted
 *   flags  with size = min(m, |T| - c): APM_LOC_SPANS if c + size - 1 >= t_begin[seq+1] (the window's last byte lies in a
 *          later sequence); APM_LOC_TRUNCATED if size < m (the reference's tail window at the end of the text)
 * A record names no window if pattern >= n_patterns, pos >= src_len, or the source byte at pos is not a kept byte: its
 * location is { 0, APM_SEQ_INVALID, 0 }.
 * Example: src = "AC\n>one x\nACGT\nAC\n>two\n>three\r\nGGTT" (35 bytes, |T| = 12) has the table [(NO_HEADER,0), (3,2), (18,8),
 * (23,8), (35,12)]; with one pattern of 4 bytes pos 0 -> (off 0, seq 0, SPANS), 10 -> (0, 1, 0), 15 -> (4, 1, SPANS: across
 * the empty sequence 2), 32 -> (1, 3, TRUNCATED); pos 3, 17, 35, 40 name no window. */
typedef struct apm_loc {
    uint64_t off;
    uint32_t seq;
    uint32_t flags;
} apm_loc; /* 16 bytes */
#define APM_SEQ_INVALID 0xFFFFFFFFu
#define APM_LOC_SPANS 1u
#define APM_LOC_TRUNCATED 2u
/* Builds the sequence table of the last apm_normalize_device into d_table (device, 8-byte aligned, `capacity` entries) and
 * sets *n_seq (host).  Single-device context, on the context's stream; three launches and ONE stream synchronisation,
 * mirroring the normalisation pass: one wavefront per 4 KiB block counts the block's header opens, one workgroup scans the
 * counts into 64-bit prefixes and the total, the host reads the total, one wavefront per block emits its entries (header
 * state and kept prefix of the block from the normalisation's map).  n_seq + 1 > capacity: APM_ERR_INVALID, nothing is
 * written to the table, *n_seq is still set (size a retry from it).  src_len == 0: the two entries {NO_HEADER,0}, {0,0},
 * n_seq = 1.  Without a valid normalisation: APM_ERR_STATE.  The source must still be alive and unchanged (as for
 * apm_map_positions_device).  The context owns the per-block count and prefix scratch (12 bytes per 4 KiB of source, grown
 * on demand, reused). */
int apm_index_sequences_device(apm_ctx *ctx, apm_seq *d_table, uint64_t capacity, uint64_t *n_seq /* host */);
/* One launch over the records d_rec[0 .. min(*d_n_rec, capacity)): d_loc[r] = the location of record r (above) in the
 * source of the last apm_normalize_device, with d_table / n_seq as apm_index_sequences_device gave them and the current
 * pattern set's lengths.  One wavefront per record: the record's 4 KiB block is resolved with the header state of the
 * normalisation's map (is the byte kept, and c), then a 64-way search of the table by hdr_off.  The records are only read;
 * nothing is written at or beyond d_loc[capacity] (*d_n_rec may exceed it).  d_rec, d_loc: device, 16-byte aligned; d_n_rec:
 * device uint64, read by the kernel.  Asynchronous on the context's stream: it may directly follow
 * apm_map_positions_device.  Errors: no pattern set or no valid normalisation APM_ERR_STATE; NULL pointers, n_seq == 0
 * APM_ERR_INVALID.  The FIRST call with a pattern set may build the record passes' pattern table (allocates, synchronises),
 * as the scoring call does. */
int apm_locate_records_device(apm_ctx *ctx, const apm_match *d_rec, uint64_t capacity, const uint64_t *d_n_rec,
                              const apm_seq *d_table, uint64_t n_seq, apm_loc *d_loc);
/* Host records with source offsets -- as the last apm_find_all_buffer, apm_find_all_dist_buffer or
 * apm_find_all_align_buffer of this context returned them in a text mode -- to their locations loc[0 .. n).  The context
 * builds its own sequence table once per normalisation and keeps it (a new host-level scan invalidates it); the records are
 * uploaded, located with one launch and the locations downloaded.  Without a text normalised by a host-level call of this
 * context resident (no text mode, no call yet): APM_ERR_STATE.  Multi-device context: APM_ERR_UNSUPPORTED (text modes are
 * single-device).  n == 0: APM_OK. */
int apm_locate_buffer(apm_ctx *ctx, const apm_match *rec, uint64_t n, apm_loc *loc);
/* That table with its sentinel: at most `capacity` entries are written to out (host), *n_seq is always exact.  States and
 * errors as apm_locate_buffer. */
int apm_get_sequences(apm_ctx *ctx, apm_seq *out, uint64_t capacity, uint64_t *n_seq);
/* Owner-computes partition helper: start positions [0, max(0,n_total-k)) cut
 * into n_shards contiguous ranges with 16-byte aligned interior boundaries. */
int apm_shard_range(uint64_t n_total, int k, int shard, int n_shards,
                    uint64_t *own_begin, uint64_t *own_end);

/* ---- synthetic text (benchmarks): deterministic counter-based DNA ----
 * byte i = "ACGT"[(splitmix64(seed ^ (i>>5)) >> (2*(i&31))) & 3].
 * Device-side fill of d_dst[0:len) with global positions [global_off, +len). */
int apm_synth_fill_device(apm_ctx *ctx, void *d_dst, uint64_t global_off,
                          uint64_t len, uint64_t seed);
/* Same bytes on the host (used to derive patterns without a device round trip). */
void apm_synth_fill_host(uint8_t *dst, uint64_t global_off, uint64_t len, uint64_t seed);

/* Generate n bytes on the device(s), scan them, return final counts. */
int apm_count_synthetic(apm_ctx *ctx, uint64_t n, uint64_t seed, uint64_t *counts);

/* ---- introspection ---- */
/* apm_count_shard_device brackets its kernels with hipEventRecord on the stream (what
 * apm_get_timing reports).  enabled=0 drops those records from the launch path. */
int apm_set_timing(apm_ctx *ctx, int enabled);
int apm_get_timing(const apm_ctx *ctx, apm_timing *out);
/* Per-launch times of the last counting call on a single-device context (timing enabled): HIP events recorded on
 * the launch stream right behind every scan-kernel launch.  Writes up to `max` durations (ms) and, if labels is
 * not NULL, a static string naming each launch ("sieve", "verify", "tile", "stream", "bitpar", ..., "score": the scoring pass, "best": the best-hit pass, "align": the align pass, "occ": the occurrence scan, "span": the span pass, "oalign": the occurrence-script pass, "nearest": the nearest-occurrence scan, "nspan": its finishing pass, "snear": the per-sequence nearest scan, "snspan": its finishing pass, "socc": the per-sequence occurrence scan, "sspan": its span pass); returns the
 * number written (>= 0) or a negative apm_status.  Synchronises with the last launch. */
int apm_get_launch_times(const apm_ctx *ctx, int max, double *ms, const char **labels);
/* Named statistics of the plan / the last counting call on device 0 (introspection for benchmarks and DESIGN.md):
 * "sieve_on", "sieve_stride" (1 or 8), "sieve_rate" (expected hits per lookup), "sieve_fused" (last call used the fused
 * kernel), "sieve_clist" (the last sieve pass handed its survivors over as a candidate list), "sieve_mask_bytes" (bytes of that
 * hand-over: list entries + the mask rows of blocks that overflowed, or all mask rows without a list; synchronises),
 * "sieve_waves" (scanning waves of the last sieve pass in its code-filter form, workgroups x waves per workgroup as launched: wave w
 * scans the 4 KiB blocks w, w + sieve_waves, ... of the scanned range; 0: the last call ran no such pass),
 * "sieve_cf_dp_form" (the window DP on codes of that pass: 0 none, 1 column form, 2 diagonal form, k <= 3),
 * "sieve_candidates" (the candidates handed over: runs a reduction kernel and synchronises with the stream), "verify_launches", "verify_image_bytes", "verify_blocks_per_cu",
 * "verify_threads", "align_rows" (trace rows = records in flight of the last align launch, 0 when there was none),
 * "norm_src_bytes", "norm_kept_bytes" (the last normalisation's source and kept lengths), "norm_ms" (HIP events around its
 * three launches, the synchronisation between them included; synchronises with the last of them; 0 with timing off),
 * "map_ms" (the same around the last position-map launch), "best_ms" (the same around the last best-hit launch), "seq_count" (n_seq of the last sequence index), "seq_index_ms"
 * (HIP events around its three launches, the synchronisation included; 0 with timing off), "locate_ms" (the same around the
 * last locate launch), "occ_segment" (S of the last occurrence scan: the bytes of ends one lane walks), "occ_lanes" (the
 * (segment, pattern) walks it launched), "nearest_segment", "nearest_lanes" (the same of the last nearest-occurrence scan),
 * "seqnear_segment", "seqnear_lanes" (the same of the last per-sequence nearest scan), "seqocc_segment", "seqocc_lanes" (the
 * same of the last per-sequence occurrence scan).
 * Unknown names: APM_ERR_INVALID. */
int apm_get_stat(const apm_ctx *ctx, const char *name, double *value);
/* Kernel variant AUTO (or the forced variant) resolves to for pattern i. */
int apm_pattern_kernel(const apm_ctx *ctx, int i);
/* Device memory helpers so that a C host needs no HIP headers. */
int apm_device_alloc(apm_ctx *ctx, void **d_ptr, uint64_t bytes);
int apm_device_free(apm_ctx *ctx, void *d_ptr);
int apm_device_upload(apm_ctx *ctx, void *d_dst, const void *src, uint64_t bytes);
int apm_device_download(apm_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);
int apm_device_memset(apm_ctx *ctx, void *d_dst, int value, uint64_t bytes);
int apm_synchronize(apm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* APM_H */
