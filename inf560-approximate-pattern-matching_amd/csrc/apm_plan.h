/*
 * apm_plan.h -- the launch plan of a pattern set: which kernel scans which pattern, in which launch, and every host
 * image, table and bitmap those launches read.  Host-only (apm_plan.cpp makes no HIP call and knows no device); the
 * runtime uploads a plan to its devices (apm_runtime.hip) and the shard scan launches from it (apm_scan.hip).
 */
#ifndef APM_PLAN_H
#define APM_PLAN_H

#include "apm_internal.h"

#include <string>
#include <vector>

struct PatternInfo {
    std::string bytes;
    int m = 0;
    int kernel = APM_KERNEL_BITPAR; // resolved variant, or -1 for "k >= m: every window matches"
};
constexpr int KERNEL_TRIVIAL = -1;

struct TiledLaunch {       // host description of one tiled scan launch
    int kind = 0;          // APM_KERNEL_BITPAR | APM_KERNEL_WAVEFRONT
    std::vector<ApmPatDesc> descs;
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> tables;
    uint8_t lut[256];
    std::vector<ApmKey> keys;         // BANDED: sub-keys
    std::vector<uint16_t> piece_off;  // BANDED: piece offsets, per pattern contiguous
    std::vector<uint16_t> table;      // BANDED: nb x 8 16-bit tags
    std::vector<uint16_t> table_kid;  // BANDED: nb x 8 key ids
    std::vector<uint32_t> ovf;        // BANDED: {tag, kid16} pairs
    std::vector<uint32_t> kinfo;      // BANDED: per key pat | off<<12 | piece<<21
    std::vector<uint32_t> pinfo;      // BANDED: per pattern {byte_off | m<<16, aux_off}
    std::vector<uint8_t> image;       // BANDED: LDS image (bytes | table | kids | ovf | kinfo | pinfo)
    int o_tab = 0, o_kid = 0, o_ovf = 0, o_kinfo = 0, o_pinfo = 0, o_next = 0, o_poff = 0;
    int o_bmp = 0, code_shift = 1; // per-position classes: key bitmap over 2-bit byte codes (leads the image)
    int o_pat = 0;                 // pattern bytes inside the image
    int o_kext = 0;                // per-position classes: packed pre-check record per key
    int key_len = 0, stride = 0;      // BANDED: (16,16), (8,8) or (8,1)
    bool sieved = false;              // BANDED per-position launch fed by the sieve pipeline (ApmPlan::sieve)
    int nb = 0, lg_nb = 0, qcap = 0;
    int a_max = 0;                    // BANDED: largest key offset
    int m_max = 0, m_min = 0, tile = 0;
};

/* Largest LDS image of a verify launch (bytes): one 512-thread workgroup with its wave buffers still fits a CU.  There is
 * no density limit on the key set any more: measured on 64 MiB of DNA (tools/density_probe.py) the pipeline beats the tile
 * kernels by 3.6x at 19 % of all code words set (800 patterns of 30, k = 3), by 90x at 48 % (200 x 16, k = 3). */
#define APM_VERIFY_IMAGE_MAX (112 * 1024)

struct VerifyLaunch {      // one apm_verify_kernel launch: a group of patterns and its LDS image (apm_verify.hip)
    std::vector<ApmPatDesc> descs;    // m, index, byte_off (into bytes), aux_off = first key, w = number of keys
    std::vector<uint8_t> bytes;       // raw pattern bytes
    std::vector<uint32_t> kinfo;      // per key = nomination unit: pat | off << 12 | unit index << 21 (a pattern's units are consecutive keys)
    std::vector<uint32_t> kpart;      // per key: partner offset inside the pattern | partner length << 16
    std::vector<uint32_t> pinfo;      // per pattern: {byte_off | m << 16, id of its first key}
    std::vector<uint8_t> image;       // bitmap16 | prefix | r2s | slots | kext | pattern bytes
    int o_prefix = 0, o_r2s = 0, o_slots = 0, o_kext = 0, o_pat = 0, o_masks = 0, o_kinfo = 0, o_pinfo = 0, o_rc = 0;
    int m_max = 0, m_min = 0;
    // stride 1 with the code filter: the launch has a SIEVE PASS OF ITS OWN -- the 18-bit bitmap of its keys alone and the
    // code-filter image over its key numbering (ApmSieve2Args::cf_image: tbl | rrec | lrec); empty: the set's shared sieve
    std::vector<uint32_t> bitmap18;
    std::vector<uint8_t> cf_image;
    int cf_o_rrec = 0, cf_o_lrec = 0;
    int cf_o_dp = 0, cf_dp_cols = 0, cf_dp_slots = 0; // window-DP slot table (ApmSieve2Args::cf_o_dp; 0: none) and its units
};

struct SievePlan {         // ONE text pass (apm_sieve2_kernel) for every per-position key of the pattern set
    bool on = false;
    int stride = 1;                   // 1: every position (per-position keys present); 8: sampled (all pieces >= 15 bytes)
    int code_shift = 1;
    int m_max = 0;
    double rate = 0;                  // expected hits per lookup on uniform codes (bitmap density)
    std::vector<uint32_t> bitmap;     // 32 KiB over the 18-bit code words of 9-byte windows: dword x & 8191, bit x >> 13
    std::vector<VerifyLaunch> launches;
    double weak_frac = 0;             // share of the key words that belong to units the code filter cannot add to
    bool per_launch_sieve = false;    // stride 1 with the code filter: every verify launch is preceded by its own sieve pass (VerifyLaunch::bitmap18)
};

struct GenericGroup {      // patterns scanned by the generic kernel, one launch (grid.y = pattern)
    std::vector<ApmPatDesc> descs; // byte_off into the all-pattern pool
    int m_max = 0;
};

struct ApmPlan {           // everything apm_build_plan decides for one pattern set (the resolved kernels go into the patterns)
    std::vector<TiledLaunch> tiled;
    SievePlan sieve;
    GenericGroup tails;   // tiled-kernel patterns with m > 128: tails by the generic kernel
    GenericGroup stails;  // tiled-kernel patterns with m <= 128: tails by the bit-vector tail kernel
    GenericGroup wtails;  // ... with 128 < m <= 512: by its 16-word form
    GenericGroup xtails;  // ... with 512 < m <= 1024: by its 32-word form (apm_bitlong.hip)
    GenericGroup longs;   // patterns scanned fully by the generic kernel
    std::vector<int> trivial; // indices with k >= m
    std::vector<uint8_t> allpat;
    int m_max = 0; // over non-trivial patterns
};

// Plans `pats` at distance k under the forced kernel (APM_KERNEL_AUTO: none) into *out and writes every pattern's
// resolved kernel into pats[i].kernel.  Returns APM_OK, or an APM_ERR_* code with its message in *err.
int apm_build_plan(std::vector<PatternInfo> &pats, int k, int forced_kernel, ApmPlan *out, std::string *err);

int wavefront_rows_per_lane(int m);
bool bitlong_rows_fit(const PatternInfo &p);

#endif /* APM_PLAN_H */
