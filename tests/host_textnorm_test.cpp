// Host test of the text-normalisation pass's shared core (csrc/apm_textnorm.h): the summary, scan, scatter and map
// kernels of csrc/apm_textnorm.hip as plain loops over 64 emulated lanes, against a byte-serial state machine.
//   host_textnorm_test <cases>     cases: lines of "<name> <flags> <hex of the source or -> <hex of the expected text or ->"
// Every case runs at several source and destination alignments; random texts over {A,C,G,T,a,c,\n,\r,>} (lengths
// 0..20000, all flags) follow.  Prints "<n> cases, <w> wrong"; exit status 1 if any is wrong.
#include "apm_textnorm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;

// ---- the reference: one byte at a time ----
static void serial(const Bytes &src, uint32_t flags, Bytes &out, std::vector<uint64_t> &src_of) {
    bool line_start = true, in_header = false;
    for (size_t i = 0; i < src.size(); ++i) {
        const uint8_t b = src[i];
        bool keep = true;
        if (flags & APM_TN_FASTA) {
            if (line_start && b == '>') in_header = true;
            if (in_header || b == '\n' || b == '\r') keep = false;
            if (b == '\n') in_header = false;
        }
        line_start = b == '\n';
        if (keep) {
            out.push_back((flags & APM_TN_UPPER) && b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b);
            src_of.push_back(i);
        }
    }
}

// ---- the kernels, lane by lane ----
struct Block { // one block resolved for one incoming state
    uint32_t w[4][64][4], keep[4][64], total, h_out;
};

static void load16(const ApmTnSrc &s, uint64_t at, uint32_t (&w)[4], uint32_t &valid) {
    valid = apm_tn_valid16(s, at);
    memset(w, 0, sizeof w);
    if (valid) memcpy(w, s.base + at, 16); // (a unit wholly outside the source is not fetched)
}

static void run_block(const ApmTnSrc &s, uint64_t b, uint32_t h, Block &o) {
    uint32_t ls = b == 0 ? 1u : (uint32_t)(s.base[b * APM_TN_BLOCK - 1] == '\n');
    o.total = 0;
    for (uint32_t c = 0; c < 4; ++c) {
        ApmTnMasks m[64];
        uint32_t valid[64], ls_in[64];
        uint64_t fixed = 0, value = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            load16(s, b * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u, o.w[c][lane], valid[lane]);
            m[lane] = apm_tn_masks(o.w[c][lane], valid[lane]);
            ls_in[lane] = lane ? m[lane - 1].nl >> 15 : ls;
            const uint32_t h_out0 = apm_tn_resolve(m[lane], valid[lane], s.flags, 0u, ls_in[lane]).h_out;
            if (apm_tn_fixes(m[lane], h_out0)) fixed |= 1ull << lane;
            if (h_out0) value |= 1ull << lane;
        }
        ls = m[63].nl >> 15;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t h_in = apm_tn_state_at(fixed, value, lane, h);
            const ApmTnLane r = apm_tn_resolve(m[lane], valid[lane], s.flags, h_in, ls_in[lane]);
            const ApmTnLane whole = apm_tn_lane(o.w[c][lane], valid[lane], s.flags, h_in, ls_in[lane]);
            if (whole.keep != r.keep || whole.count != r.count || whole.h_out != r.h_out) { printf("apm_tn_lane differs\n"); exit(2); }
            o.keep[c][lane] = r.keep;
            o.total += r.count;
        }
        h = apm_tn_state_at(fixed, value, 64u, h);
    }
    o.h_out = h;
}

struct Device { // what the pass leaves behind
    std::vector<uint32_t> summary;
    std::vector<uint64_t> map;
    uint64_t total;
};

static void summary_and_scan(const ApmTnSrc &s, Device &d) {
    const uint64_t nb = s.n_blocks;
    static Block blk;
    d.summary.assign((size_t)((nb + 4095) / 4096 * 4096), 0xdeadbeefu);
    for (uint64_t b = 0; b < nb; ++b) {
        run_block(s, b, 0u, blk);
        const uint32_t c0 = blk.total, o0 = blk.h_out;
        run_block(s, b, 1u, blk);
        d.summary[(size_t)b] = apm_tn_pack_summary(c0, blk.total, o0, blk.h_out);
    }
    // the scan: chunks of 1024 threads x 4 blocks, the threads' compositions prefixed in order
    d.map.assign((size_t)nb + 1, ~0ull);
    uint64_t before = 0;
    uint32_t state = 0;
    for (uint64_t c0 = 0; c0 < nb; c0 += 4096) {
        ApmTnFn ex = apm_tn_fn_identity();
        for (uint32_t tid = 0; tid < 1024; ++tid) {
            for (uint32_t q = 0; q < 4; ++q) {
                const uint64_t i = c0 + 4 * tid + q;
                const ApmTnFn f = i < nb ? apm_tn_fn_of(d.summary[(size_t)i]) : apm_tn_fn_identity();
                if (i < nb) d.map[(size_t)i] = apm_tn_map_entry(before, state, ex);
                ex = apm_tn_fn_then(ex, f);
            }
        }
        const uint32_t e = state ? ex.e[1] : ex.e[0];
        before += e & 0x7fffffffu;
        state = e >> 31;
    }
    d.map[(size_t)nb] = before;
    d.total = before;
}

// dst: an aligned buffer, the text goes to dst + dst_lead
static void scatter(const ApmTnSrc &s, const Device &d, uint8_t *dst, uint32_t dst_lead) {
    static Block blk;
    for (uint64_t b = 0; b < s.n_blocks; ++b) {
        const uint64_t e = d.map[(size_t)b];
        const uint64_t out = dst_lead + (e & APM_TN_PREFIX_MASK); // offset from the aligned buffer
        const uint32_t pad = (uint32_t)(out & 15u);
        uint8_t image[APM_TN_BLOCK + 32];
        memset(image, 0xEE, sizeof image);
        run_block(s, b, (uint32_t)(e >> APM_TN_STATE_BIT), blk);
        uint32_t at = pad;
        for (uint32_t c = 0; c < 4; ++c)
            for (uint32_t lane = 0; lane < 64; ++lane)
                for (uint32_t i = 0; i < 16; ++i) {
                    uint32_t x = blk.w[c][lane][i >> 2];
                    if (s.flags & APM_TN_UPPER) x = apm_tn_upper4(x);
                    if ((blk.keep[c][lane] >> i) & 1u) image[at++] = (uint8_t)(x >> (8u * (i & 3u)));
                }
        const uint32_t run = at;
        uint8_t *al = dst + (out - pad);
        const uint32_t q0 = (pad + 15u) & ~15u, q1 = run & ~15u;
        const uint32_t head_end = q0 < run ? q0 : run, tail = q1 > head_end ? q1 : head_end;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            if (pad + lane < head_end) al[pad + lane] = image[pad + lane];
            for (uint32_t u = (q0 >> 4) + lane; u < (q1 >> 4); u += 64u) memcpy(al + 16 * u, image + 16 * u, 16);
            if (tail + lane < run) al[tail + lane] = image[tail + lane];
        }
    }
}

// the map kernel for one position of the normalised text
static uint64_t g_map_block = ~0ull; // the block map_position's `blk` holds (consecutive positions share it)
static uint64_t map_position(const ApmTnSrc &s, const Device &d, uint64_t pos) {
    static Block blk;
    uint64_t lo = 0, hi = s.n_blocks;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63u) >> 6;
        uint64_t j = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t idx = lo + lane * step;
            if (idx < hi && (d.map[(size_t)idx] & APM_TN_PREFIX_MASK) <= pos) ++j;
        }
        lo += (j - 1) * step;
        hi = hi < lo + step ? hi : lo + step;
    }
    const uint64_t e = d.map[(size_t)lo];
    const uint32_t want = (uint32_t)(pos - (e & APM_TN_PREFIX_MASK));
    if (g_map_block != lo) run_block(s, lo, (uint32_t)(e >> APM_TN_STATE_BIT), blk);
    g_map_block = lo;
    uint32_t run = 0;
    for (uint32_t c = 0; c < 4; ++c)
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t cnt = (uint32_t)__builtin_popcount(blk.keep[c][lane]);
            if (want >= run && want < run + cnt)
                return lo * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u + apm_tn_select16(blk.keep[c][lane], want - run) - s.lead;
            run += cnt;
        }
    return ~0ull;
}

static long g_cases = 0, g_wrong = 0;

static void check(const std::string &name, const Bytes &src, uint32_t flags, uint32_t lead, uint32_t dst_lead, const Bytes *expect, size_t map_stride) {
    Bytes want;
    std::vector<uint64_t> src_of;
    serial(src, flags, want, src_of);
    ++g_cases;
    bool bad = expect && *expect != want; // (the serial machine here against the Python reference)
    // the source inside a 16-byte aligned buffer, foreign bytes around it that would change the result if they counted
    const size_t span = (lead + src.size() + 15) / 16 * 16;
    uint8_t *mem = (uint8_t *)aligned_alloc(16, span + 16);
    for (size_t i = 0; i < span; ++i) mem[i] = i % 3 ? (uint8_t)'>' : (uint8_t)'a';
    if (!src.empty()) memcpy(mem + lead, src.data(), src.size());
    ApmTnSrc s;
    s.base = mem;
    s.lead = lead;
    s.end = (uint64_t)lead + src.size();
    s.n_blocks = (s.end + APM_TN_BLOCK - 1) / APM_TN_BLOCK;
    s.flags = flags;
    Device d;
    if (!src.empty()) summary_and_scan(s, d);
    else { d.total = 0; d.map.assign(1, 0); }
    bad = bad || d.total != want.size();
    const size_t dspan = (dst_lead + want.size() + 64 + 15) / 16 * 16;
    uint8_t *dst = (uint8_t *)aligned_alloc(16, dspan + 16);
    memset(dst, 0xA5, dspan);
    if (!bad && !src.empty()) scatter(s, d, dst, dst_lead);
    if (!bad) {
        for (size_t i = 0; i < dspan && !bad; ++i) {
            const bool inside = i >= dst_lead && i < dst_lead + want.size();
            bad = dst[i] != (inside ? want[i - dst_lead] : (uint8_t)0xA5); // (nothing in front of or behind the text is touched)
        }
    }
    g_map_block = ~0ull;
    for (size_t p = 0; p < want.size() && !bad; p += map_stride) bad = map_position(s, d, p) != src_of[p];
    if (!bad && !want.empty()) bad = map_position(s, d, want.size() - 1) != src_of.back();
    if (bad) {
        ++g_wrong;
        if (g_wrong <= 10) printf("WRONG %s flags %u lead %u dst_lead %u (%zu bytes)\n", name.c_str(), flags, lead, dst_lead, src.size());
    }
    free(mem);
    free(dst);
}

static Bytes unhex(const std::string &h) {
    Bytes out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    // the pieces on their own
    for (uint32_t v = 0; v < 256; ++v) {
        const uint32_t w = v | (0x41u << 8) | (v << 16) | (0x7au << 24), u = apm_tn_upper4(w);
        const uint32_t up = v >= 'a' && v <= 'z' ? v - 32 : v;
        ++g_cases;
        if (u != (up | (0x41u << 8) | (up << 16) | (0x5au << 24)) || apm_tn_eq4(w, v) != (v == 0x41 ? 7u : v == 0x7a ? 13u : 5u)) ++g_wrong;
    }
    for (uint32_t mask = 1; mask < 65536; mask += 1 + mask / 97)
        for (uint32_t n = 0, bit = 0; bit < 16; ++bit)
            if ((mask >> bit) & 1u) { ++g_cases; if (apm_tn_select16(mask, n++) != bit) ++g_wrong; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string name, hs, ht;
        uint32_t flags = 0;
        if (!(ls >> name >> flags >> hs >> ht)) continue;
        const Bytes src = unhex(hs), expect = unhex(ht);
        for (uint32_t lead : {0u, 1u, 7u, 15u})
            for (uint32_t dst_lead : {0u, 3u}) check(name, src, flags, lead, dst_lead, &expect, 1);
    }
    static const char alpha[] = {'A', 'C', 'G', 'T', 'a', 'c', '\n', '\r', '>'};
    for (int it = 0; it < 240; ++it) {
        const uint32_t flags = 1u + (uint32_t)it % 3u;
        const size_t n = it < 40 ? (size_t)it : (size_t)rnd(20001);
        const uint32_t rare = it % 4 == 3 ? 1500u + rnd(6000) : 0u; // every fourth text: '\n' is rare, headers run over blocks
        Bytes src(n);
        for (size_t i = 0; i < n; ++i) {
            uint8_t b = (uint8_t)alpha[rnd(9)];
            if (rare && b == '\n' && rnd(rare)) b = (uint8_t)'>';
            src[i] = b;
        }
        check("random", src, flags, rnd(16), rnd(16), nullptr, 1);
    }
    printf("%ld cases, %ld wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
