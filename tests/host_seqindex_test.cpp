// Host test of the sequence index's shared core (csrc/apm_seqindex.h on top of csrc/apm_textnorm.h): the count, scan, emit
// and locate kernels of csrc/apm_seqindex.hip as plain loops over 64 emulated lanes, against a byte-serial state machine.
//   host_seqindex_test <cases>   cases: lines of "<name> <flags> <hex of the source or -> <table: hdr:t,hdr:t,... (hdr - = no header)>"
// Every case runs at several source alignments: the table is compared entry for entry with the one in the file (the Python
// reference's) and with the serial one here, then EVERY source offset (and two beyond the end) is located for pattern
// lengths 1, 5 and 5000.  Random texts over {A,C,G,T,a,c,\n,\r,>} (lengths 0..20000, all flags) follow.
// Prints "<n> cases, <w> wrong"; exit status 1 if any is wrong.
#include "apm_seqindex.h"

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
struct Serial {
    std::vector<apm_seq> table;      // with entry 0 and the sentinel
    std::vector<int64_t> index_of;   // source offset -> index in T, -1: not kept
    uint64_t kept;
};

static void serial(const Bytes &src, uint32_t flags, Serial &s) {
    bool line_start = true, in_header = false;
    s.table.assign(1, apm_seq{APM_SEQ_NO_HEADER, 0});
    s.index_of.assign(src.size(), -1);
    s.kept = 0;
    for (size_t i = 0; i < src.size(); ++i) {
        const uint8_t b = src[i];
        bool keep = true;
        if (flags & APM_TN_FASTA) {
            if (line_start && b == '>') {
                in_header = true;
                s.table.push_back(apm_seq{(uint64_t)i, s.kept});
            }
            if (in_header || b == '\n' || b == '\r') keep = false;
            if (b == '\n') in_header = false;
        }
        line_start = b == '\n';
        if (keep) s.index_of[i] = (int64_t)s.kept++;
    }
    s.table.push_back(apm_seq{(uint64_t)src.size(), s.kept});
}

static apm_loc serial_locate(const Bytes &src, const Serial &s, uint64_t pos, uint32_t m) {
    if (pos >= src.size() || s.index_of[(size_t)pos] < 0) return apm_sq_invalid();
    const uint64_t c = (uint64_t)s.index_of[(size_t)pos], n_seq = s.table.size() - 1;
    uint64_t a = 1, b = n_seq; // the first entry in [1, n_seq) whose header is not in front of pos; the one below it, or 0
    while (a < b) {
        const uint64_t mid = (a + b) / 2;
        if (s.table[(size_t)mid].hdr_off < pos) a = mid + 1;
        else b = mid;
    }
    const uint32_t seq = (uint32_t)(a - 1);
    const uint64_t size = s.kept - c < m ? s.kept - c : m;
    apm_loc l;
    l.off = c - s.table[seq].t_begin;
    l.seq = seq;
    l.flags = (c + size - 1 >= s.table[seq + 1].t_begin ? APM_LOC_SPANS : 0u) | (size < m ? APM_LOC_TRUNCATED : 0u);
    return l;
}

// ---- the kernels, lane by lane ----
struct Block { // one block resolved for one incoming state
    uint32_t keep[4][64], opens[4][64], n_opens, h_out;
};

static void run_block(const ApmTnSrc &s, uint64_t b, uint32_t h, Block &o) {
    uint32_t ls = b == 0 ? 1u : (uint32_t)(s.base[b * APM_TN_BLOCK - 1] == '\n');
    o.n_opens = 0;
    for (uint32_t c = 0; c < 4; ++c) {
        ApmTnMasks m[64];
        uint32_t valid[64], ls_in[64];
        uint64_t fixed = 0, value = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t at = b * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u;
            uint32_t w[4] = {0, 0, 0, 0};
            valid[lane] = apm_tn_valid16(s, at);
            if (valid[lane]) memcpy(w, s.base + at, 16); // (a unit wholly outside the source is not fetched)
            m[lane] = apm_tn_masks(w, valid[lane]);
            ls_in[lane] = lane ? m[lane - 1].nl >> 15 : ls;
            const uint32_t h_out0 = apm_tn_resolve(m[lane], valid[lane], s.flags, 0u, ls_in[lane]).h_out;
            if (apm_tn_fixes(m[lane], h_out0)) fixed |= 1ull << lane;
            if (h_out0) value |= 1ull << lane;
        }
        ls = m[63].nl >> 15;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            o.keep[c][lane] = apm_tn_resolve(m[lane], valid[lane], s.flags, apm_tn_state_at(fixed, value, lane, h), ls_in[lane]).keep;
            o.opens[c][lane] = apm_sq_opens(m[lane], s.flags, ls_in[lane]);
            o.n_opens += (uint32_t)__builtin_popcount(o.opens[c][lane]);
        }
        h = apm_tn_state_at(fixed, value, 64u, h);
    }
    o.h_out = h;
}

struct Device { // what the normalisation and the index pass leave behind
    std::vector<uint64_t> map, prefix;
    std::vector<apm_seq> table;
    uint64_t kept, n_seq;
};

static Block g_blk;

// the normalisation's map, block after block (its own scan is tests/host_textnorm_test.cpp's business)
static void make_map(const ApmTnSrc &s, Device &d) {
    d.map.assign((size_t)s.n_blocks + 1, 0);
    uint64_t before = 0;
    uint32_t h = 0;
    for (uint64_t b = 0; b < s.n_blocks; ++b) {
        d.map[(size_t)b] = before | ((uint64_t)h << APM_TN_STATE_BIT);
        run_block(s, b, h, g_blk);
        for (uint32_t c = 0; c < 4; ++c)
            for (uint32_t lane = 0; lane < 64; ++lane) before += (uint32_t)__builtin_popcount(g_blk.keep[c][lane]);
        h = g_blk.h_out;
    }
    d.map[(size_t)s.n_blocks] = before;
    d.kept = before;
}

static void index_pass(const ApmTnSrc &s, uint64_t src_len, Device &d) {
    const uint64_t nb = s.n_blocks;
    std::vector<uint32_t> count((size_t)((nb + APM_SQ_SCAN_CHUNK - 1) / APM_SQ_SCAN_CHUNK * APM_SQ_SCAN_CHUNK), 0xdeadbeefu);
    for (uint64_t b = 0; b < nb; ++b) { // count (the state handed in does not matter: both give the same opens)
        run_block(s, b, (uint32_t)(b & 1u), g_blk);
        count[(size_t)b] = g_blk.n_opens;
    }
    d.prefix.assign((size_t)nb + 1, ~0ull); // scan: chunks of 1024 threads x 4 blocks
    uint64_t before = 0;
    for (uint64_t c0 = 0; c0 < nb; c0 += APM_SQ_SCAN_CHUNK) {
        uint64_t ex = before;
        for (uint32_t tid = 0; tid < APM_SQ_SCAN_THREADS; ++tid)
            for (uint32_t q = 0; q < 4; ++q) {
                const uint64_t i = c0 + 4 * tid + q;
                if (i < nb) { d.prefix[(size_t)i] = ex; ex += count[(size_t)i]; }
            }
        before = ex;
    }
    d.prefix[(size_t)nb] = before;
    d.n_seq = 1 + before;
    d.table.assign((size_t)d.n_seq + 1, apm_seq{0x1111111111111111ull, 0x2222222222222222ull});
    d.table[0] = apm_seq{APM_SEQ_NO_HEADER, 0}; // emit
    d.table[(size_t)d.n_seq] = apm_seq{src_len, d.kept};
    for (uint64_t b = 0; b < nb; ++b) {
        const uint64_t e = d.map[(size_t)b];
        run_block(s, b, (uint32_t)(e >> APM_TN_STATE_BIT), g_blk);
        uint64_t kept = e & APM_TN_PREFIX_MASK, index = 1 + d.prefix[(size_t)b];
        for (uint32_t c = 0; c < 4; ++c)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                if (index + (uint32_t)__builtin_popcount(g_blk.opens[c][lane]) > d.n_seq) { printf("emit beyond the table\n"); exit(2); }
                index += apm_sq_emit(d.table.data(), index, g_blk.opens[c][lane], g_blk.keep[c][lane],
                                     b * APM_TN_BLOCK + c * APM_TN_CHUNK + lane * 16u, s.lead, kept);
                kept += (uint32_t)__builtin_popcount(g_blk.keep[c][lane]);
            }
    }
}

static uint64_t g_loc_block = ~0ull; // the block locate()'s `blk` holds (consecutive positions share it)
static apm_loc locate(const ApmTnSrc &s, uint64_t src_len, const Device &d, uint64_t pos, uint32_t m) {
    static Block blk;
    if (pos >= src_len) return apm_sq_invalid();
    const ApmSqAt at = apm_sq_at(pos, s.lead);
    const uint64_t e = d.map[(size_t)at.block];
    if (g_loc_block != at.block) run_block(s, at.block, (uint32_t)(e >> APM_TN_STATE_BIT), blk);
    g_loc_block = at.block;
    if (!((blk.keep[at.chunk][at.lane] >> at.bit) & 1u)) return apm_sq_invalid();
    uint64_t c_idx = e & APM_TN_PREFIX_MASK;
    for (uint32_t c = 0; c <= at.chunk; ++c)
        for (uint32_t lane = 0; lane < (c == at.chunk ? at.lane : 64u); ++lane) c_idx += (uint32_t)__builtin_popcount(blk.keep[c][lane]);
    c_idx += (uint32_t)__builtin_popcount(blk.keep[at.chunk][at.lane] & ((1u << at.bit) - 1u));
    uint64_t lo = 0, hi = d.n_seq;
    while (hi - lo > 1) {
        uint32_t n_ok = 0;
        bool gap = false;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const bool ok = apm_sq_probe(d.table.data(), lo, hi, lane, pos);
            if (ok && n_ok != lane) gap = true; // (the lanes that hold are the lowest ones)
            n_ok += ok;
        }
        if (gap || !n_ok) { printf("search: the probes are not a prefix\n"); exit(2); }
        apm_sq_narrow(lo, hi, n_ok);
    }
    return apm_sq_location(c_idx, m, d.kept, (uint32_t)lo, d.table[(size_t)lo].t_begin, d.table[(size_t)lo + 1].t_begin);
}

static long g_cases = 0, g_wrong = 0;

static bool same(const apm_seq &a, const apm_seq &b) { return a.hdr_off == b.hdr_off && a.t_begin == b.t_begin; }
static bool same(const apm_loc &a, const apm_loc &b) { return a.off == b.off && a.seq == b.seq && a.flags == b.flags; }

static void check(const std::string &name, const Bytes &src, uint32_t flags, uint32_t lead, const std::vector<apm_seq> *expect) {
    Serial want;
    serial(src, flags, want);
    ++g_cases;
    bool bad = false;
    if (expect) { // (the serial machine here against the Python reference)
        bad = expect->size() != want.table.size();
        for (size_t i = 0; i < want.table.size() && !bad; ++i) bad = !same((*expect)[i], want.table[i]);
    }
    // the source inside a 16-byte aligned buffer, foreign bytes around it that would change the result if they counted
    const size_t span = (lead + src.size() + 15) / 16 * 16;
    uint8_t *mem = (uint8_t *)aligned_alloc(16, span + 16);
    for (size_t i = 0; i < span; ++i) mem[i] = i % 3 ? (uint8_t)'>' : (uint8_t)'\n';
    if (!src.empty()) memcpy(mem + lead, src.data(), src.size());
    ApmTnSrc s;
    s.base = mem;
    s.lead = lead;
    s.end = (uint64_t)lead + src.size();
    s.n_blocks = src.empty() ? 0 : (s.end + APM_TN_BLOCK - 1) / APM_TN_BLOCK;
    s.flags = flags;
    Device d;
    make_map(s, d);
    bad = bad || d.kept != want.kept;
    if (!bad) {
        index_pass(s, src.size(), d);
        bad = d.table.size() != want.table.size();
        for (size_t i = 0; i < want.table.size() && !bad; ++i) bad = !same(d.table[i], want.table[i]);
    }
    g_loc_block = ~0ull;
    for (uint32_t m : {1u, 5u, 5000u})
        for (uint64_t pos = 0; pos < src.size() + 2 && !bad; ++pos) bad = !same(locate(s, src.size(), d, pos, m), serial_locate(src, want, pos, m));
    if (bad) {
        ++g_wrong;
        if (g_wrong <= 10) printf("WRONG %s flags %u lead %u (%zu bytes)\n", name.c_str(), flags, lead, src.size());
    }
    free(mem);
}

static Bytes unhex(const std::string &h) {
    Bytes out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static std::vector<apm_seq> untable(const std::string &t) {
    std::vector<apm_seq> out;
    std::istringstream in(t);
    std::string item;
    while (std::getline(in, item, ',')) {
        const size_t colon = item.find(':');
        const std::string h = item.substr(0, colon);
        out.push_back(apm_seq{h == "-" ? APM_SEQ_NO_HEADER : strtoull(h.c_str(), nullptr, 10), strtoull(item.c_str() + colon + 1, nullptr, 10)});
    }
    return out;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_rng >> 33) % n);
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <cases>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string name, hs, ts;
        uint32_t flags = 0;
        if (!(ls >> name >> flags >> hs >> ts)) continue;
        const Bytes src = unhex(hs);
        const std::vector<apm_seq> expect = untable(ts);
        for (uint32_t lead : {0u, 5u, 15u}) check(name, src, flags, lead, &expect);
    }
    static const char alpha[] = {'A', 'C', 'G', 'T', 'a', 'c', '\n', '\r', '>'};
    for (int it = 0; it < 160; ++it) {
        const uint32_t flags = 1u + (uint32_t)it % 3u;
        const size_t n = it < 40 ? (size_t)it : (size_t)rnd(20001);
        const uint32_t rare = it % 4 == 3 ? 1500u + rnd(6000) : 0u; // every fourth text: '\n' is rare, headers run over blocks
        Bytes src(n);
        for (size_t i = 0; i < n; ++i) {
            uint8_t b = (uint8_t)alpha[rnd(9)];
            if (rare && b == '\n' && rnd(rare)) b = (uint8_t)'>';
            src[i] = b;
        }
        check("random", src, flags, rnd(16), nullptr);
    }
    printf("%ld cases, %ld wrong\n", g_cases, g_wrong);
    return g_wrong ? 1 : 0;
}
