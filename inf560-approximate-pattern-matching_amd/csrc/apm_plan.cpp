/*
 * apm_plan.cpp -- the plan builder: kernel choice per pattern, launch grouping, LDS images, bitmaps, code-filter
 * records and window-DP slots (apm_plan.h).  Pure host code: no HIP call, no device pointer.
 */
#include "../../include/apm.h"
#include "apm_plan.h"
#include "apm_sieve.h"
#include "apm_core.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {

int plan_fail(std::string *err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *err = buf;
    return code;
}

int resolve_kernel(int forced, int m, int k, std::string *why) {
    if (forced == APM_KERNEL_AUTO) {
        if (k >= m) return KERNEL_TRIVIAL;
        if (m <= APM_BANDED_MAX_M && k <= APM_BANDED_MAX_K && m / (k + 1) >= APM_BANDED_MIN_PIECE) return APM_KERNEL_BANDED;
        if (k <= APM_NFA_MAX_K && m + k / 2 <= 32) return APM_KERNEL_NFA; // short and loose: the automaton over 32 window starts per lane (<= 16 distinct bytes: build_plan)
        if (m <= APM_BITPAR_MAX_M) return APM_KERNEL_BITPAR; // short or loose (BANDED's pigeonhole pieces too short), or long: bit-vector columns
        return APM_KERNEL_GENERIC;                           // m > 4096 only (and long patterns over big alphabets: build_plan)
    }
    switch (forced) {
    case APM_KERNEL_GENERIC: return APM_KERNEL_GENERIC;
    case APM_KERNEL_WAVEFRONT:
        if (m > APM_WAVEFRONT_MAX_M) { *why = "WAVEFRONT kernel supports pattern length <= 256"; return -100; }
        return APM_KERNEL_WAVEFRONT;
    case APM_KERNEL_BITPAR:
        if (m > APM_BITPAR_MAX_M) { *why = "BITPAR kernel supports pattern length <= 4096"; return -100; }
        return APM_KERNEL_BITPAR;
    case APM_KERNEL_NFA:
        if (k > APM_NFA_MAX_K || m + k / 2 > 32) { *why = "NFA kernel needs m + k/2 <= 32 and k <= 7"; return -100; }
        return APM_KERNEL_NFA;
    case APM_KERNEL_BANDED:
        if (m > APM_BANDED_MAX_M || k > APM_BANDED_MAX_K || m / (k + 1) < APM_BANDED_MIN_PIECE) {
            *why = "BANDED kernel needs m <= 512, k <= 7 and m/(k+1) >= 4 (pigeonhole keys of >= 4 bytes)";
            return -100;
        }
        return APM_KERNEL_BANDED;
    default: *why = "unknown kernel variant"; return -100;
    }
}

// Enter one per-position key into an 8 KiB presence bitmap over 8-byte code words (2-bit codes
// (b >> shift) & 3, byte z of the window in bits 2z..): the piece itself (its first min(len, 8) bytes) must be
// intact; what the window shows behind a piece shorter than 8 bytes is the text that follows it.  If the
// piece's partner of the pair pre-check lies there (forward partner), only continuations that can still pass
// the one-edit extension (apm_ext1_core16 semantics, bytes beyond the window = wildcards) are entered -- a
// superset of what the pre-check accepts, several times smaller than "every continuation", which is what a
// piece with its partner in front of it (or none) gets.
// Without the pair pre-check (band 0: k <= 1) a nomination is just "the key bytes match", and the dedup of the
// kernels relies on exactly that predicate -- so there only the key itself is entered, with every continuation.
// fn(xx) for every 16-bit code word xx the 8-byte window at the start of piece q may show (see above).
// pat = the pattern's bytes, poffs = its `pieces` piece offsets, m its length; plain_len = the key length used
// without the pair pre-check.
template <typename F>
void enum_key_windows(const uint8_t *pat, int m, const uint16_t *poffs, int pieces, int q, int plain_len, int shift, bool pairs, F fn) {
    auto piece_begin = [&](int qq) { return qq >= pieces ? m : (int)poffs[qq]; };
    auto code = [&](int y) { return (uint32_t)((pat[y] >> shift) & 3); };
    const int at = piece_begin(q);
    const int len = pairs ? piece_begin(q + 1) - at : plain_len; // (stride 1: the key starts the piece)
    const int vis = std::min(len, 8), ext = 8 - vis;
    uint32_t x = 0;
    for (int z = 0; z < vis; ++z) x |= code(at + z) << (2 * z);
    const int pq = q ^ 1;
    const bool forward = pairs && pq < pieces && pq > q;
    const int n = forward ? piece_begin(pq + 1) - piece_begin(pq) : 0;
    const int pa = at + len; // partner start (forward case)
    for (uint32_t p = 0; p < (1u << (2 * ext)); ++p) {
        bool ok = true;
        if (forward && ext > 0) {
            auto t = [&](int j) { return (p >> (2 * j)) & 3u; }; // visible text code j behind the piece
            int i = 0;
            while (i < n && i < ext && t(i) == code(pa + i)) ++i;
            if (!(i >= ext || i >= n - 1)) {
                ok = true; // substitution at i
                for (int j = i + 1; j < n && j < ext && ok; ++j) ok = t(j) == code(pa + j);
                if (!ok) {
                    ok = true; // pattern byte i has no text counterpart
                    for (int j = i + 1; j < n && j - 1 < ext && ok; ++j) ok = t(j - 1) == code(pa + j);
                }
                if (!ok) {
                    ok = true; // one extra text byte before pattern byte i
                    for (int j = i; j < n && j + 1 < ext && ok; ++j) ok = t(j + 1) == code(pa + j);
                }
            }
        }
        if (ok) fn(x | (p << (2 * vis)));
    }
}

void mark_key_windows(std::vector<uint8_t> &bmp, const TiledLaunch &L, const ApmKey &kk, int pieces, int shift, bool pairs) {
    const ApmPatDesc &dd = L.descs[kk.pat];
    enum_key_windows(L.bytes.data() + dd.byte_off, (int)dd.m, L.piece_off.data() + dd.aux_off, pieces, (int)kk.piece, L.key_len, shift, pairs,
                     [&](uint32_t xx) { bmp[xx & 8191u] |= (uint8_t)(1u << (xx >> 13)); });
}

// Plan of the sieve + verify pipeline for all BANDED patterns of the set (see build_plan): one sieve bitmap for the set,
// the patterns split into verify launches by LDS image size.  Leaves plan.sieve.on false only when a launch does not fit
// the index formats (the splitting keeps clear of that).
int build_sieve_plan(const std::vector<PatternInfo> &pats, int k, SievePlan &S, int stride) {
    S.stride = stride;
    const int P = (int)pats.size();
    const int pieces = k + 1;
    const bool pairs = k / 2 >= 1;
    std::vector<int> idx;
    for (int i = 0; i < P; ++i)
        if (pats[i].kernel == APM_KERNEL_BANDED) idx.push_back(i);
    // one code shift for the whole set: spread the pattern bytes over the four 2-bit codes as evenly as possible
    // (s = 1 separates A,C,G,T and a,c,g,t exactly)
    long best = -1;
    for (int sft = 0; sft < 7; ++sft) {
        long hist[4] = {0, 0, 0, 0};
        for (int i : idx)
            for (unsigned char c : pats[i].bytes) ++hist[(c >> sft) & 3];
        const long score = std::min(std::min(hist[0], hist[1]), std::min(hist[2], hist[3])) * 4 +
                           (hist[0] > 0) + (hist[1] > 0) + (hist[2] > 0) + (hist[3] > 0) + (sft == 1);
        if (score > best) { best = score; S.code_shift = sft; }
    }
    S.bitmap.assign(8192, 0u);
    std::vector<uint8_t> seen16(8192, 0); // union of the launches' 16-bit code words (byte x & 8191, bit x >> 13)
    std::vector<uint32_t> even18(8192, 0); // union of the units' 18-bit words over nine bytes (dword x & 8191, bit x >> 13)
    // nomination units of a pattern (apm_core.h, ApmUnit): per pair of pigeonhole pieces (A, B) either the two
    // piece units "A intact + B within one edit behind it" and "B intact + A within one edit in front of it", or --
    // when both pieces are short -- ONE pair unit "A+B within one edit"; whichever shows fewer 8-byte code words to
    // the sieve.  The unpaired last piece (even k) is a unit without partner; without the pair pre-check (k <= 1)
    // every piece is.  Every window with <= k edits has a unit whose predicate holds at the right text position.
    auto count_words = [&](const uint8_t *pat, const std::vector<ApmUnit> &us) {
        std::vector<uint32_t> w;
        for (const ApmUnit &u : us) apm_enum_unit_windows(pat, u, S.code_shift, [&](uint32_t x) { w.push_back(x); });
        std::sort(w.begin(), w.end());
        return (size_t)(std::unique(w.begin(), w.end()) - w.begin());
    };
    auto units_of = [&](const uint8_t *pat, int m) {
        std::vector<ApmUnit> us;
        auto a = [&](int q) { return q >= pieces ? m : (int)((int64_t)q * m / pieces); };
        for (int q = 0; q < pieces; q += pairs ? 2 : 1) {
            const int lenA = a(q + 1) - a(q);
            if (!pairs || q + 1 >= pieces) {
                us.push_back(ApmUnit{a(q), lenA, 0, 0, 0});
                continue;
            }
            const int lenB = a(q + 2) - a(q + 1);
            const std::vector<ApmUnit> by_piece = {ApmUnit{a(q), lenA, a(q + 1), lenB, 1}, ApmUnit{a(q + 1), lenB, a(q), lenA, 2}};
            const std::vector<ApmUnit> by_pair = {ApmUnit{a(q), 0, a(q), lenA + lenB, 1}};
            if (lenA + lenB <= 16 && lenA < 8 && lenB < 8 && count_words(pat, by_pair) < count_words(pat, by_piece)) us.push_back(by_pair[0]);
            else us.insert(us.end(), by_piece.begin(), by_piece.end());
        }
        return us;
    };
    static const int cf_env = getenv("APM_SIEVE_CF") ? atoi(getenv("APM_SIEVE_CF")) : 1;
    const bool cf_on = cf_env && stride == 1;
    double words_weak = 0, words_strong = 0; // key words of units the code filter can / cannot add to (see `weak` below)
    for (size_t pos = 0; pos < idx.size();) {
        VerifyLaunch V;
        std::vector<uint8_t> v_seen16(8192, 0);  // this launch's 16-bit code words / 18-bit words (as seen16 / even18 of the set)
        std::vector<uint32_t> v_even18(8192, 0);
        std::vector<ApmUnit> units; // per key, offsets relative to the pattern
        size_t n_words = 0;         // code words of the launch's units, counted per pattern (>= the distinct ones)
        for (; pos < idx.size(); ++pos) {
            const PatternInfo &pi = pats[idx[pos]];
            const std::vector<ApmUnit> us = units_of(reinterpret_cast<const uint8_t *>(pi.bytes.data()), pi.m);
            const size_t pw = stride == 8 ? us.size() * 8 : count_words(reinterpret_cast<const uint8_t *>(pi.bytes.data()), us);
            // the image must fit a CU's LDS beside the wave buffers of one workgroup, and the slot indices 15 bits:
            // bitmap + prefix (12 KiB), rank -> key and key lists (<= 2 + 2 bytes per word), key records, pattern bytes
            const size_t est = 12288 + 4 * (n_words + pw) + 8 * (V.kinfo.size() + us.size()) + 8 * (V.descs.size() + 1) + V.bytes.size() + (size_t)pi.m + 512;
            // (with the code filter the launch's sieve pass keeps 8 bytes per key word in LDS beside its 32 KiB bitmap: <= 80 KiB)
            if (!V.descs.empty() && (V.bytes.size() + (size_t)pi.m > 24576 || V.kinfo.size() + us.size() > (stride == 8 ? 2048u : 8192u) || V.descs.size() >= 4096 ||
                                     est > APM_VERIFY_IMAGE_MAX || n_words + pw >= 0x7000 || (cf_on && 8 * (n_words + pw) > 80 * 1024)))
                break;
            n_words += pw;
            ApmPatDesc d{};
            d.m = (uint32_t)pi.m;
            d.index = (uint32_t)idx[pos];
            d.byte_off = (uint32_t)V.bytes.size();
            d.aux_off = (uint32_t)V.kinfo.size(); // first key
            V.bytes.insert(V.bytes.end(), pi.bytes.begin(), pi.bytes.end());
            d.w = (uint32_t)us.size();
            for (size_t ui = 0; ui < us.size(); ++ui) {
                V.kinfo.push_back((uint32_t)V.descs.size() | ((uint32_t)us[ui].off << 12) | ((uint32_t)ui << 21));
                V.kpart.push_back((uint32_t)us[ui].poff | ((uint32_t)us[ui].plen << 16));
                units.push_back(us[ui]);
            }
            V.pinfo.push_back(d.byte_off | (d.m << 16));
            V.pinfo.push_back(d.aux_off);
            V.descs.push_back(d);
            V.m_max = std::max(V.m_max, pi.m);
            V.m_min = V.m_min ? std::min(V.m_min, pi.m) : pi.m;
        }
        while (V.bytes.size() % 16) V.bytes.push_back(0);
        // (code word, key) pairs in rank order: the verify kernel keeps the words as dword x & 2047, bit x >> 11
        auto rank_key = [](uint32_t x) { return ((x & 2047u) << 5) | (x >> 11); };
        std::vector<uint64_t> wk;
        std::vector<uint32_t> kext, krec;
        for (size_t kid = 0; kid < units.size(); ++kid) {
            const ApmUnit &u = units[kid];
            const ApmPatDesc &dd = V.descs[V.kinfo[kid] & 0xfffu];
            if (stride == 8) {
                // sampled: whatever the piece's position, one of its blocks [r, r+8), r = 0..7, starts at a multiple of 8 in
                // the text; the key-list payload carries r above the key id (11 bits)
                for (uint32_t r = 0; r < 8; ++r) {
                    uint32_t xx = 0;
                    for (int z = 0; z < 8; ++z) xx |= (uint32_t)((V.bytes[dd.byte_off + (uint32_t)u.off + r + (uint32_t)z] >> S.code_shift) & 3) << (2 * z);
                    wk.push_back(((uint64_t)rank_key(xx) << 32) | ((uint64_t)xx << 16) | (uint64_t)(kid | (r << 11)));
                }
            } else {
                const size_t wk0 = wk.size();
                apm_enum_unit_windows(V.bytes.data() + dd.byte_off, u, S.code_shift,
                                      [&](uint32_t xx) { wk.push_back(((uint64_t)rank_key(xx) << 32) | ((uint64_t)xx << 16) | (uint64_t)kid); });
                // a unit the code filter cannot judge any better than the 8-byte bitmap has: everything it would test lies inside the window
                const bool weak = (u.side == 0 && u.len <= 9) || (u.side == 1 && u.len == 0 && u.plen <= 9);
                (weak ? words_weak : words_strong) += (double)(wk.size() - wk0);
                // the sieve looks at NINE bytes where the key window starts at an even position: the unit's 18-bit words
                // (a ninth exact byte, or what one edit leaves of the partner there)
                apm_enum_unit_windows(V.bytes.data() + dd.byte_off, u, S.code_shift, [&](uint32_t x18) { even18[x18 & 8191u] |= 1u << (x18 >> 13); v_even18[x18 & 8191u] |= 1u << (x18 >> 13); }, 9);
            }
            // packed pre-check record: byte offset of the exact part in the pattern pool | its length << 16 |
            // partner length << 24 (31 = beyond 16) | side << 29
            kext.push_back((uint32_t)(dd.byte_off + (uint32_t)u.off) | (std::min<uint32_t>((uint32_t)u.len, 255u) << 16) |
                           ((u.plen > 16 ? 31u : (uint32_t)u.plen) << 24) | ((uint32_t)u.side << 29));
            uint32_t rx, ry;
            apm_cf_record(V.bytes.data() + dd.byte_off, u, S.code_shift, &rx, &ry);
            krec.push_back(rx);
            krec.push_back(ry);
        }
        std::sort(wk.begin(), wk.end());
        wk.erase(std::unique(wk.begin(), wk.end()), wk.end());
        std::vector<uint32_t> bmp16(2048, 0u);
        std::vector<uint16_t> prefix(2048, 0), r2s, slots;
        for (size_t i = 0; i < wk.size();) {
            size_t j = i;
            while (j < wk.size() && (wk[j] >> 32) == (wk[i] >> 32)) ++j;
            const uint32_t xx = (uint32_t)(wk[i] >> 16) & 0xffffu;
            bmp16[xx & 2047u] |= 1u << (xx >> 11);
            seen16[xx & 8191u] |= (uint8_t)(1u << (xx >> 13));
            v_seen16[xx & 8191u] |= (uint8_t)(1u << (xx >> 13));
            if (j - i == 1) {
                r2s.push_back((uint16_t)(0x8000u | (wk[i] & 0x7fffu)));
            } else {
                r2s.push_back((uint16_t)slots.size());
                for (size_t z = i; z < j; ++z) slots.push_back((uint16_t)((wk[z] & 0x7fffu) | (z + 1 == j ? 0x8000u : 0u)));
            }
            i = j;
        }
        if (slots.size() >= 0x8000 || V.kinfo.size() > 0x7fffu) return APM_OK; // (15-bit slot / key indices; the splitting above keeps clear of it)
        uint32_t run = 0;
        for (int w = 0; w < 2048; ++w) {
            prefix[w] = (uint16_t)run;
            run += (uint32_t)__builtin_popcount(bmp16[w]);
        }
        auto append = [&](const void *src, size_t bytes) {
            const size_t at = V.image.size();
            V.image.resize(at + ((bytes + 15) & ~(size_t)15), 0);
            if (bytes) memcpy(V.image.data() + at, src, bytes);
            return (int)at;
        };
        append(bmp16.data(), bmp16.size() * 4); // = 0
        V.o_prefix = append(prefix.data(), prefix.size() * 2);
        V.o_r2s = append(r2s.data(), r2s.size() * 2);
        V.o_slots = append(slots.data(), slots.size() * 2);
        V.o_kext = append(kext.data(), kext.size() * 4);
        {
            std::vector<uint8_t> masks(17 * 16, 0);
            for (int n = 0; n <= 16; ++n)
                for (int b = 0; b < n; ++b) masks[(size_t)n * 16 + (size_t)b] = 0xff;
            V.o_masks = append(masks.data(), masks.size());
        }
        V.o_pat = append(V.bytes.data(), V.bytes.size());
        V.o_kinfo = append(V.kinfo.data(), V.kinfo.size() * 4);
        V.o_pinfo = append(V.pinfo.data(), V.pinfo.size() * 4);
        // sampled sets of up to 128 units: the operands of the fused form's REGISTER COMPARE, ready made -- per (unit, offset r
        // of the sampled block inside its piece, half t of the lane's 16 bytes) the codes of the pattern bytes that face the
        // lane's bytes, packed like the text, and the mask of the code bits the piece covers (apm_verify_body packs them
        // out of the pattern bytes otherwise: five LDS reads and four packs per hit).  16 bytes per (unit, r).
        V.o_rc = 0;
        static const int rc_env = getenv("APM_FUSED_RC") ? atoi(getenv("APM_FUSED_RC")) : 1; // (A/B aid: 0 = pack the operands per hit)
        if (rc_env && stride == 8 && units.size() <= 128) {
            std::vector<uint32_t> rc(units.size() * 8 * 4, 0u);
            for (size_t kid = 0; kid < units.size(); ++kid) {
                const int at = (int)(kext[kid] & 0xffffu), len = (int)((kext[kid] >> 16) & 0xffu);
                for (int r = 0; r < 8; ++r)
                    for (int t = 0; t < 2; ++t) {
                        const int sh8 = 8 * t - r; // lane byte i <-> pattern pool byte at - sh8 + i
                        const int i0 = sh8 > 0 ? sh8 : 0, i1 = len + sh8 < 16 ? len + sh8 : 16;
                        uint32_t pc = 0, mask = 0;
                        for (int i = i0; i < i1; ++i) {
                            pc |= (uint32_t)((V.bytes[(size_t)(at - sh8 + i)] >> S.code_shift) & 3) << (2 * i);
                            mask |= 3u << (2 * i);
                        }
                        rc[((kid * 8 + (size_t)r) * 2 + (size_t)t) * 2] = pc;
                        rc[((kid * 8 + (size_t)r) * 2 + (size_t)t) * 2 + 1] = mask;
                    }
            }
            V.o_rc = append(rc.data(), rc.size() * 4);
        }
        S.m_max = std::max(S.m_max, V.m_max);
        // the launch's own sieve pass (stride 1 with the code filter): the bitmap of ITS keys -- built like the set's below -- and
        // the code-filter tables over its key numbering.  A big set thus scans the text once per launch group, each pass
        // with a sparser bitmap and the filter in front of its verify launch: 2000 patterns of 50 bytes, k = 5, took one
        // sieve + five verify launches of 2.5 - 3 ms per GiB each; a sieve pass is 0.3 and its verify launch then near nothing.
        if (cf_on) {
            V.bitmap18.assign(8192, 0u);
            for (uint32_t x = 0; x < 65536u; ++x) {
                if (!((v_seen16[x & 8191u] >> (x >> 13)) & 1u)) continue;
                for (uint32_t f = 0; f < 4; ++f) {
                    const uint32_t c18 = (x << 2) | f;
                    V.bitmap18[c18 & 8191u] |= 1u << (c18 >> 13);
                }
            }
            for (uint32_t i = 0; i < 8192u; ++i) V.bitmap18[i] |= v_even18[i];
            // the third stage (ApmSieve2Args::cf_o_dp): window-DP slots for units of short patterns (m + 2k <= APM_CF_DP_COLS), the
            // units that show the sieve the most code words first (pair units of 8 bytes within one edit: ~10^-3 of all positions
            // each, nearly all of them rejected by the DP).  A unit without a slot keeps the filter's two stages.
            std::vector<uint32_t> dp_tab(4 * (APM_CF_DP_SLOTS + 1), 0u);
            {
                std::vector<size_t> nwords(units.size(), 0);
                for (uint64_t e : wk) ++nwords[e & 0x7fffu];
                std::vector<uint32_t> cand;
                for (size_t kid = 0; kid < units.size(); ++kid)
                    if ((int)V.descs[V.kinfo[kid] & 0xfffu].m + 2 * k <= APM_CF_DP_COLS) cand.push_back((uint32_t)kid);
                std::stable_sort(cand.begin(), cand.end(), [&](uint32_t x, uint32_t y) { return nwords[x] > nwords[y]; });
                if (cand.size() > APM_CF_DP_SLOTS) cand.resize(APM_CF_DP_SLOTS);
                V.cf_dp_slots = (int)cand.size();
                for (size_t i = 0; i < cand.size(); ++i) {
                    const uint32_t kid = cand[i], slot = (uint32_t)i + 1u;
                    const ApmPatDesc &dd = V.descs[V.kinfo[kid] & 0xfffu];
                    uint32_t b0 = 0, b1 = 0;
                    for (uint32_t y = 0; y < dd.m; ++y) {
                        const uint32_t code = (uint32_t)((V.bytes[dd.byte_off + y] >> S.code_shift) & 3);
                        b0 |= (code & 1u) << y;
                        b1 |= (code >> 1) << y;
                    }
                    const uint32_t cols = dd.m + 2u * (uint32_t)k;
                    dp_tab[4 * slot] = b0;
                    dp_tab[4 * slot + 1] = b1;
                    dp_tab[4 * slot + 2] = dd.m | ((uint32_t)units[kid].off << 8) | (cols << 16);
                    V.cf_dp_cols = std::max(V.cf_dp_cols, (int)cols);
                    krec[2 * kid + 1] |= slot << 28;
                }
            }
            std::vector<uint32_t> tbl(4096), rrec, lrec;
            for (int w = 0; w < 2048; ++w) { tbl[2 * w] = bmp16[w]; tbl[2 * w + 1] = prefix[w]; }
            for (size_t i = 0; i < wk.size();) { // (rank order, as r2s above)
                size_t j = i;
                while (j < wk.size() && (wk[j] >> 32) == (wk[i] >> 32)) ++j;
                if (j - i == 1) {
                    const uint32_t kid = (uint32_t)(wk[i] & 0x7fffu);
                    rrec.push_back(krec[2 * kid]);
                    rrec.push_back(krec[2 * kid + 1]);
                } else {
                    rrec.push_back(0xC0000000u | (uint32_t)(lrec.size() / 2));
                    rrec.push_back(0u);
                    for (size_t z = i; z < j; ++z) {
                        const uint32_t kid = (uint32_t)(wk[z] & 0x7fffu);
                        lrec.push_back(krec[2 * kid]);
                        lrec.push_back(krec[2 * kid + 1] | (z + 1 == j ? 0x80000000u : 0u));
                    }
                }
                i = j;
            }
            auto cf_append = [&](const std::vector<uint32_t> &v) {
                const size_t at = V.cf_image.size(), bytes = v.size() * 4;
                V.cf_image.resize(at + ((bytes + 15) & ~(size_t)15) + 16, 0); // (+16: a lane without a word reads record 0)
                if (bytes) memcpy(V.cf_image.data() + at, v.data(), bytes);
                return (int)at;
            };
            cf_append(tbl);
            V.cf_o_rrec = cf_append(rrec);
            V.cf_o_lrec = cf_append(lrec);
            V.cf_o_dp = V.cf_dp_slots ? cf_append(dp_tab) : 0;
            if (lrec.size() / 2 > 0xffffu) V.cf_image.clear(); // (list indices are 16 bits)
        }
        S.launches.push_back(std::move(V));
    }
    S.per_launch_sieve = cf_on && !S.launches.empty();
    for (const VerifyLaunch &V : S.launches)
        if (V.cf_image.empty()) S.per_launch_sieve = false;
    S.weak_frac = words_weak + words_strong > 0 ? words_weak / (words_weak + words_strong) : 0.0;
    // A single group whose hits nearly all come from such units gains nothing from the filter and pays its instructions
    // (60 patterns of 16 bytes, k = 3 -- pair units of 8 bytes: 0.395 -> 0.459 ms per 64 MiB); APM_SIEVE_CF=2 keeps it on.
    if (cf_env != 2 && S.launches.size() == 1 && S.weak_frac > 0.8) S.per_launch_sieve = false;
    // the sieve's bitmap.  Stride 1: over 9-byte windows at EVEN positions -- a key window may start at the even position
    // (the unit's own nine-byte words, apm_enum_unit_windows with W = 9) or at the odd one behind it (its 16-bit word x,
    // the first byte free).
    // Stride 8: the 16-bit words themselves (dword x & 2047, bit x >> 11).
    long pop16 = 0, pop18 = 0;
    for (uint32_t x = 0; x < 65536u; ++x) {
        if (!((seen16[x & 8191u] >> (x >> 13)) & 1u)) continue;
        ++pop16;
        if (stride == 8) {
            S.bitmap[x & 2047u] |= 1u << (x >> 11);
            continue;
        }
        for (uint32_t f = 0; f < 4; ++f) { // the key window starts at the odd position behind the lookup: the first byte is free
            const uint32_t c18 = (x << 2) | f;
            S.bitmap[c18 & 8191u] |= 1u << (c18 >> 13);
        }
    }
    if (stride == 1)
        for (uint32_t i = 0; i < 8192u; ++i) { // ... at the lookup's own position: the units' nine-byte words
            S.bitmap[i] |= even18[i];
            pop18 += __builtin_popcount(S.bitmap[i]);
        }
    S.rate = stride == 8 ? (double)pop16 / 65536.0 : (double)pop18 / 262144.0;
    S.on = !S.launches.empty();
    return APM_OK;
}

} // namespace
// ---------------------------------------------------------------------------
// plan: which kernel scans which pattern, in which launch
// ---------------------------------------------------------------------------
int wavefront_rows_per_lane(int m) {
    // minimise VALU work per window: steps (m + Lm - 1) x (overhead + 4R ops) / S windows per sweep
    int best_r = 0;
    double best = 1e30;
    for (int r : {1, 2, 4}) {
        const int lm = (m + r - 1) / r;
        if (lm > 64) continue;
        const int s = 64 / lm;
        const double cost = double(m + lm - 1) * (11.0 + 4.0 * r) / s;
        if (cost < best) { best = cost; best_r = r; }
    }
    return best_r; // 0: does not fit (m > 256)
}

// one window per wave (BITPAR, 1025 .. 4096 bytes): the pattern's Eq rows (64 or 128 words per distinct byte, + the "absent"
// row) must fit 60 KiB of LDS
bool bitlong_rows_fit(const PatternInfo &p) {
    bool seen[256] = {false};
    int nc = 1;
    for (unsigned char c : p.bytes) if (!seen[c]) { seen[c] = true; ++nc; }
    return (size_t)std::min(nc, 256) * (p.m <= 2048 ? 64 : 128) * 4 <= 60 * 1024;
}

int apm_build_plan(std::vector<PatternInfo> &pats, int k, int forced_kernel, ApmPlan *out, std::string *err) {
    ApmPlan &plan = *out;
    plan = ApmPlan();
    const int P = (int)pats.size();
    std::vector<uint32_t> raw_off(P);
    for (int i = 0; i < P; ++i) {
        std::string why;
        int kv = resolve_kernel(forced_kernel, pats[i].m, k, &why);
        if (kv == -100) return plan_fail(err, APM_ERR_UNSUPPORTED, "pattern %d (length %d): %s", i, pats[i].m, why.c_str());
        if (kv == APM_KERNEL_NFA) { // every distinct pattern byte is a class of the launch: at most 16
            bool seen[256] = {false};
            int nc = 0;
            for (unsigned char c : pats[i].bytes) if (!seen[c]) { seen[c] = true; ++nc; }
            if (nc > 16) {
                if (forced_kernel == APM_KERNEL_NFA)
                    return plan_fail(err, APM_ERR_UNSUPPORTED, "pattern %d (length %d): NFA kernel takes at most 16 distinct pattern bytes", i, pats[i].m);
                kv = APM_KERNEL_BITPAR;
            }
        }
        if (kv == APM_KERNEL_BITPAR && pats[i].m > 1024) {
            if (!bitlong_rows_fit(pats[i])) {
                if (forced_kernel == APM_KERNEL_BITPAR)
                    return plan_fail(err, APM_ERR_UNSUPPORTED, "pattern %d (length %d): BITPAR beyond 1024 bytes needs an alphabet whose Eq rows fit 60 KiB of LDS", i, pats[i].m);
                kv = APM_KERNEL_GENERIC;
            }
        }
        pats[i].kernel = kv;
        raw_off[i] = (uint32_t)plan.allpat.size();
        plan.allpat.insert(plan.allpat.end(), pats[i].bytes.begin(), pats[i].bytes.end());
        if (kv == KERNEL_TRIVIAL) { plan.trivial.push_back(i); continue; }
        plan.m_max = std::max(plan.m_max, pats[i].m);
        ApmPatDesc d{};
        d.m = (uint32_t)pats[i].m;
        d.byte_off = raw_off[i];
        d.index = (uint32_t)i;
        if (kv == APM_KERNEL_BITPAR && pats[i].m > 1024) {
            // (the one-window-per-wave kernel evaluates its truncated windows itself)
        } else if (kv != APM_KERNEL_GENERIC) { // GENERIC scans truncated windows itself (mode 2)
            GenericGroup &tg = pats[i].m <= 128 ? plan.stails : (pats[i].m <= 512 ? plan.wtails : plan.xtails);
            tg.descs.push_back(d);
            tg.m_max = std::max(tg.m_max, pats[i].m);
        } else {
            plan.longs.descs.push_back(d);
            plan.longs.m_max = std::max(plan.longs.m_max, pats[i].m);
        }
    }

    // ---- BITPAR launches: group by LDS table budget; one text->code LUT per launch ----
    {
        std::vector<int> idx;
        for (int i = 0; i < P; ++i) if (pats[i].kernel == APM_KERNEL_BITPAR) idx.push_back(i);
        // width classes, each with launches (and kernels) of its own, picked by the launch's m_max (apm_launch_bitpar):
        // <= 128 bytes (1 - 4 words per column), <= 512 (8 / 16: a register-hungry instantiation), <= 1024 (24 / 32 words,
        // one-pass column step: apm_bitlong.hip), <= 4096 (one window per WAVE, one pattern per launch: apm_bitlong.hip)
        auto width_class = [](int m) { return m <= 128 ? 0 : (m <= 512 ? 1 : (m <= 1024 ? 2 : 3)); };
        std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return width_class(pats[x].m) < width_class(pats[y].m); });
        size_t pos = 0;
        while (pos < idx.size()) {
            TiledLaunch L;
            L.kind = APM_KERNEL_BITPAR;
            const int wclass = width_class(pats[idx[pos]].m);
            L.tile = 1024;
            bool present[256] = {false};
            int n_codes = 1; // code 0 = absent
            size_t words = 0;
            std::vector<int> members;
            while (pos < idx.size() && members.size() < (wclass == 3 ? 1u : 1024u)) {
                const PatternInfo &pi = pats[idx[pos]];
                if (width_class(pi.m) != wclass) break;
                bool p2[256];
                memcpy(p2, present, sizeof p2);
                int nc = n_codes;
                for (unsigned char c : pi.bytes) if (!p2[c]) { p2[c] = true; ++nc; }
                const int entries = nc > 256 ? 256 : nc;
                // every member's table is re-laid with the launch's final code count: bound with `entries`
                size_t w_total = 0;
                auto stride_of = [](int m) { const int w = (m + 31) / 32; return w <= 2 ? w : (w <= 4 ? 4 : (w <= 8 ? 8 : (w <= 16 ? 16 : (w <= 24 ? 24 : (w <= 32 ? 32 : (w <= 64 ? 64 : 128)))))); };
                for (int mi : members) w_total += (size_t)entries * stride_of(pats[mi].m);
                w_total += (size_t)entries * stride_of(pi.m);
                if (!members.empty() && w_total * 4 > APM_LDS_TABLE_BUDGET) break;
                memcpy(present, p2, sizeof present);
                n_codes = nc;
                members.push_back(idx[pos]);
                ++pos;
                words = w_total;
            }
            (void)words;
            // LUT: 256 distinct bytes => identity, no "absent" code
            const bool full = n_codes > 256;
            int next = 1;
            for (int c = 0; c < 256; ++c) L.lut[c] = full ? (uint8_t)c : (present[c] ? (uint8_t)next++ : 0);
            const int entries = full ? 256 : n_codes;
            for (int mi : members) {
                const PatternInfo &pi = pats[mi];
                ApmPatDesc d{};
                d.m = (uint32_t)pi.m;
                const uint32_t w32 = (uint32_t)((pi.m + 31) / 32);      // words of the bit vector: 1, 2, 3, 4, then 8, 16, 24, 32; one window
                d.w = w32 <= 4 ? w32 : (w32 <= 8 ? 8u : (w32 <= 16 ? 16u : (w32 <= 24 ? 24u : (w32 <= 32 ? 32u : (w32 <= 64 ? 64u : 128u))))); // per wave: 64, 128 (the rows past m never reach the distance)
                d.stride = d.w == 3 ? 4 : d.w;
                d.index = (uint32_t)mi;
                d.byte_off = 0;
                while (L.tables.size() % 4) L.tables.push_back(0);
                d.aux_off = (uint32_t)L.tables.size();
                L.tables.resize(L.tables.size() + (size_t)entries * d.stride, 0u);
                for (int y = 0; y < pi.m; ++y) {
                    const uint32_t code = L.lut[(unsigned char)pi.bytes[y]];
                    L.tables[d.aux_off + (size_t)code * d.stride + (y >> 5)] |= 1u << (y & 31);
                }
                L.descs.push_back(d);
                L.m_max = std::max(L.m_max, pi.m);
                L.m_min = L.m_min ? std::min(L.m_min, pi.m) : pi.m;
            }
            plan.tiled.push_back(std::move(L));
        }
    }
    // ---- NFA launches: <= 16 byte classes and <= 512 patterns per launch ----
    {
        std::vector<int> idx;
        for (int i = 0; i < P; ++i) if (pats[i].kernel == APM_KERNEL_NFA) idx.push_back(i);
        for (size_t pos = 0; pos < idx.size();) {
            TiledLaunch L;
            L.kind = APM_KERNEL_NFA;
            memset(L.lut, 0, sizeof L.lut);
            int cls_of[256];
            for (int c = 0; c < 256; ++c) cls_of[c] = -1;
            int nc = 0;
            for (; pos < idx.size() && L.descs.size() < 512; ++pos) {
                const PatternInfo &pi = pats[idx[pos]];
                int add = 0;
                bool seen[256] = {false};
                for (unsigned char c : pi.bytes) if (cls_of[c] < 0 && !seen[c]) { seen[c] = true; ++add; }
                if (!L.descs.empty() && nc + add > 16) break;
                for (unsigned char c : pi.bytes) if (cls_of[c] < 0) { cls_of[c] = nc; L.lut[nc++] = c; }
                ApmPatDesc d{};
                d.m = (uint32_t)pi.m;
                d.index = (uint32_t)idx[pos];
                d.byte_off = (uint32_t)L.bytes.size();
                // 16 bytes per pattern: the class number of pattern byte x in nibble x (the kernel reads them with one
                // scalar 16-byte load and shifts the next one out per column)
                L.bytes.resize(L.bytes.size() + 16, 0);
                for (size_t x = 0; x < pi.bytes.size(); ++x)
                    L.bytes[d.byte_off + x / 2] |= (uint8_t)(cls_of[(unsigned char)pi.bytes[x]] << (4 * (x & 1)));
                L.descs.push_back(d);
                L.m_max = std::max(L.m_max, pi.m);
                L.m_min = L.m_min ? std::min(L.m_min, pi.m) : pi.m;
            }
            L.nb = nc; // classes; their bytes: lut[0 .. nc)
            plan.tiled.push_back(std::move(L));
        }
    }
    // ---- WAVEFRONT launches: up to 64 patterns, raw bytes in LDS ----
    {
        std::vector<int> idx;
        for (int i = 0; i < P; ++i) if (pats[i].kernel == APM_KERNEL_WAVEFRONT) idx.push_back(i);
        for (size_t pos = 0; pos < idx.size();) {
            TiledLaunch L;
            L.kind = APM_KERNEL_WAVEFRONT;
            L.tile = 512;
            memset(L.lut, 0, sizeof L.lut);
            for (; pos < idx.size() && L.descs.size() < 64; ++pos) {
                const PatternInfo &pi = pats[idx[pos]];
                ApmPatDesc d{};
                d.m = (uint32_t)pi.m;
                d.w = (uint32_t)wavefront_rows_per_lane(pi.m);
                d.index = (uint32_t)idx[pos];
                d.byte_off = (uint32_t)L.bytes.size();
                L.bytes.insert(L.bytes.end(), pi.bytes.begin(), pi.bytes.end());
                L.descs.push_back(d);
                L.m_max = std::max(L.m_max, pi.m);
                L.m_min = L.m_min ? std::min(L.m_min, pi.m) : pi.m;
            }
            plan.tiled.push_back(std::move(L));
        }
    }

    // ---- sieve + verify pipeline (apm_sieve.hip): as soon as one BANDED pattern needs every text position looked at
    // (pieces shorter than 15 bytes), ONE sieve pass serves all BANDED patterns of the set -- those with longer
    // pieces join with one key per piece instead of a sampled family -- and the verify launches work off its
    // candidate list.  The LDS-tile / stream launches of the same patterns are still planned below: they run as
    // for text the sieve cannot take (unaligned, >= 4 GiB).
    // APM_SIEVE=0 switches the pipeline off (A/B aid). ----
    {
        static const int sieve_env = getenv("APM_SIEVE") ? atoi(getenv("APM_SIEVE")) : 1;
        bool has_s1 = false, has_banded = false;
        size_t stream_keys = 0, stream_bytes = 0, n_banded = 0; // what one stream launch would have to hold (limits of the class loop below)
        for (int i = 0; i < P; ++i) {
            if (pats[i].kernel != APM_KERNEL_BANDED) continue;
            has_banded = true;
            const int piece = pats[i].m / (k + 1);
            if (piece < 15) has_s1 = true;
            stream_keys += (size_t)(k + 1) * (piece >= 31 ? 16u : 8u);
            stream_bytes += (size_t)pats[i].m;
            ++n_banded;
        }
        const bool stream_splits = stream_keys > 4096 || stream_bytes > 16384 || n_banded > 1024;
        // sets of long pieces only: the sampled form of the pipeline (one lookup per 8 bytes, sieve and verification fused
        // in one launch) when verification is the heavy part (k >= 2: pair pre-check + banded DP, which stall the stream
        // kernel's loads) or when the set is too big for ONE stream launch (1000 patterns of 32, k = 0: four stream
        // launches 0.60 ms per 256 MiB, two fused ones 0.23); a small set with k <= 1 stays on the stream kernel, which
        // sits on the HBM ceiling there (cfg2: 0.046 ms against 0.060) -- tools/sampled_k_probe.py
        const int stride = has_s1 ? 1 : 8;
#ifdef APM_MEASURE
        static const int sampled_min_k = getenv("APM_SAMPLED_MIN_K") ? atoi(getenv("APM_SAMPLED_MIN_K")) : 2;
#else
        constexpr int sampled_min_k = 2;
#endif
        if (sieve_env && has_banded && (has_s1 || k >= sampled_min_k || stream_splits)) {
            const int rc = build_sieve_plan(pats, k, plan.sieve, stride);
            if (rc) return rc;
        }
    }

    // ---- BANDED launches: patterns grouped by (key length, sampling stride); k+1 pigeonhole pieces each ----
    for (int cls = 0; cls < 5; ++cls) {
        static const int kl_of[5] = {16, 8, 8, 6, 4}, st_of[5] = {16, 8, 1, 1, 1};
        const int klen = kl_of[cls];
        const int stride = st_of[cls];
        auto class_of = [&](int m) {
            const int piece = m / (k + 1);
            if (plan.sieve.on && plan.sieve.stride == 1 && piece >= 8) return 2; // (same coverage as the sieve pipeline: these launches are its fallback)
            return piece >= 31 ? 0 : (piece >= 15 ? 1 : (piece >= 8 ? 2 : (piece >= 6 ? 3 : 4)));
        };
        std::vector<int> idx;
        for (int i = 0; i < P; ++i)
            if (pats[i].kernel == APM_KERNEL_BANDED && class_of(pats[i].m) == cls) idx.push_back(i);
        auto dword = [](const unsigned char *b) {
            return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        };
        auto fp8 = [](uint32_t lo, uint32_t hi) { return lo + (hi << 3); };
        auto slot_hash = [](uint32_t f) {
            return (uint32_t)((uint64_t)(f & 0xffffffu) * 0x9E3779u) + (uint32_t)((uint64_t)((f >> 12) & 0xffffffu) * 0x85EBCAu);
        };
        for (size_t pos = 0; pos < idx.size();) {
            TiledLaunch L;
            L.kind = APM_KERNEL_BANDED;
            L.key_len = klen;
            L.stride = stride;
            L.sieved = plan.sieve.on && (stride == 1 || plan.sieve.stride == 8);
            L.qcap = stride == 1 ? 1024 : 512;
            memset(L.lut, 0, sizeof L.lut);
            const int pieces = k + 1;
            for (; pos < idx.size(); ++pos) {
                const PatternInfo &pi = pats[idx[pos]];
#ifdef APM_MEASURE
                static const size_t max_keys = getenv("APM_MAX_KEYS") ? std::min<size_t>(32767, std::max<long>(1, atol(getenv("APM_MAX_KEYS")))) : 4096;
#else
                constexpr size_t max_keys = 4096; // (15-bit key ids: never above 32767)
#endif
                if (!L.descs.empty() && (L.bytes.size() + (size_t)pi.m > 16384 ||
                                         L.keys.size() + (size_t)pieces * stride > max_keys || L.descs.size() >= 1024 ||
                                         L.piece_off.size() + (size_t)pieces > 60000))
                    break;
                ApmPatDesc d{};
                d.m = (uint32_t)pi.m;
                d.index = (uint32_t)idx[pos];
                d.byte_off = (uint32_t)L.bytes.size();
                d.aux_off = (uint32_t)L.piece_off.size();
                d.w = (uint32_t)pieces;
                L.bytes.insert(L.bytes.end(), pi.bytes.begin(), pi.bytes.end());
                for (int q = 0; q < pieces; ++q) {
                    const int aq = (int)((int64_t)q * pi.m / pieces);
                    L.piece_off.push_back((uint16_t)aq);
                    for (int r = 0; r < stride; ++r) {
                        unsigned char b[16] = {0}; // key bytes, zero padded past the end of the pattern
                        for (int z = 0; z < klen && aq + r + z < pi.m; ++z) b[z] = (unsigned char)pi.bytes[aq + r + z];
                        ApmKey key{};
                        key.pat = (uint16_t)L.descs.size();
                        key.off = (uint16_t)(aq + r);
                        key.piece = (uint16_t)q;
                        key.next = 0;
                        if (klen == 16) key.fp = fp8(dword(b), dword(b + 4)) + (fp8(dword(b + 8), dword(b + 12)) & 0xffffffu) * 0x9E3779u;
                        else if (klen == 4) key.fp = dword(b);
                        else key.fp = fp8(dword(b), dword(b + 4)); // bytes past klen are zero (masked on the device)
                        L.keys.push_back(key);
                        L.a_max = std::max(L.a_max, aq + r);
                    }
                }
                L.descs.push_back(d);
                L.m_max = std::max(L.m_max, pi.m);
                L.m_min = L.m_min ? std::min(L.m_min, pi.m) : pi.m;
            }
            const int band = k / 2;
            const int front = band > 0 ? 16 : 0;
            L.tile = (APM_FILTER_POS - front - L.m_max - band) & ~31; // every window + its keys inside 4096 staged bytes
            while (L.bytes.size() % 16) L.bytes.push_back(0);
            // compact per-key / per-pattern records the verify stage reads from LDS
            for (const ApmKey &kk : L.keys)
                L.kinfo.push_back((uint32_t)kk.pat | ((uint32_t)kk.off << 12) | ((uint32_t)kk.piece << 21));
            for (const ApmPatDesc &dd : L.descs) {
                L.pinfo.push_back(dd.byte_off | (dd.m << 16));
                L.pinfo.push_back(dd.aux_off);
            }
            // hash table: 8-way buckets of 16-bit tags (low half of the slot hash), bucket = top bits;
            // keys with equal tags in one bucket are chained behind a single entry
            int nb = 16, lg = 4;
            while (nb * 2 < (int)L.keys.size() && nb < 512) { nb *= 2; ++lg; }
            for (;;) {
                L.table.assign((size_t)nb * 8, 0xffffu);
                L.table_kid.assign((size_t)nb * 8, 0xffffu);
                L.ovf.clear();
                std::vector<int> fill((size_t)nb, 0);
                for (auto &kk : L.keys) kk.next = 0;
                for (size_t kid = 0; kid < L.keys.size(); ++kid) {
                    const uint32_t h = klen == 16 ? L.keys[kid].fp : slot_hash(L.keys[kid].fp);
                    const uint32_t slot = h >> (32 - lg);
                    const uint16_t tag = (uint16_t)(h & 0xffffu);
                    int head = -1;
                    uint16_t *head_kid = nullptr;
                    for (int wv = 0; wv < fill[slot]; ++wv)
                        if (L.table[slot * 8 + wv] == tag) {
                            head = L.table_kid[slot * 8 + wv] & 0x7fff;
                            head_kid = &L.table_kid[slot * 8 + wv];
                        }
                    uint32_t *head_ovf = nullptr;
                    if (head < 0)
                        for (size_t o = 0; o + 1 < L.ovf.size(); o += 2)
                            if (L.ovf[o] == tag && (L.ovf[o + 1] >> 16) == slot) {
                                head = (int)(L.ovf[o + 1] & 0x7fff);
                                head_ovf = &L.ovf[o + 1];
                            }
                    if (head >= 0) { // chain behind the existing entry with this tag
                        int tail = head;
                        while (L.keys[tail].next) tail = L.keys[tail].next - 1;
                        L.keys[tail].next = (uint16_t)(kid + 1);
                        if (head_kid) *head_kid |= 0x8000u;
                        if (head_ovf) *head_ovf |= 0x8000u;
                    } else if (fill[slot] < 8) {
                        L.table[slot * 8 + fill[slot]] = tag;
                        L.table_kid[slot * 8 + fill[slot]] = (uint16_t)kid;
                        ++fill[slot];
                    } else {
                        L.ovf.push_back(tag);
                        L.ovf.push_back((uint32_t)kid | (slot << 16));
                    }
                }
                if (L.ovf.size() / 2 <= 4 || nb >= 1024) break;
                nb *= 2;
                ++lg;
            }
            for (size_t o = 1; o < L.ovf.size(); o += 2) L.ovf[o] &= 0xffffu; // drop the slot annotation
            L.nb = nb;
            L.lg_nb = lg;
            // one contiguous image, laid out exactly like its LDS copy
            auto append = [&](const void *src, size_t bytes) {
                const size_t at = L.image.size();
                L.image.resize(at + ((bytes + 15) & ~(size_t)15), 0);
                if (bytes) memcpy(L.image.data() + at, src, bytes);
                return (int)at;
            };
            if (stride == 1) {
                // First-level filter of the per-position classes: a presence bitmap indexed by the 2-bit
                // codes (b >> s) & 3 of the key bytes.  s is picked to spread this launch's pattern bytes
                // over the four codes as evenly as possible (s = 1 separates A,C,G,T and a,c,g,t exactly).
                long best = -1;
                for (int sft = 0; sft < 7; ++sft) {
                    long hist[4] = {0, 0, 0, 0};
                    for (const ApmPatDesc &dd : L.descs)
                        for (uint32_t y = 0; y < dd.m; ++y) ++hist[(L.bytes[dd.byte_off + y] >> sft) & 3];
                    const long score = std::min(std::min(hist[0], hist[1]), std::min(hist[2], hist[3])) * 4 +
                                       (hist[0] > 0) + (hist[1] > 0) + (hist[2] > 0) + (hist[3] > 0) + (sft == 1);
                    if (score > best) { best = score; L.code_shift = sft; }
                }
                std::vector<uint8_t> bmp(8192, 0); // over 8-byte code words whatever the key length
                for (const ApmKey &kk : L.keys) mark_key_windows(bmp, L, kk, pieces, L.code_shift, k / 2 >= 1);
                L.o_bmp = append(bmp.data(), bmp.size()); // = 0: a compile-time LDS address for the probes
            }
            L.o_pat = append(L.bytes.data(), L.bytes.size());
            L.o_tab = append(L.table.data(), L.table.size() * 2);
            L.o_kid = append(L.table_kid.data(), L.table_kid.size() * 2);
            L.o_ovf = append(L.ovf.data(), L.ovf.size() * 4);
            L.o_kinfo = append(L.kinfo.data(), L.kinfo.size() * 4);
            L.o_pinfo = append(L.pinfo.data(), L.pinfo.size() * 4);
            std::vector<uint16_t> nxt;
            for (const ApmKey &kk : L.keys) nxt.push_back(kk.next);
            L.o_next = append(nxt.data(), nxt.size() * 2);
            L.o_poff = append(L.piece_off.data(), L.piece_off.size() * 2);
            if (stride == 1) { // one packed record per key for the pair pre-check (see ApmFilterArgs::o_kext)
                std::vector<uint32_t> kext;
                for (const ApmKey &kk : L.keys) {
                    const ApmPatDesc &dd = L.descs[kk.pat];
                    auto piece_begin = [&](int q) { return q >= pieces ? (int)dd.m : (int)L.piece_off[dd.aux_off + q]; };
                    const int q = kk.piece, pq = q ^ 1;
                    const uint32_t len = (uint32_t)(piece_begin(q + 1) - piece_begin(q));
                    uint32_t side = 0, plen = 0;
                    if (pq < pieces) {
                        side = pq > q ? 1u : 2u;
                        plen = (uint32_t)(piece_begin(pq + 1) - piece_begin(pq));
                    }
                    kext.push_back((uint32_t)(dd.byte_off + kk.off) | (std::min<uint32_t>(len, 255u) << 16) |
                                   ((plen > 16 ? 31u : plen) << 24) | (side << 29));
                }
                L.o_kext = append(kext.data(), kext.size() * 4);
            }
            if (stride == 1) {
                // the tile kernel's LDS: 4 tile buffers + image + 2 queues + counters + survivor lists (see
                // apm_filter_lds_bytes); a big image (cfg5: 57 KB) leaves room for two workgroups per CU only with
                // the smaller candidate queue -- overflowing it is correct, just slow (dense pass)
                auto lds_with = [&](int qcap) {
                    return (size_t)4 * APM_FILTER_POS + L.image.size() + 2 * (size_t)qcap * 4 + ((L.descs.size() + 3) & ~(size_t)3) * 4 + 32 + 2048 + 16;
                };
                const size_t cu_lds = 160 * 1024;
                if (cu_lds / lds_with(512) > cu_lds / lds_with(1024)) L.qcap = 512;
            }
            plan.tiled.push_back(std::move(L));
        }
    }
    return APM_OK;
}
