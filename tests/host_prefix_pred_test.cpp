// Host test of the prefix form of the nomination predicate (csrc/apm_core.h, apm_unit_pred16; no GPU, own main).
// For every nomination unit of a pattern -- split as the plan builder's units_of splits it -- and every text position
// near the unit's place in a text built from the pattern with 0..k+2 edits, it asserts
//   (a) the full predicate (byte loops over the whole exact part and the whole partner, as the sampled sets keep it)
//       implies the prefix form: no window the pigeonhole argument relies on is lost;
//   (b) the prefix form implies that the position's 16-bit code word, and its 18-bit word over nine bytes, is among the
//       unit's enumerated words (apm_enum_unit_windows): the sieve's bitmaps and the verify image's key lists show it;
//   (c) the prefix form implies apm_cf_pass on the codes: the sieve's code filter lets the position through.
// (b) and (c) are what makes the dedup's "first true nominator" an item that really ran.
// Prints "<checks> checks, <n> wrong"; the counts of positions at which only the prefix form holds show that the texts
// reach the case the change is about.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "apm_core.h"

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    g_rng = apm_splitmix64(g_rng);
    return (uint32_t)((g_rng >> 20) % n);
}

// csrc/apm_plan.cpp, units_of
static size_t count_words(const uint8_t *pat, const std::vector<ApmUnit> &us, int shift) {
    std::vector<uint32_t> w;
    for (const ApmUnit &u : us) apm_enum_unit_windows(pat, u, shift, [&](uint32_t x) { w.push_back(x); });
    std::sort(w.begin(), w.end());
    return (size_t)(std::unique(w.begin(), w.end()) - w.begin());
}
static std::vector<ApmUnit> units_of(const uint8_t *pat, int m, int k, int shift) {
    const int pieces = k + 1;
    const bool pairs = k / 2 >= 1;
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
        if (lenA + lenB <= 16 && lenA < 8 && lenB < 8 && count_words(pat, by_pair, shift) < count_words(pat, by_piece, shift)) us.push_back(by_pair[0]);
        else us.insert(us.end(), by_piece.begin(), by_piece.end());
    }
    return us;
}

struct Text {
    std::vector<uint8_t> b;
    int at(int64_t i) const { return i < 0 || i >= (int64_t)b.size() ? 0 : b[(size_t)i]; } // outside the text: zero, as the kernels read it
};

// the full predicate, byte by byte (apm_verify.hip, stage1 without PREFIX; apm_ext_fwd / apm_ext_bwd semantics)
static bool pred_full(const uint8_t *pat, const ApmUnit &u, const Text &t, int64_t s) {
    if (s + u.len > (int64_t)t.b.size()) return false;
    for (int x = 0; x < u.len; ++x)
        if (t.at(s + x) != pat[u.off + x]) return false;
    if (u.side == 0) return true;
    const bool fwd = u.side == 1;
    const int nn = u.plen;
    auto T = [&](int i) { return fwd ? t.at(s + u.len + i) : t.at(s - 1 - i); };
    auto P = [&](int i) { return fwd ? (int)pat[u.poff + i] : (int)pat[u.poff + nn - 1 - i]; };
    int i = 0;
    while (i < nn && T(i) == P(i)) ++i;
    if (i >= nn - 1) return true;
    bool ok = true;
    for (int j = i + 1; j < nn && ok; ++j) ok = T(j) == P(j);
    if (ok) return true;
    ok = true;
    for (int j = i + 1; j < nn && ok; ++j) ok = T(j - 1) == P(j);
    if (ok) return true;
    ok = true;
    for (int j = i; j < nn && ok; ++j) ok = T(j + 1) == P(j);
    return ok;
}

// the prefix form through apm_unit_pred16, its operands gathered as stage1 gathers them
static bool pred_prefix(const uint8_t *pat, int m, const ApmUnit &u, const Text &t, int64_t s) {
    if (s + u.len > (int64_t)t.b.size()) return false;
    uint8_t tb[16] = {0}, tpb[20] = {0}, pb[16] = {0}, ppb[16] = {0};
    for (int i = 0; i < 16; ++i) tb[i] = (uint8_t)t.at(s + i);
    for (int i = 0; i < 16; ++i) pb[i] = u.off + i < m ? pat[u.off + i] : (uint8_t)(0xa5 + i); // (beyond the part: whatever the pool holds)
    for (int i = 0; i < 20; ++i) tpb[i] = (uint8_t)(u.side == 1 ? t.at(s + u.len + i) : t.at(s - 1 - i));
    for (int i = 0; i < 16; ++i) {
        const int y = u.side == 1 ? u.poff + i : u.poff + u.plen - 1 - i; // the partner's byte i, read away from the exact part
        ppb[i] = (u.side != 0 && y >= 0 && y < m) ? pat[y] : (uint8_t)(0x5a + i);
    }
    uint32_t tw[4], tpw[5], pw[4], ppw[4];
    memcpy(tw, tb, 16); memcpy(tpw, tpb, 20); memcpy(pw, pb, 16); memcpy(ppw, ppb, 16);
    return apm_unit_pred16(tw, tpw, pw, ppw, u.len, u.plen, u.side);
}

static uint32_t codes(const Text &t, int64_t from, int step, int n, int shift) {
    uint32_t x = 0;
    for (int i = 0; i < n; ++i) x |= (uint32_t)((t.at(from + (int64_t)step * i) >> shift) & 3) << (2 * i);
    return x;
}

int main() {
    long checks = 0, wrong = 0, n_full = 0, n_prefix_only = 0, n_patterns = 0;
    auto fail = [&](const char *what, int m, int k, size_t ui, int64_t s) {
        if (wrong++ < 20) printf("WRONG %s: m %d k %d unit %zu position %lld\n", what, m, k, ui, (long long)s);
    };
    std::vector<int> ms;
    for (int m = 17; m <= 140; ++m) ms.push_back(m);
    for (int m : {150, 171, 200, 255, 256, 257, 300, 384, 511, 512}) ms.push_back(m);
    static const char *const alphabets[] = {"ACGT", "A", "AC", "ACGT"}; // [3]: a tandem repeat of period 5
    for (int m : ms)
        for (int k = 0; k <= 7; ++k) {
            if (m > 140 && (k & 1) && k != 7) continue; // (the long ones: every band once)
            const int kind = (int)rnd(8) < 5 ? 0 : 1 + (int)rnd(3);
            const char *al = alphabets[kind];
            const int na = (int)strlen(al), shift = 1; // (bits 1..2 separate A, C, G, T)
            std::vector<uint8_t> pat((size_t)m);
            for (int i = 0; i < m; ++i) pat[(size_t)i] = (uint8_t)(kind == 3 ? (i < 5 ? al[rnd(4)] : pat[(size_t)i - 5]) : al[rnd((uint32_t)na)]);
            const std::vector<ApmUnit> us = units_of(pat.data(), m, k, shift);
            ++n_patterns;
            std::vector<std::vector<bool>> w16(us.size()), w18(us.size());
            std::vector<uint32_t> rx(us.size()), ry(us.size());
            for (size_t ui = 0; ui < us.size(); ++ui) {
                w16[ui].assign(1u << 16, false);
                w18[ui].assign(1u << 18, false);
                apm_enum_unit_windows(pat.data(), us[ui], shift, [&](uint32_t x) { w16[ui][x & 0xffffu] = true; });
                apm_enum_unit_windows(pat.data(), us[ui], shift, [&](uint32_t x) { w18[ui][x & 0x3ffffu] = true; }, 9);
                apm_cf_record(pat.data(), us[ui], shift, &rx[ui], &ry[ui]);
            }
            const int n_texts = m > 140 ? 6 : 10;
            for (int ti = 0; ti < n_texts; ++ti) {
                // the pattern with e edits, placed by zone: an exact part or a partner, in front of or behind its 16th byte
                // counted from the seam between the two
                const int e = ti == 0 ? 0 : (int)rnd((uint32_t)k + 3);
                std::vector<int> where;
                for (int j = 0; j < e; ++j) {
                    const ApmUnit &u = us[rnd((uint32_t)us.size())];
                    const int zone = (int)rnd(5);
                    int y = (int)rnd((uint32_t)m);
                    if (zone == 0 && u.len > 0) y = u.off + (int)rnd((uint32_t)std::min(u.len, 16));
                    if (zone == 1 && u.len > 16) y = u.off + 16 + (int)rnd((uint32_t)(u.len - 16));
                    if (zone == 2 && u.side != 0) { const int d = (int)rnd((uint32_t)std::min(u.plen, 16)); y = u.side == 1 ? u.poff + d : u.poff + u.plen - 1 - d; }
                    if (zone == 3 && u.side != 0 && u.plen > 16) { const int d = 16 + (int)rnd((uint32_t)(u.plen - 16)); y = u.side == 1 ? u.poff + d : u.poff + u.plen - 1 - d; }
                    where.push_back(y);
                }
                std::sort(where.begin(), where.end(), [](int x, int y) { return x > y; });
                std::vector<uint8_t> body(pat);
                for (int y : where) {
                    if ((size_t)y >= body.size()) continue; // (two deletions at the last byte)
                    const int type = (int)rnd(3);
                    const uint8_t c = (uint8_t)"ACGT"[rnd(4)];
                    if (type == 0) body[(size_t)y] = body[(size_t)y] == c ? (uint8_t)(c == 'A' ? 'C' : 'A') : c;
                    else if (type == 1) body.insert(body.begin() + y, c);
                    else if (body.size() > 1) body.erase(body.begin() + y);
                }
                Text t;
                const int lead = ti % 3 == 1 ? (int)rnd(20) : 24 + (int)rnd(16), trail = ti % 3 == 2 ? (int)rnd(20) : 24 + (int)rnd(16);
                for (int i = 0; i < lead; ++i) t.b.push_back((uint8_t)al[rnd((uint32_t)na)]);
                t.b.insert(t.b.end(), body.begin(), body.end());
                for (int i = 0; i < trail; ++i) t.b.push_back((uint8_t)al[rnd((uint32_t)na)]);
                for (size_t ui = 0; ui < us.size(); ++ui) {
                    const ApmUnit &u = us[ui];
                    for (int64_t s = lead + u.off - k - 4; s <= lead + u.off + k + 4; ++s) {
                        if (s < 0 || s >= (int64_t)t.b.size()) continue;
                        const bool full = pred_full(pat.data(), u, t, s), pre = pred_prefix(pat.data(), m, u, t, s);
                        ++checks;
                        n_full += full;
                        n_prefix_only += pre && !full;
                        if (full && !pre) fail("full predicate true, prefix form false", m, k, ui, s);
                        if (!pre) continue;
                        if (!w16[ui][codes(t, s, 1, 8, shift)]) fail("16-bit word not enumerated", m, k, ui, s);
                        if (!w18[ui][codes(t, s, 1, 9, shift)]) fail("18-bit word not enumerated", m, k, ui, s);
                        const uint32_t c0 = codes(t, s, 1, 16, shift);
                        const uint32_t tw = u.side == 2 ? codes(t, s - 1, -1, 16, shift) : codes(t, s + u.len, 1, 16, shift);
                        if (!apm_cf_pass(rx[ui], ry[ui], c0, tw, true)) fail("apm_cf_pass false", m, k, ui, s);
                    }
                }
            }
        }
    printf("%ld patterns, %ld positions with the full predicate true, %ld with the prefix form alone\n", n_patterns, n_full, n_prefix_only);
    if (n_full < 1000 || n_prefix_only < 100) { printf("WRONG: the texts do not reach the cases\n"); ++wrong; }
    printf("%ld checks, %ld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
