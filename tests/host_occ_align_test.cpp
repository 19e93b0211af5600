// Host test of csrc/apm_occ_align.h (g++, address and undefined-behaviour sanitizers, no GPU): the script of one occurrence
// against a literal full-matrix DP and the pinned rule, both written here.  W = 1..4; m at 1, 2, 31, 32, 33, 63, 64, 65, 96,
// 97, 127, 128 (and the small m up to 12); k from 0 to m - 1 for m <= 12, k in {0, 1, 7, m / 2, m - 1} beyond; every text length
// L in [max(1, m - k), m + k] for the small m, the extremes and L = m beyond; the bytes 0x00, 0xFF and '\n'; pairs farther than
// k (0, nothing stored) and tie-rich pairs (homopolymers, ACG repeats).
#include "apm_occ_align.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

static long checks = 0, wrong = 0;
#define EXPECT(cond, ...)                                 \
    do {                                                  \
        ++checks;                                         \
        if (!(cond)) {                                    \
            if (++wrong <= 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                 \
    } while (0)

static const uint32_t kSentinel = 0xA5C3F00Du;

// the literal matrix: cell[x][y] = the distance of the first x bytes of t and the first y bytes of p
static std::vector<std::vector<int>> literal_matrix(const std::vector<uint8_t> &p, const std::vector<uint8_t> &t) {
    const int m = (int)p.size(), L = (int)t.size();
    std::vector<std::vector<int>> c((size_t)L + 1, std::vector<int>((size_t)m + 1));
    for (int x = 0; x <= L; ++x) c[x][0] = x;
    for (int y = 0; y <= m; ++y) c[0][y] = y;
    for (int x = 1; x <= L; ++x)
        for (int y = 1; y <= m; ++y)
            c[x][y] = std::min({c[x - 1][y - 1] + (p[y - 1] != t[x - 1] ? 1 : 0), c[x][y - 1] + 1, c[x - 1][y] + 1});
    return c;
}

// the pinned rule on the literal matrix: the ops first to last
static std::vector<int> literal_script(const std::vector<uint8_t> &p, const std::vector<uint8_t> &t, const std::vector<std::vector<int>> &c) {
    std::vector<int> ops;
    int x = (int)t.size(), y = (int)p.size();
    while (x > 0 || y > 0) {
        int op;
        if (y == 0) op = APM_OP_INS;
        else if (x == 0) op = APM_OP_DEL;
        else if (c[x - 1][y - 1] + (p[y - 1] != t[x - 1] ? 1 : 0) == c[x][y]) op = p[y - 1] != t[x - 1] ? APM_OP_SUB : APM_OP_EQ;
        else if (c[x][y - 1] + 1 == c[x][y]) op = APM_OP_DEL;
        else op = APM_OP_INS;
        ops.push_back(op);
        x -= op != APM_OP_DEL;
        y -= op != APM_OP_INS;
    }
    std::reverse(ops.begin(), ops.end());
    return ops;
}

template <int W>
struct Eq {
    std::vector<uint32_t> tab;
    explicit Eq(const std::vector<uint8_t> &p) : tab(256 * W, 0u) {
        for (int i = 0; i < (int)p.size(); ++i) tab[(size_t)p[i] * W + (i >> 5)] |= 1u << (i & 31);
    }
    void get(int c, uint32_t (&eq)[W]) const {
        for (int w = 0; w < W; ++w) eq[w] = tab[(size_t)c * W + w];
    }
};

template <int W>
struct Trace { // exactly (L + 1) columns: a column outside them is the sanitizer's to catch
    std::vector<uint32_t> v;
    bool closed = false, late_store = false;
    explicit Trace(int L) : v((size_t)(L + 1) * 2 * W, 0xdeadbeefu) {}
    void put(int col, int w, uint32_t pv, uint32_t mv) {
        if (closed) late_store = true; // (a store behind done())
        v.at((size_t)col * 2 * W + w) = pv;
        v.at((size_t)col * 2 * W + W + w) = mv;
    }
    void done() { closed = true; }
    uint32_t pv(int col, int w) const { return v.at((size_t)col * 2 * W + w); }
    uint32_t mv(int col, int w) const { return v.at((size_t)col * 2 * W + W + w); }
};

struct Out {
    std::vector<uint32_t> row;
    int stores = 0;
    explicit Out(int words) : row((size_t)words, kSentinel) {}
    void store(int word, uint32_t v) {
        ++stores;
        row.at((size_t)word) = v;
    }
};

template <int W>
static void check_pair_w(const std::vector<uint8_t> &p, const std::vector<uint8_t> &t, int k) {
    const int m = (int)p.size(), L = (int)t.size();
    const auto c = literal_matrix(p, t);
    const int d = c[L][m];
    const Eq<W> eq(p);
    Trace<W> tr(L);
    Out out(apm_occ_align_row_words_of(m, k) + 1); // one word more than a row: it must keep the sentinel
    auto txt = [&](int i) { return (int)t.at((size_t)i); };
    const int n = apm_occ_align<W>(eq, txt, m, L, k, tr, out);
    EXPECT(!tr.late_store, "W %d m %d L %d k %d: a trace store behind done()", W, m, L, k);
    if (d > k) {
        EXPECT(n == 0 && out.stores == 0, "W %d m %d L %d k %d: distance %d is beyond k, got n_ops %d and %d stores", W, m, L, k, d, n, out.stores);
        return;
    }
    const std::vector<int> want = literal_script(p, t, c);
    EXPECT(n == (int)want.size(), "W %d m %d L %d k %d d %d: n_ops %d, want %zu", W, m, L, k, d, n, want.size());
    if (n != (int)want.size()) return;
    std::vector<uint32_t> row(out.row.size(), kSentinel);
    for (int j = 0; j < n; ++j) {
        if ((j & 15) == 0) row[(size_t)(1 + (j >> 4))] = 0u;
        row[(size_t)(1 + (j >> 4))] |= (uint32_t)want[(size_t)j] << (2 * (j & 15));
    }
    EXPECT(out.row == row, "W %d m %d L %d k %d d %d: the row's words differ from the rule's", W, m, L, k, d);
    // the consequences the header states
    int ni = 0, nd = 0, cost = 0;
    for (int op : want) ni += op == APM_OP_INS, nd += op == APM_OP_DEL, cost += op != APM_OP_EQ;
    EXPECT(nd - ni == m - L && n == m + ni && n <= m + k && cost == d, "W %d m %d L %d k %d: #D %d #I %d n_ops %d cost %d d %d", W, m, L, k, nd, ni, n, cost, d);
}

static void check_pair(const std::vector<uint8_t> &p, const std::vector<uint8_t> &t, int k) {
    switch (apm_occ_words((int)p.size())) {
    case 1: check_pair_w<1>(p, t, k); break;
    case 2: check_pair_w<2>(p, t, k); break;
    case 3: check_pair_w<3>(p, t, k); break;
    default: check_pair_w<4>(p, t, k); break;
    }
}

// p turned into a string of L bytes with at most k edits: the |L - m| net insertions or deletions, then substitutions and
// insertion / deletion pairs out of what is left of k
static std::vector<uint8_t> edited(const std::vector<uint8_t> &p, int L, int k, const std::vector<uint8_t> &alphabet, std::mt19937 &rng) {
    std::vector<uint8_t> s = p;
    int left = k - std::abs(L - (int)p.size());
    while ((int)s.size() < L) s.insert(s.begin() + (long)(rng() % (s.size() + 1)), alphabet[rng() % alphabet.size()]);
    while ((int)s.size() > L) s.erase(s.begin() + (long)(rng() % s.size()));
    int spend = left > 0 ? (int)(rng() % (unsigned)(left + 1)) : 0;
    while (spend > 0) {
        if (spend >= 2 && rng() % 2u) {
            s.erase(s.begin() + (long)(rng() % s.size()));
            s.insert(s.begin() + (long)(rng() % (s.size() + 1)), alphabet[rng() % alphabet.size()]);
            spend -= 2;
        } else {
            s[rng() % s.size()] = alphabet[rng() % alphabet.size()];
            spend -= 1;
        }
    }
    return s;
}

static void check_m_k(int m, int k, bool small, std::mt19937 &rng) {
    static const std::vector<uint8_t> dna = {'A', 'C', 'G', 'T'}, odd = {0x00, 0xFF, '\n', 'A'}, two = {'a', 'b'};
    std::set<int> lens;
    const int lo = std::max(1, m - k), hi = m + k;
    if (small) for (int L = lo; L <= hi; ++L) lens.insert(L);
    else lens = {lo, m, hi};
    for (int L : lens)
        for (const auto *a : {&dna, &odd, &two}) {
            std::vector<uint8_t> p((size_t)m);
            for (auto &ch : p) ch = (*a)[rng() % a->size()];
            for (int rep = 0; rep < (small ? 2 : 3); ++rep) check_pair(p, edited(p, L, k, *a, rng), k);
            std::vector<uint8_t> r((size_t)L); // an unrelated text: beyond k for all but the widest k
            for (auto &ch : r) ch = (*a)[rng() % a->size()];
            check_pair(p, r, k);
            if (a != &dna) continue;
            // tie-rich: homopolymers (with one foreign byte, and without), ACG repeats against each other at every phase
            std::vector<uint8_t> hp((size_t)m, 'A'), ht((size_t)L, 'A');
            check_pair(hp, ht, k);
            ht[(size_t)(L / 2)] = 'C';
            check_pair(hp, ht, k);
            hp[(size_t)(m - 1)] = 'C';
            check_pair(hp, ht, k);
            for (int phase = 0; phase < 3; ++phase) {
                std::vector<uint8_t> rp((size_t)m), rt((size_t)L);
                for (int i = 0; i < m; ++i) rp[(size_t)i] = (uint8_t)"ACG"[i % 3];
                for (int i = 0; i < L; ++i) rt[(size_t)i] = (uint8_t)"ACG"[(i + phase) % 3];
                check_pair(rp, rt, k);
            }
        }
}

int main() {
    std::mt19937 rng(20261020u);
    std::set<int> ms = {1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128};
    for (int m = 3; m <= 12; ++m) ms.insert(m);
    for (int m : ms) {
        std::set<int> ks;
        if (m <= 12) for (int k = 0; k < m; ++k) ks.insert(k);
        else ks = {0, 1, 7, m / 2, m - 1};
        for (int k : ks)
            if (k < m) check_m_k(m, k, m <= 12, rng);
    }
    // the row size: the count and 16 ops per dword of the most ops a script has
    EXPECT(apm_occ_align_row_words_of(128, 127) == 17 && apm_occ_align_row_words_of(12, 4) == 2 && apm_occ_align_row_words_of(12, 5) == 3 &&
               apm_occ_align_row_words_of(1, 0) == 2,
           "row words");
    printf("%ld checked, %ld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
