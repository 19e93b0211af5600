// Host test of csrc/apm_occ.h (g++, address and undefined-behaviour sanitizers, no GPU): the segment walk and the span walk
// against a literal DP written here.  W = 1..4; m at 1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128; k from 0 up to m - 1 for
// the small m; every walk starts exactly m + k bytes in front of its first end and reads poison outside the bytes the
// lemma allows it; segments of length 1; bytes 0x00, 0xFF and '\n'.
#include "apm_occ.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef long long i64;

static long checks = 0, wrong = 0;
#define EXPECT(cond, ...)                                 \
    do {                                                  \
        ++checks;                                         \
        if (!(cond)) {                                    \
            if (++wrong <= 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                 \
    } while (0)

// E(e) = C[m][e + 1] of the literal recurrence, free start
static std::vector<int> literal_E(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p) {
    const int m = (int)p.size();
    std::vector<int> col(m + 1), nw(m + 1), E(t.size());
    for (int y = 0; y <= m; ++y) col[y] = y;
    for (size_t x = 0; x < t.size(); ++x) {
        nw[0] = 0;
        for (int y = 1; y <= m; ++y) nw[y] = std::min({col[y - 1] + (p[y - 1] != t[x] ? 1 : 0), col[y] + 1, nw[y - 1] + 1});
        col.swap(nw);
        E[x] = col[m];
    }
    return E;
}

// the pinned span of end e: dist(p, T[e + 1 - L : e + 1)) by the literal square DP for every L on its own
static void literal_span(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, int k, i64 e, int *d_star, int *l_star) {
    const int m = (int)p.size();
    const int most = (int)std::min<i64>(m + k, e + 1);
    *d_star = 1 << 20;
    *l_star = 0;
    std::vector<int> col(m + 1), nw(m + 1);
    for (int L = 1; L <= most; ++L) {
        for (int y = 0; y <= m; ++y) col[y] = y;
        for (int x = 1; x <= L; ++x) {
            const uint8_t c = t[(size_t)(e + 1 - L + x - 1)];
            nw[0] = x;
            for (int y = 1; y <= m; ++y) nw[y] = std::min({col[y - 1] + (p[y - 1] != c ? 1 : 0), col[y] + 1, nw[y - 1] + 1});
            col.swap(nw);
        }
        if (col[m] < *d_star) {
            *d_star = col[m];
            *l_star = L;
        }
    }
}

template <int W>
struct Eq {
    std::vector<uint32_t> tab;
    Eq(const std::vector<uint8_t> &p, bool reversed) : tab(256 * W, 0u) {
        const int m = (int)p.size();
        for (int i = 0; i < m; ++i) tab[(size_t)p[reversed ? m - 1 - i : i] * W + (i >> 5)] |= 1u << (i & 31);
    }
    void get(int c, uint32_t (&eq)[W]) const {
        for (int w = 0; w < W; ++w) eq[w] = tab[(size_t)c * W + w];
    }
};

// the text a walk may read: [lo, hi]; every other byte is poison that would match the pattern's first byte
struct Txt {
    const std::vector<uint8_t> *t;
    i64 lo, hi;
    uint8_t poison;
    void load16(i64 x, uint32_t (&w)[4]) const {
        for (int i = 0; i < 4; ++i) w[i] = 0u;
        for (int b = 0; b < 16; ++b) {
            const i64 q = x + b;
            const uint8_t c = (q >= lo && q <= hi) ? (*t)[(size_t)q] : poison;
            w[b >> 2] |= (uint32_t)c << (8 * (b & 3));
        }
    }
};

struct Sink {
    std::vector<std::pair<i64, int>> hits;
    void operator()(bool hit, i64 end, int dist) {
        if (hit) hits.push_back({end, dist});
    }
};

template <int W>
static void check_set(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, int k, int max_spans, std::mt19937 &rng) {
    const int m = (int)p.size();
    const i64 n = (i64)t.size();
    const std::vector<int> E = literal_E(t, p);
    const Eq<W> eq(p, false), req(p, true);
    const int segs[] = {1, 5, 16, 61, (int)n};
    for (unsigned flags = 0; flags <= 1; ++flags) {
        std::vector<std::pair<i64, int>> want;
        for (i64 e = 0; e < n; ++e) {
            if (E[(size_t)e] > k) continue;
            const int prev = e ? E[(size_t)e - 1] : m;
            if (flags == APM_OCC_LOCAL_MIN && !(prev > E[(size_t)e] && (e + 1 == n || E[(size_t)e + 1] >= E[(size_t)e]))) continue;
            want.push_back({e, E[(size_t)e]});
        }
        for (int S : segs) {
            if (S == 1 && n > 300 && m > 64) continue; // (time: the short texts cover segments of one byte at every W)
            Sink sink;
            unsigned found = 0;
            const i64 first = (i64)(rng() % 7u); // an own range that starts at an arbitrary x0
            for (i64 b = first; b < n; b += S) {
                const i64 e = std::min<i64>(n, b + S);
                const Txt txt{&t, std::max<i64>(0, b - (m + k)), std::min<i64>(e, n - 1), p[0]};
                found += apm_occ_walk<W>(txt, eq, m, k, b, e, n, flags, apm_occ_steps(S, m, k), sink);
            }
            std::vector<std::pair<i64, int>> w2;
            for (auto &h : want)
                if (h.first >= first) w2.push_back(h);
            EXPECT(sink.hits == w2 && found == w2.size(), "walk: W %d m %d k %d flags %u S %d: %zu ends, want %zu", W, m, k, flags, S, sink.hits.size(),
                   w2.size());
        }
    }
    // spans: reported ends first, then arbitrary positions
    std::vector<i64> ends;
    for (i64 e = 0; e < n && (int)ends.size() < max_spans; ++e)
        if (E[(size_t)e] <= k) ends.push_back(e);
    for (int i = 0; i < max_spans / 2 + 1; ++i) ends.push_back((i64)(rng() % (unsigned)n));
    ends.push_back(0);
    ends.push_back(n - 1);
    for (i64 e : ends) {
        int wd = 0, wl = 0, gd = 0, gl = 0;
        literal_span(t, p, k, e, &wd, &wl);
        const int cols = apm_occ_span_cols(m, k, (unsigned long long)e);
        auto back = [&](int i) { return (int)t[(size_t)(e - i)]; };
        apm_occ_span_walk<W>(req, back, m, cols, &gd, &gl);
        EXPECT(gd == wd && gl == wl, "span: W %d m %d k %d e %lld: (%d, %d), want (%d, %d)", W, m, k, e, gd, gl, wd, wl);
        if (E[(size_t)e] <= k) {
            EXPECT(wd == E[(size_t)e] && wl >= m - k && wl <= m + k, "span rule: m %d k %d e %lld: d* %d E %d L* %d", m, k, e, wd, E[(size_t)e], wl);
        }
    }
}

static void check_m(int m, int k, const std::vector<uint8_t> &alphabet, int n, int max_spans, std::mt19937 &rng) {
    std::vector<uint8_t> t((size_t)n), p((size_t)m);
    for (auto &c : t) c = alphabet[rng() % alphabet.size()];
    for (auto &c : p) c = alphabet[rng() % alphabet.size()];
    // plant copies with substitutions, deletions and insertions
    for (int c = 0; c < 6 && n > 2 * m; ++c) {
        std::vector<uint8_t> s = p;
        const int edits = k ? (int)(rng() % (unsigned)(std::min(k, 6) + 1)) : 0;
        for (int i = 0; i < edits; ++i) {
            const unsigned kind = rng() % 3u;
            if (kind == 0 || s.size() <= 1) s[rng() % s.size()] = alphabet[rng() % alphabet.size()];
            else if (kind == 1) s.erase(s.begin() + (long)(rng() % s.size()));
            else s.insert(s.begin() + (long)(rng() % (s.size() + 1)), alphabet[rng() % alphabet.size()]);
        }
        const size_t at = rng() % (size_t)(n - (int)s.size() + 1);
        std::copy(s.begin(), s.end(), t.begin() + (long)at);
    }
    switch (apm_occ_words(m)) {
    case 1: check_set<1>(t, p, k, max_spans, rng); break;
    case 2: check_set<2>(t, p, k, max_spans, rng); break;
    case 3: check_set<3>(t, p, k, max_spans, rng); break;
    default: check_set<4>(t, p, k, max_spans, rng); break;
    }
}

int main() {
    std::mt19937 rng(20261020u);
    const std::vector<uint8_t> dna = {'A', 'C', 'G', 'T'}, two = {'a', 'b'}, odd = {0x00, 0xFF, '\n', 'A'};
    const int ms[] = {1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128};
    for (int m : ms) {
        std::vector<int> ks;
        if (m <= 33) for (int k = 0; k < m; ++k) ks.push_back(k);
        else ks = {0, 1, 3, 7, m - 1};
        for (int k : ks)
            for (const auto *a : {&dna, &two, &odd}) {
                if (a != &dna && k > 3 && k != m - 1) continue; // (every k on DNA, the other alphabets at the small k and at m - 1)
                check_m(m, k, *a, m <= 33 ? 200 : 420, m <= 33 ? 10 : (k <= 7 ? 5 : 0), rng);
                if (m <= 33 && k <= 3) check_m(m, k, *a, std::max(1, m - 1 - (int)(rng() % 3u)), 2, rng); // n < m, n = 1
            }
    }
    // the segment chooser: whole 16-byte blocks, never below the warm-up, 1.25 at most on large ranges
    for (int m_max : {1, 20, 128})
        for (int k : {0, 3})
            for (unsigned long long range : {1ull, 4096ull, 300000ull, 1ull << 30, 1ull << 36})
                for (int P : {1, 3, 32, 1000}) {
                    if (k >= m_max) continue;
                    const int S = apm_occ_segment(m_max, k, range, 256, P);
                    EXPECT(S % 16 == 0 && S >= m_max + k && S <= 16 * (m_max + k) + 15, "segment: m_max %d k %d range %llu P %d: S %d", m_max, k, range, P, S);
                    if (range >= (1ull << 30)) EXPECT(S >= 4 * (m_max + k), "segment overhead: m_max %d k %d: S %d", m_max, k, S);
                }
    printf("%ld checks, %ld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
