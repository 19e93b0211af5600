// Host test of csrc/apm_nearest.h (g++, address and undefined-behaviour sanitizers, no GPU): the segment walks with the
// nearest sink, their keys merged in shuffled order, against a literal DP written here.  W = 1..4; m at 1, 2, 31, 32, 33, 63,
// 64, 65, 96, 97, 127, 128; segments of 1 byte and of 16 bytes (and 61, and the whole text); every walk reads poison outside the
// 2 m - 1 bytes in front of its first end, its own ends and the look-ahead byte; bytes 0x00, 0xFF and '\n'; planted copies
// (small d), unplanted random patterns (large d), patterns that share no byte with the text (none), texts shorter than the
// pattern; the key at end = 2^56 - 1.
#include "apm_nearest.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef long long i64;
typedef unsigned long long u64;

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

// the pinned key of the ends [first, n): the smallest E below m and the first end that attains it
static u64 literal_key(const std::vector<int> &E, int m, i64 first) {
    u64 best = APM_NEAREST_NONE;
    for (i64 e = first; e < (i64)E.size(); ++e)
        if (E[(size_t)e] < m && (best == APM_NEAREST_NONE || (unsigned)E[(size_t)e] < APM_NEAREST_DIST(best))) best = ((u64)E[(size_t)e] << 56) | (u64)e;
    return best;
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

template <int W>
static void check_set(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, std::mt19937 &rng, const char *what) {
    const int m = (int)p.size();
    const i64 n = (i64)t.size();
    const std::vector<int> E = literal_E(t, p);
    const Eq<W> eq(p);
    for (int S : {1, 16, 61, (int)std::max<i64>(n, 1)}) {
        const i64 first = (i64)(rng() % 7u) % std::max<i64>(n, 1); // an own range that starts at an arbitrary x0
        std::vector<u64> keys;
        for (i64 b = first; b < n; b += S) {
            const i64 e = std::min<i64>(n, b + S);
            const Txt txt{&t, std::max<i64>(0, b - (2 * m - 1)), std::min<i64>(e, n - 1), p[0]};
            keys.push_back(apm_nearest_walk<W>(txt, eq, m, b, e, n, apm_nearest_steps(S, m)));
        }
        // a lane behind the last segment walks an empty range
        const Txt none{&t, 0, -1, p[0]};
        keys.push_back(apm_nearest_walk<W>(none, eq, m, n, n, n, apm_nearest_steps(S, m)));
        EXPECT(keys.back() == APM_NEAREST_NONE, "empty walk: W %d m %d S %d: key %llx", W, m, S, keys.back());
        std::shuffle(keys.begin(), keys.end(), rng);
        u64 got = APM_NEAREST_NONE;
        for (u64 k : keys) got = std::min(got, k);
        const u64 want = literal_key(E, m, first);
        EXPECT(got == want, "%s: W %d m %d n %lld S %d first %lld: key (%u, %llu), want (%u, %llu)", what, W, m, n, S, first, APM_NEAREST_DIST(got),
               APM_NEAREST_END(got), APM_NEAREST_DIST(want), APM_NEAREST_END(want));
    }
}

static void check(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, std::mt19937 &rng, const char *what) {
    switch (apm_occ_words((int)p.size())) {
    case 1: check_set<1>(t, p, rng, what); break;
    case 2: check_set<2>(t, p, rng, what); break;
    case 3: check_set<3>(t, p, rng, what); break;
    default: check_set<4>(t, p, rng, what); break;
    }
}

static std::vector<uint8_t> random_bytes(int n, const std::vector<uint8_t> &alphabet, std::mt19937 &rng) {
    std::vector<uint8_t> v((size_t)n);
    for (auto &c : v) c = alphabet[rng() % alphabet.size()];
    return v;
}

static void check_m(int m, const std::vector<uint8_t> &alphabet, int n, std::mt19937 &rng) {
    const std::vector<uint8_t> p = random_bytes(m, alphabet, rng);
    std::vector<uint8_t> t = random_bytes(n, alphabet, rng);
    check(t, p, rng, "unplanted");
    // two copies at the same distance (substitutions only, at distinct places): the first end must win
    const int edits = (int)(rng() % (unsigned)std::min(m, 5));
    if (n > 3 * m) {
        for (int c = 0; c < 2; ++c) {
            std::vector<uint8_t> s = p;
            for (int i = 0; i < edits; ++i) s[(size_t)((i * 7 + c) % m)] ^= 0x55;
            const size_t at = (size_t)(c ? n - m - (int)(rng() % 3u) : m + (int)(rng() % 16u));
            std::copy(s.begin(), s.end(), t.begin() + (long)at);
        }
        check(t, p, rng, "two copies");
    }
    // a copy with insertions and deletions
    std::vector<uint8_t> s = p;
    for (int i = 0; i < edits; ++i) {
        if ((rng() & 1u) && s.size() > 1) s.erase(s.begin() + (long)(rng() % s.size()));
        else s.insert(s.begin() + (long)(rng() % (s.size() + 1)), alphabet[rng() % alphabet.size()]);
    }
    if ((int)s.size() <= n) {
        std::vector<uint8_t> t2 = random_bytes(n, alphabet, rng);
        std::copy(s.begin(), s.end(), t2.begin() + (long)(rng() % (size_t)(n - (int)s.size() + 1)));
        check(t2, p, rng, "indel copy");
    }
    // no byte shared: none, whatever the poison says
    check(std::vector<uint8_t>((size_t)n, 0x7e), p, rng, "none");
    // a text shorter than the pattern, and of one byte
    check(random_bytes(std::max(1, m - 1 - (int)(rng() % 3u)), alphabet, rng), p, rng, "short text");
    check(random_bytes(1, alphabet, rng), p, rng, "one byte");
}

int main() {
    std::mt19937 rng(20261021u);
    const std::vector<uint8_t> dna = {'A', 'C', 'G', 'T'}, two = {'a', 'b'}, odd = {0x00, 0xFF, '\n', 'A'};
    for (int m : {1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128})
        for (const auto *a : {&dna, &two, &odd}) check_m(m, *a, m <= 33 ? 200 : 420, rng);

    // the key: order, pack and unpack, the largest end
    const u64 top = APM_NEAREST_MAX_TEXT - 1;
    EXPECT(APM_NEAREST_END(apm_nearest_key(127, top)) == top && APM_NEAREST_DIST(apm_nearest_key(127, top)) == 127u, "key at 2^56 - 1");
    EXPECT(apm_nearest_key(127, top) != APM_NEAREST_NONE && apm_nearest_key(127, top) < APM_NEAREST_NONE, "a real key is below NONE");
    EXPECT(apm_nearest_key(0, 0) == 0ull && APM_NEAREST_DIST(APM_NEAREST_NONE) == 255u, "key of (0, 0); distance field of NONE");
    EXPECT(apm_nearest_key(3, top) < apm_nearest_key(4, 0), "the smaller distance wins over any end");
    EXPECT(apm_nearest_key(3, 5) < apm_nearest_key(3, 6), "at equal distance the smaller end wins");
    // the sink: a hit replaces the best only at a strictly smaller distance; a column that is no hit changes nothing
    ApmNearestSink s;
    EXPECT(s.best == APM_NEAREST_NONE, "a fresh sink holds NONE");
    s(false, 1, 0);
    EXPECT(s.best == APM_NEAREST_NONE, "no hit, no change");
    s(true, 10, 5);
    s(true, 11, 5);
    EXPECT(s.best == apm_nearest_key(5, 10), "equal distance keeps the first end");
    s(true, 12, 6);
    EXPECT(s.best == apm_nearest_key(5, 10), "a larger distance changes nothing");
    s(true, (i64)top, 4);
    EXPECT(s.best == apm_nearest_key(4, top), "a smaller distance replaces");
    // steps and segment are the occurrence search's at k = m - 1
    for (int m_max : {1, 20, 128})
        for (u64 range : {1ull, 4096ull, 40000ull, 1ull << 30}) {
            const int S = apm_nearest_segment(m_max, range, 256, 32);
            EXPECT(S % 16 == 0 && S >= 2 * m_max - 1 && S == apm_occ_segment(m_max, m_max - 1, range, 256, 32), "segment: m_max %d range %llu: S %d", m_max, range, S);
            EXPECT(apm_nearest_steps(S, m_max) % 16 == 0 && apm_nearest_steps(S, m_max) >= S + 2 * m_max, "steps: m_max %d S %d", m_max, S);
        }
    printf("%ld checks, %ld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
