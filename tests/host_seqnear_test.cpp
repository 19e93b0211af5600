// Host test of csrc/apm_seqnear.h (g++, address and undefined-behaviour sanitizers, no GPU): the per-sequence walk cut into
// segments, every segment flushing into one key per sequence, against a literal DP run on every sequence as a text of its
// own.  W = 1..4; m at 1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128; segments of 1, 16 and 61 bytes and the whole text;
// boundaries at a segment's first end b, at b +- 1, b - m and b - (2 m - 1) +- 1; runs of empty sequences; 1-byte sequences;
// random tables; every walk reads poison outside [max(b - (2 m - 1), t_begin[s_b]), e); the bounded table search on tables
// that break their promise.
#include "apm_seqnear.h"

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

// the pinned key of sequence [lo, hi) for the ends >= first: the literal recurrence with C[y][0] = y at lo
static u64 literal_key(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, i64 lo, i64 hi, i64 first) {
    const int m = (int)p.size();
    std::vector<int> col(m + 1), nw(m + 1);
    for (int y = 0; y <= m; ++y) col[y] = y;
    u64 best = APM_NEAREST_NONE;
    for (i64 x = lo; x < hi; ++x) {
        nw[0] = 0;
        for (int y = 1; y <= m; ++y) nw[y] = std::min({col[y - 1] + (p[y - 1] != t[(size_t)x] ? 1 : 0), col[y] + 1, nw[y - 1] + 1});
        col.swap(nw);
        if (x >= first && col[m] < m && (unsigned)col[m] < APM_NEAREST_DIST(best)) best = ((u64)col[m] << 56) | (u64)x;
    }
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

struct Tab {
    const std::vector<u64> *begin_;
    u64 begin(u64 s) const { return (*begin_)[(size_t)s]; } // (.at-like: the sanitizer sees an index beyond n_seq)
};

struct Keys {
    std::vector<u64> *keys;
    void operator()(u64 s, u64 key) const {
        if (s >= keys->size() || key == APM_NEAREST_NONE) { ++wrong; return; }
        (*keys)[(size_t)s] = std::min((*keys)[(size_t)s], key);
    }
};

// begins: t_begin[0 .. n_seq], begins[0] = 0, begins.back() = n
template <int W>
static void check_table(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, const std::vector<u64> &begins, int S, i64 first, const char *what) {
    const int m = (int)p.size();
    const i64 n = (i64)t.size();
    const u64 n_seq = begins.size() - 1;
    const Eq<W> eq(p);
    const Tab tab{&begins};
    std::vector<u64> keys((size_t)n_seq, APM_NEAREST_NONE);
    const Keys flush{&keys};
    const int steps = apm_seqnear_steps(S, m);
    for (i64 b = first; b < n; b += S) {
        const i64 e = std::min<i64>(n, b + S);
        const u64 sb = apm_seqnear_find(tab, n_seq, (u64)b);
        const Txt txt{&t, std::max<i64>(b - (2 * m - 1), (i64)begins[(size_t)sb]), e - 1, p[0]};
        u64 best = 0, s = 0;
        apm_seqnear_walk<W>(txt, eq, tab, n_seq, flush, m, b, e, steps, &best, &s);
        EXPECT(s < n_seq && begins[(size_t)s] <= (u64)(e - 1) && (u64)(e - 1) < begins[(size_t)s + 1], "%s: the walk [%lld, %lld) ended in sequence %llu", what, b, e, s);
        if (best != APM_NEAREST_NONE) flush(s, best);
    }
    // a lane behind the last segment walks an empty range
    u64 best = 0, s = 0;
    const Txt none{&t, 0, -1, p[0]};
    apm_seqnear_walk<W>(none, eq, tab, n_seq, flush, m, n, n, steps, &best, &s);
    EXPECT(best == APM_NEAREST_NONE, "empty walk: W %d m %d S %d: key %llx", W, m, S, best);
    for (u64 q = 0; q < n_seq; ++q) {
        const u64 want = literal_key(t, p, (i64)begins[(size_t)q], (i64)begins[(size_t)q + 1], first);
        EXPECT(keys[(size_t)q] == want, "%s: W %d m %d n %lld S %d first %lld seq %llu [%llu, %llu): key (%u, %llu), want (%u, %llu)", what, W, m, n, S, first, q,
               begins[(size_t)q], begins[(size_t)q + 1], APM_NEAREST_DIST(keys[(size_t)q]), APM_NEAREST_END(keys[(size_t)q]), APM_NEAREST_DIST(want),
               APM_NEAREST_END(want));
    }
}

static void check(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, std::vector<u64> cuts, int S, i64 first, const char *what) {
    const u64 n = t.size();
    std::vector<u64> begins{0};
    std::sort(cuts.begin(), cuts.end());
    for (u64 c : cuts) begins.push_back(std::min(c, n));
    begins.push_back(n);
    switch (apm_occ_words((int)p.size())) {
    case 1: check_table<1>(t, p, begins, S, first, what); break;
    case 2: check_table<2>(t, p, begins, S, first, what); break;
    case 3: check_table<3>(t, p, begins, S, first, what); break;
    default: check_table<4>(t, p, begins, S, first, what); break;
    }
}

static std::vector<uint8_t> random_bytes(int n, const std::vector<uint8_t> &alphabet, std::mt19937 &rng) {
    std::vector<uint8_t> v((size_t)n);
    for (auto &c : v) c = alphabet[rng() % alphabet.size()];
    return v;
}

static void check_m(int m, const std::vector<uint8_t> &alphabet, std::mt19937 &rng) {
    const int n = m <= 33 ? 260 : 560;
    const std::vector<uint8_t> p = random_bytes(m, alphabet, rng);
    std::vector<uint8_t> t = random_bytes(n, alphabet, rng);
    // near copies all over the text, so that distances are small and a byte from the wrong side of a boundary shows
    for (int at = 3; at + m <= n; at += m + 1 + (int)(rng() % 5u)) {
        std::copy(p.begin(), p.end(), t.begin() + at);
        if (m > 2) t[(size_t)(at + (int)(rng() % (unsigned)m))] ^= 0x55;
    }
    for (int S : {1, 16, 61, n}) {
        const i64 first = (i64)(rng() % 7u);
        check(t, p, {}, S, first, "one sequence");
        // one boundary against the first ends of the segments 1, 2 and 3 (and the last one)
        for (i64 q : {(i64)1, (i64)2, (i64)3, (i64)((n - 1 - first) / S)}) {
            const i64 b = first + q * S;
            for (i64 c : {b, b - 1, b + 1, b - m, b - (2 * m - 1) - 1, b - (2 * m - 1), b - (2 * m - 1) + 1})
                if (c > 0 && c < n) check(t, p, {(u64)c}, S, first, "one boundary");
            // a run of empty sequences at the boundary, and 1-byte sequences behind it
            if (b > 0 && b + 3 < n) {
                check(t, p, {(u64)b, (u64)b, (u64)b, (u64)b}, S, first, "empty run");
                check(t, p, {(u64)b - 1, (u64)b, (u64)b + 1, (u64)b + 2, (u64)b + 2, (u64)b + 3}, S, first, "1-byte sequences");
            }
        }
        // empty sequences at both ends of the text; every byte a sequence
        check(t, p, {0, 0, (u64)n, (u64)n}, S, first, "empty at the ends");
        if (m <= 33 || S >= 16) {
            std::vector<u64> all;
            for (int c = 1; c < n; ++c) all.push_back((u64)c);
            check(t, p, all, S, first, "every byte a sequence");
        }
        // random tables: some dense, with empties
        for (int r = 0; r < 3; ++r) {
            std::vector<u64> cuts;
            const int k = 1 + (int)(rng() % 40u);
            for (int i = 0; i < k; ++i) {
                cuts.push_back(rng() % (unsigned)(n + 1));
                if (rng() % 4u == 0) cuts.push_back(cuts.back());
            }
            check(t, p, cuts, S, first, "random table");
        }
    }
    // no byte shared: none in every sequence, whatever the poison says
    check(std::vector<uint8_t>((size_t)n, 0x7e), p, {17, 18, 100}, 16, 0, "none");
    // a text of one byte
    check(random_bytes(1, alphabet, rng), p, {}, 16, 0, "one byte");
    check(random_bytes(1, alphabet, rng), p, {0, 1}, 16, 0, "one byte between empties");
}

int main() {
    std::mt19937 rng(20261021u);
    const std::vector<uint8_t> dna = {'A', 'C', 'G', 'T'}, odd = {0x00, 0xFF, '\n', 'A'};
    for (int m : {1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128})
        for (const auto *a : {&dna, &odd}) check_m(m, *a, rng);

    // the table search: the largest s with t_begin[s] <= x; among equal begins the last; bounded and inside [0, n_seq) on
    // tables that break the order
    const std::vector<u64> good = {0, 0, 5, 5, 5, 9, 20};
    const Tab tg{&good};
    for (u64 x = 0; x < 20; ++x) {
        u64 want = 0;
        for (u64 s = 0; s < 6; ++s) if (good[(size_t)s] <= x) want = s;
        EXPECT(apm_seqnear_find(tg, 6, x) == want, "find(%llu) = %llu, want %llu", x, apm_seqnear_find(tg, 6, x), want);
    }
    const std::vector<u64> bad = {7, 3, 90, 0, 2, 1, 4};
    const Tab tb{&bad};
    for (u64 x = 0; x < 100; ++x) EXPECT(apm_seqnear_find(tb, 6, x) < 6, "find on a broken table left [0, n_seq)");
    EXPECT(apm_seqnear_find(tg, 1, 3) == 0, "n_seq = 1");
    // a broken table: the walk stays inside the table and the keys (the sanitizers and Keys watch)
    {
        const std::vector<uint8_t> p = {'A', 'C', 'G', 'T', 'A'};
        const std::vector<uint8_t> t = random_bytes(200, dna, rng);
        const std::vector<u64> before = bad;
        std::vector<u64> keys(6, APM_NEAREST_NONE);
        const Keys flush{&keys};
        const Eq<1> eq(p);
        for (i64 b = 0; b < 200; b += 16) {
            u64 best = 0, s = 0;
            const Txt txt{&t, 0, 199, 'A'};
            apm_seqnear_walk<1>(txt, eq, tb, 6, flush, 5, b, std::min<i64>(200, b + 16), apm_seqnear_steps(16, 5), &best, &s);
            EXPECT(s < 6, "broken table: s = %llu", s);
        }
        EXPECT(bad == before, "the table is only read");
    }
    for (int m : {1, 20, 128})
        for (int S : {16, 48, 4096}) EXPECT(apm_seqnear_steps(S, m) % 16 == 0 && apm_seqnear_steps(S, m) >= S + 2 * m - 1, "steps: m %d S %d", m, S);
    printf("%ld checks, %ld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
