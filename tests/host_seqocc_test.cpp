// Host test of csrc/apm_seqocc.h (g++, address and undefined-behaviour sanitizers, no GPU): the per-sequence occurrence walk
// cut into segments, the union of what the segments report against the literal recurrence run on every sequence as a text of
// its own -- exactly: no duplicate at a seam, no lost end.  Both flags; k in {0, 1, 3, m - 1}; W = 1..4; m at 1, 2, 31, 32,
// 33, 64, 65, 96, 97, 127, 128; segments of 1, 16 and 61 bytes and the whole text; boundaries at a segment's first end b, at
// b +- 1, at its end e, e +- 1, at b - (m + k) and b - (m + k) +- 1; runs of empty sequences; 1-byte sequences; random tables;
// every walk reads poison outside [max(b - (m + k), t_begin[s_b]), min(e, n - 1)]; a table that breaks its promise; the span
// columns clamped to the sequence.
#include "apm_seqocc.h"

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

struct End {
    i64 e;
    int d;
    bool operator==(const End &o) const { return e == o.e && d == o.d; }
    bool operator<(const End &o) const { return e < o.e; }
};

// the pinned result of sequence [lo, hi): the literal recurrence with C[y][0] = y at lo, the report rule on E_s alone
static void literal(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, i64 lo, i64 hi, int k, unsigned flags, i64 first, std::vector<End> &out) {
    const int m = (int)p.size();
    std::vector<int> col(m + 1), nw(m + 1), E;
    for (int y = 0; y <= m; ++y) col[y] = y;
    for (i64 x = lo; x < hi; ++x) {
        nw[0] = 0;
        for (int y = 1; y <= m; ++y) nw[y] = std::min({col[y - 1] + (p[y - 1] != t[(size_t)x] ? 1 : 0), col[y] + 1, nw[y - 1] + 1});
        col.swap(nw);
        E.push_back(col[m]);
    }
    for (size_t i = 0; i < E.size(); ++i) {
        if (E[i] > k || lo + (i64)i < first) continue;
        if (flags & APM_OCC_LOCAL_MIN) {
            const int prev = i ? E[i - 1] : m;
            if (!(prev > E[i])) continue;
            if (i + 1 < E.size() && !(E[i + 1] >= E[i])) continue;
        }
        out.push_back(End{lo + (i64)i, E[i]});
    }
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
    u64 begin(u64 s) const { return begin_->at((size_t)s); } // (an index beyond n_seq throws)
};

struct Sink { // every column once, in order; a hit's distance is its E_s
    std::vector<End> *out;
    i64 next;
    long calls = 0;
    void operator()(bool hit, i64 end, int dist) {
        ++calls;
        if (end != next) ++wrong;
        next = end + 1;
        if (hit) out->push_back(End{end, dist});
    }
};

// begins: t_begin[0 .. n_seq], begins[0] = 0, begins.back() = n
template <int W>
static void check_table(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, const std::vector<u64> &begins, int k, unsigned flags, int S, i64 first,
                        const char *what) {
    const int m = (int)p.size();
    const i64 n = (i64)t.size();
    const u64 n_seq = begins.size() - 1;
    const Eq<W> eq(p);
    const Tab tab{&begins};
    const int steps = apm_occ_steps(S, m, k);
    std::vector<End> got, want;
    unsigned found = 0;
    for (i64 b = first; b < n; b += S) {
        const i64 e = std::min<i64>(n, b + S);
        const u64 sb = apm_seqnear_find(tab, n_seq, (u64)b);
        const Txt txt{&t, std::max<i64>(b - (m + k), (i64)begins[(size_t)sb]), std::min<i64>(e, n - 1), p[0]};
        Sink sink{&got, b - (m + k) - 1};
        found += apm_seqocc_walk<W>(txt, eq, tab, n_seq, m, k, b, e, n, flags, steps, sink);
        EXPECT(sink.calls == steps, "%s: the sink was called %ld times in %d columns", what, sink.calls, steps);
    }
    // a lane behind the last segment walks an empty range and reads nothing
    {
        std::vector<End> none;
        const Txt txt{&t, 0, -1, p[0]};
        Sink sink{&none, n - (m + k) - 1};
        const unsigned f = apm_seqocc_walk<W>(txt, eq, tab, n_seq, m, k, n, n, n, flags, steps, sink);
        EXPECT(f == 0 && none.empty() && sink.calls == steps, "empty walk: W %d m %d S %d", W, m, S);
    }
    for (u64 q = 0; q < n_seq; ++q) literal(t, p, (i64)begins[(size_t)q], (i64)begins[(size_t)q + 1], k, flags, first, want);
    std::sort(got.begin(), got.end()); // (segments are walked in order: already sorted unless an end is doubled)
    EXPECT(found == got.size(), "%s: the walks returned %u ends and reported %zu", what, found, got.size());
    EXPECT(got == want, "%s: W %d m %d k %d flags %u n %lld S %d first %lld n_seq %llu: %zu ends, want %zu", what, W, m, k, flags, n, S, first, n_seq,
           got.size(), want.size());
    if (!(got == want) && wrong <= 20) {
        for (size_t i = 0; i < std::max(got.size(), want.size()); ++i) {
            const End g = i < got.size() ? got[i] : End{-1, -1}, w = i < want.size() ? want[i] : End{-1, -1};
            if (!(g == w)) { printf("  first difference at %zu: got (%lld, %d), want (%lld, %d)\n", i, g.e, g.d, w.e, w.d); break; }
        }
    }
}

static void check(const std::vector<uint8_t> &t, const std::vector<uint8_t> &p, std::vector<u64> cuts, int k, int S, i64 first, const char *what) {
    const u64 n = t.size();
    std::vector<u64> begins{0};
    std::sort(cuts.begin(), cuts.end());
    for (u64 c : cuts) begins.push_back(std::min(c, n));
    begins.push_back(n);
    for (unsigned flags : {APM_OCC_ALL, APM_OCC_LOCAL_MIN}) {
        switch (apm_occ_words((int)p.size())) {
        case 1: check_table<1>(t, p, begins, k, flags, S, first, what); break;
        case 2: check_table<2>(t, p, begins, k, flags, S, first, what); break;
        case 3: check_table<3>(t, p, begins, k, flags, S, first, what); break;
        default: check_table<4>(t, p, begins, k, flags, S, first, what); break;
        }
    }
}

static std::vector<uint8_t> random_bytes(int n, const std::vector<uint8_t> &alphabet, std::mt19937 &rng) {
    std::vector<uint8_t> v((size_t)n);
    for (auto &c : v) c = alphabet[rng() % alphabet.size()];
    return v;
}

static void check_m(int m, const std::vector<uint8_t> &alphabet, std::mt19937 &rng) {
    const int n = m <= 33 ? 230 : 500;
    const std::vector<uint8_t> p = random_bytes(m, alphabet, rng);
    std::vector<uint8_t> t = random_bytes(n, alphabet, rng);
    // near copies all over the text, so that ends are reported everywhere and a byte from the wrong side of a boundary shows
    for (int at = 3; at + m <= n; at += m + 1 + (int)(rng() % 5u)) {
        std::copy(p.begin(), p.end(), t.begin() + at);
        if (m > 2) t[(size_t)(at + (int)(rng() % (unsigned)m))] ^= 0x55;
    }
    std::vector<int> ks;
    for (int k : {0, 1, 3, m - 1})
        if (k >= 0 && k < m && std::find(ks.begin(), ks.end(), k) == ks.end()) ks.push_back(k);
    for (int k : ks) {
        for (int S : {1, 16, 61, n}) {
            const i64 first = (i64)(rng() % 7u);
            check(t, p, {}, k, S, first, "one sequence");
            // one boundary against the segments 1 and 2 and the last one
            for (i64 q : {(i64)1, (i64)2, (i64)((n - 1 - first) / S)}) {
                const i64 b = first + q * S, e = std::min<i64>(n, b + S);
                for (i64 c : {b, b - 1, b + 1, e, e - 1, e + 1, b - (m + k), b - (m + k) - 1, b - (m + k) + 1})
                    if (c > 0 && c < n) check(t, p, {(u64)c}, k, S, first, "one boundary");
                // a run of empty sequences at the boundary, and 1-byte sequences behind it
                if (b > 0 && b + 3 < n) {
                    check(t, p, {(u64)b, (u64)b, (u64)b, (u64)b}, k, S, first, "empty run");
                    check(t, p, {(u64)b - 1, (u64)b, (u64)b + 1, (u64)b + 2, (u64)b + 2, (u64)b + 3}, k, S, first, "1-byte sequences");
                }
            }
            // empty sequences at both ends of the text; every byte a sequence
            check(t, p, {0, 0, (u64)n, (u64)n}, k, S, first, "empty at the ends");
            if (m <= 2 && S >= 16) {
                std::vector<u64> all;
                for (int c = 1; c < n; ++c) all.push_back((u64)c);
                check(t, p, all, k, S, first, "every byte a sequence");
            }
            // random tables: some dense, with empties
            for (int r = 0; r < 2; ++r) {
                std::vector<u64> cuts;
                const int c = 1 + (int)(rng() % 40u);
                for (int i = 0; i < c; ++i) {
                    cuts.push_back(rng() % (unsigned)(n + 1));
                    if (rng() % 4u == 0) cuts.push_back(cuts.back());
                }
                check(t, p, cuts, k, S, first, "random table");
            }
        }
        // a text of one byte
        check(random_bytes(1, alphabet, rng), p, {}, k, 16, 0, "one byte");
        check(random_bytes(1, alphabet, rng), p, {0, 1}, k, 16, 0, "one byte between empties");
    }
}

int main() {
    std::mt19937 rng(20261021u);
    const std::vector<uint8_t> dna = {'A', 'C', 'G', 'T'}, odd = {0x00, 0xFF, '\n', 'A'};
    for (int m : {1, 2, 31, 32, 33, 64, 65, 96, 97, 127, 128})
        for (const auto *a : {&dna, &odd}) check_m(m, *a, rng);

    // the example: GATTACA across the boundary of two sequences
    {
        const char *s = "CCCCCCCCCCGATTACACCCCCCCC";
        const std::vector<uint8_t> t(s, s + 25), p = {'G', 'A', 'T', 'T', 'A', 'C', 'A'};
        const std::vector<u64> begins = {0, 12, 25};
        const Tab tab{&begins};
        const Eq<1> eq(p);
        for (int S : {1, 16, 25}) {
            std::vector<End> got;
            for (i64 b = 0; b < 25; b += S) {
                const Txt txt{&t, 0, 24, 'G'};
                Sink sink{&got, b - 9 - 1};
                apm_seqocc_walk<1>(txt, eq, tab, 2, 7, 2, b, std::min<i64>(25, b + S), 25, APM_OCC_LOCAL_MIN, apm_occ_steps(S, 7, 2), sink);
            }
            EXPECT(got.size() == 1 && got[0] == (End{16, 2}), "GATTACA: S %d: %zu ends", S, got.size());
        }
        EXPECT(apm_seqocc_span_cols(7, 2, 16, 12) == 5 && apm_seqocc_span_cols(7, 2, 24, 12) == 9 && apm_seqocc_span_cols(7, 2, 12, 12) == 1, "span columns");
    }
    // a broken table: the walk stays inside the table (Tab throws beyond it) and calls its sink once per column
    {
        const std::vector<u64> bad = {7, 3, 90, 0, 2, 1, 4};
        const std::vector<u64> before = bad;
        const Tab tb{&bad};
        const std::vector<uint8_t> p = {'A', 'C', 'G', 'T', 'A'};
        const std::vector<uint8_t> t = random_bytes(200, dna, rng);
        const Eq<1> eq(p);
        for (i64 b = 0; b < 200; b += 16) {
            std::vector<End> got;
            const Txt txt{&t, 0, 199, 'A'};
            Sink sink{&got, b - 7 - 1};
            apm_seqocc_walk<1>(txt, eq, tb, 6, 5, 2, b, std::min<i64>(200, b + 16), 200, APM_OCC_ALL, apm_occ_steps(16, 5, 2), sink);
            EXPECT(sink.calls == apm_occ_steps(16, 5, 2), "broken table: %ld sink calls", sink.calls);
            for (const End &g : got) EXPECT(g.e >= b && g.e < b + 16 && g.d <= 2, "broken table: an end outside the walk's range");
        }
        EXPECT(bad == before, "the table is only read");
    }
    printf("%ld checks, %ld wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
