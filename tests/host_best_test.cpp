// Host-side check of the best-hit pass's arithmetic (csrc/apm_best.h) against a brute force of the rule over the oracle's
// literal window DP: apm_best_decide -- the lane form at k <= 7, the wave form's emulated lanes at every k -- must keep
// exactly the records the rule of include/apm.h keeps, with their scores, at every pos of every text, and the coverage
// predicate must say exactly when a shard holds every byte a decision reads.  Stand-alone, no input; built with
// -fsanitize=address,undefined and run by tests/test_best_host.py.
#include "apm_best.h"
#include "apm_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// The text as the kernels' sources see a shard of it: a window at `rel` of a heap copy that holds exactly the bytes
// [lo, hi) of the text, so that the sanitizer sees every read beyond.  byte() may be asked inside the window's size only;
// load16 may run past it (those bytes count for nothing) but never fetches outside the shard, like the device's guarded load.
struct Shard {
    const unsigned char *b; // the copy: b[0] is byte lo of the text
    long lo, hi, rel;       // rel: the window's start in the text
    void load16(int off, uint32_t (&w)[4]) const {
        for (int i = 0; i < 4; ++i) w[i] = 0u;
        for (int i = 0; i < 16; ++i) {
            const long q = rel + off + i;
            if (q >= lo && q < hi) w[i >> 2] |= (uint32_t)b[q - lo] << (8 * (i & 3));
        }
    }
    int byte(int i) const {
        const long q = rel + i;
        if (q < lo || q >= hi) { fprintf(stderr, "text byte %ld read outside the shard [%ld, %ld)\n", q, lo, hi); abort(); }
        return b[q - lo];
    }
    Shard at(int o) const { Shard s = *this; s.rel += o; return s; }
};

struct Pattern { // exactly m bytes on the heap; the device rows are zero padded, here the padding is made up
    const unsigned char *b;
    int n;
    void load16(int off, uint32_t (&w)[4]) const {
        for (int i = 0; i < 4; ++i) w[i] = 0u;
        for (int i = 0; i < 16; ++i)
            if (off + i >= 0 && off + i < n) w[i >> 2] |= (uint32_t)b[off + i] << (8 * (i & 3));
    }
    int byte(int i) const {
        if (i < 0 || i >= n) { fprintf(stderr, "pattern byte %d read outside [0, %d)\n", i, n); abort(); }
        return b[i];
    }
};

typedef std::vector<unsigned char> Str;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd(unsigned n) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((rng_state >> 33) % n);
}
static Str dna(int n) {
    Str s((size_t)n);
    for (auto &c : s) c = (unsigned char)"ACGT"[rnd(4)];
    return s;
}
static Str tandem(const char *unit, int reps) {
    Str s;
    for (int i = 0; i < reps; ++i)
        for (const char *c = unit; *c; ++c) s.push_back((unsigned char)*c);
    return s;
}

// s(j) of the rule for every start j of the text, by the oracle
static std::vector<int> scores(const Str &text, const Str &pat, int k) {
    const long n = (long)text.size();
    std::vector<int> s((size_t)n), col(pat.size() + 1);
    for (long j = 0; j < n; ++j) {
        const int size = (int)std::min<long>((long)pat.size(), n - j);
        Str p(pat.begin(), pat.begin() + size), t(text.begin() + j, text.begin() + j + size); // exactly `size` bytes each
        const int d = oracle_window_distance(p.data(), t.data(), size, col.data());
        s[(size_t)j] = d < k + 1 ? d : k + 1;
    }
    return s;
}

// the rule, literally
static bool rule(const std::vector<int> &s, long pos, int k, int r) {
    const long n = (long)s.size(), w_end = n > k ? n - k : 0;
    if (s[(size_t)pos] > k) return false;
    for (long j = pos - r; j < pos; ++j)
        if (j >= 0 && j < w_end && s[(size_t)j] <= s[(size_t)pos]) return false;
    for (long j = pos + 1; j <= pos + r; ++j)
        if (j < w_end && s[(size_t)j] < s[(size_t)pos]) return false;
    return true;
}

static const int RADII[] = {0, 1, 2, 5, 64};
static long checked = 0, kept_total = 0, bad = 0, truncated = 0, k_ge_m = 0, m_gt_n = 0, covered_yes = 0, covered_no = 0;
static std::vector<int> band(APM_SCORE_BAND_CELLS);

static void check_text(const Str &text, const std::vector<Str> &pats, const char *what) {
    const long n = (long)text.size();
    const Shard whole{text.data(), 0, n, 0};
    for (const Str &pat : pats) {
        const int m = (int)pat.size();
        const Pattern p{pat.data(), m};
        m_gt_n += m > n;
        for (int k = 0; k <= 9; ++k) {
            const std::vector<int> s = scores(text, pat, k);
            k_ge_m += k >= m;
            for (int r : RADII)
                for (long pos = 0; pos < n; ++pos) {
                    const bool want = rule(s, pos, k, r);
                    const int want_v = want ? s[(size_t)pos] : (s[(size_t)pos] > k ? APM_BEST_DROPPED : APM_BEST_SUPPRESSED);
                    truncated += want && pos + m > n;
                    kept_total += want;
                    for (int wave = (k <= APM_SCORE_LANE_MAX_K ? 0 : 1); wave < 2; ++wave) {
                        const int got = apm_best_decide(p, whole.at((int)pos), m, (unsigned long long)pos, (unsigned long long)n, k, r, band.data(), wave != 0);
                        ++checked;
                        if (got != want_v && ++bad <= 8)
                            printf("%s n %ld m %d k %d r %d pos %ld %s: %d, want %d\n", what, n, m, k, r, pos, wave ? "WAVE" : "LANE", got, want_v);
                    }
                }
        }
    }
}

// every cut c of the text into the shards [0, c) and [c, n): the predicate is true exactly when the shard holds
// [max(pos, r) - r, min(n, pos + r + m)), and then the decision made on the shard's bytes alone is the whole text's
static void check_coverage(const Str &text, const Str &pat, int k) {
    const long n = (long)text.size();
    const int m = (int)pat.size();
    const Pattern p{pat.data(), m};
    const Shard whole{text.data(), 0, n, 0};
    for (long c = 0; c <= n; ++c)
        for (int side = 0; side < 2; ++side) {
            const long lo = side ? c : 0, hi = side ? n : c;
            const Str copy(text.begin() + lo, text.begin() + hi);
            const Shard shard{copy.data(), lo, hi, 0};
            for (int r : RADII)
                for (long pos = 0; pos < n; ++pos) {
                    const long need_lo = std::max<long>(pos, r) - r, need_hi = std::min<long>(n, pos + r + m);
                    const bool want = need_lo >= lo && need_hi <= hi;
                    const bool got = apm_best_covered((unsigned long long)pos, m, r, (unsigned long long)n, (unsigned long long)lo, (unsigned long long)(hi - lo));
                    ++checked;
                    (want ? covered_yes : covered_no) += 1;
                    if (got != want && ++bad <= 8) printf("COVER n %ld m %d r %d pos %ld shard [%ld, %ld): %d, want %d\n", n, m, r, pos, lo, hi, (int)got, (int)want);
                    if (!want) continue;
                    for (int wave = 0; wave < 2; ++wave) {
                        const int a = apm_best_decide(p, shard.at((int)pos), m, (unsigned long long)pos, (unsigned long long)n, k, r, band.data(), wave != 0);
                        const int b = apm_best_decide(p, whole.at((int)pos), m, (unsigned long long)pos, (unsigned long long)n, k, r, band.data(), wave != 0);
                        ++checked;
                        if (a != b && ++bad <= 8) printf("SHARD n %ld m %d r %d pos %ld shard [%ld, %ld): %d, whole text %d\n", n, m, r, pos, lo, hi, a, b);
                    }
                }
        }
}

int main() {
    // random DNA of 40 .. 400 bytes with copies of the patterns at 0 .. 3 edits planted
    const int lens[] = {40, 97, 180, 400};
    for (int n : lens) {
        Str text = dna(n);
        std::vector<Str> pats;
        const int ms[] = {1, 2, 5, 9, 16, 17, 24};
        for (int m : ms) pats.push_back(dna(m));
        long at = 3;
        for (size_t q = 0; q < pats.size() && at + 24 < n; ++q) {
            Str w = pats[q];
            for (unsigned e = 0; e < q % 4 && e < w.size(); ++e) w[rnd((unsigned)w.size())] = (unsigned char)"ACGT"[rnd(4)];
            if (w.size() > 8 && q % 2) { w.erase(w.begin() + 3); w.insert(w.begin() + 7, 'T'); } // a deletion and an insertion: seen one column off
            for (size_t i = 0; i < w.size(); ++i) text[(size_t)at + i] = w[i];
            at += (long)w.size() + 11;
        }
        check_text(text, pats, "DNA");
    }
    // low entropy: plateaus and chains of equal distances; the short ones have m > n
    check_text(tandem("A", 200), {tandem("A", 16), tandem("A", 1), tandem("A", 24)}, "POLYA");
    check_text(tandem("A", 7), {tandem("A", 16), tandem("A", 3)}, "POLYA");
    check_text(tandem("ACG", 80), {tandem("ACG", 6), tandem("ACG", 1), tandem("ACG", 8)}, "ACG");
    check_text(tandem("ACG", 4), {tandem("ACG", 6), tandem("CG", 2)}, "ACG");
    // what include/apm.h states about ACG x 80, pattern ACG x 6, k = 3: 237 matches, 79 kept at r = 1 or 2, 1 at r >= 3
    {
        const Str text = tandem("ACG", 80), pat = tandem("ACG", 6);
        const std::vector<int> s = scores(text, pat, 3);
        long matches = 0, kept[4] = {0, 0, 0, 0};
        const int rs[4] = {1, 2, 3, 64};
        for (long j = 0; j < (long)text.size() - 3; ++j) matches += s[(size_t)j] <= 3;
        for (int q = 0; q < 4; ++q)
            for (long j = 0; j < (long)text.size() - 3; ++j) kept[q] += rule(s, j, 3, rs[q]); // (the find calls' records: the starts in W)
        if (matches != 237 || kept[0] != 79 || kept[1] != 79 || kept[2] != 1 || kept[3] != 1) {
            printf("ACG x 80: %ld matches, kept %ld %ld %ld %ld\n", matches, kept[0], kept[1], kept[2], kept[3]);
            ++bad;
        }
    }
    {
        Str text = dna(61);
        const Str pat = dna(9);
        for (size_t i = 0; i < pat.size(); ++i) text[20 + i] = text[47 + i] = pat[i];
        check_coverage(text, pat, 3);
        check_coverage(text, pat, 8);
    }
    printf("%ld checks, %ld best hits (%ld truncated), %ld k >= m, %ld m > n, coverage %ld yes %ld no, %ld wrong\n", checked, kept_total, truncated, k_ge_m,
           m_gt_n, covered_yes, covered_no, bad);
    if (checked < 100000 || kept_total < 1000 || truncated < 10 || k_ge_m < 10 || m_gt_n < 2 || covered_yes < 1000 || covered_no < 1000 || bad) return 1;
    return 0;
}
