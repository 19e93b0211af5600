// Host-side check of apm_code_dp_diag (csrc/apm_core.h), the diagonal form of the code-filter sieve's window DP for k <= 3,
// against the oracle's literal window DP.  A unit at pattern offset o nominates, from the text position s, the window
// starts j = s - o - dl, |dl| <= B = k / 2 (what the verify launch tests); the sieve judges the region
// [c - B, c + m + B), c = s - o.  For every centre c:
//   (a) never false when some dl has window distance <= k on the bytes;
//   (b) equal to that condition on the codes -- on ACGT, whose codes tell the letters apart, on the bytes;
//   (c) whatever it passes, apm_code_dp_pass passes on the wide region [c - k, c + m + k).
// Bytes outside the text read as zeros, as beyond a shard.  Built and run by tests/test_code_dp_diag_host.py (g++, no GPU).
#include "apm_core.h"
#include "apm_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static const char *kAcgt = "ACGT";
static const char *kAmino = "ACDEFGHIKLMNPQRSTVWY";
static const int PAD = 40; // zeros on either side of the text

static void planes(const unsigned char *p, int m, int shift, uint32_t *b0, uint32_t *b1) {
    *b0 = *b1 = 0u;
    for (int y = 0; y < m; y++) {
        const uint32_t code = (p[y] >> shift) & 3u;
        *b0 |= (code & 1u) << y;
        *b1 |= (code >> 1) << y;
    }
}

struct Case {
    std::vector<unsigned char> tb, tc; // text bytes and codes, PAD zeros on either side
    unsigned char p[32], pc[32];
    int m, k, shift, n;
    uint32_t b0, b1;
};

static long g_checked = 0, g_miss = 0, g_extra = 0, g_notcol = 0, g_dist_k = 0, g_dist_k1 = 0;

static bool diag(const Case &c, int centre) {
    const int B = c.k / 2;
    uint32_t t0, t1;
    planes(c.tc.data() + PAD + centre - B, c.m + 2 * B, 0, &t0, &t1);
    return B ? apm_code_dp_diag<1>(c.b0, c.b1, c.m, t0, t1, c.k) : apm_code_dp_diag<0>(c.b0, c.b1, c.m, t0, t1, c.k);
}

static void check_centre(const Case &c, int centre, bool acgt) {
    static std::vector<int> col(64);
    const int B = c.k / 2;
    bool on_bytes = false, on_codes = false;
    for (int dl = -B; dl <= B; dl++) {
        const int db = oracle_window_distance(c.p, c.tb.data() + PAD + centre - dl, c.m, col.data());
        const int dc = oracle_window_distance(c.pc, c.tc.data() + PAD + centre - dl, c.m, col.data());
        on_bytes |= db <= c.k;
        on_codes |= dc <= c.k;
        g_dist_k += db == c.k;
        g_dist_k1 += db == c.k + 1;
    }
    const bool got = diag(c, centre);
    ++g_checked;
    const bool inside = centre - B >= 0 && centre + c.m + B <= c.n; // (outside, a zero byte and an 'A' share a code)
    if ((on_bytes && !got) || (on_codes && !got)) {
        if (++g_miss <= 5) printf("MISS shift=%d k=%d m=%d centre=%d\n", c.shift, c.k, c.m, centre);
    } else if (got && (!on_codes || (acgt && inside && !on_bytes))) {
        if (++g_extra <= 5) printf("EXTRA shift=%d k=%d m=%d centre=%d\n", c.shift, c.k, c.m, centre);
    }
    if (got) {
        uint32_t cw[3] = {0u, 0u, 0u};
        const int cols = c.m + 2 * c.k;
        for (int i = 0; i < cols; i++) cw[i >> 4] |= (uint32_t)c.tc[(size_t)(PAD + centre - c.k + i)] << (2 * (i & 15));
        if (!apm_code_dp_pass<3>(c.b0, c.b1, c.m, cw, cols, c.k) && ++g_notcol <= 5)
            printf("NOT IN COLUMN FORM shift=%d k=%d m=%d centre=%d\n", c.shift, c.k, c.m, centre);
    }
}

// the pattern under an edit script, planted at `at`; kind: 0 random edits (`edits` of them), 1 one insertion in the first
// two bytes + one deletion in the last two (the path lives on diagonal +1), 2 the reverse (diagonal -1), 3 `edits` substitutions
// at distinct rows (distance exactly `edits`)
static void plant(Case &c, const char *abc, int na, int at, int kind, int edits) {
    std::vector<unsigned char> w(c.p, c.p + c.m);
    auto other = [&](unsigned char b) { unsigned char x; do x = (unsigned char)abc[rand() % na]; while (x == b); return x; };
    if (kind == 0) {
        for (int e = 0; e < edits && !w.empty(); e++) {
            const int i = rand() % (int)w.size(), what = rand() % 3;
            if (what == 0) w[i] = other(w[i]);
            else if (what == 1) w.erase(w.begin() + i);
            else w.insert(w.begin() + i, (unsigned char)abc[rand() % na]);
        }
    } else if (kind == 1) {
        w.erase(w.begin() + (c.m - 1 - rand() % 2));
        w.insert(w.begin() + rand() % 2, (unsigned char)abc[rand() % na]);
    } else if (kind == 2) {
        w.insert(w.begin() + (c.m - rand() % 2), (unsigned char)abc[rand() % na]);
        w.erase(w.begin() + rand() % 2);
    } else {
        for (int e = 0; e < edits; e++) { const int i = (e * c.m) / edits + rand() % (c.m / edits); w[i] = other(w[i]); }
    }
    for (size_t i = 0; i < w.size() && at + (int)i < c.n; i++)
        if (at + (int)i >= 0) c.tb[(size_t)(PAD + at + (int)i)] = w[i];
}

int main() {
    srand(11);
    for (int alpha = 0; alpha < 2; alpha++) {
        const char *abc = alpha ? kAmino : kAcgt;
        const int na = alpha ? 20 : 4;
        for (int shift = (alpha ? 0 : 1); shift <= (alpha ? 6 : 1); shift++)
            for (int k = 0; k <= 3; k++)
                for (int m = 4 * (k + 1); m <= 30 - 2 * k; m++) // every m the plan gives a slot (m + 2k <= APM_CF_DP_COLS)
                    for (int trial = 0; trial < (alpha ? 6 : 40); trial++) {
                        Case c;
                        c.m = m; c.k = k; c.shift = shift; c.n = 3 * m + 40;
                        c.tb.assign((size_t)(c.n + 2 * PAD), 0);
                        for (int y = 0; y < m; y++) c.p[y] = (unsigned char)abc[rand() % na];
                        for (int x = 0; x < c.n; x++) c.tb[(size_t)(PAD + x)] = (unsigned char)abc[rand() % na];
                        // occurrences: at the text's start (the region begins in front of it), in the middle, at its end
                        const int at[3] = {0, m + 20, c.n - m};
                        for (int o = 0; o < 3; o++) {
                            const int kind = k >= 2 ? (trial + o) % 4 : ((trial + o) % 2 ? 3 : 0);
                            const int edits = kind == 3 ? (k + (trial & 1)) : rand() % (k + 2); // exactly k or k + 1 / 0 .. k + 1 random
                            if (kind == 3 && edits == 0) continue;
                            plant(c, abc, na, at[o], kind, edits);
                        }
                        c.tc.resize(c.tb.size());
                        for (size_t i = 0; i < c.tb.size(); i++) c.tc[i] = (c.tb[i] >> shift) & 3u;
                        for (int y = 0; y < m; y++) c.pc[y] = (c.p[y] >> shift) & 3u;
                        planes(c.p, m, shift, &c.b0, &c.b1);
                        for (int o = 0; o < 3; o++)
                            for (int centre = at[o] - 3; centre <= at[o] + 3; centre++) check_centre(c, centre, !alpha);
                    }
    }
    // the kernel's way from a queue entry's two dwords of codes to the bit planes
    long planes_bad = 0;
    for (int it = 0; it < 100000; it++) {
        const uint32_t lo = ((uint32_t)rand() << 16) ^ (uint32_t)rand(), hi = ((uint32_t)rand() << 16) ^ (uint32_t)rand();
        uint32_t t0, t1, w0 = 0u, w1 = 0u;
        apm_code_planes(lo, hi, t0, t1);
        for (int i = 0; i < 32; i++) {
            const uint32_t code = ((i < 16 ? lo : hi) >> (2 * (i & 15))) & 3u;
            w0 |= (code & 1u) << i;
            w1 |= (code >> 1) << i;
        }
        planes_bad += t0 != w0 || t1 != w1;
    }
    if (planes_bad) { printf("apm_code_planes differs from the plain loop in %ld cases\n", planes_bad); return 1; }
    // both forms on random DNA regions of the headline's shortest pattern: the diagonal form passes no more than the column form
    long pass_diag = 0, pass_col = 0;
    const int trials = 2000000;
    for (int it = 0; it < trials; it++) {
        unsigned char p[16], t[22];
        for (int y = 0; y < 16; y++) p[y] = (unsigned char)((kAcgt[rand() % 4] >> 1) & 3);
        for (int x = 0; x < 22; x++) t[x] = (unsigned char)((kAcgt[rand() % 4] >> 1) & 3);
        uint32_t b0, b1, t0, t1, cw[3] = {0u, 0u, 0u};
        planes(p, 16, 0, &b0, &b1);
        planes(t + 2, 18, 0, &t0, &t1); // [c - 1, c + 17) of the wide region [c - 3, c + 19)
        for (int i = 0; i < 22; i++) cw[i >> 4] |= (uint32_t)t[i] << (2 * (i & 15));
        pass_diag += apm_code_dp_diag<1>(b0, b1, 16, t0, t1, 3);
        pass_col += apm_code_dp_pass<3>(b0, b1, 16, cw, 22, 3);
    }
    printf("checked %ld centres: %ld missed, %ld extra, %ld not passed by the column form; window distances == k: %ld, == k + 1: %ld; "
           "m=16 k=3 random pass rate %.2e (column form %.2e)\n",
           g_checked, g_miss, g_extra, g_notcol, g_dist_k, g_dist_k1, (double)pass_diag / trials, (double)pass_col / trials);
    if (g_checked < 100000 || g_miss || g_extra || g_notcol || g_dist_k < 1000 || g_dist_k1 < 1000 || pass_diag > pass_col) return 1;
    return 0;
}
