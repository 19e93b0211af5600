// Host-side check of apm_code_dp_pass (csrc/apm_core.h), the code-filter sieve's window DP on 2-bit codes, against the
// oracle's literal window DP.  A unit at pattern offset o nominates the window starting at j from the text position
// s = j + o + dl, |dl| <= k; the sieve then judges the region [s - o - k, s - o + m + k) = [j + dl - k, j + dl + m + k).
// For every window within k edits of the pattern and every such dl, the predicate must pass.  Built and run by
// tests/test_code_dp_host.py (g++, no GPU).
#include "apm_core.h"
#include "apm_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static const char *kAcgt = "ACGT";
static const char *kAmino = "ACDEFGHIKLMNPQRSTVWY";

// region codes [r, r + cols) of text t[0..n); bytes outside the text read as zero (as beyond a shard)
static void region_codes(const unsigned char *t, int n, int r, int cols, int shift, uint32_t (&c)[3]) {
    c[0] = c[1] = c[2] = 0u;
    for (int i = 0; i < cols; i++) {
        const int x = r + i;
        const unsigned b = (x >= 0 && x < n) ? t[x] : 0u;
        c[i >> 4] |= ((b >> shift) & 3u) << (2 * (i & 15));
    }
}

static void planes(const unsigned char *p, int m, int shift, uint32_t *b0, uint32_t *b1) {
    *b0 = *b1 = 0u;
    for (int y = 0; y < m; y++) {
        const uint32_t code = (p[y] >> shift) & 3u;
        *b0 |= (code & 1u) << y;
        *b1 |= (code >> 1) << y;
    }
}

int main() {
    srand(7);
    long checked = 0, bad = 0;
    std::vector<int> col(64);
    for (int alpha = 0; alpha < 2; alpha++) {
        const char *abc = alpha ? kAmino : kAcgt;
        const int na = alpha ? 20 : 4;
        for (int shift = (alpha ? 0 : 1); shift <= (alpha ? 6 : 1); shift++)
            for (int k = 0; k <= 7; k++)
                for (int m = 4 * (k + 1); m <= 32; m++)
                    for (int trial = 0; trial < (alpha ? 6 : 24); trial++) {
                        unsigned char p[32], t[160];
                        for (int y = 0; y < m; y++) p[y] = (unsigned char)abc[rand() % na];
                        // text: random, with the pattern planted at 40 under up to k random edits
                        const int n = 40 + m + 48;
                        for (int x = 0; x < n; x++) t[x] = (unsigned char)abc[rand() % na];
                        std::vector<unsigned char> w(p, p + m);
                        const int edits = rand() % (k + 1);
                        for (int e = 0; e < edits && !w.empty(); e++) {
                            const int at = rand() % (int)w.size(), kind = rand() % 3;
                            if (kind == 0) w[at] = (unsigned char)abc[rand() % na];
                            else if (kind == 1) w.erase(w.begin() + at);
                            else w.insert(w.begin() + at, (unsigned char)abc[rand() % na]);
                        }
                        for (size_t i = 0; i < w.size() && 40 + i < (size_t)n; i++) t[40 + i] = w[i];
                        uint32_t b0, b1;
                        planes(p, m, shift, &b0, &b1);
                        const int cols = m + 2 * k;
                        for (int j = 0; j + m <= n; j++) {
                            if (oracle_window_distance(p, t + j, m, col.data()) > k) continue;
                            for (int dl = -k; dl <= k; dl++) {
                                uint32_t c[3];
                                region_codes(t, n, j + dl - k, cols, shift, c);
                                ++checked;
                                if (!apm_code_dp_pass<3>(b0, b1, m, c, cols, k)) {
                                    if (++bad <= 5)
                                        printf("MISS alpha=%d shift=%d k=%d m=%d j=%d dl=%d\n", na, shift, k, m, j, dl);
                                }
                            }
                        }
                    }
    }
    // the two-word form the kernel runs (cols <= 30) agrees with the three-word form
    long diff = 0;
    for (int it = 0; it < 200000; it++) {
        const int k = rand() % 4, m = 4 * (k + 1) + rand() % (30 - 2 * k - 4 * (k + 1) + 1), cols = m + 2 * k;
        unsigned char p[32], t[64];
        for (int y = 0; y < m; y++) p[y] = (unsigned char)kAcgt[rand() % 4];
        for (int x = 0; x < cols; x++) t[x] = (unsigned char)kAcgt[rand() % 4];
        uint32_t b0, b1, c3[3];
        planes(p, m, 1, &b0, &b1);
        region_codes(t, cols, 0, cols, 1, c3);
        const uint32_t c2[2] = {c3[0], c3[1] | (5u << 28)}; // (the kernel keeps the slot in the top two codes: never read)
        diff += apm_code_dp_pass<2>(b0, b1, m, c2, cols, k) != apm_code_dp_pass<3>(b0, b1, m, c3, cols, k);
    }
    // it is a filter worth running: random DNA regions of the cfg3 short patterns rarely pass (m = 16, k = 3: ~1e-3)
    long pass16 = 0;
    const int trials = 200000;
    for (int it = 0; it < trials; it++) {
        unsigned char p[16], t[22];
        for (int y = 0; y < 16; y++) p[y] = (unsigned char)kAcgt[rand() % 4];
        for (int x = 0; x < 22; x++) t[x] = (unsigned char)kAcgt[rand() % 4];
        uint32_t b0, b1, c[3];
        planes(p, 16, 1, &b0, &b1);
        region_codes(t, 22, 0, 22, 1, c);
        pass16 += apm_code_dp_pass<3>(b0, b1, 16, c, 22, 3);
    }
    printf("checked %ld (window, shift) pairs, %ld missed; two-word form differs in %ld; m=16 k=3 random pass rate %.2e\n",
           checked, bad, diff, (double)pass16 / trials);
    if (checked < 10000 || bad || diff || pass16 > trials / 100) return 1;
    return 0;
}
