// Host-side check of the scoring pass's arithmetic core (csrc/apm_score.h) against the oracle's literal window DP: the
// lane form (one pair per lane, band in registers, k <= 7) and the wave form as its plain loop over 64 emulated lanes
// (chunks of 64 diagonals, carry from chunk to chunk) must both return min(dist, k + 1), on whole pairs and on pairs
// truncated to size < m as the windows at the end of a text are.  Input: a file of "<pattern hex> <window hex>" lines
// (helpers.window_distance_pairs()).  Built with -fsanitize=address,undefined and run by tests/test_score_host.py.
#include "apm_score.h"
#include "apm_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// a string as the kernels' sources see it: exactly n bytes on the heap, so that the sanitizer sees every read beyond
struct Bytes {
    const unsigned char *b;
    int n;
    void load16(int off, uint32_t (&w)[4]) const { // (the device rows are zero padded; here the padding is made up)
        for (int i = 0; i < 4; ++i) w[i] = 0u;
        for (int i = 0; i < 16; ++i)
            if (off + i >= 0 && off + i < n) w[i >> 2] |= (uint32_t)b[off + i] << (8 * (i & 3));
    }
    int byte(int i) const {
        if (i < 0 || i >= n) { fprintf(stderr, "byte %d read outside [0, %d)\n", i, n); abort(); }
        return b[i];
    }
};

template <int BAND>
static int lane(const Bytes &p, const Bytes &t, int size, int k) { return apm_score_lane<BAND>(p, t, size, k); }

static int lane_form(const Bytes &p, const Bytes &t, int size, int k) {
    switch (k / 2) {
    case 0: return lane<0>(p, t, size, k);
    case 1: return lane<1>(p, t, size, k);
    case 2: return lane<2>(p, t, size, k);
    default: return lane<3>(p, t, size, k);
    }
}

static std::vector<unsigned char> unhex(const char *s, size_t n) {
    std::vector<unsigned char> v(n / 2);
    for (size_t i = 0; i < v.size(); ++i) {
        unsigned x = 0;
        sscanf(s + 2 * i, "%2x", &x);
        v[i] = (unsigned char)x;
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    static const int lane_ks[] = {0, 1, 2, 3, 4, 5, 6, 7};
    static const int wave_ks[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 40, 130, 300};
    std::vector<int> band(APM_SCORE_BAND_CELLS), col(1024);
    long pairs = 0, checked = 0, bad = 0, multi_chunk = 0, truncated = 0;
    char line[1024];
    while (fgets(line, sizeof line, f)) {
        char *sp = strchr(line, ' ');
        if (!sp) continue;
        size_t tl = strlen(sp + 1);
        while (tl && (sp[tl] == '\n' || sp[tl] == '\r')) --tl;
        const std::vector<unsigned char> P = unhex(line, (size_t)(sp - line)), T = unhex(sp + 1, tl);
        if (P.empty() || P.size() != T.size()) { fprintf(stderr, "bad line %ld\n", pairs); return 2; }
        const int m = (int)P.size();
        ++pairs;
        // the whole pair, and (where m > 1) one truncation to size < m: 1, m - 1 or something between, by turns
        int sizes[2] = {m, m};
        if (m > 1) sizes[1] = pairs % 3 == 0 ? 1 : (pairs % 3 == 1 ? m - 1 : 1 + (int)((pairs * 7) % (m - 1)));
        for (int s = 0; s < (m > 1 ? 2 : 1); ++s) {
            const int size = sizes[s];
            // exactly `size` bytes each: a read behind the window is a heap overflow
            std::vector<unsigned char> pp(P.begin(), P.begin() + size), tt(T.begin(), T.begin() + size);
            const Bytes p{pp.data(), size}, t{tt.data(), size};
            const int d = oracle_window_distance(pp.data(), tt.data(), size, col.data());
            truncated += size < m;
            for (int k : lane_ks) {
                const int want = d < k + 1 ? d : k + 1, got = lane_form(p, t, size, k);
                ++checked;
                if (got != want && ++bad <= 8) printf("LANE pair %ld size %d k %d: %d, want %d\n", pairs, size, k, got, want);
            }
            for (int k : wave_ks) {
                const int want = d < k + 1 ? d : k + 1, got = apm_score_wave_lanes(p, t, size, k, band.data());
                ++checked;
                multi_chunk += 2 * (k / 2 < size - 1 ? k / 2 : size - 1) + 1 > 64;
                if (got != want && ++bad <= 8) printf("WAVE pair %ld size %d k %d: %d, want %d\n", pairs, size, k, got, want);
            }
        }
    }
    fclose(f);
    printf("%ld pairs, %ld truncated, %ld checks (%ld with more than one chunk of 64 diagonals), %ld wrong\n", pairs, truncated, checked,
           multi_chunk, bad);
    if (pairs < 3000 || truncated < 1000 || multi_chunk < 100 || bad) return 1;
    return 0;
}
