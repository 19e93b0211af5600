// Host-side check of the align pass's arithmetic core (csrc/apm_align.h): the lane form (one pair per lane, the trace
// in a workspace) and the wave form as its plain loop over 64 emulated lanes must both give n_ops == 0 exactly when
// dist > k and otherwise, bit for bit, the canonical script -- the literal full-matrix DP and the walk back of the rule
// (diagonal, else D, else I) written out below -- on whole pairs and on pairs truncated to size < m.  The full matrix's
// corner is cross-checked against the oracle's window distance.  Input: a file of "<pattern hex> <window hex>" lines
// (helpers.window_distance_pairs()).  Built with -fsanitize=address,undefined and run by tests/test_align_host.py.
#include "apm_align.h"
#include "apm_oracle.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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

// a lane's trace row: exactly `size` columns
struct Trace {
    std::vector<uint16_t> w;
    void put(int col, uint32_t v) { w.at((size_t)col) = (uint16_t)v; }
    uint32_t get(int col) const { return w.at((size_t)col); }
};

// a record's row: exactly the words a script of the pair may take; every store is remembered
struct Row {
    std::vector<uint32_t> w;
    std::vector<char> stored;
    explicit Row(int words) : w((size_t)words, 0xdeadbeefu), stored((size_t)words, 0) {}
    void store(int word, uint32_t v) { w.at((size_t)word) = v; stored.at((size_t)word) = 1; }
};

// the truth: the literal full matrix, then the canonical walk; ops first to last
static int truth(const unsigned char *p, const unsigned char *t, int size, std::vector<int> &ops) {
    const int W = size + 1;
    std::vector<int> c((size_t)W * W); // c[x * W + y]
    for (int x = 0; x <= size; ++x) c[(size_t)x * W] = x;
    for (int y = 0; y <= size; ++y) c[(size_t)y] = y;
    for (int x = 1; x <= size; ++x)
        for (int y = 1; y <= size; ++y) {
            int v = c[(size_t)(x - 1) * W + y - 1] + (p[y - 1] != t[x - 1]);
            if (c[(size_t)(x - 1) * W + y] + 1 < v) v = c[(size_t)(x - 1) * W + y] + 1;
            if (c[(size_t)x * W + y - 1] + 1 < v) v = c[(size_t)x * W + y - 1] + 1;
            c[(size_t)x * W + y] = v;
        }
    ops.clear();
    int x = size, y = size;
    while (x > 0 || y > 0) {
        if (y == 0) { ops.push_back(2); --x; }
        else if (x == 0) { ops.push_back(3); --y; }
        else if (c[(size_t)(x - 1) * W + y - 1] + (p[y - 1] != t[x - 1]) == c[(size_t)x * W + y]) { ops.push_back(p[y - 1] != t[x - 1]); --x; --y; }
        else if (c[(size_t)x * W + y - 1] + 1 == c[(size_t)x * W + y]) { ops.push_back(3); --y; }
        else { ops.push_back(2); --x; }
    }
    for (size_t i = 0, j = ops.size(); i + 1 < j; ++i) { --j; const int s = ops[i]; ops[i] = ops[j]; ops[j] = s; }
    return c[(size_t)size * W + size];
}

// does the row hold exactly the script `ops` (n_ops as returned), stored word for word and nothing else?
static bool same(const Row &r, int n_ops, const std::vector<int> &ops, bool within) {
    if (!within) {
        for (char s : r.stored) if (s) return false; // farther than k: nothing stored
        return n_ops == 0;
    }
    if (n_ops != (int)ops.size()) return false;
    std::vector<uint32_t> want((size_t)apm_align_words(n_ops), 0u);
    for (int j = 0; j < n_ops; ++j) want[(size_t)(1 + j / 16)] |= (uint32_t)ops[(size_t)j] << (2 * (j % 16));
    for (size_t i = 1; i < r.w.size(); ++i) {
        const bool used = i < want.size();
        if (used != (r.stored[i] != 0)) return false;
        if (used && r.w[i] != want[i]) return false;
    }
    return !r.stored[0];
}

template <int BAND>
static int lane(const Bytes &p, const Bytes &t, int size, int k, Trace &tr, Row &out) { return apm_align_lane<BAND>(p, t, size, k, tr, out); }

static int lane_form(const Bytes &p, const Bytes &t, int size, int k, Trace &tr, Row &out) {
    switch (k / 2) {
    case 0: return lane<0>(p, t, size, k, tr, out);
    case 1: return lane<1>(p, t, size, k, tr, out);
    case 2: return lane<2>(p, t, size, k, tr, out);
    default: return lane<3>(p, t, size, k, tr, out);
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
    std::vector<int> band(APM_SCORE_BAND_CELLS), col(1024), ops;
    long pairs = 0, checked = 0, bad = 0, multi_chunk = 0, truncated = 0, with_indel = 0, scripts = 0;
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
            const int d = truth(pp.data(), tt.data(), size, ops);
            if (d != oracle_window_distance(pp.data(), tt.data(), size, col.data())) { printf("pair %ld size %d: the full matrix disagrees with the oracle\n", pairs, size); ++bad; }
            int edits = 0, ins = 0, del = 0;
            for (int o : ops) { edits += o != 0; ins += o == 2; del += o == 3; }
            if (edits != d || ins != del || (int)ops.size() != size + ins) { printf("pair %ld size %d: the reference script is no script of cost %d\n", pairs, size, d); ++bad; }
            with_indel += ins > 0;
            truncated += size < m;
            for (int k : lane_ks) {
                Trace tr{std::vector<uint16_t>((size_t)size, 0xffffu)};
                Row row(apm_align_words(apm_align_max_ops(size, k)));
                const int got = lane_form(p, t, size, k, tr, row);
                ++checked;
                scripts += d <= k;
                if (!same(row, got, ops, d <= k) && ++bad <= 8) printf("LANE pair %ld size %d k %d dist %d: n_ops %d, want %d\n", pairs, size, k, d, got, d <= k ? (int)ops.size() : 0);
            }
            for (int k : wave_ks) {
                const int h = k / 2 < size - 1 ? k / 2 : size - 1, chunks = (2 * h + 1 + 63) >> 6;
                std::vector<unsigned long long> ws((size_t)2 * size * chunks, ~0ull);
                Row row(apm_align_words(apm_align_max_ops(size, k)));
                const int got = apm_align_wave_lanes(p, t, size, k, band.data(), ws.data(), row);
                ++checked;
                scripts += d <= k;
                multi_chunk += chunks > 1;
                if (!same(row, got, ops, d <= k) && ++bad <= 8) printf("WAVE pair %ld size %d k %d dist %d: n_ops %d, want %d\n", pairs, size, k, d, got, d <= k ? (int)ops.size() : 0);
            }
        }
    }
    fclose(f);
    printf("%ld pairs, %ld truncated, %ld with an insertion and a deletion, %ld scripts, %ld with more than one chunk of 64 diagonals: %ld checked, %ld wrong\n",
           pairs, truncated, with_indel, scripts, multi_chunk, checked, bad);
    if (pairs < 3000 || truncated < 1000 || with_indel < 100 || multi_chunk < 100 || scripts < 10000 || bad) return 1;
    return 0;
}
