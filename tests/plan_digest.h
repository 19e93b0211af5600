/*
 * plan_digest.h -- prints a launch plan's structure and a 64-bit FNV-1a digest over everything in it that reaches a
 * device buffer or a launch argument (tests/host_plan_test.cpp; tests/golden/plan_digests.json holds the output).
 * The parts of the plan are template parameters so that the same code, hashing the same fields in the same order, can
 * be pointed at any holder of them.
 */
#ifndef PLAN_DIGEST_H
#define PLAN_DIGEST_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

struct PlanDigest {
    uint64_t h = 0xcbf29ce484222325ull;
    void raw(const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    }
    void num(int64_t v) { raw(&v, 8); }
    void real(double v) { raw(&v, 8); }
    template <typename T> void vec(const std::vector<T> &v) { // (T: no padding bytes -- integers, ApmPatDesc, ApmKey)
        num((int64_t)v.size());
        if (!v.empty()) raw(v.data(), v.size() * sizeof(T));
    }
};

template <typename Group> void plan_digest_group(PlanDigest &d, const Group &g) {
    d.vec(g.descs);
    d.num(g.m_max);
}

template <typename Tiled> void plan_digest_tiled(PlanDigest &d, const Tiled &L) {
    d.num(L.kind);
    d.vec(L.descs); d.vec(L.bytes); d.vec(L.tables);
    d.raw(L.lut, 256);
    d.vec(L.keys); d.vec(L.piece_off); d.vec(L.table); d.vec(L.table_kid); d.vec(L.ovf); d.vec(L.kinfo); d.vec(L.pinfo); d.vec(L.image);
    for (int v : {L.o_tab, L.o_kid, L.o_ovf, L.o_kinfo, L.o_pinfo, L.o_next, L.o_poff, L.o_bmp, L.code_shift, L.o_pat, L.o_kext, L.key_len,
                  L.stride, (int)L.sieved, L.nb, L.lg_nb, L.qcap, L.a_max, L.m_max, L.m_min, L.tile})
        d.num(v);
}

template <typename Verify> void plan_digest_verify(PlanDigest &d, const Verify &V) {
    d.vec(V.descs); d.vec(V.bytes); d.vec(V.kinfo); d.vec(V.kpart); d.vec(V.pinfo); d.vec(V.image);
    for (int v : {V.o_prefix, V.o_r2s, V.o_slots, V.o_kext, V.o_pat, V.o_masks, V.o_kinfo, V.o_pinfo, V.o_rc, V.m_max, V.m_min}) d.num(v);
    d.vec(V.bitmap18); d.vec(V.cf_image);
    for (int v : {V.cf_o_rrec, V.cf_o_lrec, V.cf_o_dp, V.cf_dp_cols, V.cf_dp_slots}) d.num(v);
}

// status / err: what the plan builder returned; the rest: the patterns it resolved and the parts of the plan it filled
template <typename Pats, typename TiledVec, typename Sieve, typename Group>
void plan_report(FILE *f, const char *name, int status, const std::string &err, const Pats &pats, const TiledVec &tiled, const Sieve &S,
                 const Group &tails, const Group &stails, const Group &wtails, const Group &xtails, const Group &longs,
                 const std::vector<int> &trivial, const std::vector<uint8_t> &allpat, int m_max) {
    fprintf(f, "set %s\nstatus %d %s\n", name, status, status ? err.c_str() : "");
    if (status) return;
    // resolved kernels, run-length coded
    fprintf(f, "kernels");
    for (size_t i = 0; i < pats.size();) {
        size_t j = i;
        while (j < pats.size() && pats[j].kernel == pats[i].kernel) ++j;
        fprintf(f, " %dx%zu", pats[i].kernel, j - i);
        i = j;
    }
    fprintf(f, "\n");
    PlanDigest d;
    for (const auto &p : pats) d.num(p.kernel);
    d.num((int64_t)tiled.size());
    for (const auto &L : tiled) {
        fprintf(f, "tiled kind=%d key_len=%d stride=%d sieved=%d m_min=%d m_max=%d pats=%zu\n", L.kind, L.key_len, L.stride, (int)L.sieved, L.m_min,
                L.m_max, L.descs.size());
        plan_digest_tiled(d, L);
    }
    fprintf(f, "sieve on=%d stride=%d code_shift=%d per_launch_sieve=%d m_max=%d launches=%zu\n", (int)S.on, S.stride, S.code_shift,
            (int)S.per_launch_sieve, S.m_max, S.launches.size());
    d.num(S.on); d.num(S.stride); d.num(S.code_shift); d.num(S.m_max); d.real(S.rate); d.vec(S.bitmap); d.real(S.weak_frac); d.num(S.per_launch_sieve);
    d.num((int64_t)S.launches.size());
    for (const auto &V : S.launches) {
        fprintf(f, "verify m_min=%d m_max=%d pats=%zu keys=%zu dp_slots=%d\n", V.m_min, V.m_max, V.descs.size(), V.kinfo.size(), V.cf_dp_slots);
        plan_digest_verify(d, V);
    }
    fprintf(f, "groups tails=%zu stails=%zu wtails=%zu xtails=%zu longs=%zu trivial=%zu m_max=%d\n", tails.descs.size(), stails.descs.size(),
            wtails.descs.size(), xtails.descs.size(), longs.descs.size(), trivial.size(), m_max);
    plan_digest_group(d, tails); plan_digest_group(d, stails); plan_digest_group(d, wtails); plan_digest_group(d, xtails); plan_digest_group(d, longs);
    d.vec(trivial); d.vec(allpat); d.num(m_max);
    fprintf(f, "digest %016llx\n", (unsigned long long)d.h);
}

// one input line: <name> <k> <forced kernel> <pattern as hex>...
struct PlanRequest {
    std::string name;
    int k = 0, kernel = 0;
    std::vector<std::string> pats;
};

inline bool plan_read_request(FILE *f, PlanRequest *r) {
    std::string line;
    for (int c; (c = fgetc(f)) != EOF && c != '\n';) line.push_back((char)c);
    if (line.empty()) return false;
    std::vector<std::string> tok;
    for (size_t i = 0; i < line.size();) {
        size_t j = line.find(' ', i);
        if (j == std::string::npos) j = line.size();
        if (j > i) tok.push_back(line.substr(i, j - i));
        i = j + 1;
    }
    if (tok.size() < 4) return false;
    r->name = tok[0];
    r->k = atoi(tok[1].c_str());
    r->kernel = atoi(tok[2].c_str());
    r->pats.clear();
    auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    for (size_t t = 3; t < tok.size(); ++t) {
        std::string b;
        for (size_t i = 0; i + 1 < tok[t].size(); i += 2) b.push_back((char)(nib(tok[t][i]) * 16 + nib(tok[t][i + 1])));
        r->pats.push_back(b);
    }
    return true;
}

#endif /* PLAN_DIGEST_H */
