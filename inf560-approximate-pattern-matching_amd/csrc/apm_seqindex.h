/*
 * apm_seqindex.h -- the sequence index behind the text modes (include/apm.h: "sequences"): the table of a normalised
 * source's FASTA sequences and the location of a match record in it.  The arithmetic -- which bytes open a header, what a
 * lane emits for them, the 64-way search of the table, the flags of a location -- compiles for host and device: the kernels
 * (apm_seqindex.hip) and tests/host_seqindex_test.cpp run this very code.  The launch arguments are the `__HIPCC__` part.
 *
 * The passes read the source as the normalisation pass does (apm_textnorm.h): 4 KiB blocks on the 16-byte grid of memory,
 * one wavefront per block, four chunks of 64 lanes x 16 bytes, and they lean on its map: the kept bytes in front of every
 * block and the header state the block is entered in.
 *   count    per block the number of header opens: '>' at a line start, LS & GT of the lane's masks -- no header state needed
 *   scan     ONE workgroup turns the counts into 64-bit prefixes and the total (n_seq - 1)
 *   emit     per block again, the state now from the map: entry 1 + prefix + rank of every open = { its source offset, the
 *            kept bytes in front of it }; a lane holds up to 8 opens ("\n>\n>...")
 *   locate   one wavefront per record: block (pos + lead) / 4096 directly, its lanes resolved with the map's state (is the
 *            byte kept, and its index c in T), then the table searched by hdr_off, 64 probes a round
 */
#ifndef APM_SEQINDEX_H
#define APM_SEQINDEX_H

#include "../../include/apm.h"
#include "apm_textnorm.h"

// the lane's header opens, bit i = byte i: a '>' at a line start (ls_in: the lane's first byte is one); none without FASTA
APM_TN_FN uint32_t apm_sq_opens(const ApmTnMasks &m, uint32_t flags, uint32_t ls_in) {
    if (!(flags & APM_TN_FASTA)) return 0u;
    return ((m.nl << 1) | (ls_in & 1u)) & m.gt & 0xffffu;
}

// The entries of a lane: `at` = offset of the lane's first byte from the source's base, `kept_before` = kept bytes of T in
// front of the lane, `index` = table index of the lane's first open.  keep: the lane's keep mask (header bytes are not
// kept, so the kept bytes below an open are those in front of it).  Returns the number of entries written.
APM_TN_FN uint32_t apm_sq_emit(apm_seq *table, uint64_t index, uint32_t opens, uint32_t keep, uint64_t at, uint32_t lead, uint64_t kept_before) {
    uint32_t n = 0u;
    for (uint32_t left = opens; left; left &= left - 1u, ++n) {
        const uint32_t i = (uint32_t)__builtin_ctz(left);
        table[index + n].hdr_off = at + i - lead;
        table[index + n].t_begin = kept_before + (uint32_t)__builtin_popcount(keep & ((1u << i) - 1u));
    }
    return n;
}

// ---- the search: the largest i in [0, n_seq) with hdr_off[i] < pos, entry 0 (no header) standing for "none" ----
// Throughout pred(lo) holds and pred(hi) does not (hi == n_seq: the sentinel); a round probes lo + lane * step in every
// lane, the lanes that hold are the lowest n_ok ones (hdr_off is strictly increasing from entry 1 on; lane 0 always holds).
APM_TN_FN uint64_t apm_sq_step(uint64_t lo, uint64_t hi) { return (hi - lo + 63u) >> 6; }

APM_TN_FN bool apm_sq_probe(const apm_seq *table, uint64_t lo, uint64_t hi, uint32_t lane, uint64_t pos) {
    const uint64_t idx = lo + lane * apm_sq_step(lo, hi);
    return idx < hi && (idx == 0u || table[idx].hdr_off < pos);
}

APM_TN_FN void apm_sq_narrow(uint64_t &lo, uint64_t &hi, uint32_t n_ok) {
    const uint64_t step = apm_sq_step(lo, hi);
    lo += (uint64_t)(n_ok - 1u) * step;
    hi = hi < lo + step ? hi : lo + step;
}

// ---- a location ----
APM_TN_FN apm_loc apm_sq_invalid() {
    apm_loc l;
    l.off = 0u;
    l.seq = APM_SEQ_INVALID;
    l.flags = 0u;
    return l;
}

// c = index in T of the record's byte (c < total = |T|), m = its pattern's length, t_begin / t_next = those of its sequence
// and of the entry behind it
APM_TN_FN apm_loc apm_sq_location(uint64_t c, uint32_t m, uint64_t total, uint32_t seq, uint64_t t_begin, uint64_t t_next) {
    apm_loc l;
    const uint64_t left = total - c, size = left < m ? left : m;
    l.off = c - t_begin;
    l.seq = seq;
    l.flags = (c + size - 1u >= t_next ? APM_LOC_SPANS : 0u) | (size < m ? APM_LOC_TRUNCATED : 0u);
    return l;
}

// where a source offset lies in its block: chunk, lane, byte of the lane
struct ApmSqAt { uint64_t block; uint32_t chunk, lane, bit; };

APM_TN_FN ApmSqAt apm_sq_at(uint64_t pos, uint32_t lead) {
    ApmSqAt a;
    const uint64_t x = pos + lead;
    a.block = x / APM_TN_BLOCK;
    const uint32_t q = (uint32_t)(x % APM_TN_BLOCK);
    a.chunk = q / APM_TN_CHUNK;
    a.lane = (q % APM_TN_CHUNK) / 16u;
    a.bit = q % 16u;
    return a;
}

#define APM_SQ_SCAN_THREADS 1024u
#define APM_SQ_SCAN_CHUNK 4096u /* blocks per round of the scan: four per thread (the counts are allocated in whole chunks) */

#if defined(__HIPCC__)
struct ApmSqIndexArgs {
    ApmTnSrc src;
    const unsigned long long *map;   // the normalisation's map (apm_tn_map_entry), n_blocks + 1 entries
    uint32_t *count;                 // header opens per block, allocated in whole scan chunks
    unsigned long long *prefix;      // opens in front of every block, n_blocks + 1 entries (the last = the total)
    unsigned long long *total;       // the total once more, for the host
    apm_seq *table;                  // emit: n_seq + 1 entries
    unsigned long long n_seq;        // emit: 1 + the total
    unsigned long long src_len, kept; // the sentinel
};

struct ApmSqLocateArgs {
    ApmTnSrc src;
    const unsigned long long *map;
    const uint4 *rec;                  // apm_match records, only read
    unsigned long long cap;
    const unsigned long long *n_rec;
    const apm_seq *table;
    unsigned long long n_seq;
    const uint2 *pat;                  // {row offset, m} per pattern (the score pass's table)
    uint32_t n_patterns;
    unsigned long long src_len, kept;
    apm_loc *loc;
};

/* apm_seqindex.hip */
hipError_t apm_launch_sq_count(const ApmSqIndexArgs &a, int n_cu, hipStream_t s);
hipError_t apm_launch_sq_scan(const ApmSqIndexArgs &a, hipStream_t s);
hipError_t apm_launch_sq_emit(const ApmSqIndexArgs &a, int n_cu, hipStream_t s);
hipError_t apm_launch_sq_locate(const ApmSqLocateArgs &a, int n_cu, hipStream_t s);
#endif

#endif /* APM_SEQINDEX_H */
