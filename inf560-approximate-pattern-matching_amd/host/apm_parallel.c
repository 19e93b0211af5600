/*
 * apm_parallel -- command-line host of the MI355X engine, plain C over the C ABI
 * (include/apm.h); no HIP headers, no MPI, no OpenMP.
 *
 * Keeps the reference's process contract:
 *   apm_parallel <distance> <text_file> <pattern_1> ... <pattern_P>
 *                [DB_OVER_RANKS|PATTERNS_OVER_RANKS] [--gpus N] [--kernel NAME] [--positions] [--distances] [--alignments]
 *                [--fasta] [--upper] [--sequences] [--best[=R]] [--occurrences[=all|best]] [--occurrence-scripts[=all|best]]
 *                [--nearest] [--nearest-per-sequence] [--occurrences-per-sequence[=all|best]]
 *                [--occurrence-scripts-per-sequence[=all|best]]
 *   --occurrences-per-sequence[=all|best] (needs --fasta; --upper is allowed with it): the occurrence search with every
 *   sequence of the file a text of its own (include/apm.h: "occurrence search per sequence") -- no occurrence crosses a
 *   header, and none that would can hide one inside a sequence.  The "Number of matches" lines of --occurrences, then per
 *   pattern "Occurrences for pattern <p>: NAME:off-len:dist ..." -- NAME as --sequences prints it, off the residue offset of
 *   the occurrence's first byte inside the sequence, len its residues.  --occurrence-scripts-per-sequence[=all|best]: the same
 *   with every occurrence's edit script, NAME:off-len:dist:SCRIPT.  Both are refused together with --positions, --distances,
 *   --alignments, --best, --occurrences, --occurrence-scripts, --nearest, --nearest-per-sequence and --sequences.
 *   --nearest-per-sequence (needs --fasta; --upper is allowed with it): every pattern's nearest occurrence in EVERY sequence of
 *   the file (include/apm.h: "nearest occurrences per sequence"; no occurrence crosses a header), whatever the distance
 *   argument says (parsed and ignored).  Per pattern, then per sequence in file order, one line
 *   "Nearest occurrence of pattern <p> in <NAME>: off-len:dist" -- NAME as --sequences prints it, off the residue offset of the
 *   occurrence's first byte inside the sequence, len its residues -- or "... in <NAME>: none".  Sequence 0, the bytes in
 *   front of the first header, is listed only when it has bytes.  Refused together with everything --nearest is refused
 *   with, and with --nearest itself.
 *   --nearest: every pattern's nearest occurrence in the text, whatever the distance argument says (it is parsed and ignored;
 *   include/apm.h: "nearest occurrences") -- one line "Nearest occurrence of pattern <p>: start-end:dist" per pattern, the
 *   first end of the smallest distance and its shortest span, or "none" where the pattern shares no byte with the text; with
 *   --fasta / --upper offsets in the file.  No "Number of matches" lines.  Patterns of at most 128 bytes.  Refused together with
 *   --positions, --distances, --alignments, --best, --occurrences, --occurrence-scripts and --sequences.
 *   --occurrences[=all|best]: the occurrence search instead of the window scan (include/apm.h: "occurrence search") -- for
 *   every text position the smallest distance between the whole pattern and a substring that ENDS there.  best (the
 *   default): the first end of every local minimum within the distance; all: every end within it.  The "Number of matches"
 *   lines then count occurrences, and a line "Occurrences for pattern <p>: start-end:dist ..." follows per pattern (offsets
 *   of the occurrence's first and last byte; with --fasta / --upper offsets in the file; with --sequences NAME:off-len:dist,
 *   located by the start, an occurrence that runs into a later sequence left out).  Patterns of at most 128 bytes, distance
 *   < pattern length.  It cannot be combined with --positions, --distances, --alignments or --best.
 *   --occurrence-scripts[=all|best] (implies --occurrences, same modes): every occurrence with its edit script (include/apm.h:
 *   "occurrence scripts"), start-end:dist:SCRIPT -- the whole pattern against the bytes start..end, in the run-length letters
 *   of --alignments, e.g. 1700-1722:2:11=1D7=1X4= -- and with --fasta --sequences NAME:off-len:dist:SCRIPT.  Refused together
 *   with --positions, --distances, --alignments and --best, as --occurrences is.
 *   --best[=R] (implies --distances): of every run of neighbouring offsets one occurrence leaves behind, only the best hit
 *   at radius R is printed (include/apm.h: "best hits"; R <= 64, default max(1, distance)), in the formats the other flags
 *   define; the "Number of matches" lines stay the reference's contract and are NOT thinned.
 *   --sequences (with --fasta; implies --positions): every match is printed as NAME:off -- the sequence it lies in (the
 *   bytes behind the '>' of its header up to the first blank; "-" in front of the first header) and the residue offset inside
 *   it, line breaks not counted -- then :dist and :SCRIPT as before.  Matches whose window runs into a later sequence or is
 *   the truncated tail window at the end of the text are left out of that list; the "Number of matches" lines stay the
 *   reference's contract and are NOT adjusted for them.
 *   argv grammar + usage line        /root/reference/src/sequential.c:35-77
 *   optional trailing approach flag  /root/reference/src/main.c:66-86 (accepted, ignored:
 *                                    the text is always sharded over the GPUs)
 *   banner  "Approximate Pattern Mathing: ..." (sic)   src/sequential.c:79-82,
 *                                                       src/database_over_ranks.c:97-100
 *   timing  "APM done in %lf s"                         src/sequential.c:151
 *   result  "Number of matches for pattern <%s>: %d"    src/sequential.c:157-160
 *   errors on stderr, exit code 1                       src/utils.c:20-23, src/sequential.c:65-68
 * Replaces the MPI/OpenMP dispatch of src/main.c, src/patterns_over_ranks.c and
 * src/database_over_ranks.c with one process driving all GPUs of the node.
 * Counts are printed as 64-bit values (identical text whenever they fit an int).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <unistd.h>

#include "apm.h"

static int kernel_by_name(const char *s) {
    if (!strcmp(s, "auto")) return APM_KERNEL_AUTO;
    if (!strcmp(s, "generic")) return APM_KERNEL_GENERIC;
    if (!strcmp(s, "wavefront")) return APM_KERNEL_WAVEFRONT;
    if (!strcmp(s, "bitpar")) return APM_KERNEL_BITPAR;
    if (!strcmp(s, "banded")) return APM_KERNEL_BANDED;
    if (!strcmp(s, "nfa")) return APM_KERNEL_NFA;
    return -1;
}

/* --sequences: the locations of the records and the sequence table behind them (*seqs: malloc'ed, the caller frees) */
static int sequences_of(apm_ctx *ctx, const apm_match *rec, uint64_t n_rec, apm_loc *loc, apm_seq **seqs) {
    uint64_t n_seq = 0;
    int rc = apm_locate_buffer(ctx, rec, n_rec, loc);
    if (rc == APM_OK) rc = apm_get_sequences(ctx, NULL, 0, &n_seq);
    if (rc != APM_OK) return rc;
    *seqs = (apm_seq *)malloc((size_t)(n_seq + 1) * sizeof(apm_seq));
    if (!*seqs) return APM_ERR_NOMEM;
    return apm_get_sequences(ctx, *seqs, n_seq + 1, &n_seq);
}

/* the name of the sequence whose header opens at hdr_off of the mapped file: the bytes behind the '>' up to the first blank
   or line end; "-" for the bytes in front of the first header */
static void print_name(const uint8_t *buf, uint64_t n, uint64_t hdr_off) {
    if (hdr_off == APM_SEQ_NO_HEADER) {
        printf("-");
        return;
    }
    uint64_t e = hdr_off + 1;
    while (e < n && buf[e] != ' ' && buf[e] != '\t' && buf[e] != '\r' && buf[e] != '\n') ++e;
    fwrite(buf + hdr_off + 1, 1, (size_t)(e - hdr_off - 1), stdout);
}

/* a row of ops as runs of equal ops: <length><letter> */
static void print_script(const uint32_t *row) {
    for (uint32_t j = 0, run = 0; j < row[0]; ++j) {
        const unsigned op = (row[1 + j / 16] >> (2 * (j % 16))) & 3u;
        ++run;
        if (j + 1 == row[0] || ((row[1 + (j + 1) / 16] >> (2 * ((j + 1) % 16))) & 3u) != op) {
            printf("%u%c", (unsigned)run, "=XID"[op]);
            run = 0;
        }
    }
}

/* the whole text file mapped read-only (an empty file: *buf = NULL, *n = 0); 0, or 1 with the reference's message */
static int map_text_file(const char *filename, uint8_t **buf, uint64_t *n) {
    *buf = NULL;
    *n = 0;
    const int fd = open(filename, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0) {
        fprintf(stderr, "Unable to open the text file <%s>\n", filename);
        if (fd >= 0) close(fd);
        return 1;
    }
    if (st.st_size > 0) {
        void *mp = mmap(NULL, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (mp == MAP_FAILED) {
            fprintf(stderr, "Unable to map the text file <%s>\n", filename);
            close(fd);
            return 1;
        }
        *buf = (uint8_t *)mp;
        *n = (uint64_t)st.st_size;
    }
    close(fd);
    return 0;
}

/* --occurrences: one apm_find_occ_buffer call over the mapped file, a second one if the first buffer was too small;
   want_scripts (--occurrence-scripts): apm_find_occ_align_buffer in its place, the same sizing, a row of ops per record;
   per_seq (--occurrences-per-sequence, --occurrence-scripts-per-sequence): apm_find_occ_seq_buffer in place of both, listed
   as with --sequences */
static int run_occurrences(apm_ctx *ctx, const char *filename, char **pats, int nb_patterns, unsigned flags, int want_sequences, int want_scripts,
                           int per_seq) {
    uint8_t *buf = NULL;
    uint64_t n = 0;
    if (map_text_file(filename, &buf, &n)) return 1;
    int status = 1;
    uint64_t cap = (uint64_t)1 << 16, found = 0;
    uint64_t *counts = (uint64_t *)calloc((size_t)nb_patterns, sizeof(uint64_t));
    apm_match *end = NULL, *start = NULL;
    uint32_t *ops = NULL;
    const int row_words = want_scripts ? apm_occ_align_row_words(ctx) : 0;
    if (row_words < 0) {
        fprintf(stderr, "%s\n", apm_last_error(ctx));
        free(counts);
        if (buf) munmap(buf, (size_t)n);
        return 1;
    }
    const uint32_t stride = (uint32_t)row_words;
    apm_loc *loc = NULL;
    apm_seq *seqs = NULL;
    struct timeval t1, t2;
    gettimeofday(&t1, NULL);
    for (int pass = 0; pass < 2 && counts; ++pass) {
        free(end);
        free(start);
        free(ops);
        end = (apm_match *)malloc((size_t)cap * sizeof(apm_match));
        start = (apm_match *)malloc((size_t)cap * sizeof(apm_match));
        ops = want_scripts ? (uint32_t *)malloc((size_t)cap * stride * sizeof(uint32_t)) : NULL;
        if (!end || !start || (want_scripts && !ops)) {
            fprintf(stderr, "Unable to allocate %llu occurrence records\n", (unsigned long long)cap);
            goto done;
        }
        if ((per_seq        ? apm_find_occ_seq_buffer(ctx, buf, n, flags, end, start, NULL, cap, &found, counts, ops, stride)
             : want_scripts ? apm_find_occ_align_buffer(ctx, buf, n, flags, end, start, cap, &found, counts, ops, stride)
                            : apm_find_occ_buffer(ctx, buf, n, flags, end, start, cap, &found, counts)) != APM_OK) {
            fprintf(stderr, "%s\n", apm_last_error(ctx));
            goto done;
        }
        if (found <= cap) break;
        cap = found;
    }
    if (!counts || found > cap) goto done;
    gettimeofday(&t2, NULL);
    printf("APM done in %lf s\n", (double)(t2.tv_sec - t1.tv_sec) + (double)(t2.tv_usec - t1.tv_usec) / 1e6);
    for (int i = 0; i < nb_patterns; ++i) printf("Number of matches for pattern <%s>: %llu\n", pats[i], (unsigned long long)counts[i]);
    if (per_seq) want_sequences = 1;
    if (want_sequences) { /* the locations of starts [0, found) and of ends [found, 2 found) */
        apm_match *both = (apm_match *)malloc((size_t)(found ? 2 * found : 1) * sizeof(apm_match));
        loc = (apm_loc *)malloc((size_t)(found ? 2 * found : 1) * sizeof(apm_loc));
        if (!both || !loc) {
            fprintf(stderr, "Unable to allocate %llu occurrence records\n", (unsigned long long)(2 * found));
            free(both);
            goto done;
        }
        memcpy(both, start, (size_t)found * sizeof(apm_match));
        memcpy(both + found, end, (size_t)found * sizeof(apm_match));
        const int rc = sequences_of(ctx, both, 2 * found, loc, &seqs);
        free(both);
        if (rc != APM_OK) {
            fprintf(stderr, "%s\n", apm_last_error(ctx));
            goto done;
        }
    }
    uint64_t q = 0; /* the records come sorted by (pattern, end) */
    for (int i = 0; i < nb_patterns; ++i) {
        printf("Occurrences for pattern <%s>:", pats[i]);
        for (; q < found && end[q].pattern == (uint32_t)i; ++q) {
            if (start[q].pos == APM_OCC_NO_START) continue;
            if (want_sequences) {
                const apm_loc *ls = &loc[q], *le = &loc[found + q];
                if (ls->seq == APM_SEQ_INVALID || le->seq != ls->seq) continue; /* runs into a later sequence */
                printf(" ");
                print_name(buf, n, seqs[ls->seq].hdr_off);
                printf(":%llu-%llu:%u", (unsigned long long)ls->off, (unsigned long long)(le->off - ls->off + 1), (unsigned)end[q].reserved);
            } else {
                printf(" %llu-%llu:%u", (unsigned long long)start[q].pos, (unsigned long long)end[q].pos, (unsigned)end[q].reserved);
            }
            if (want_scripts) {
                printf(":");
                print_script(ops + q * stride);
            }
        }
        printf("\n");
    }
    status = 0;
done:
    free(counts);
    free(end);
    free(start);
    free(ops);
    free(loc);
    free(seqs);
    if (buf) munmap(buf, (size_t)n);
    return status;
}

/* --nearest: one apm_find_nearest_buffer call over the mapped file; a line per pattern, start-end:dist or none */
static int run_nearest(apm_ctx *ctx, const char *filename, char **pats, int nb_patterns) {
    uint8_t *buf = NULL;
    uint64_t n = 0;
    if (map_text_file(filename, &buf, &n)) return 1;
    int status = 1;
    apm_match *end = (apm_match *)malloc((size_t)nb_patterns * sizeof(apm_match));
    apm_match *start = (apm_match *)malloc((size_t)nb_patterns * sizeof(apm_match));
    struct timeval t1, t2;
    gettimeofday(&t1, NULL);
    if (!end || !start) {
        fprintf(stderr, "Unable to allocate %d nearest-occurrence records\n", nb_patterns);
    } else if (apm_find_nearest_buffer(ctx, buf, n, end, start) != APM_OK) {
        fprintf(stderr, "%s\n", apm_last_error(ctx));
    } else {
        gettimeofday(&t2, NULL);
        printf("APM done in %lf s\n", (double)(t2.tv_sec - t1.tv_sec) + (double)(t2.tv_usec - t1.tv_usec) / 1e6);
        for (int i = 0; i < nb_patterns; ++i) {
            if (end[i].pos == APM_OCC_NO_START || start[i].pos == APM_OCC_NO_START)
                printf("Nearest occurrence of pattern <%s>: none\n", pats[i]);
            else
                printf("Nearest occurrence of pattern <%s>: %llu-%llu:%u\n", pats[i], (unsigned long long)start[i].pos, (unsigned long long)end[i].pos,
                       (unsigned)end[i].reserved);
        }
        status = 0;
    }
    free(end);
    free(start);
    if (buf) munmap(buf, (size_t)n);
    return status;
}

/* --nearest-per-sequence: one apm_find_nearest_seq_buffer call over the mapped file, a second one if the first arrays held
   too few sequences; the starts and the ends located (apm_locate_buffer); a line per (pattern, sequence) */
static int run_nearest_per_sequence(apm_ctx *ctx, const char *filename, char **pats, int nb_patterns) {
    uint8_t *buf = NULL;
    uint64_t n = 0;
    if (map_text_file(filename, &buf, &n)) return 1;
    int status = 1;
    const uint64_t P = (uint64_t)nb_patterns;
    uint64_t cap = 1024, n_seq = 0;
    apm_match *both = NULL; /* the starts [0, rows) and the ends [rows, 2 rows) */
    apm_loc *loc = NULL;
    apm_seq *seqs = NULL;
    struct timeval t1, t2;
    gettimeofday(&t1, NULL);
    for (int pass = 0; pass < 2; ++pass) {
        free(both);
        both = (apm_match *)malloc((size_t)(2 * cap * P) * sizeof(apm_match));
        if (!both) {
            fprintf(stderr, "Unable to allocate %llu nearest-occurrence records\n", (unsigned long long)(2 * cap * P));
            goto done;
        }
        const int rc = apm_find_nearest_seq_buffer(ctx, buf, n, both + cap * P, both, cap, &n_seq);
        if (rc == APM_OK) break;
        if (rc != APM_ERR_INVALID || n_seq <= cap || pass) {
            fprintf(stderr, "%s\n", apm_last_error(ctx));
            goto done;
        }
        cap = n_seq;
    }
    gettimeofday(&t2, NULL);
    {
        const uint64_t rows = n_seq * P;
        memmove(both + rows, both + cap * P, (size_t)rows * sizeof(apm_match)); /* (the ends right behind the starts) */
        loc = (apm_loc *)malloc((size_t)(2 * rows) * sizeof(apm_loc));
        if (!loc) {
            fprintf(stderr, "Unable to allocate %llu locations\n", (unsigned long long)(2 * rows));
            goto done;
        }
        if (sequences_of(ctx, both, 2 * rows, loc, &seqs) != APM_OK) {
            fprintf(stderr, "%s\n", apm_last_error(ctx));
            goto done;
        }
        printf("APM done in %lf s\n", (double)(t2.tv_sec - t1.tv_sec) + (double)(t2.tv_usec - t1.tv_usec) / 1e6);
        for (int i = 0; i < nb_patterns; ++i)
            for (uint64_t s = 0; s < n_seq; ++s) {
                if (s == 0 && seqs[1].t_begin == seqs[0].t_begin) continue; /* nothing in front of the first header */
                const uint64_t r = s * P + (uint64_t)i;
                const apm_loc *ls = &loc[r], *le = &loc[rows + r];
                printf("Nearest occurrence of pattern <%s> in <", pats[i]);
                print_name(buf, n, seqs[s].hdr_off);
                if (both[r].pos == APM_OCC_NO_START || both[rows + r].pos == APM_OCC_NO_START || ls->seq != (uint32_t)s || le->seq != (uint32_t)s)
                    printf(">: none\n");
                else
                    printf(">: %llu-%llu:%u\n", (unsigned long long)ls->off, (unsigned long long)(le->off - ls->off + 1), (unsigned)both[rows + r].reserved);
            }
        status = 0;
    }
done:
    free(both);
    free(loc);
    free(seqs);
    if (buf) munmap(buf, (size_t)n);
    return status;
}

/* --NAME or --NAME=all|best: 1 and *flags set if `arg` is that option, 0 if it is another one, -1 (reported) on a bad MODE */
static int occ_mode_option(const char *arg, const char *name, unsigned *flags) {
    const size_t len = strlen(name);
    if (strncmp(arg, name, len) || (arg[len] && arg[len] != '=')) return 0;
    if (!arg[len]) return 1;
    if (!strcmp(arg + len + 1, "all")) *flags = APM_OCC_ALL;
    else if (!strcmp(arg + len + 1, "best")) *flags = APM_OCC_LOCAL_MIN;
    else {
        fprintf(stderr, "%s=MODE: MODE must be all or best, not <%s>\n", name, arg + len + 1);
        return -1;
    }
    return 1;
}

int main(int argc, char **argv) {
    int n_gpus = 0; /* 0 = all visible */
    int kernel = APM_KERNEL_AUTO;
    int verbose = 0;
    int want_positions = 0; /* extension: also print the matching offsets */
    int want_distances = 0; /* --distances (implies --positions): every offset as pos:dist, the match's edit distance */
    int want_alignments = 0; /* --alignments (implies --distances): every offset as pos:dist:SCRIPT, the match's edit script,
                                run-length coded in the letters of include/apm.h: = X I D */
    unsigned text_mode = 0; /* --fasta, --upper: APM_TEXT_* (include/apm.h); the sequence is searched, not the file layout, and
                               the offsets printed are offsets in the file.  One device: without --gpus, --gpus 1 is taken */
    int want_sequences = 0; /* --sequences (needs --fasta, implies --positions): NAME:off instead of the file offset */
    int want_best = 0;      /* --best[=R] (implies --distances): only the best hits at radius R.  One device, as with a text mode */
    long best_radius = -1;  /* < 0: the default, max(1, distance) */
    int want_occ = 0;       /* --occurrences[=all|best]: the occurrence search.  One device, as with a text mode */
    unsigned occ_flags = APM_OCC_LOCAL_MIN;
    int want_occ_scripts = 0; /* --occurrence-scripts[=all|best] (implies --occurrences): start-end:dist:SCRIPT */
    int listing_flags = 0;  /* --positions, --distances, --alignments, --best: what --occurrences cannot be combined with */
    int want_nearest = 0;   /* --nearest: every pattern's nearest occurrence; the distance argument is parsed and ignored.  One device */
    int want_nearest_seq = 0; /* --nearest-per-sequence (needs --fasta): the same per sequence of the file.  One device */
    int want_occ_seq = 0;   /* --occurrences-per-sequence[=all|best] (needs --fasta): the occurrence search per sequence.  One device */
    int want_occ_seq_scripts = 0; /* --occurrence-scripts-per-sequence[=all|best]: and every occurrence's edit script */
    int per_seq_option = 0;
    int status = 0;

    /* strip our own options (anywhere after the pattern list starts is fine:
       the reference has none, so nothing is taken away from its grammar) */
    int w = 1;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--gpus") && i + 1 < argc) {
            n_gpus = atoi(argv[++i]);
        } else if (!strcmp(argv[i], "--kernel") && i + 1 < argc) {
            kernel = kernel_by_name(argv[++i]);
            if (kernel < 0) {
                fprintf(stderr, "Unknown kernel variant <%s>\n", argv[i]);
                return 1;
            }
        } else if (!strcmp(argv[i], "--verbose")) {
            verbose = 1;
        } else if (!strcmp(argv[i], "--positions")) {
            want_positions = listing_flags = 1;
        } else if (!strcmp(argv[i], "--distances")) {
            want_positions = want_distances = listing_flags = 1;
        } else if (!strcmp(argv[i], "--alignments")) {
            want_positions = want_distances = want_alignments = listing_flags = 1;
        } else if ((per_seq_option = occ_mode_option(argv[i], "--occurrences-per-sequence", &occ_flags)) != 0) {
            if (per_seq_option < 0) return 1;
            want_occ_seq = 1;
        } else if ((per_seq_option = occ_mode_option(argv[i], "--occurrence-scripts-per-sequence", &occ_flags)) != 0) {
            if (per_seq_option < 0) return 1;
            want_occ_seq = want_occ_seq_scripts = 1;
        } else if (!strcmp(argv[i], "--occurrences") || !strncmp(argv[i], "--occurrences=", 14)) {
            want_occ = 1;
            if (argv[i][13] == '=') {
                if (!strcmp(argv[i] + 14, "all")) occ_flags = APM_OCC_ALL;
                else if (!strcmp(argv[i] + 14, "best")) occ_flags = APM_OCC_LOCAL_MIN;
                else {
                    fprintf(stderr, "--occurrences=MODE: MODE must be all or best, not <%s>\n", argv[i] + 14);
                    return 1;
                }
            }
        } else if (!strcmp(argv[i], "--occurrence-scripts") || !strncmp(argv[i], "--occurrence-scripts=", 21)) {
            want_occ = want_occ_scripts = 1;
            if (argv[i][20] == '=') {
                if (!strcmp(argv[i] + 21, "all")) occ_flags = APM_OCC_ALL;
                else if (!strcmp(argv[i] + 21, "best")) occ_flags = APM_OCC_LOCAL_MIN;
                else {
                    fprintf(stderr, "--occurrence-scripts=MODE: MODE must be all or best, not <%s>\n", argv[i] + 21);
                    return 1;
                }
            }
        } else if (!strcmp(argv[i], "--nearest")) {
            want_nearest = 1;
        } else if (!strcmp(argv[i], "--nearest-per-sequence")) {
            want_nearest_seq = 1;
        } else if (!strcmp(argv[i], "--fasta")) {
            text_mode |= APM_TEXT_FASTA;
        } else if (!strcmp(argv[i], "--upper")) {
            text_mode |= APM_TEXT_UPPER;
        } else if (!strcmp(argv[i], "--sequences")) {
            want_positions = want_sequences = 1;
        } else if (!strcmp(argv[i], "--best") || !strncmp(argv[i], "--best=", 7)) {
            want_positions = want_distances = want_best = listing_flags = 1;
            if (argv[i][6] == '=') {
                char *end = NULL;
                best_radius = strtol(argv[i] + 7, &end, 10);
                if (argv[i][7] < '0' || argv[i][7] > '9' || *end || best_radius > APM_BEST_MAX_RADIUS) {
                    fprintf(stderr, "--best=R: R must be a number from 0 to %d, not <%s>\n", APM_BEST_MAX_RADIUS, argv[i] + 7);
                    return 1;
                }
            }
        } else {
            argv[w++] = argv[i];
        }
    }
    argc = w;
    if (want_occ && listing_flags) {
        fprintf(stderr, "%s cannot be combined with --positions, --distances, --alignments or --best: it lists start-end:dist%s itself\n",
                want_occ_scripts ? "--occurrence-scripts" : "--occurrences", want_occ_scripts ? ":SCRIPT" : "");
        return 1;
    }
    if (want_nearest && (listing_flags || want_occ || want_sequences)) {
        fprintf(stderr, "--nearest cannot be combined with --positions, --distances, --alignments, --best, --occurrences, --occurrence-scripts or "
                        "--sequences: it lists one start-end:dist per pattern itself\n");
        return 1;
    }
    if (want_nearest_seq && (listing_flags || want_occ || want_sequences || want_nearest)) {
        fprintf(stderr, "--nearest-per-sequence cannot be combined with --positions, --distances, --alignments, --best, --occurrences, "
                        "--occurrence-scripts, --sequences or --nearest: it lists one off-len:dist per pattern and sequence itself\n");
        return 1;
    }
    if (want_nearest_seq && !(text_mode & APM_TEXT_FASTA)) {
        fprintf(stderr, "--nearest-per-sequence needs --fasta: sequences are what FASTA headers open\n");
        return 1;
    }
    if (want_occ_seq && (listing_flags || want_occ || want_sequences || want_nearest || want_nearest_seq)) {
        fprintf(stderr, "%s cannot be combined with --positions, --distances, --alignments, --best, --occurrences, --occurrence-scripts, "
                        "--nearest, --nearest-per-sequence or --sequences: it lists NAME:off-len:dist%s itself\n",
                want_occ_seq_scripts ? "--occurrence-scripts-per-sequence" : "--occurrences-per-sequence", want_occ_seq_scripts ? ":SCRIPT" : "");
        return 1;
    }
    if (want_occ_seq && !(text_mode & APM_TEXT_FASTA)) {
        fprintf(stderr, "%s needs --fasta: sequences are what FASTA headers open\n",
                want_occ_seq_scripts ? "--occurrence-scripts-per-sequence" : "--occurrences-per-sequence");
        return 1;
    }
    if (want_sequences && !(text_mode & APM_TEXT_FASTA)) {
        fprintf(stderr, "--sequences needs --fasta: sequences are what FASTA headers open\n");
        return 1;
    }

    /* trailing approach flag of the reference's apm_parallel (src/main.c:66-86) */
    int partition = APM_PARTITION_TEXT; /* DB_OVER_RANKS, and the default: the text is sharded over the devices */
    if (argc >= 2 && (!strcmp(argv[argc - 1], "DB_OVER_RANKS") || !strcmp(argv[argc - 1], "PATTERNS_OVER_RANKS"))) {
        if (!strcmp(argv[argc - 1], "PATTERNS_OVER_RANKS")) partition = APM_PARTITION_PATTERNS; /* the pattern list is (with --gpus > 1) */
        argc -= 1;
    }

    if (argc < 4) {
        printf("Usage: %s approximation_factor dna_database pattern1 pattern2 ...\n", argv[0]);
        return 1;
    }

    const int approx_factor = atoi(argv[1]);
    if (best_radius < 0) best_radius = approx_factor > 1 ? approx_factor : 1;
    if (best_radius > APM_BEST_MAX_RADIUS) best_radius = APM_BEST_MAX_RADIUS;
    const char *filename = argv[2];
    const int nb_patterns = argc - 3;

    int *len = (int *)malloc((size_t)nb_patterns * sizeof(int));
    uint64_t *n_matches = (uint64_t *)malloc((size_t)nb_patterns * sizeof(uint64_t));
    if (!len || !n_matches) {
        fprintf(stderr, "Unable to allocate array of pattern of size %d\n", nb_patterns);
        return 1;
    }
    for (int i = 0; i < nb_patterns; ++i) {
        len[i] = (int)strlen(argv[i + 3]);
        if (len[i] <= 0) {
            fprintf(stderr, "Error while parsing argument %d\n", i + 3);
            return 1;
        }
    }

    printf("Approximate Pattern Mathing: looking for %d pattern(s) in file %s w/ distance of %d\n",
           nb_patterns, filename, approx_factor);
    fflush(stdout);

    /* the reference opens the file before anything else can fail (src/sequential.c:84) */
    FILE *probe = fopen(filename, "rb");
    if (!probe) {
        fprintf(stderr, "Unable to open the text file <%s>\n", filename);
        return 1;
    }
    fclose(probe);

    apm_ctx *ctx = NULL;
    int rc = apm_create(&ctx, (text_mode || want_best || want_occ || want_nearest) && n_gpus == 0 ? 1 : n_gpus); /* (all four are single-device) */
    if (rc != APM_OK) {
        fprintf(stderr, "apm_parallel: %s\n", apm_last_error(NULL));
        return 1;
    }
    if ((rc = apm_set_partition(ctx, partition)) != APM_OK) {
        fprintf(stderr, "apm_parallel: %s\n", apm_last_error(ctx));
        apm_destroy(ctx);
        return 1;
    }
    if (kernel != APM_KERNEL_AUTO && (rc = apm_set_kernel(ctx, kernel)) != APM_OK) {
        fprintf(stderr, "apm_parallel: %s\n", apm_last_error(ctx));
        apm_destroy(ctx);
        return 1;
    }
    rc = apm_set_patterns(ctx, nb_patterns, (const char *const *)(argv + 3), len, approx_factor);
    if (rc != APM_OK) {
        fprintf(stderr, "apm_parallel: %s\n", apm_last_error(ctx));
        apm_destroy(ctx);
        return 1;
    }
    if (text_mode && (rc = apm_set_text_mode(ctx, text_mode)) != APM_OK) {
        fprintf(stderr, "apm_parallel: %s\n", apm_last_error(ctx));
        apm_destroy(ctx);
        return 1;
    }

    if (want_occ || want_nearest || want_nearest_seq || want_occ_seq) { /* the occurrence searches stand in for the window scan: their own counts, their own listing */
        status = want_nearest_seq ? run_nearest_per_sequence(ctx, filename, argv + 3, nb_patterns)
                 : want_nearest   ? run_nearest(ctx, filename, argv + 3, nb_patterns)
                 : want_occ_seq   ? run_occurrences(ctx, filename, argv + 3, nb_patterns, occ_flags, 1, want_occ_seq_scripts, 1)
                              : run_occurrences(ctx, filename, argv + 3, nb_patterns, occ_flags, want_sequences, want_occ_scripts, 0);
        apm_destroy(ctx);
        free(len);
        free(n_matches);
        return status;
    }

    struct timeval t1, t2;
    gettimeofday(&t1, NULL);
    rc = apm_count_file(ctx, filename, n_matches);
    gettimeofday(&t2, NULL);
    if (rc != APM_OK) {
        fprintf(stderr, "%s\n", apm_last_error(ctx));
        apm_destroy(ctx);
        return 1;
    }
    const double duration = (double)(t2.tv_sec - t1.tv_sec) + (double)(t2.tv_usec - t1.tv_usec) / 1e6;
    printf("APM done in %lf s\n", duration);

    if (verbose) {
        apm_timing tm;
        if (apm_get_timing(ctx, &tm) == APM_OK)
            fprintf(stderr,
                    "[apm] devices=%d launches=%d h2d=%.3f ms kernels=%.3f ms reduce=%.3f ms total=%.3f ms "
                    "windows=%llu algorithmic_cells=%.4g (%.4g cells/s)\n",
                    tm.n_devices, tm.n_launches, tm.h2d_ms, tm.kernel_ms, tm.reduce_ms, tm.total_ms,
                    (unsigned long long)tm.windows, tm.cells_algorithmic,
                    tm.total_ms > 0 ? tm.cells_algorithmic / (tm.total_ms * 1e-3) : 0.0);
    }

    for (int i = 0; i < nb_patterns; ++i)
        printf("Number of matches for pattern <%s>: %llu\n", argv[i + 3], (unsigned long long)n_matches[i]);

    if (want_positions) { /* off by default: stdout stays identical to the reference */
        /* the text is mapped, not read a second time into a heap buffer */
        uint8_t *buf = NULL;
        uint64_t n = 0;
        const int fd = open(filename, O_RDONLY);
        struct stat st;
        if (fd >= 0 && fstat(fd, &st) == 0 && st.st_size > 0) {
            void *mp = mmap(NULL, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (mp != MAP_FAILED) {
                buf = (uint8_t *)mp;
                n = (uint64_t)st.st_size;
            }
        }
        if (fd >= 0) close(fd);
        if (!buf && fd >= 0 && st.st_size > 0) {
            fprintf(stderr, "Unable to map the text file for the positions pass\n");
            apm_destroy(ctx);
            return 1;
        }
        const uint64_t pcap = (uint64_t)1 << 20;
        /* ONE apm_find_all_buffer call over the mapped file, sized from the counts above: the text is uploaded and
           scanned once for all patterns, by the kernels that counted.  The per-pattern loop below is the fallback only:
           a pattern with more than 2^20 matches (it prints its first 2^20 positions and " ..."), or a record buffer
           beyond 1 GiB (16 bytes per match, once on the host and once per device). */
        const int row_words = want_alignments ? apm_align_row_words(ctx) : 0; /* (< 0: the find call below reports it) */
        const uint32_t stride = row_words > 0 ? (uint32_t)row_words : 2;
        const uint64_t rec_budget = ((uint64_t)1 << 30) / (sizeof(apm_match) + (want_alignments ? 4 * (size_t)stride : 0));
        uint64_t total = 0;
        int one_pass = 1;
        for (int i = 0; i < nb_patterns; ++i) {
            if (n_matches[i] > pcap) one_pass = 0;
            total += n_matches[i];
        }
        if (total > rec_budget) one_pass = 0;
        if (one_pass) {
            apm_match *rec = (apm_match *)malloc((size_t)(total ? total : 1) * sizeof(apm_match));
            uint32_t *ops = want_alignments ? (uint32_t *)malloc((size_t)(total ? total : 1) * stride * sizeof(uint32_t)) : NULL;
            uint64_t found = 0, n_best = 0;
            apm_loc *loc = want_sequences ? (apm_loc *)malloc((size_t)(total ? total : 1) * sizeof(apm_loc)) : NULL;
            apm_seq *seqs = NULL; /* --sequences: the table, for the names */
            if (!rec || (want_alignments && !ops) || (want_sequences && !loc)) {
                fprintf(stderr, "Unable to allocate %llu match records\n", (unsigned long long)total);
            } else if ((want_best ? apm_find_best_buffer(ctx, buf, n, (uint32_t)best_radius, rec, total, &n_best, &found, ops, stride)
                        : want_alignments ? apm_find_all_align_buffer(ctx, buf, n, rec, total, &found, ops, stride)
                        : want_distances ? apm_find_all_dist_buffer(ctx, buf, n, rec, total, &found)
                                       : apm_find_all_buffer(ctx, buf, n, rec, total, &found)) != APM_OK) {
                fprintf(stderr, "%s\n", apm_last_error(ctx));
                if (want_best) status = 1;
            } else if (want_sequences && sequences_of(ctx, rec, want_best ? n_best : (found < total ? found : total), loc, &seqs) != APM_OK) {
                fprintf(stderr, "%s\n", apm_last_error(ctx));
                status = 1;
            } else {
                uint64_t q = 0; /* the records come sorted by (pattern, pos) */
                const uint64_t have = want_best ? n_best : (found < total ? found : total); /* (n_best <= found <= total) */
                for (int i = 0; i < nb_patterns; ++i) {
                    printf("Positions for pattern <%s>:", argv[i + 3]);
                    for (; q < have && rec[q].pattern == (uint32_t)i; ++q) {
                        if (want_sequences) {
                            if (loc[q].seq == APM_SEQ_INVALID || loc[q].flags) continue; /* spans two sequences, or the truncated tail */
                            printf(" ");
                            print_name(buf, n, seqs[loc[q].seq].hdr_off);
                            printf(":%llu", (unsigned long long)loc[q].off);
                            if (want_distances) printf(":%u", (unsigned)rec[q].reserved);
                        } else if (want_distances) printf(" %llu:%u", (unsigned long long)rec[q].pos, (unsigned)rec[q].reserved);
                        else printf(" %llu", (unsigned long long)rec[q].pos);
                        if (want_alignments) { /* runs of equal ops: <length><letter> */
                            printf(":");
                            print_script(ops + q * stride);
                        }
                    }
                    printf("\n");
                }
            }
            free(rec);
            free(ops);
            free(loc);
            free(seqs);
        }
        if (!one_pass && want_sequences) { /* (as the text modes: the per-pattern call serves neither) */
            fprintf(stderr, "--sequences: too many matches for the one-pass record buffer\n");
            if (buf) munmap(buf, (size_t)n);
            apm_destroy(ctx);
            return 1;
        }
        if (!one_pass && want_best)
            fprintf(stderr, "--best: too many matches for the one-pass record buffer, falling back to --distances\n");
        if (!one_pass && want_distances)
            fprintf(stderr, "--distances: too many matches for the one-pass record buffer, printing bare positions\n");
        uint64_t *pos = one_pass ? NULL : (uint64_t *)malloc((size_t)pcap * sizeof(uint64_t));
        for (int i = 0; pos && i < nb_patterns; ++i) {
            uint64_t found = 0;
            if (apm_find_buffer(ctx, buf, n, i, pos, pcap, &found) != APM_OK) {
                fprintf(stderr, "%s\n", apm_last_error(ctx));
                if (text_mode) status = 1; /* (the per-pattern call does not serve a text mode) */
                break;
            }
            printf("Positions for pattern <%s>:", argv[i + 3]);
            for (uint64_t q = 0; q < found && q < pcap; ++q) printf(" %llu", (unsigned long long)pos[q]);
            printf(found > pcap ? " ...\n" : "\n");
        }
        free(pos);
        if (buf) munmap(buf, (size_t)n);
    }

    apm_destroy(ctx);
    free(len);
    free(n_matches);
    return status;
}
