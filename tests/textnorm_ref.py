"""The text modes of include/apm.h (APM_TEXT_FASTA, APM_TEXT_UPPER) as a byte-serial state machine: the reference the
normalisation pass is pinned to, and the layouts its tests share."""
import random

FASTA, UPPER = 1, 2
BLOCK = 4096


def normalize(src, flags):
    """(T, src_of): the kept bytes in order, and src_of[c] = offset in src of T[c]"""
    out, src_of = bytearray(), []
    line_start, in_header = True, False
    for i, b in enumerate(src):
        keep = True
        if flags & FASTA:
            if line_start and b == 0x3E:
                in_header = True
            if in_header or b in (0x0A, 0x0D):
                keep = False
            if b == 0x0A:
                in_header = False
        line_start = b == 0x0A
        if keep:
            out.append(b - 32 if flags & UPPER and 0x61 <= b <= 0x7A else b)
            src_of.append(i)
    return bytes(out), src_of


def dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def fasta(rng, n_seq, cols=50, header=b">seq one\n", eol=b"\n"):
    """a header and n_seq sequence bytes in lines of `cols`"""
    seq = dna(rng, n_seq)
    return header + b"".join(seq[i:i + cols] + eol for i in range(0, n_seq, cols))


def _at(rng, n, patches):
    """n bytes of DNA with the patches {offset: bytes} laid over them"""
    t = bytearray(dna(rng, n))
    for off, p in patches.items():
        t[off:off + len(p)] = p
    return bytes(t[:n])


def layouts(seed=11):
    """name -> source: the layouts where a block-wise pass can go wrong (4 KiB blocks, 16-byte lanes)"""
    rng = random.Random(seed)
    n = 3 * BLOCK + 5
    hdr = lambda k: b">" + b"h" * (k - 2) + b"\n"           # a header of k bytes, its '\n' included
    out = {
        "fasta50_header_at_0": fasta(rng, 3 * BLOCK),
        "header_4090_to_4100": _at(rng, n, {4089: b"\n", 4090: hdr(11)}),
        "header_5000": _at(rng, n, {3999: b"\n", 4000: hdr(5000)}),     # block 1 is entered and left inside it
        "header_9000": _at(rng, n, {2999: b"\n", 3000: hdr(9000)}),
        "nl_ends_block_gt_starts_next": _at(rng, n, {BLOCK - 1: b"\n", BLOCK: b">name\n", 2 * BLOCK - 1: b"\n>x\n"}),
        "gt_starts_block_not_line_start": _at(rng, n, {BLOCK - 1: b"A", BLOCK: b">", 2 * BLOCK - 1: b"\r", 2 * BLOCK: b">"}),
        "crlf": fasta(rng, 2 * BLOCK + 77, cols=60, header=b">crlf\r\n", eol=b"\r\n"),
        "only_newlines": b"\n" * n,
        "no_newline": dna(rng, n),
        "no_newline_header": b">" + dna(rng, n - 1),
        "unterminated_header_at_end": fasta(rng, 2 * BLOCK) + b">tail without an end " + dna(rng, 4200),
        "upper_edges": _at(rng, n, {0: b"`{az\x80\xffAZ@[", 4090: b"acgt`{\x80\xff\xe1\xfaacgt", 8191: b"a", 8192: b"z"}),
        "gt_everywhere": bytes(rng.choice(b">\n>A") for _ in range(n)),
        "lower_stretches": b"".join(dna(rng, 37, b"acgtn") if i % 3 == 1 else dna(rng, 41) for i in range(200)),
    }
    return out


def random_text(rng, n, alphabet=b"ACGTac\n\r>"):
    return bytes(rng.choice(alphabet) for _ in range(n))
