"""The device buffers a context keeps between host-level calls -- the match records and the rows of ops of the find calls,
the raw text and the normalisation map of the text modes, the text itself, the align pass's trace workspace -- through
allocate, grow and reuse: one context makes calls whose sizes go small, large, small, with pattern set changes in
between (they free the score image and the trace workspace with the plan), and every call is checked against the oracle.

The large FASTA sources are a 64 KiB block repeated, plus a tail.  The block ends with a newline outside a header, where
the byte-serial reference (textnorm_ref.normalize) is back in its start state, so the normalised text of block * r + tail
is normalize(block) * r + normalize(tail); the test checks that identity on block + tail and then builds the 1 MiB and
16 MiB references from it instead of running the Python state machine over them."""
import random

import pytest

import helpers as H
import textnorm_ref as R

pytestmark = pytest.mark.gpu

EQ, SUB, INS, DEL = range(4)
BLOCK = 64 << 10
FASTA_SIZES = (2 << 10, (1 << 20) + (4 << 10) + 17, (16 << 20) + (4 << 10) + 5, 2 << 10)   # below / past the 1 MiB pinned-ring threshold / past one 4096-block chunk of the map
CAPACITIES = (64, 4096, 64)


def rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def substituted(rng, p, e):
    w = bytearray(p)
    for at in rng.sample(range(len(w)), e):
        w[at] = rng.choice([c for c in b"ACGT" if c != w[at]])
    return bytes(w)


def align_case():
    """64 KiB of DNA with 40 copies of two patterns at exactly k substitutions (no neighbouring window is within k of
    such a copy, so the matches stay below the smallest capacity)"""
    rng = random.Random(808)
    k, pats = 2, [rand(rng, 24), rand(rng, 37)]
    text = bytearray(rand(rng, 64 << 10))
    for q in range(40):
        p = pats[q % 2]
        at = 700 + q * 1600 + q % 16
        text[at:at + len(p)] = substituted(rng, p, k if q % 5 else q % 3)
    return pats, k, bytes(text)


def window(text, p, j):
    size = min(len(p), len(text) - j)
    return p[:size], text[j:j + size]


def apply_script(p, t, ops):
    out, x, y = bytearray(), 0, 0
    for op in ops:
        if op == EQ:
            assert p[y] == t[x]
        if op != DEL:
            out.append(t[x])
        x += op != DEL
        y += op != INS
    assert y == len(p) and x == len(t)
    return bytes(out), sum(1 for op in ops if op != EQ)


def fasta_block(rng, pat):
    """BLOCK bytes: headers, lines of 60 in both cases with a few 'n', copies of the pattern (lower case, one substitution
    in every other one) that the line ends cut; the last byte is the newline of a sequence line"""
    out = bytearray()
    while len(out) < BLOCK - 200:
        out += b">seq %d of the block\n" % len(out)
        seq = bytearray(rand(rng, rng.randrange(900, 4000), b"ACGTacgtn"))
        for q in range(len(seq) // 700):
            at = 50 + q * 700 + rng.randrange(60)
            seq[at:at + len(pat)] = substituted(rng, pat, q % 2).lower()
        for i in range(0, len(seq), 60):
            out += seq[i:i + 60] + (b"\r\n" if rng.random() < 0.05 else b"\n")
    out = out[:BLOCK - 200]
    if out[-1:] != b"\n":
        out += b"\n"
    out += b">the last one\n"
    out += rand(rng, BLOCK - 1 - len(out)) + b"\n"
    assert len(out) == BLOCK
    return bytes(out)


def fasta_cases():
    """[(source, normalised text)] of FASTA_SIZES"""
    rng = random.Random(909)
    pat = rand(rng, 12)
    block = fasta_block(rng, pat)
    t_block = R.normalize(block, R.FASTA | R.UPPER)[0]
    cases = []
    for n in FASTA_SIZES:
        r, rest = divmod(n, BLOCK)
        tail = block[:rest]
        t_tail = R.normalize(tail, R.FASTA | R.UPPER)[0]
        if r == 0:
            assert R.normalize(block + tail, R.FASTA | R.UPPER)[0] == t_block + t_tail       # the identity the large ones are built on
        cases.append((block * r + tail, t_block * r + t_tail))
        assert len(cases[-1][0]) == n and len(cases[-1][1]) < n - n // 50
    return pat, cases


def align_sequence(ctx, pats, k, text, want):
    ctx.set_text_mode(0)
    ctx.set_patterns(pats, k)
    for cap in CAPACITIES:
        got, total = ctx.find_all_align_buffer(text, cap)
        assert total == len(want) <= cap, cap
        assert [(i, j) for i, j, _, _ in got] == want, cap
        for i, j, dist, ops in got:
            p, t = window(text, pats[i], j)
            assert dist == H.window_distance(p, t) <= k, (cap, i, j)
            assert apply_script(p, t, ops) == (t, dist), (cap, i, j)


def fasta_sequence(apm, ctx, pat, cases, want, fresh):
    ctx.set_patterns([pat], 1)
    ctx.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
    for (src, _), w in zip(cases, want):
        assert ctx.count_buffer(src) == [w], len(src)
        assert ctx.stat("norm_src_bytes") == len(src)
        if fresh:
            with apm.ApmContext(device=0) as other:
                other.set_patterns([pat], 1)
                other.set_text_mode(apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)
                assert other.count_buffer(src) == [w], len(src)


def test_buffers_grow_behind_the_stream_and_are_reused():
    apm = H.pkg()
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    pats, k, text = align_case()
    want_rec = [(i, j) for i, p in enumerate(pats) for j in H.oracle_positions(text, p, k)]
    assert 40 <= len(want_rec) <= min(CAPACITIES)
    pat, cases = fasta_cases()
    want_counts = [H.oracle_counts(t, [pat], 1, banded=True)[0] for _, t in cases]
    assert all(w >= 2 for w in want_counts) and want_counts[2] > want_counts[1] > want_counts[0]
    with apm.ApmContext(device=0) as ctx:
        align_sequence(ctx, pats, k, text, want_rec)
        fasta_sequence(apm, ctx, pat, cases, want_counts, fresh=True)
        # once more behind the pattern set changes: every buffer is there and large enough, the score image and the trace
        # workspace went with the plan
        align_sequence(ctx, pats, k, text, want_rec)
        fasta_sequence(apm, ctx, pat, cases, want_counts, fresh=False)
