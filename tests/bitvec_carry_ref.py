"""A big-integer model of the Myers / Hyyro column of csrc/apm_core.h, a census of the carries of its one addition, and the
pattern families and texts that drive those carries through the column's words (tests/test_bitpar_carry_chains.py).

The kernels advance a column with (Eq & Pv) + Pv.  How the carry of that addition travels depends on the form: an
add-with-carry chain over 32-bit words (bp_step, bp_step_seq), or two ballots and a scalar add over the lanes of a wave
(apm_bitlong_kernel: 32 rows per lane up to 2048 bytes, 64 beyond).  The model does the addition on Python ints, so it has
no words and no carry handling of its own: it is a second reference of the distance, independent of oracle/, and the
census says what a B-bit form would have had to do in every column -- the proof that an input reaches the propagate path.

Rows: bit y - 1 is pattern row y.  The column is held in L * B bits, L = ceil(m / B): the rows above m in the top word
have Eq = 0 and start with Pv = 1, exactly as in the kernels, which never mask them (they cannot influence the rows
below); the distance reads the m pattern rows only."""
import random
import struct

DNA = b"ACGT"
FOREIGN = b"\x00N"          # text-only bytes: no pattern contains them
FAMILIES = ("runs", "dna+run", "head+run")


def word_bits(m):
    """B of the form that runs a pattern of m bytes: 32-bit words, 64 rows per lane beyond 2048 bytes"""
    return 64 if m > 2048 else 32


def walk(pattern, window, B):
    """(distance, census) of one window: the global distance cell(len(window), len(pattern)) of the recurrence at the top
    of apm_core.h, and census = (columns with a run >= 1, >= 2, >= 8, longest run over the window), a run being
    consecutive words of one column that each receive a carry and pass it on because their own sum is all ones."""
    m = len(pattern)
    L = (m + B - 1) // B
    bits = L * B
    full, low = (1 << bits) - 1, (1 << m) - 1
    word_full = (1 << B) - 1
    fmt = "<%d%s" % (L, "I" if B == 32 else "Q")
    nbytes = bits // 8
    peq = {}
    for y, c in enumerate(pattern):
        peq[c] = peq.get(c, 0) | (1 << y)
    pv, mv = full, 0
    ge1 = ge2 = ge8 = longest = 0
    for c in window:
        eq = peq.get(c, 0)
        t = eq & pv
        # ---- census: the same addition, word by word
        tw = struct.unpack(fmt, t.to_bytes(nbytes, "little"))
        pw = struct.unpack(fmt, pv.to_bytes(nbytes, "little"))
        sums = [a + b for a, b in zip(tw, pw)]
        if word_full in sums:          # (no all-ones word: nothing can propagate)
            carry, run, best = 0, 0, 0
            for s in sums:
                if carry and s == word_full:
                    run += 1           # receives a carry, passes it on (s + 1 overflows); s itself generated none
                    if run > best:
                        best = run
                else:
                    run = 0
                    carry = (s + carry) >> B
            ge1 += best >= 1
            ge2 += best >= 2
            ge8 += best >= 8
            if best > longest:
                longest = best
        # ---- the column step on the whole column at once
        xh = (((t + pv) ^ pv) | eq) & full
        ph = (mv | ~(xh | pv)) & full
        mh = pv & xh
        phs = ((ph << 1) | 1) & full   # row 0's horizontal delta is +1
        mhs = (mh << 1) & full
        xv = eq | mv
        pv = (mhs | ~(xv | phs)) & full
        mv = phs & xv
    dist = len(window) + bin(pv & low).count("1") - bin(mv & low).count("1")
    return dist, (ge1, ge2, ge8, longest)


def walk_losing_propagated_carries(pattern, window, B):
    """the distance a B-bit form would report if a word took its carry-out from its own sum alone, i.e. generated carries
    arrive next door but never pass a word whose sum is all ones (the P ballot of the wave form forced to 0).  It tells
    which inputs DECIDE on that path: a case can only catch such a fault where this differs from walk()."""
    m = len(pattern)
    L = (m + B - 1) // B
    full, low, word_full = (1 << (L * B)) - 1, (1 << m) - 1, (1 << B) - 1
    peq = {}
    for y, c in enumerate(pattern):
        peq[c] = peq.get(c, 0) | (1 << y)
    pv, mv = full, 0
    for c in window:
        eq = peq.get(c, 0)
        t = eq & pv
        s = carry = 0
        for w in range(L):
            s0 = ((t >> (w * B)) & word_full) + ((pv >> (w * B)) & word_full)
            s |= ((s0 + carry) & word_full) << (w * B)
            carry = s0 >> B
        xh = ((s ^ pv) | eq) & full
        ph = (mv | ~(xh | pv)) & full
        mh = pv & xh
        phs = ((ph << 1) | 1) & full
        mhs = (mh << 1) & full
        xv = eq | mv
        pv = (mhs | ~(xv | phs)) & full
        mv = phs & xv
    return len(window) + bin(pv & low).count("1") - bin(mv & low).count("1")


# ---------------------------------------------------------------- the families
def dna(rnd, n):
    return bytes(rnd.choices(DNA, k=n))


def family_pattern(family, m, B, seed):
    rnd = random.Random("%s/%d/%d" % (family, m, seed))
    if family == "runs":           # A, C, G, T in turn; the run borders drift across the word borders
        out = bytearray()
        i = 0
        while len(out) < m:
            out += DNA[i % 4:i % 4 + 1] * (3 * B + (i % 3) - 1)
            i += 1
        return bytes(out[:m])
    if family == "dna+run":        # a carry generated in random rows crosses a quarter of the column
        return dna(rnd, m // 4) + b"A" * (m // 2) + dna(rnd, m - m // 4 - m // 2)
    if family == "head+run":       # a carry generated in word 0 crosses every other word
        return dna(rnd, min(B, m)) + b"A" * max(0, m - B)
    raise ValueError(family)


def condition(family, m, B):
    """((least longest run, exact?), (census index, least columns)) of a family at a length, None below the lengths of
    the table: the two components every planted full window has to meet"""
    L = (m + B - 1) // B
    if family == "head+run" and m >= 33:
        return (L - 1, True), (0, 15)
    if family == "runs" and m >= 257:
        return (5, False), (1, (m + 1) // 2)
    if family == "dna+run" and m >= 256:
        return ((L + 3) // 4, False), (1, (m + 7) // 8)
    return None


def meets(family, m, B, census):
    cond = condition(family, m, B)
    if cond is None:
        return True
    (run, exact), (idx, cols) = cond
    return (census[3] == run if exact else census[3] >= run) and census[idx] >= cols


def other_letter(rnd, c):
    return rnd.choice([x for x in DNA if x != c])


def planted_windows(rnd, pat, k):
    """[(kind, bytes)]: the full windows planted per pattern, each of len(pat) bytes"""
    m = len(pat)
    out = [("exact", pat)]
    w = bytearray(pat)
    for pos in rnd.sample(range(m), min(k, 4)):
        w[pos] = other_letter(rnd, w[pos])
    out.append(("subst", bytes(w)))
    front, back = min(7, m // 4), m - 1 - min(7, m // 4)
    w = bytearray(pat)
    del w[front]
    w.insert(back, other_letter(rnd, pat[back]))
    out.append(("del+ins", bytes(w)))
    w = bytearray(pat)
    w.insert(front, other_letter(rnd, pat[front]))
    del w[back + 1]
    out.append(("ins+del", bytes(w)))
    out.append(("rotated", pat[1:] + pat[:1]))
    assert all(len(x) == m for _, x in out)
    return out


class Planted:
    """text, and where what lies in it: full = [(kind, offset)] of the planted full windows of `pat`, stretch = offset
    of pattern + pattern, cut = offset of the occurrence that the end of the text cuts"""


def build_text(pat, k, seed):
    """3 m + 3000 bytes of random DNA with the two foreign bytes, and between them the plants of one pattern: five full
    windows, pattern + pattern, and at the very end the pattern's first 2 m / 3 bytes (the plants alone are 7 2/3 m
    bytes, so the text is that much longer than its filler)"""
    m = len(pat)
    rnd = random.Random("text/%d/%d/%d" % (m, k, seed))
    wins = planted_windows(rnd, pat, k)
    pieces = [w for _, w in wins] + [pat + pat, pat[:max(k + 2, 2 * m // 3)]]
    gap = (3 * m + 3000) // len(pieces)
    first = 3 * m + 3000 - gap * (len(pieces) - 1)
    text = bytearray()
    offsets = []
    for i, piece in enumerate(pieces):
        text += bytes(rnd.choices(DNA * 4 + FOREIGN, k=first if i == 0 else gap))
        offsets.append(len(text))
        text += piece
    r = Planted()
    r.text = bytes(text)
    r.pat = pat
    r.full = [(kind, o) for (kind, _), o in zip(wins, offsets)] + [("stretch+0", offsets[-2]), ("stretch+m", offsets[-2] + m)]
    r.stretch = offsets[-2]
    r.cut = offsets[-1]
    assert len(r.text) == 3 * m + 3000 + sum(len(p) for p in pieces) and r.cut + len(pieces[-1]) == len(r.text)
    return r
