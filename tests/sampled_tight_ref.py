"""Planter and census for the sampled filter kernels (pure Python, no GPU).

The BANDED path is exact by the pigeonhole argument: a window within k edits keeps one of its k+1 pieces intact,
shifted by at most B = k // 2.  Its sampled forms look at every KL-th text position only (KL = 16 for pieces of
>= 31 bytes, else 8), which is enough because an intact piece of >= 2*KL-1 bytes contains a KL-aligned block -- for a
piece of exactly 15 or 31 bytes standing at s = 1 (mod KL) ONE such block, r = KL-1, and nothing else finds the window.

A TIGHT plant (q, dl, rot) is a window of exactly m bytes in which piece q stands intact at offset a_q + dl and every
other piece carries exactly one edit (k edits in all): the |dl| pieces nearest to q on one side take an insertion, the
|dl| nearest on the other side a deletion (which side follows the sign of dl), the rest a substitution.  Only
|dl| <= min(q, k-q) can be had that way.  With no edits at all the same planter gives an exact occurrence.

build(family) lays such plants into random filler:
  residue  every valid (q, dl) with the intact piece's text start s at every residue 0..15 (mod 16),
  seam     s = 4096*c - x for every x in [0, longest piece + 16): piece and aligned block walk over a 4 KiB seam,
  ends     window starts 0 (q = 0) and n - m (q = k), n no multiple of 16,
  exact    one exact occurrence per residue of its start.
The seam plants stand one per 4 KiB block; the other sections fill the room between them.
"""
import random

import helpers as H

DNA = b"ACGT"
PROSE = b"etaoin shrdlucETAOIN\n.,"   # 2-bit codes collide: the register compare is a filter there, not a decision

# (alphabet name, m, k)
STREAM16 = [("dna", 31, 0), ("dna", 62, 1), ("dna", 64, 1), ("dna", 93, 2), ("dna", 248, 7)]     # class (16,16): pieces >= 31
STREAM8 = [("dna", 15, 0), ("dna", 16, 0), ("dna", 30, 1)]                                        # class (8,8): pieces 15..30
SIEVE8 = [("dna", 45, 2), ("dna", 47, 2), ("dna", 64, 3), ("dna", 75, 4), ("dna", 90, 5), ("dna", 105, 6), ("dna", 120, 7)]
COLLIDING = [("prose", 30, 1), ("prose", 64, 3)]
FAMILIES = STREAM16 + STREAM8 + SIEVE8 + COLLIDING
ALPHABETS = {"dna": DNA, "prose": PROSE}
# family -> seed where the default one leaves the census' conditions little room (a pattern whose pieces hold runs of
# equal letters: sole-nominator shares 0.805 and 0.818 against the 0.8 asked for)
SEEDS = {("dna", 45, 2): "sampled-tight dna 45 2 #2", ("dna", 105, 6): "sampled-tight dna 105 6 #1"}
GAP = 64                              # filler bytes between plants, at least


def family_id(fam):
    return "%s-%d-%d" % fam


def piece_offsets(m, k):
    """a_0 .. a_k and m, as apm_plan.cpp cuts the pieces"""
    return [q * m // (k + 1) for q in range(k + 2)]


def valid_shifts(k):
    return [(q, dl) for q in range(k + 1) for dl in range(-min(q, k - q), min(q, k - q) + 1)]


def key_len(m, k):
    return 16 if m // (k + 1) >= 31 else 8


def _places(L):
    return (0, 1, L // 2, L - 2, L - 1)


def _other(alphabet, avoid, turn):
    """a letter of the alphabet that is none of `avoid`, rotating with `turn`"""
    cands = [c for c in alphabet if c not in avoid]
    return cands[turn % len(cands)]


def plant_window(P, k, q, dl, rot, alphabet, edits=True):
    """the m bytes of the plant (q, dl, rot) for pattern P; edits=False: P itself"""
    m = len(P)
    if not edits:
        return bytes(P)
    assert abs(dl) <= min(q, k - q)
    a = piece_offsets(m, k)
    out = bytearray()
    for i in range(k + 1):
        piece = bytearray(P[a[i]:a[i + 1]])
        L = len(piece)
        if i == q:
            assert len(out) == a[q] + dl
            out += piece
            continue
        before = i < q
        near = abs(i - q) <= abs(dl)
        if near and ((dl > 0) == before):
            kind = "ins"
        elif near:
            kind = "del"
        else:
            kind = "sub"
        turn = (rot + i) % 5
        at = _places(L)[turn]
        if kind == "sub":
            piece[at] = _other(alphabet, (piece[at],), rot + i)
        elif kind == "ins":
            at = max(at, 1)           # in front of byte 0 the piece would stay intact, merely shifted
            piece.insert(at, _other(alphabet, (piece[at], piece[at - 1]), rot + i))
        else:
            # inside a run of equal letters a deletion is the deletion of any of them, and the neighbouring edit may
            # then pair up with it: take the first place of the rotation whose byte differs from both neighbours
            for step in range(5):
                c = _places(L)[(turn + step) % 5]
                if (c == 0 or piece[c - 1] != piece[c]) and (c == L - 1 or piece[c + 1] != piece[c]):
                    at = c
                    break
            del piece[at]
        out += piece
    assert len(out) == m
    return bytes(out)


def nominators(P, k, W):
    """the (piece, shift) pairs, |shift| <= k // 2, whose piece stands intact at a_piece + shift in the window W"""
    m = len(P)
    a = piece_offsets(m, k)
    B = k // 2
    out = []
    for q in range(k + 1):
        piece = P[a[q]:a[q + 1]]
        for d in range(-B, B + 1):
            o = a[q] + d
            if o >= 0 and o + len(piece) <= m and W[o:o + len(piece)] == piece:
                out.append((q, d))
    return out


class Family:
    """pattern, text and plants of one (alphabet, m, k); plants: dicts of section, q, dl, rot, j (window start), s (text
    start of the intact piece; of the window for the exact section), x (seam section)"""


def _filler(rng, n, alphabet):
    table = bytes(alphabet[b % len(alphabet)] for b in range(256))
    return bytearray(rng.randbytes(n).translate(table))


def build(fam):
    name, m, k = fam
    alphabet = ALPHABETS[name]
    rng = random.Random(SEEDS.get(fam, "sampled-tight %s %d %d" % fam))
    F = Family()
    F.fam, F.alphabet, F.m, F.k = fam, alphabet, m, k
    F.P = bytes(_filler(rng, m, alphabet))
    a = piece_offsets(m, k)
    lens = [a[q + 1] - a[q] for q in range(k + 1)]
    V = valid_shifts(k)
    plants = []
    rot = [0]

    def add(section, q, dl, j, exact=False, x=None):
        plants.append(dict(section=section, q=q, dl=dl, rot=rot[0], j=j, s=j if exact else j + a[q] + dl, x=x, exact=exact))
        rot[0] += 1

    # seam section first: its places are fixed
    n_seam = max(lens) + 16
    for x in range(n_seam):
        q, dl = V[x % len(V)]
        s = 4096 * (x + 1) - x
        add("seam", q, dl, s - a[q] - dl, x=x)
    reserved = sorted((p["j"] - GAP, p["j"] + m + GAP) for p in plants)
    add("ends", 0, 0, 0)
    cursor = [m + GAP]

    def place(residue, lead):
        """the next free window start j >= cursor with j + lead = residue (mod 16)"""
        j = cursor[0]
        while True:
            j += (residue - (j + lead)) % 16
            hit = next((r for r in reserved if j < r[1] and j + m > r[0]), None)
            if hit is None:
                cursor[0] = j + m + GAP
                return j
            j = hit[1]

    for q, dl in V:
        for residue in range(16):
            add("residue", q, dl, place(residue, a[q] + dl))
    for residue in range(16):
        add("exact", 0, 0, place(residue, 0), exact=True)
    end = max(cursor[0], reserved[-1][1])
    n = end + m
    n += (11 - n) % 16                # the last piece's last aligned 8-byte block lies in the final partial 16 bytes
    add("ends", k, 0, n - m)
    text = _filler(rng, n, alphabet)
    for p in plants:
        W = plant_window(F.P, k, p["q"], p["dl"], p["rot"], alphabet, edits=not p["exact"])
        text[p["j"]:p["j"] + m] = W
    F.text = bytes(text)
    F.n = n
    F.plants = plants
    return F


_families = {}


def family(fam):
    """build(fam), once per process"""
    if fam not in _families:
        _families[fam] = build(fam)
    return _families[fam]


def census(F):
    """per plant (q, dl, s mod 16, s mod 4096, distance, nominators)"""
    if not hasattr(F, "_census"):
        out = []
        for p in F.plants:
            W = F.text[p["j"]:p["j"] + F.m]
            out.append((p["q"], p["dl"], p["s"] % 16, p["s"] % 4096, H.window_distance(F.P, W), nominators(F.P, F.k, W)))
        F._census = out
    return F._census


def plant_name(F, p):
    """(family, q, dl, s mod 16, s mod 4096): what a failure message names a plant by"""
    return (family_id(F.fam), p["q"], p["dl"], p["s"] % 16, p["s"] % 4096)


def expected_positions(F):
    """the matching window starts, sorted: full DP (H.window_distance) over the windows within +-k of each plant, and over
    the windows the end of the text truncates (j > n - m, which match a prefix of the pattern as the reference's scan
    has it; with k edits allowed the shortest of them nearly always do)"""
    if not hasattr(F, "_expected"):
        n, m, k = F.n, F.m, F.k
        zone = set(range(n - m + 1, n - k))
        for p in F.plants:
            zone.update(range(max(0, p["j"] - k), min(n - k, p["j"] + k + 1)))
        out = []
        for j in sorted(zone):
            size = min(m, n - j)
            if H.window_distance(F.P[:size], F.text[j:j + size]) <= k:
                out.append(j)
        F._expected = out
    return F._expected


def plant_near(F, j):
    """the plant whose window start lies nearest to j"""
    return min(F.plants, key=lambda p: abs(p["j"] - j))
