"""CPU: the big-integer column model of bitvec_carry_ref.py against the oracle, and the gap it was written for --
random DNA never makes the column's carry pass through a word whose sum is all ones, so before
test_bitpar_carry_chains.py no test ran the propagate path of any bit-vector kernel."""
import random

import pytest

import bitvec_carry_ref as R
import helpers as H


def test_model_equals_oracle_on_the_golden_window_pairs():
    pairs = H.window_distance_pairs()
    assert max(len(p) for p, _ in pairs) == 140 and min(len(p) for p, _ in pairs) == 1
    for p, t in pairs:
        want = H.window_distance(p, t)
        assert R.walk(p, t, 32)[0] == want and R.walk(p, t, 64)[0] == want, (p, t)


FAMILY_LENGTHS = (33, 96, 129, 257, 300, 513, 769, 1025, 1100)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_model_equals_oracle_on_family_pairs(family):
    """every planted full window of the family's text at nine lengths up to 1100 (7 windows each), a truncated pair,
    and the pattern against a pattern of another family: 3 x 9 x 9 pairs; the words may be 32 or 64 bits wide, the
    distance is the same"""
    for m in FAMILY_LENGTHS:
        k = 9 if m <= 512 else 12
        pat = R.family_pattern(family, m, 32, 0)
        pl = R.build_text(pat, k, 0)
        pairs = [(pat, pl.text[o:o + m]) for _, o in pl.full]
        size = len(pl.text) - pl.cut
        pairs.append((pat[:size], pl.text[pl.cut:]))
        pairs.append((pat, R.family_pattern(R.FAMILIES[(R.FAMILIES.index(family) + 1) % 3], m, 32, 1)))
        for p, t in pairs:
            want = H.window_distance(p, t)
            assert R.walk(p, t, 32)[0] == want and R.walk(p, t, 64)[0] == want, (family, m)
        assert all(R.walk(p, t, 32)[0] <= 4 for p, t in pairs[:-1])          # (the plants are near matches)


@pytest.mark.parametrize("m", [300, 1024])
def test_random_dna_never_propagates_a_carry(m):
    """The gap, written down: a random pattern against the exact window, an edited one, a shifted one and a random one
    -- no column in which a carry passes through an all-ones word, at either word width.  (Windows with far more
    substitutions than any test plants, 6 % and more, show a single propagating 32-bit word now and then -- 8 windows in 60
    at m = 300, 62 columns in one of them -- never a 64-bit one, never two words in a row.)"""
    rnd = random.Random(5 * m)
    for _ in range(6):
        pat = R.dna(rnd, m)
        for kind, w in R.planted_windows(rnd, pat, 9) + [("random", R.dna(rnd, m))]:
            for B in (32, 64):
                dist, census = R.walk(pat, w, B)
                assert census == (0, 0, 0, 0), (m, kind, B, census)
                assert dist == H.window_distance(pat, w)


@pytest.mark.parametrize("m,B", [(33, 32), (129, 32), (1025, 32), (2049, 64)])
def test_random_dna_reaches_the_top_word_only(m, B):
    """What the gap is NOT: where the top word holds a single pattern row (m = 32 q + 1, or 64 q + 1 in the 64-bit form)
    that row's Eq bit is 0 for three text bytes in four, the rows above it keep Pv = 1, and the word below generates a
    carry in most columns -- so the top word alone does propagate on random DNA, in hundreds of columns per window
    (measured: 1540 of 2049 at m = 2049, 760 of 1025 at m = 1025; 700 and 355 against a random window).  The carry ends
    there.  What random DNA never shows is a carry passing a word full of pattern rows, or two words in a row."""
    rnd = random.Random(m)
    pat = R.dna(rnd, m)
    for kind, w in R.planted_windows(rnd, pat, 9) + [("random", R.dna(rnd, m))]:
        ge1, ge2, ge8, longest = R.walk(pat, w, B)[1]
        assert ge1 >= m // 8 and (ge2, ge8, longest) == (0, 0, 1), (m, kind)
    cut = pat[:-1]                                            # one row less: the top word is full, and nothing propagates
    assert R.walk(cut, cut, B)[1] == (0, 0, 0, 0)


def census_by_cells(pattern, window, B):
    """the census once more, from the literal DP: the column as cells over L B rows (the rows above m are rows of a
    byte that matches nothing), Pv read off its vertical deltas, and no carry followed -- the carries INTO every bit of
    a + b are (a + b) ^ a ^ b, so word w propagates iff that has bit w B set and the word's own sum is all ones"""
    m = len(pattern)
    L = (m + B - 1) // B
    rows = L * B
    pat = list(pattern) + [None] * (rows - m)
    word = (1 << B) - 1
    peq = {c: sum(1 << y for y in range(m) if pattern[y] == c) for c in set(pattern)}
    col = list(range(rows + 1))
    ge1 = ge2 = ge8 = longest = 0
    for x, c in enumerate(window):
        pv = sum(1 << y for y in range(rows) if col[y + 1] - col[y] == 1)
        t = pv & peq.get(c, 0)
        into = (t + pv) ^ t ^ pv
        best = run = 0
        for w in range(L):
            s = ((t >> (w * B)) & word) + ((pv >> (w * B)) & word)
            run = run + 1 if (into >> (w * B)) & 1 and s == word else 0
            best = max(best, run)
        ge1, ge2, ge8, longest = ge1 + (best >= 1), ge2 + (best >= 2), ge8 + (best >= 8), max(longest, best)
        new = [x + 1]
        for y in range(1, rows + 1):
            new.append(min(col[y] + 1, new[y - 1] + 1, col[y - 1] + (pat[y - 1] != c)))
        col = new
    return col[m], (ge1, ge2, ge8, longest)


def test_census_equals_the_one_read_off_the_literal_dp():
    """walk()'s census against census_by_cells on family windows (where it is not zero: asserted) and on random ones"""
    rnd = random.Random(99)
    seen = 0
    for family in R.FAMILIES:
        for m in (33, 65, 130, 257):
            pat = R.family_pattern(family, m, 32, 0)
            for kind, w in R.planted_windows(rnd, pat, 9)[:2] + [("random", R.dna(rnd, m))]:
                for B in (32, 64):
                    got = R.walk(pat, w, B)
                    assert got == census_by_cells(pat, w, B), (family, m, kind, B)
                    seen += got[1][3] >= 2
    assert seen >= 20


def test_where_a_lost_propagated_carry_changes_the_distance():
    """Reaching the path is not deciding on it.  A carry that passes a whole word joins rows more than B apart, so what it
    changes lies far from the diagonal: on every near-match window the families plant, the column without propagated
    carries (walk_losing_propagated_carries) ends at the same distance.  Shifted against itself by more than a word, the
    `runs` pattern does decide: the distance is twice the shift, and one less without the propagated carries -- the cases
    of test_shifted_runs_where_the_propagated_carry_decides."""
    for family in R.FAMILIES:
        for m in (300, 769):
            pat = R.family_pattern(family, m, 32, 0)
            pl = R.build_text(pat, 12, 0)
            for kind, o in pl.full:
                w = pl.text[o:o + m]
                assert R.walk_losing_propagated_carries(pat, w, 32) == R.walk(pat, w, 32)[0] <= 4, (family, m, kind)
    pat = R.family_pattern("runs", 768, 32, 0)
    two = pat + pat
    for d, lost in ((34, 68), (35, 69), (40, None)):
        w = two[d:d + 768]
        assert R.walk(pat, w, 32)[0] == 2 * d == H.window_distance(pat, w)
        got = R.walk_losing_propagated_carries(pat, w, 32)
        assert got == lost if lost else got < 2 * d
