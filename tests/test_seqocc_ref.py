"""CPU: tests/seqocc_ref.py on the example that motivates the per-sequence occurrence search -- GATTACA across the boundary
of two sequences: the whole-text search reports the crossing occurrence and hides the real one -- and against a literal
full-table DP on random tables with empty and 1-byte sequences, both flags."""
import random

import occ_ref as O
import seqocc_ref as R

P = b"GATTACA"
S0, S1 = b"CCCCCCCCCCGA", b"TTACACCCCCCCC"
T = S0 + S1
BEGINS = [0, len(S0), len(T)]


def test_the_gattaca_example():
    assert len(T) == 25
    # k = 2, LOCAL_MIN: the whole text reports the crossing occurrence, the per-sequence search the real hit TTACA
    assert O.records_with_starts(T, [P], 2, O.LOCAL_MIN) == [(0, 16, 0, 10)]
    assert R.records_with_starts(T, [P], 2, R.LOCAL_MIN, BEGINS) == [(0, 16, 2, 12, 1)]
    # k = 2, ALL
    assert [e for _, e, _ in O.records(T, [P], 2, O.ALL)] == [14, 15, 16, 17, 18]
    assert R.records(T, [P], 2, R.ALL, BEGINS) == [(0, 16, 2)]
    # k = 1
    assert len(O.records(T, [P], 1, O.ALL)) == 3
    assert R.records(T, [P], 1, R.ALL, BEGINS) == [] and R.records(T, [P], 1, R.LOCAL_MIN, BEGINS) == []


def test_one_sequence_is_the_whole_text_search():
    rng = random.Random(3)
    text = bytes(rng.choice(b"ACGT") for _ in range(150))
    pats = [b"ACGTA", b"GGTTGGTTAC", b"AC"]
    for flags in (R.ALL, R.LOCAL_MIN):
        assert R.records(text, pats, 1, flags, [0, len(text)]) == O.records(text, pats, 1, flags)
        assert [r[:4] for r in R.records_with_starts(text, pats, 1, flags, [0, len(text)])] == O.records_with_starts(text, pats, 1, flags)


def test_records_equal_the_literal_definition():
    rng = random.Random(5)
    for n in (1, 7, 40, 90):
        text = bytes(rng.choice(b"AC") for _ in range(n))
        pats = [b"A", b"AC", b"ACCAA", b"CCACCAACAC"]
        tables = [R.begins_of([rng.randrange(n + 1) for _ in range(rng.randrange(0, 9))] * 2, n) for _ in range(4)]
        tables += [R.begins_of(range(1, n), n), [0, 0, 0, n, n]]
        for begins in tables:
            for k in (0, 1, 3):
                served = [p for p in pats if k < len(p)]
                for flags in (R.ALL, R.LOCAL_MIN):
                    got = R.records(text, served, k, flags, begins)
                    for i, p in enumerate(served):
                        assert [(e, d) for j, e, d in got if j == i] == R.literal(text, p, k, flags, begins), (n, begins, k, flags, p)


def test_spans_stay_inside_their_sequence():
    rng = random.Random(8)
    text = bytes(rng.choice(b"AC") for _ in range(120))
    begins = [0, 30, 30, 77, 78, 120]
    pats = [b"ACCA", b"CCCCCC"]
    for flags in (R.ALL, R.LOCAL_MIN):
        rows = R.records_with_starts(text, pats, 2, flags, begins)
        assert rows
        for i, e, d, start, s in rows:
            assert begins[s] <= start <= e < begins[s + 1] and begins[s] < begins[s + 1]
            assert O.global_dist(pats[i], text[start:e + 1]) == d
    # ends of a range: the two halves make the whole
    full = R.records(text, pats, 2, R.LOCAL_MIN, begins)
    for cut in (1, 30, 31, 77, 78, 100):
        assert sorted(R.records(text, pats, 2, R.LOCAL_MIN, begins, 0, cut) + R.records(text, pats, 2, R.LOCAL_MIN, begins, cut, None)) == full
