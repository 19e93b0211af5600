"""CPU: tests/seqnear_ref.py against a brute-force literal DP on tiny cases -- every (sequence, pattern) pair of small
texts with random tables, empty and 1-byte sequences; a pattern planted across a boundary belongs to neither side; the ends
[lo, hi) of a shard; source offsets on the sequence index's example."""
import random

import nearest_ref as N
import seqindex_ref as SQ
import seqnear_ref as R


def _check(text, pats, begins):
    ends, starts = R.records(text, pats, begins)
    ks = R.keys(text, pats, begins)
    P = len(pats)
    assert len(ends) == len(starts) == len(ks) == (len(begins) - 1) * P
    for s in range(len(begins) - 1):
        for i, p in enumerate(pats):
            w = R.literal(text, p, begins[s], begins[s + 1])
            r = s * P + i
            if w is None:
                assert ends[r] == starts[r] == (R.NO_START, i, len(p)) and ks[r] == R.NONE, (s, i)
            else:
                assert ends[r] == (w[1], i, w[0]) and starts[r] == (w[2], i, w[0]) and ks[r] == N.key(w[0], w[1]), (s, i, w, ends[r], starts[r])
                assert begins[s] <= w[2] <= w[1] < begins[s + 1]


def test_records_equal_the_literal_definition():
    rng = random.Random(5)
    for n in (1, 7, 40, 90):
        text = bytes(rng.choice(b"ACGT") for _ in range(n))
        pats = [b"A", b"AC", b"ACGTA", b"GGTTGGTTAC", b"ZZ"]
        for trial in range(4):
            cuts = [rng.randrange(n + 1) for _ in range(rng.randrange(0, 9))]
            cuts += cuts[:2]  # empties
            _check(text, pats, R.begins_of(cuts, n))
        _check(text, pats, R.begins_of(range(1, n), n))  # 1-byte sequences
        _check(text, pats, [0, 0, 0, n, n])


def test_a_pattern_across_a_boundary_belongs_to_neither_side():
    p = b"ACGTTGCA"
    text = b"TTTTTTTT" + p + b"TTTTTTTT"
    whole = N.nearest(text, p)
    assert whole[0] == 0
    begins = [0, 12, len(text)]
    ends, _ = R.records(text, [p], begins)
    assert all(0 < r[2] < len(p) for r in ends), ends
    _check(text, [p], begins)
    assert R.keys(text, [p], begins) != N.keys(text, [p]) * 2


def test_a_range_of_ends_and_an_offset():
    rng = random.Random(9)
    text = bytes(rng.choice(b"AC") for _ in range(120))
    pats = [b"ACCA", b"CCCCCC"]
    begins = [0, 30, 30, 77, 120]
    full = R.keys(text, pats, begins)
    for cut in (1, 30, 31, 76, 77, 100):
        a, b = R.keys(text, pats, begins, 0, cut), R.keys(text, pats, begins, cut, None)
        assert [min(x, y) for x, y in zip(a, b)] == full, cut
    off = 1 << 33
    assert R.keys(text, pats, begins, off=off) == [k if k == R.NONE else k + off for k in full]
    e0, s0 = R.records(text, pats, begins)
    e1, s1 = R.records(text, pats, begins, off=off)
    assert [(p if p == R.NO_START else p + off, i, d) for p, i, d in e0] == e1 and [(p if p == R.NO_START else p + off, i, d) for p, i, d in s0] == s1


def test_source_offsets_on_the_index_example():
    src = SQ.EXAMPLE  # T = "AC" | "ACGTAC" | "" | "GGTT"
    n_seq, ends, starts = R.source_records(src, 1, [b"ACGT", b"GG"])
    assert n_seq == 4
    assert ends[0] == (1, 0, 2) and starts[0] == (0, 0, 2)          # "AC" of sequence 0: two deletions
    assert ends[2] == (13, 0, 0) and starts[2] == (10, 0, 0)        # "ACGT" in sequence 1, source offsets 10..13
    assert ends[4] == starts[4] == (R.NO_START, 0, 4)               # the empty sequence
    assert ends[7] == (32, 1, 0) and starts[7] == (31, 1, 0)        # "GG" behind ">three\r\n"
    assert ends[1] == starts[1] == (R.NO_START, 1, 2)               # no G in "AC"
