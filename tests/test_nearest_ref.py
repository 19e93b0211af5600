"""CPU: tests/nearest_ref.py against itself -- the many-pattern form the GPU tests use equals the literal definition
(occ_ref.ends_scores, the first end of the smallest E, occ_ref.span at k := d), on planted and unplanted patterns of mixed
lengths, on a range of ends, and where there is no answer; and the figures the GPU tests' cases rest on."""
import numpy as np

import nearest_ref as N
import occ_ref as R


def test_best_ends_equals_the_literal_definition():
    pats, text = R.planted(5, [1, 2, 7, 31, 33, 64], 3, 1500)
    pats = pats + [b"ZZZZ", b"ACGTTGCAACGTTGCAAC"]
    got = N.best_ends(text, pats)
    for p, g in zip(pats, got):
        w = N.nearest(text, p)
        assert g == (None if w is None else w[:2]), p
    assert got[-2] is None
    for lo, hi in ((0, 100), (700, 900), (1499, 1500), (10, 10)):
        for p, g in zip(pats, N.best_ends(text, pats, lo, hi)):
            E = R.ends_scores(text, p)[lo:hi]
            want = None if not len(E) or E.min() >= len(p) else (int(E.min()), lo + int(np.argmax(E == E.min())))
            assert g == want, (p, lo, hi)
    ends, starts = N.records(text, pats)
    for i, p in enumerate(pats):
        w = N.nearest(text, p)
        assert (ends[i], starts[i]) == (((N.NO_START, i, len(p)),) * 2 if w is None else ((w[1], i, w[0]), (w[2], i, w[0])))
    assert N.records(b"", pats)[0] == [(N.NO_START, i, len(p)) for i, p in enumerate(pats)]


def test_keys_order_like_the_answers():
    assert N.key(3, (1 << 56) - 1) < N.key(4, 0) < N.NONE and N.key(3, 5) < N.key(3, 6)
    k = N.key(127, (1 << 56) - 1)
    assert (N.key_dist(k), N.key_end(k)) == (127, (1 << 56) - 1)


def test_random_dna_exercises_large_distances():
    rs = np.random.RandomState(3)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = a[rs.randint(0, 4, size=20000)].tobytes()
    pats = [a[rs.randint(0, 4, size=m)].tobytes() for m in (16, 64, 128)]
    d = [r[0] for r in N.best_ends(text, pats)]
    assert 2 <= d[0] <= 6 and 18 <= d[1] <= 30 and 45 <= d[2] <= 65, d
