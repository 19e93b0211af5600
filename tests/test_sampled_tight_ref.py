"""The planter of tests/sampled_tight_ref.py really plants what the GPU sweep relies on (CPU only): pigeonhole-tight
windows whose ONLY nominator is the piece, shift and residue they are named by."""
import pytest

import helpers as H
import sampled_tight_ref as T


@pytest.fixture(scope="module", params=T.FAMILIES, ids=T.family_id)
def F(request):
    return T.family(request.param)


def _tight(F):
    return [(p, c) for p, c in zip(F.plants, T.census(F)) if not p["exact"]]


def test_layout(F):
    m, k, n = F.m, F.k, F.n
    assert n % 16 != 0 and 100 * 1024 <= n <= 300 * 1024
    a = T.piece_offsets(m, k)
    spans = sorted((p["j"], p["j"] + m) for p in F.plants)
    assert spans[0][0] == 0 and spans[-1][1] == n
    assert all(nxt[0] - cur[1] >= T.GAP for cur, nxt in zip(spans, spans[1:])), "at least 64 filler bytes between plants"
    by = {}
    for p in F.plants:
        by.setdefault(p["section"], []).append(p)
        if not p["exact"]:
            assert abs(p["dl"]) <= min(p["q"], k - p["q"]) and p["s"] == p["j"] + a[p["q"]] + p["dl"]
            assert F.text[p["s"]:p["s"] + a[p["q"] + 1] - a[p["q"]]] == F.P[a[p["q"]]:a[p["q"] + 1]], "the named piece stands intact at s"
    # every valid (q, dl) at every residue of s
    assert {(p["q"], p["dl"], p["s"] % 16) for p in by["residue"]} == {(q, dl, r) for q, dl in T.valid_shifts(k) for r in range(16)}
    assert len(by["residue"]) == 16 * len(T.valid_shifts(k))
    # every x of the walk over a 4 KiB seam, for the longest piece (hence for every piece), on successive seams
    longest = max(a[q + 1] - a[q] for q in range(k + 1))
    assert [p["x"] for p in by["seam"]] == list(range(longest + 16))
    assert [p["s"] for p in by["seam"]] == [4096 * (x + 1) - x for x in range(longest + 16)]
    assert {(p["q"], p["dl"]) for p in by["seam"]} == set(T.valid_shifts(k)[:longest + 16])
    assert [(p["j"], p["q"]) for p in by["ends"]] == [(0, 0), (n - m, k)]
    assert sorted(p["j"] % 16 for p in by["exact"]) == list(range(16))
    assert all(F.text[p["j"]:p["j"] + m] == F.P for p in by["exact"])


def test_census(F):
    k = F.k
    cen = T.census(F)
    assert all(c[4] <= k for c in cen), "every plant is a match"
    assert all(c[4] == 0 and len(c[5]) >= k + 1 for p, c in zip(F.plants, cen) if p["exact"]), "in an exact occurrence every piece nominates"
    tight = _tight(F)
    assert all((p["q"], p["dl"]) in c[5] for p, c in tight)
    at_k = sum(c[4] == k for _, c in tight) / len(tight)
    sole = sum(c[5] == [(p["q"], p["dl"])] for p, c in tight) / len(tight)
    print("%s: %d tight plants, distance exactly k %.3f, sole nominator %.3f" % (T.family_id(F.fam), len(tight), at_k, sole))
    assert at_k >= 0.9, at_k
    assert sole >= 0.8, sole
    # the tightest case of the argument: a piece of exactly 2*KL-1 bytes at s = 1 (mod KL) has ONE aligned block
    a = T.piece_offsets(F.m, k)
    for tight_len, kl in ((15, 8), (31, 16)):
        for q in range(k + 1):
            if a[q + 1] - a[q] != tight_len:
                continue
            assert any(p["q"] == q and p["s"] % kl == 1 and c[5] == [(q, p["dl"])] for p, c in tight), (tight_len, q)


def test_expected_positions_are_what_the_oracle_finds(F):
    exp = T.expected_positions(F)
    assert len(set(exp)) == len(exp)
    assert {p["j"] for p in F.plants} <= set(exp)
    assert len({p["j"] for p in F.plants}) == len(F.plants)
    assert H.oracle_counts(F.text, [F.P], F.k, banded=True) == [len(exp)]
