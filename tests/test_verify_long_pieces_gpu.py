"""Per-position sets whose units have parts BEYOND 16 BYTES: the nomination predicate judges the exact part by its first 16
bytes and the partner by the 16 bytes that adjoin the exact part (csrc/apm_core.h, apm_unit_pred16;
ApmVerifyCore<BAND, PREFIX = true> in csrc/apm_verify.hip), the banded DP
decides, and the dedup asks the same predicate for a window's earlier nominators.  What can go wrong that short parts cannot
get wrong: a window counted twice or not at all because the candidate path and the dedup disagree about a unit whose
tail is damaged, a nominator the dedup defers to that the sieve never delivered, a near-copy that nominates (every unit
intact on its 16 + 16 bytes) and must be rejected by the DP, the shifts of the band around all of them.

One case per (m, k): m in 65, 68, 96, 128, 200, 512 at k = 0, 1 (band 0, parts without partner) and 2, 3 (band 1; k = 2 has the
unpaired last piece); m in 128, 200, 512 at k = 4, 5 (band 2); m = 512 at k = 7 (band 3).  A set of long pieces alone takes
the sampled sieve, so every set holds a second pattern of 10 (k + 1) bytes: its pieces of 10 bytes make the sieve
per-position (asserted: sieve_stride 1).  The text is 80 KiB + 333 bytes of seeded ACGT with these plants of the long pattern,
all in every case's text:
  - an exact copy; copies at byte 3, across a 4 KiB block border and flush with the text's end (the windows behind it
    are truncated by the text's end and count by the reference's rule: the oracle's counts hold them);
  - d = 1..k substitutions, d insertions, d deletions, each placed (i) in the last piece beyond its 16th byte (the piece
    is an exact part there), (ii) in a partner beyond its 16th byte counted from the exact part -- two of them make the
    full predicate false where the prefix form is true, and an insertion or deletion there moves the later units to
    another shift of the band -- and (iii) in the first 16 bytes of a piece.  The partner plants with d >= 2 are the ones
    that put a position at which the prefix form holds and the full predicate does not INSIDE a matching window: the
    dedup's verdict for that window depends on the form;
  - a near-copy: every piece keeps its first 16 bytes and (k >= 2) its last 16, every byte between them is changed -- all
    units nominate, the window does not match wherever more than k bytes change (asserted where at least 2 k + 2 do).
    That needs pieces beyond 16 bytes (k <= 1) or beyond 32 (k >= 2): the near-copy is REAL, a string that nominates and
    does not match, at k = 0, 1 for every m (33..496 bytes changed), at k = 2 for m = 128, 200, 512 (32, 104, 416), at
    k = 3, 4 for m = 200, 512 (72 and 40, 384 and 352), at k = 5, 7 for m = 512 (320, 256).  At m = 200, k = 5 eight bytes
    change (below the 2 k + 2 of the assertion: the oracle decides); at m = 65, 68, 96 with k = 2, 3 and at m = 128 with
    k = 3, 4, 5 no byte lies outside the tested prefixes, nothing changes and the three near-copy plants are plain copies;
  - a true occurrence with a near-copy flush against either end of it, no byte between them;
  - a copy with one byte inserted behind the 16th byte of the last piece: its units nominate two neighbouring windows.
Two strings that differ cannot overlap literally; nominations that overlap at every shift come from the LOW-ENTROPY case:
a text of 64 KiB of one letter with a pattern of 96 of that letter, and a tandem repeat of period 5 with a pattern of 100
bytes of it, k = 3: every position nominates and the dedup runs for every window (the two forms of the predicate agree
at every position of such a text: what these cases add is the overlap, not a difference between the forms).

Hand-over forms, forced through the environment in one fresh child each (the switches are read once per process): the
default (candidate list in pools), APM_SIEVE_CLIST=0 (hit masks), APM_SIEVE_CF=0 (no code filter), APM_CLIST_REGION_CAP=1
(overflow rows and the block list carry the set), APM_FUSED=1 (sieve and verify in one launch).  Every form runs every case
through the counting call and the find call (the record build).  Expected: the counts of the CPU oracle (banded form,
exact within k; computed once per case); records distinct, as many as the counts, every one of them within k by the
oracle's window distance -- so the records ARE the matching positions; every plant among them exactly if its own window
distance is within k."""
import concurrent.futures
import functools
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ACGT = b"ACGT"
N = (80 << 10) + 333
LOW_N = 64 << 10
CASES = ([(m, k) for k in (0, 1, 2, 3) for m in (65, 68, 96, 128, 200, 512)] +
         [(m, k) for k in (4, 5) for m in (128, 200, 512)] + [(512, 7)])
FORMS = {"default": {}, "clist_0": {"APM_SIEVE_CLIST": "0"}, "cf_0": {"APM_SIEVE_CF": "0"},
         "region_cap_1": {"APM_CLIST_REGION_CAP": "1"}, "fused_1": {"APM_FUSED": "1"}}
SWITCHES = ("APM_SIEVE_CLIST", "APM_SIEVE_CF", "APM_CLIST_REGION_CAP", "APM_FUSED", "APM_CLIST_POOLS", "APM_SIEVE")
STATS = ("sieve_on", "sieve_stride", "sieve_fused", "sieve_cf", "sieve_clist", "sieve_waves", "sieve_mask_bytes")


def _other(rnd, b):
    return rnd.choice([x for x in ACGT if x != b])


def _pieces(m, k):
    return [q * m // (k + 1) for q in range(k + 1)] + [m]


def _edited(rnd, p, kind, where):
    """pattern p with one edit of `kind` at each pattern index of `where` (applied from the back: the indices stay valid)"""
    w = bytearray(p)
    for y in sorted(where, reverse=True):
        if kind == "sub":
            w[y] = _other(rnd, w[y])
        elif kind == "ins":
            w.insert(y, _other(rnd, w[y]))
        else:
            del w[y]
    return bytes(w)


def _zone(m, k, zone, d):
    """d distinct pattern indices in a zone: 'tail' = the last piece beyond its 16th byte, 'partner' = the second piece beyond
    its 16th byte from the seam with the first (the partner of unit 0 where k >= 2), 'head' = the first 16 bytes of the
    second-to-last piece (of the only one at k = 0).  A piece too short for the zone gives its last bytes."""
    a = _pieces(m, k)
    if zone == "tail":
        lo, hi = a[k] + 16, m
    elif zone == "partner":
        q = 1 if k >= 1 else 0
        lo, hi = a[q] + 16, a[q + 1]
    else:
        q = max(k - 1, 0)
        lo, hi = a[q], min(a[q] + 16, a[q + 1])
    if hi - lo < d:
        lo = max(hi - d, 0)
    step = max((hi - lo) // d, 1)
    return [lo + i * step for i in range(d)]


def _near_copy(rnd, p, k):
    """every piece keeps its first 16 bytes and (paired units, k >= 2) its last 16; (near-copy, bytes changed)"""
    a = _pieces(len(p), k)
    w = bytearray(p)
    changed = 0
    for q in range(k + 1):
        for y in range(a[q] + 16, a[q + 1] - (16 if k >= 2 else 0)):
            w[y] = _other(rnd, w[y])
            changed += 1
    return bytes(w), changed


@functools.lru_cache(maxsize=None)
def _case(m, k):
    """(patterns [long, short], text, plants [(name, window start)], bytes the near-copy changes)"""
    rnd = random.Random(1700 + 8 * m + k)
    table = bytes(ACGT[b & 3] for b in range(256))
    text = bytearray(rnd.randbytes(N).translate(table))
    p = bytes(rnd.choice(ACGT) for _ in range(m))
    short = bytes(rnd.choice(ACGT) for _ in range(10 * (k + 1)))
    plants = []

    def put(name, pos, w):
        assert 0 <= pos and pos + len(w) <= N
        text[pos:pos + len(w)] = w
        plants.append((name, pos))

    near, changed = _near_copy(rnd, p, k)
    put("exact at byte 3", 3, p)
    put("across a block border", 2 * 4096 - m // 2 - 1, p)
    cursor = [3 * 4096 + 77]

    def place(name, w):
        put(name, cursor[0], w)
        cursor[0] += len(w) + 67 + rnd.randrange(8)

    place("exact", p)
    for d in range(1, k + 1):
        for kind in ("sub", "ins", "del"):
            for zone in ("tail", "partner", "head"):
                place("%d %s %s" % (d, kind, zone), _edited(rnd, p, kind, _zone(m, k, zone, d)))
    place("near-copy", near)
    put("near-copy in front", cursor[0], near)
    put("occurrence between near-copies", cursor[0] + m, p)
    put("near-copy behind", cursor[0] + 2 * m, near)
    cursor[0] += 3 * m + 71
    a = _pieces(m, k)
    place("two windows", _edited(rnd, p, "ins", [min(a[k] + 16, m - 1)]))
    place("short pattern", short)
    assert cursor[0] < N - 2 * m - 64, (m, k, cursor[0])
    put("flush with the end", N - m, p)
    put("short pattern", N - m - 16 - len(short), short)
    return [p, short], bytes(text), plants, changed


@functools.lru_cache(maxsize=None)
def _low():
    """name -> (patterns, text, k): one letter, and a tandem repeat of period 5 (with a short pattern: see above)"""
    unit = b"ACGTA"
    return {"one_letter": ([b"A" * 96, b"A" * 40], b"A" * LOW_N, 3),
            "period_5": ([(unit * 20)[:100], (unit * 8)[:40]], (unit * (LOW_N // 5 + 1))[:LOW_N], 3)}


def _all_cases():
    out = {"m%d_k%d" % (m, k): (_case(m, k)[0], _case(m, k)[1], k) for m, k in CASES}
    out.update(_low())
    return out


@functools.lru_cache(maxsize=None)
def _want(name):
    pats, text, k = _all_cases()[name]
    return H.oracle_counts(text, pats, k, banded=True)


def _worker():
    apm = H.pkg()
    out = {}
    for name, (pats, text, k) in _all_cases().items():
        with apm.ApmContext(device=0) as ctx:
            ctx.set_patterns(pats, k)
            counts = ctx.count_buffer(text)
            stats = {s: ctx.stat(s) for s in STATS}
            rec, total = ctx.find_all_buffer(text, sum(counts) + 64)
            res = dict(counts=counts, stats=stats, rec_stats={s: ctx.stat(s) for s in STATS}, n_found=total, n_records=len(rec),
                       unique=len(set(rec)) == len(rec), per_pattern=[sum(1 for q, _ in rec if q == i) for i in range(len(pats))])
            if name in _low():
                res["first"] = sorted(rec)[:200]
                res["span"] = [min(j for q, j in rec if q == 0), max(j for q, j in rec if q == 0)]
            else:
                res["records"] = sorted(rec)
            out[name] = res
    print(json.dumps(out))


def _child(form):
    env = {key: val for key, val in os.environ.items() if key not in SWITCHES}
    env.update(FORMS[form])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (form, r.stderr.decode()[-3000:])
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def _results():
    with concurrent.futures.ThreadPoolExecutor(len(FORMS)) as pool:
        return dict(zip(FORMS, pool.map(_child, FORMS)))


def _check_form(form, res, where):
    for st in (res["stats"], res["rec_stats"]):
        assert st["sieve_on"] == 1 and st["sieve_stride"] == 1, (where, st)      # the per-position pipeline
        assert (st["sieve_fused"] == 1) == (form == "fused_1"), (where, st)
        if form != "fused_1":
            assert (st["sieve_cf"] != 0) == (form != "cf_0"), (where, st)
            assert st["sieve_clist"] == (1 if form in ("default", "region_cap_1") else 0), (where, st)
        if form == "region_cap_1":
            # in effect, not merely asked for: sieve_mask_bytes = 4 per list entry + 256 per block on the overflow list, and a
            # region (a scanning workgroup's stretch) holds one entry -- what is above 4 per region are rows of listed blocks
            regions = st["sieve_waves"] // (st["sieve_cf"] // 64)
            assert regions >= 1 and st["sieve_mask_bytes"] - 4 * regions >= 256, (where, st)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("m,k", CASES, ids=["m%d_k%d" % c for c in CASES])
def test_long_pieces_counts_records_and_plants(m, k, form):
    pats, text, plants, changed = _case(m, k)
    name = "m%d_k%d" % (m, k)
    want = _want(name)
    res, where = _results()[form][name], (name, form)
    _check_form(form, res, where)
    assert res["counts"] == want, where
    assert res["n_found"] == res["n_records"] == sum(want) and res["unique"] and res["per_pattern"] == want, where
    rec = [tuple(r) for r in res["records"]]
    for q, j in rec:                                     # distinct, as many as match, each within k: the matching positions
        size = min(len(pats[q]), N - j)
        assert H.window_distance(pats[q][:size], text[j:j + size]) <= k, (where, q, j)
    found = set(rec)
    n_match = 0
    for pname, j in plants:                              # every plant: among the records exactly if its window is within k
        q = 1 if pname == "short pattern" else 0
        dist = H.window_distance(pats[q], text[j:j + len(pats[q])])
        n_match += dist <= k
        assert ((q, j) in found) == (dist <= k), (where, pname, j, dist)
        if pname.startswith("near-copy") and changed >= 2 * k + 2:
            assert dist > k, (where, pname, changed, dist)
        if pname.startswith("exact") or pname in ("across a block border", "flush with the end", "occurrence between near-copies", "short pattern"):
            assert dist == 0, (where, pname)
        if pname.endswith(" sub tail") or pname.endswith(" sub partner") or pname.endswith(" sub head"):
            assert dist <= k, (where, pname, dist)
    assert n_match >= 7 + 3 * k + (k >= 2), (where, n_match)   # the exact ones, the substitutions, the inserted byte
    assert (0, N - m) in found and (0, 3) in found, where


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["one_letter", "period_5"])
def test_low_entropy_text_every_position_nominates(name, form):
    pats, text, k = _low()[name]
    want = _want(name)
    res, where = _results()[form][name], (name, form)
    _check_form(form, res, where)
    assert want[0] >= LOW_N // 5 - 100
    assert res["counts"] == want, where
    assert res["n_found"] == res["n_records"] == sum(want) and res["unique"] and res["per_pattern"] == want, where
    assert res["span"][0] == 0, where
    for q, j in res["first"]:
        size = min(len(pats[q]), LOW_N - j)
        assert H.window_distance(pats[q][:size], text[j:j + size]) <= k, (where, q, j)
    if name == "one_letter":                              # (the reference scans window starts up to n - k, truncated at the end)
        assert want[0] == LOW_N - k and res["span"][1] == LOW_N - k - 1, where


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker()
