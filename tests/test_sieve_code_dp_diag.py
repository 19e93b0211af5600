"""The DIAGONAL form of the code-filter sieve's window DP on codes (apm_sieve2cfdg_kernel, apm_code_dp_diag; k <= 3): the
region of a queue entry is trimmed to [s - off - B, s - off + m + B), B = k / 2 -- the window starts the verify launch
tries -- and each start is decided on the diagonals |d| <= B.  What can go wrong that the column form cannot get wrong:

* paths that live on a band-edge diagonal for the whole window: one insertion in the first two bytes and one deletion in the
  last two, and the reverse;
* the trimmed region's own strip test, r >= -16 and r + m + 2B <= 4128: occurrences whose region ends at 4127, 4128 and
  4129 of the strip (the last one takes the bit), occurrences at window start 0 and 1 (the region begins in front of the
  shard) and at the last full window;
* every slotted length's masks: the shortest and the longest m of every k, and for k = 3 the lengths of the headline.

A set = one short pattern (its units hold the slots), COMPANIONS patterns of 64 bytes that keep the code filter on, and a
period-2 short pattern whose own text makes every queue entry pass.  Texts of 64..170 KiB, DNA and a 20-letter alphabet
(four codes for twenty letters: the DP on codes passes what the verify launch rejects).  For every case AUTO's counts and
records equal the forced full-DP BITPAR kernel's, the records are the same with APM_CF_DP_DIAG unset and =0, the
candidates handed over are not more with the diagonal form, and the statistic sieve_cf_dp_form names the form that ran.

The switch is read once per process: one worker per setting runs every case (helpers: test_sieve_code_dp_queue.py)."""
import functools
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H
import test_sieve_code_dp_queue as Q

pytestmark = pytest.mark.gpu

BLOCK, ACGT, AMINO = Q.BLOCK, Q.ACGT, Q.AMINO
CASES = [(3, 16), (3, 23), (3, 24), (2, 12), (2, 26), (1, 8), (1, 28), (0, 30)]   # (k, m): m + 2k <= 30
K4_CASE = (4, 20)                                                                 # k >= 4 keeps the column kernel
BLOCKS = 40
N = BLOCKS * BLOCK + 777
PERIOD_N = 16 * BLOCK
SETTINGS = {"diag": {}, "column": {"APM_CF_DP_DIAG": "0"}}


def _companions(k):
    """lengths of the patterns beside the short ones.  One 64-byte companion does not keep the code filter on: the plan drops
    it when more than 80 % of the key words come from weak units (the short patterns' 8-byte pairs; checked with
    tests/host_plan_test.cpp), so there are as many as keep every set of the k below that line.  k = 0: a 14-byte one keeps the
    sieve per-position (pieces of 15 bytes and more take the sampled form, which has no code filter)"""
    return {0: [14] + [64] * 100, 1: [64] * 150}.get(k, [64] * 70)


def _other(rnd, alpha, b):
    return rnd.choice([x for x in alpha if x != b])


def _subs(rnd, p, alpha, n):
    w = bytearray(p)
    for i in rnd.sample(range(len(p)), n):
        w[i] = _other(rnd, alpha, w[i])
    return bytes(w)


def _ins_del(rnd, p, alpha):
    """one insertion in the first two bytes, one deletion in the last two: the path runs on diagonal +1"""
    w = bytearray(p)
    del w[len(w) - 1 - rnd.randrange(2)]
    w.insert(rnd.randrange(2), rnd.choice(alpha))
    return bytes(w)


def _del_ins(rnd, p, alpha):
    """the reverse: diagonal -1"""
    w = bytearray(p)
    w.insert(len(w) - rnd.randrange(2), rnd.choice(alpha))
    del w[rnd.randrange(2)]
    return bytes(w)


@functools.lru_cache(maxsize=None)
def _case(k, m, alpha):
    """(patterns: the short one, the period-2 one, the companions; text; planted window starts of the short pattern)"""
    rnd = random.Random(7000 + 100 * k + m + len(alpha))
    short = bytes(rnd.choice(alpha) for _ in range(m))
    period = bytes(alpha[i & 1] for i in range(m))
    pats = [short, period] + [bytes(rnd.choice(alpha) for _ in range(n)) for n in _companions(k)]
    text = Q._random_text(7100 + 100 * k + m + len(alpha), N, alpha)
    B = k // 2
    plants = []

    def put(pos, w):
        text[pos:pos + len(w)] = w
        plants.append(pos)

    put(0 if alpha == ACGT else 1, short)                 # window start 0 / 1: the region begins in front of the shard
    put(N - m, short)                                     # the last full window
    b = 2
    for end in (4127, 4128, 4129):                        # the trimmed region [j - B, j + m + B) ends here inside its block's strip
        put(b * BLOCK + end - m - B, short)
        b += 2
    for i in range(6):                                    # distance exactly k and k + 1 (substitutions), inside blocks and across seams
        put(b * BLOCK + (700 + 40 * i if i < 4 else -5 - i), _subs(rnd, short, alpha, k + (i & 1)))
        b += 1
    if k >= 2:
        for i in range(8):                                # the band-edge scripts, at even and odd positions, k = 3: one substitution more
            w = (_ins_del if i & 1 else _del_ins)(rnd, short, alpha)
            if k == 3 and i >= 4:
                j = 3 + rnd.randrange(m - 6)
                w = w[:j] + bytes([_other(rnd, alpha, w[j])]) + w[j + 1:]
            put(b * BLOCK + 1001 + 3 * i, w)
            b += 1
    assert b < BLOCKS - 2
    at = (BLOCKS - 2) * BLOCK + 100                       # a companion's occurrence
    text[at:at + len(pats[-1])] = pats[-1]
    return pats, bytes(text), plants


def _digest(rec):
    return hashlib.sha256(json.dumps(sorted(map(tuple, rec))).encode()).hexdigest()


def _evaluate(ctx, text, want_from_plants=None):
    ctx.set_kernel("auto")
    counts = ctx.count_buffer(text)
    stats = {s: ctx.stat(s) for s in ("sieve_on", "sieve_stride", "sieve_cf", "sieve_cf_dp_slots", "sieve_cf_dp_form", "sieve_clist",
                                      "sieve_candidates")}
    rec, total = ctx.find_all_buffer(text, sum(counts) + 64)
    ctx.set_kernel("bitpar")
    b_counts = ctx.count_buffer(text)
    b_rec, b_total = ctx.find_all_buffer(text, sum(b_counts) + 64)
    ctx.set_kernel("auto")
    rec = [tuple(r) for r in rec]
    return dict(stats=stats, counts=counts, bitpar_counts=b_counts, n_found=total, bitpar_n_found=b_total, n_records=len(rec),
                records_equal=sorted(rec) == sorted(tuple(r) for r in b_rec), records_unique=len(set(rec)) == len(rec),
                digest=_digest(rec), short_starts=sorted(j for q, j in rec if q == 0)[:4096])


def _worker():
    apm = H.pkg()
    out = {}
    for k, m in CASES + [K4_CASE]:
        for alpha in (ACGT, AMINO):
            pats, text, _ = _case(k, m, alpha)
            with apm.ApmContext(device=0) as ctx:
                ctx.set_patterns(pats, k)
                name = "%d:%d:%d" % (k, m, len(alpha))
                out[name] = _evaluate(ctx, text)
                if alpha == ACGT and (k, m) != K4_CASE:   # the period-2 text: every window of the period-2 pattern matches
                    out[name + ":period"] = _evaluate(ctx, bytes(ACGT[i & 1] for i in range(PERIOD_N)))
    print(json.dumps(out))


@functools.lru_cache(maxsize=None)
def _run(setting):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, env=dict(os.environ, **SETTINGS[setting]), timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


def _check_equals_bitpar(res, where):
    st = res["stats"]
    assert st["sieve_on"] == 1 and st["sieve_stride"] == 1 and st["sieve_cf"] > 0 and st["sieve_clist"] == 1 and st["sieve_cf_dp_slots"] > 0, \
        ("the window-DP stage did not run", where, st)
    assert res["counts"] == res["bitpar_counts"], where
    assert res["n_found"] == res["bitpar_n_found"] == res["n_records"] == sum(res["counts"]), where
    assert res["records_equal"] and res["records_unique"], where


@pytest.mark.parametrize("alpha", [ACGT, AMINO], ids=["dna", "amino"])
@pytest.mark.parametrize("k,m", CASES)
def test_diagonal_form_equals_bitpar_and_column_form(k, m, alpha):
    name = "%d:%d:%d" % (k, m, len(alpha))
    diag, col = _run("diag")[name], _run("column")[name]
    assert diag["stats"]["sieve_cf_dp_form"] == 2 and col["stats"]["sieve_cf_dp_form"] == 1, (name, diag["stats"], col["stats"])
    _check_equals_bitpar(diag, name)
    _check_equals_bitpar(col, name + " (column)")
    assert diag["digest"] == col["digest"] and diag["counts"] == col["counts"], name
    print("%s sieve_candidates: %d diagonal, %d column" % (name, diag["stats"]["sieve_candidates"], col["stats"]["sieve_candidates"]))
    assert diag["stats"]["sieve_candidates"] <= col["stats"]["sieve_candidates"], name
    # the planted windows that are within k of the short pattern are among the records
    pats, text, plants = _case(k, m, alpha)
    near = [j for j in plants if H.window_distance(pats[0], text[j:j + m]) <= k]
    assert len(near) >= (8 if k < 2 else 12), (name, len(near), len(plants))
    assert set(near) <= set(diag["short_starts"]), name


@pytest.mark.parametrize("k,m", CASES)
def test_period_two_text_every_entry_passes(k, m):
    name = "%d:%d:4:period" % (k, m)
    diag, col = _run("diag")[name], _run("column")[name]
    assert diag["stats"]["sieve_cf_dp_form"] == 2 and col["stats"]["sieve_cf_dp_form"] == 1, name
    _check_equals_bitpar(diag, name)
    assert diag["digest"] == col["digest"], name
    assert diag["stats"]["sieve_candidates"] <= col["stats"]["sieve_candidates"], name
    # every even window start matches the period-2 pattern exactly; with k >= 2 the odd ones do within two edits
    assert diag["counts"][1] >= (PERIOD_N - m + 1 if k >= 2 else (PERIOD_N - m) // 2 + 1), (name, diag["counts"][:2])


def test_k4_keeps_the_column_form():
    for alpha in (ACGT, AMINO):
        name = "%d:%d:%d" % (K4_CASE + (len(alpha),))
        diag = _run("diag")[name]
        assert diag["stats"]["sieve_cf_dp_form"] == 1, (name, diag["stats"])
        _check_equals_bitpar(diag, name)
        assert diag["digest"] == _run("column")[name]["digest"], name


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker()
