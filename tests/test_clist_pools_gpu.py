"""The POOLED hand-over of the sieve's candidate list (ApmSieve2PoolArgs, apm_sieve2cfdg_kernel; APM_CLIST_POOLS): a scanning
workgroup that ends moves its region's entries into pool g % P, and the verify launch is given the P pools as its regions.
What can go wrong that the regions cannot get wrong: an entry lost or doubled on its way (the reservation, the copy of what
other waves of the workgroup stored), a pool counter that is not zero when a launch starts (two sets, alternating, and launches
that differ in their pools: the owner ranges below have 6 and 11 regions, and run twice), a workgroup
without entries that reserves all the same, and the overflow rows and the block list beside the pools.

The base case: 1 MiB of seeded ACGT text, k = 3, patterns of 16 and 19 bytes (their units hold the window-DP slots: the
diagonal kernel runs) and of 64, 96 and 128 bytes; 48 occurrences of the long ones inside one 64 KiB stretch that starts
777 bytes behind a region's border -- two of the text's 17 regions take them all -- exact, with 1..3 substitutions and
with an insertion / deletion pair; some more spread over the text and over block seams; truncated windows at the text's end.
The expected counts come from the CPU oracle; the records of apm_find_all_buffer are distinct, as many as the counts, each
within k, every plant among them.  The same text from byte 3 on as a shard with owner ranges cut inside the cluster (at an
aligned device pointer, and at a pointer + 3, which the sieve pipeline does not take: records only), its first
8 KiB (one workgroup; in the 1 MiB text most of the 17 have no entries and reserve nothing), a period-two text of 256 KiB
with a period-two pattern (every entry passes, the regions overflow), and k = 4 (the column kernel: never pooled).

Settings: APM_CLIST_POOLS unset, 0, 1, 7, 4096, each with APM_CLIST_REGION_CAP unset, 1 and 5 (overflow rows and the block list
carry most of the set).  The switches are read once per process: one fresh child per setting runs every case, eight
children at a time.  Every setting gives the counts and sorted records of pools = 0, and the same sieve_candidates where no
region overflows (see _check_candidates).  The expected counts are the oracle's banded form (exact within k; the full DP
over 1 MiB takes 9 s for the same numbers).

NOT tested here, for they need texts of tens of MiB: a wave that takes a second batch of a pool (more than 64 entries per
wave of the verify launch), and a text big enough for many waves per pool to have work.  Both stay with the full-size cfg3
workload tests and the soak tests."""
import concurrent.futures
import functools
import hashlib
import json
import os
import random
import struct
import subprocess
import sys

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

ACGT = b"ACGT"
K = 3
N = (1 << 20) + 333
REGION = 64 << 10                      # a workgroup's 16 blocks: the text's regions are its 64 KiB stretches
CLUSTER = 5 * REGION + 777             # the cluster's stretch [CLUSTER, CLUSTER + 64 KiB)
SMALL_N = 8 << 10
PERIOD_N = 256 << 10
K4_N = 7 * REGION                     # (the cluster inside)
POOLS = [None, 0, 1, 7, 4096]
CAPS = [None, 1, 5]
DEFAULT_POOLS = 8


def _text(seed, n):
    table = bytes(ACGT[b & 3] for b in range(256))
    return bytearray(random.Random(seed).randbytes(n).translate(table))


def _other(rnd, b):
    return rnd.choice([x for x in ACGT if x != b])


def _variant(rnd, p, i):
    """occurrence i of pattern p: exact, 1..3 substitutions, or one insertion and one deletion (distance <= 2, + one substitution)"""
    w = bytearray(p)
    kind = i % 5
    if 1 <= kind <= 3:
        for j in rnd.sample(range(len(p)), kind):
            w[j] = _other(rnd, w[j])
    elif kind == 4:
        del w[len(w) - 1 - rnd.randrange(8)]
        w.insert(3 + rnd.randrange(8), rnd.choice(ACGT))
        if i % 2:
            j = len(w) // 2
            w[j] = _other(rnd, w[j])
    return bytes(w)


@functools.lru_cache(maxsize=None)
def _base():
    """(patterns, text, plants [(pattern, window start)])"""
    rnd = random.Random(1101)
    pats = [bytes(rnd.choice(ACGT) for _ in range(m)) for m in (16, 19, 64, 96, 128)]
    text = _text(1102, N)
    plants = []

    def put(q, pos, w):
        text[pos:pos + len(w)] = w
        plants.append((q, pos))

    for i in range(48):                                   # the cluster: one occurrence per 1365 bytes of the stretch
        q = 2 + i % 3
        put(q, CLUSTER + (REGION * i) // 48 + rnd.randrange(40), _variant(rnd, pats[q], i))
    for i, pos in enumerate((0, 4096 - 50, 3 * REGION - 64, 9 * REGION + 4090, 13 * REGION + 12345, 15 * REGION + 8191 - 17)):
        q = i % 5                                         # spread: the text's start, block seams, a region's border
        put(q, pos, _variant(rnd, pats[q], i))
    tail = pats[4][:70]                                   # truncated windows of the 128-byte pattern at the text's end
    text[N - len(tail):] = tail
    plants.append((4, N - len(tail)))
    return pats, bytes(text), plants


@functools.lru_cache(maxsize=None)
def _period():
    pats, _, _ = _base()
    return [bytes(ACGT[i & 1] for i in range(16))] + list(pats[1:]), bytes(ACGT[i & 1] for i in range(PERIOD_N))


def _cases():
    """name -> (patterns, text, k)"""
    pats, text, _ = _base()
    ppats, ptext = _period()
    return {"base": (pats, text, K), "small": (pats, text[:SMALL_N], K), "period": (ppats, ptext, K), "k4": (pats, text[:K4_N], 4)}


@functools.lru_cache(maxsize=None)
def _want(name):
    pats, text, k = _cases()[name]
    return H.oracle_counts(text, pats, k, banded=True)


def _digest(rec):
    return hashlib.sha256(json.dumps(sorted(map(list, rec))).encode()).hexdigest()


STATS = ("sieve_cf_dp_form", "sieve_clist", "sieve_clist_pools", "sieve_cf", "sieve_waves", "sieve_candidates")


def _sharded(ctx, text, capacity, mis):
    """the text from byte 3 on as a shard (every block, pair and region border moves by 3 against the plants), two owner ranges
    cut inside the cluster.  mis = 0: at an aligned device pointer; mis = 3: at a pointer + 3 -- the sieve pipeline takes
    16-byte aligned texts only, so that shard runs without it: the records, not the statistics"""
    n = len(text)
    cut = (CLUSTER + REGION // 2) | 1
    d_text, d_rec, d_n = ctx.device_alloc(n + 64), ctx.device_alloc(16 * capacity), ctx.device_alloc(16)
    try:
        ctx.device_upload(d_text + mis, text[3:])
        ctx.device_memset(d_n, 0, 16)
        ctx.synchronize()
        pools = []
        for ob, oe in ((3, cut), (cut, n)):
            ctx.find_shard_device(d_text + mis, 3, n - 3, n, ob, oe, d_rec, capacity, d_n, None)
            pools.append({s: ctx.stat(s) for s in STATS[:5]})
        ctx.synchronize()
        total = struct.unpack("<Q", ctx.device_download(d_n, 8))[0]
        raw = ctx.device_download(d_rec, 16 * min(total, capacity))
        return sorted((q, pos) for pos, q, _ in (struct.unpack_from("<QII", raw, 16 * i) for i in range(len(raw) // 16))), total, pools
    finally:
        for d in (d_text, d_rec, d_n):
            ctx.device_free(d)


def _worker():
    apm = H.pkg()
    out = {}
    for name, (pats, text, k) in _cases().items():
        with apm.ApmContext(device=0) as ctx:
            ctx.set_patterns(pats, k)
            for rep in range(2):          # (twice: the second pass counts in the other set of pool counters, zeroed by the first)
                counts = ctx.count_buffer(text)
                stats = {s: ctx.stat(s) for s in STATS}
                rec, total = ctx.find_all_buffer(text, sum(counts) + 64)
                res = dict(counts=counts, stats=stats, rec_stats={s: ctx.stat(s) for s in STATS[:5]}, n_found=total, n_records=len(rec),
                           unique=len(set(rec)) == len(rec), digest=_digest(rec), per_pattern=[sum(1 for q, _ in rec if q == i) for i in range(len(pats))])
                if name != "period":
                    res["records"] = sorted(rec)
                out["%s:%d" % (name, rep)] = res
            if name == "base":
                for mis in (0, 3):
                    rec, total, pools = _sharded(ctx, text, sum(counts) + 64, mis)
                    out["shard%d" % mis] = dict(records=rec, n_found=total, stats=pools)
    print(json.dumps(out))


def _env(pools, cap):
    env = {key: val for key, val in os.environ.items() if key not in ("APM_CLIST_POOLS", "APM_CLIST_REGION_CAP")}
    if pools is not None:
        env["APM_CLIST_POOLS"] = str(pools)
    if cap is not None:
        env["APM_CLIST_REGION_CAP"] = str(cap)
    return env


def _child(setting):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, env=_env(*setting), timeout=300)
    assert r.returncode == 0, (setting, r.stderr.decode()[-3000:])
    return json.loads(r.stdout.decode().strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def _results():
    settings = [(p, c) for c in CAPS for p in POOLS]
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        return dict(zip(settings, pool.map(_child, settings)))


def _pools_expected(pools, st):
    """the setting clamped to the pass's regions = its scanning workgroups (sieve_waves over the waves of a workgroup)"""
    regions = st["sieve_waves"] // (st["sieve_cf"] // 64)
    assert regions >= 1 and st["sieve_waves"] % (st["sieve_cf"] // 64) == 0, st
    return min(DEFAULT_POOLS if pools is None else pools, regions)


def _check_candidates(res, name, cap, where):
    """sieve_candidates equals the pass's of pools = 0.  Asserted where no region overflows (no APM_CLIST_REGION_CAP): which of two
    waves' window-DP entries still finds room in a full region is a race between them, the one without room leaves as a mask bit
    without the DP's verdict, so the sum may differ from run to run there, with or without pools; printed for those."""
    got, ref = res["stats"]["sieve_candidates"], _results()[(0, cap)][name]["stats"]["sieve_candidates"]
    print("%r sieve_candidates %d, pools 0: %d" % (where, got, ref))
    if cap is None:
        assert got == ref, where


SETTINGS = pytest.mark.parametrize("pools,cap", [(p, c) for c in CAPS for p in POOLS],
                                   ids=["pools_%s-cap_%s" % (p, c) for c in CAPS for p in POOLS])


@SETTINGS
def test_base_case_counts_and_records(pools, cap):
    pats, text, plants = _base()
    want = _want("base")
    assert sum(want[2:]) >= 48
    ref = _results()[(0, cap)]
    for rep in range(2):
        res, where = _results()[(pools, cap)]["base:%d" % rep], ("base", pools, cap, rep)
        for st in (res["stats"], res["rec_stats"]):
            assert st["sieve_cf_dp_form"] == 2 and st["sieve_clist"] == 1, (where, st)
            assert st["sieve_clist_pools"] == _pools_expected(pools, st), (where, st)
            assert st["sieve_waves"] // (st["sieve_cf"] // 64) >= 16, (where, st)             # (regions: 64 KiB stretches of the text)
        assert res["counts"] == want, where
        assert res["n_found"] == res["n_records"] == sum(want) and res["unique"], where
        assert res["per_pattern"] == want, where
        assert res["records"] == ref["base:0"]["records"] and res["digest"] == ref["base:0"]["digest"], where
        _check_candidates(res, "base:0", cap, where)
    if pools == 0 and cap is None:                                # the records themselves, once: every setting equals these
        rec = [tuple(r) for r in res["records"]]
        for q, j in rec:
            size = min(len(pats[q]), len(text) - j)
            assert H.window_distance(pats[q][:size], text[j:j + size]) <= K, (q, j)
        near = [(q, j) for q, j in plants if H.window_distance(pats[q][:min(len(pats[q]), N - j)], text[j:j + len(pats[q])]) <= K]
        assert len(near) >= 48 and set(near) <= set(rec), sorted(set(near) - set(rec))
        in_cluster = [j for q, j in rec if CLUSTER <= j < CLUSTER + REGION + 64]
        assert len(in_cluster) >= 48


@SETTINGS
def test_pointer_plus_3_and_owner_ranges_cut_inside_the_cluster(pools, cap):
    res, ref = _results()[(pools, cap)], _results()[(0, None)]
    want = [r for r in ref["base:0"]["records"] if r[1] >= 3]
    assert len(want) < len(ref["base:0"]["records"])              # (the plant at 0 belongs to nobody's range)
    # aligned: the sieve ran over each owner range (its regions: the range's 64 KiB stretches), pooled as set
    for st in res["shard0"]["stats"]:
        assert st["sieve_cf_dp_form"] == 2 and st["sieve_clist"] == 1, (pools, cap, st)
        assert st["sieve_clist_pools"] == _pools_expected(pools, st), (pools, cap, st)
        assert st["sieve_waves"] // (st["sieve_cf"] // 64) >= 5, (pools, cap, st)
    for mis in (0, 3):
        got = res["shard%d" % mis]["records"]
        assert got == want, (pools, cap, mis, [r for r in got if r not in want], [r for r in want if r not in got])
        assert res["shard%d" % mis]["n_found"] == len(want), (pools, cap, mis)


@SETTINGS
def test_8_kib_text_one_workgroup(pools, cap):
    want = _want("small")
    assert sum(want) >= 1
    for rep in range(2):
        res, where = _results()[(pools, cap)]["small:%d" % rep], ("small", pools, cap, rep)
        assert res["stats"]["sieve_cf_dp_form"] == 2 and res["stats"]["sieve_clist"] == 1, (where, res["stats"])
        assert res["stats"]["sieve_clist_pools"] == _pools_expected(pools, res["stats"]) == min(1, DEFAULT_POOLS if pools is None else pools), (where, res["stats"])
        assert res["counts"] == want and res["n_found"] == res["n_records"] == sum(want) and res["unique"], where
        assert res["records"] == _results()[(0, None)]["small:0"]["records"], where
        _check_candidates(res, "small:0", cap, where)


@SETTINGS
def test_period_two_text_every_entry_passes_and_the_regions_overflow(pools, cap):
    want = _want("period")
    assert want[0] >= PERIOD_N - 16 + 1                          # every window start matches the period-two pattern within two edits
    for rep in range(2):
        res, where = _results()[(pools, cap)]["period:%d" % rep], ("period", pools, cap, rep)
        assert res["stats"]["sieve_cf_dp_form"] == 2 and res["stats"]["sieve_clist"] == 1, (where, res["stats"])
        assert res["stats"]["sieve_clist_pools"] == _pools_expected(pools, res["stats"]), (where, res["stats"])
        assert res["counts"] == want and res["n_found"] == res["n_records"] == sum(want) and res["unique"], where
        assert res["per_pattern"] == want, where
        assert res["digest"] == _results()[(0, None)]["period:0"]["digest"], where
        _check_candidates(res, "period:0", cap, where)
        # one candidate per pair of positions, give or take the text's ends: far beyond what the regions hold (512 entries each)
        assert res["stats"]["sieve_candidates"] >= PERIOD_N // 2 - 4096, where


@pytest.mark.parametrize("pools", POOLS)
def test_k4_keeps_its_regions(pools):
    want = _want("k4")
    res = _results()[(pools, None)]["k4:1"]
    # (this set at k = 4: the plain code-filter kernel with the list, no window DP on codes -- form 0; a set with slots: form 1)
    assert res["stats"]["sieve_cf_dp_form"] in (0, 1) and res["stats"]["sieve_clist"] == 1 and res["stats"]["sieve_clist_pools"] == 0, (pools, res["stats"])
    assert res["rec_stats"]["sieve_clist_pools"] == 0, pools
    assert res["counts"] == want and res["n_found"] == res["n_records"] == sum(want) and res["unique"], pools
    assert res["records"] == _results()[(0, None)]["k4:0"]["records"], pools


if __name__ == "__main__":
    sys.path.insert(0, H.ROOT)
    _worker()
