"""The SAMPLED filter kernels on pigeonhole-tight windows (tests/sampled_tight_ref.py): every window whose only
nominator is one piece at one shift, with that piece at every residue of the sampling stride, walking over a 4 KiB block
seam byte by byte, and at both ends of the text.  A fault in one residue's key, in one (r, t) operand of the register
compare, in a mask at r = 7, in the dedup's idea of the nominating block, or in the test that admits the block in the
text's last partial 16 bytes loses or doubles exactly such windows and nothing else.

Every kernel form that lives on the sampled argument runs the sweep (a worker process per switch setting: the switches
are read once per process), and the launch labels and statistics show that it is that form which ran:
  stream kernel <16,16> and <8,8>, the LDS-tile fallback with the same strides (LDS-DMA and register staged), the sampled
  sieve + verify launch, the fused kernel with ready-made register-compare operands and with per-hit packing.
Counts equal the oracle's; the records of apm_find_all_buffer are distinct, each a window within k, as many as the oracle
counts, every planted window among them.  A failure names the plants lost or doubled as
(family, q, dl, s mod 16, s mod 4096)."""
import collections
import json
import os
import random
import subprocess
import sys

import pytest

import helpers as H
import sampled_tight_ref as T

pytestmark = pytest.mark.gpu

BANDED = 4

_WORKER = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import helpers as H
import sampled_tight_ref as T
apm = H.pkg()
out = {}
for fam in T.FAMILIES:
    fid = T.family_id(fam)
    if fid not in sys.argv[3].split(","):
        continue
    F = T.family(fam)
    with apm.ApmContext(device=0) as ctx:
        ctx.set_kernel("auto")
        ctx.set_timing(True)
        ctx.set_patterns([F.P], F.k)
        counts = ctx.count_buffer(F.text)
        labels = [l for l, _ in ctx.launch_times()]
        recs, total = ctx.find_all_buffer(F.text)
        labels += [l for l, _ in ctx.launch_times()]
        out[fid] = dict(counts=counts, records=recs, total=total, kernel=ctx.pattern_kernel(0),
                        stride=ctx.stat("sieve_stride"), fused=ctx.stat("sieve_fused"), labels=labels)
print(json.dumps(out))
"""

# (switches, the scan launches of the families with k <= 1, those of the families with k >= 2, sieve_stride and sieve_fused of the latter)
SETTINGS = [
    ({}, {"stream"}, {"fused"}, (8, 1)),
    ({"APM_FUSED": "0"}, {"stream"}, {"sieve", "verify"}, (8, 0)),
    ({"APM_FUSED_RC": "0"}, {"stream"}, {"fused"}, (8, 1)),                       # per-hit packing of the register compare's operands
    ({"APM_SIEVE": "0"}, {"stream"}, {"stream"}, None),                           # k >= 2: the stream kernel with bands 1..3
    ({"APM_SIEVE": "0", "APM_FILTER_STREAM": "0"}, {"tile"}, {"tile"}, None),     # LDS-DMA tile kernel
    ({"APM_SIEVE": "0", "APM_FILTER_STREAM": "0", "APM_FILTER_DMA": "0"}, {"tile"}, {"tile"}, None),  # register-staged tile kernel
]
SCAN_LABELS = {"stream", "tile", "fused", "sieve", "verify", "bitpar", "nfa", "wavefront", "generic"}
HALVES = [T.FAMILIES[0::2], T.FAMILIES[1::2]]   # (two ids per setting: a few seconds each)


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


_want = {}


def _oracle_count(F):
    if F.fam not in _want:
        _want[F.fam] = H.oracle_counts(F.text, [F.P], F.k, banded=True)[0]
    return _want[F.fam]


def _named(F, positions):
    """the plants next to these window starts, as (family, q, dl, s mod 16, s mod 4096) + the distance of the start from the plant's"""
    out = []
    for j in sorted(positions)[:12]:
        p = T.plant_near(F, j)
        out.append(T.plant_name(F, p) + (p["section"], j - p["j"]))
    return out


def _msg(*parts):
    """a string: pytest shortens the repr of anything else in an assertion message, and the plants named are the diagnosis"""
    return repr(parts)


def _check_count(F, count, where):
    want = _oracle_count(F)
    assert count == want, _msg(where, "count", count, "oracle", want)


def _check_records(F, positions, where):
    """positions: the window starts of F.P's records"""
    k, m, n = F.k, F.m, F.n
    exp = set(T.expected_positions(F))
    seen = collections.Counter(positions)
    doubled = [j for j, c in seen.items() if c > 1]
    assert not doubled, _msg(where, "doubled", _named(F, doubled))
    beyond = [j for j in seen if j not in exp
              and (j >= n - k or H.window_distance(F.P[:min(m, n - j)], F.text[j:j + min(m, n - j)]) > k)]
    assert not beyond, _msg(where, "records of windows beyond k", sorted(beyond)[:12])
    missing = [p["j"] for p in F.plants if p["j"] not in seen]
    assert not missing, _msg(where, "lost", _named(F, missing))
    assert len(positions) == _oracle_count(F), _msg(where, "records", len(positions), "oracle", _oracle_count(F), "lost", _named(F, exp - set(seen)))


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join("%s=%s" % (k[4:], v) for k, v in s[0].items()) or "default")
def test_tight_plants_through_every_sampled_form(setting, half):
    env, labels_k01, labels_k2, sieve = setting
    fams = HALVES[half]
    r = subprocess.run([sys.executable, "-c", _WORKER, H.ROOT, os.path.join(H.ROOT, "tests"), ",".join(T.family_id(f) for f in fams)],
                       capture_output=True, env=dict(os.environ, **env), timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert sorted(got) == sorted(T.family_id(f) for f in fams)
    for fam in fams:
        F = T.family(fam)
        res = got[T.family_id(fam)]
        where = (T.family_id(fam), env)
        # the form that ran
        assert res["kernel"] == BANDED, where
        ran = set(res["labels"]) & SCAN_LABELS
        assert ran == (labels_k01 if F.k <= 1 else labels_k2), (where, res["labels"])
        if F.k >= 2 and sieve:
            assert (res["stride"], res["fused"]) == sieve, (where, res["stride"], res["fused"])
        else:
            assert res["stride"] == 0 and res["fused"] == 0, (where, res["stride"], res["fused"])
        # what it found
        assert len(res["counts"]) == 1 and res["total"] == len(res["records"]) and all(pat == 0 for pat, _ in res["records"]), where
        positions = [pos for _, pos in res["records"]]
        _check_records(F, positions, where)
        _check_count(F, res["counts"][0], where)


@pytest.mark.parametrize("fam", [("dna", 45, 2), ("dna", 64, 3)], ids=T.family_id)
def test_big_set_packs_the_register_compare_per_hit(ctx, apm, fam):
    """more than 128 units in the set: no ready-made operands, the fused kernel packs them per hit, and the key lists of a
    code word hold several keys (keys.next)"""
    F = T.family(fam)
    rnd = random.Random("companions %d %d" % (F.m, F.k))
    pats = [F.P] + [bytes(rnd.choice(T.DNA) for _ in range(F.m)) for _ in range(128 // (F.k + 1) + 6)]
    assert (F.k + 1) * len(pats) > 128
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, F.k)
    counts = ctx.count_buffer(F.text)
    assert ctx.stat("sieve_stride") == 8 and ctx.stat("sieve_fused") == 1
    recs, total = ctx.find_all_buffer(F.text)
    assert ctx.stat("sieve_fused") == 1
    assert all(ctx.pattern_kernel(i) == BANDED for i in range(len(pats)))
    where = (T.family_id(fam), "big set")
    assert total == len(recs)
    _check_records(F, [pos for pat, pos in recs if pat == 0], where)
    _check_count(F, counts[0], where)
    want = H.oracle_counts(F.text, pats, F.k, banded=True)
    assert counts == want, where
    per_pat = collections.Counter(pat for pat, _ in recs)
    assert [per_pat[i] for i in range(len(pats))] == want and len(set(recs)) == len(recs), where


def _shard_count(ctx, d_text, text_off, text_len, n, b, e, d_cnt):
    ctx.count_shard_device(d_text, text_off, text_len, n, b, e, d_cnt)
    ctx.synchronize()


@pytest.mark.parametrize("fam", [("dna", 31, 0), ("dna", 30, 1), ("dna", 47, 2), ("dna", 120, 7)], ids=T.family_id)
def test_unaligned_text_pointer(ctx, apm, fam):
    """text that does not start at a multiple of 16 bytes in memory: no sieve pipeline, no 16-byte loads -- the
    register-staged tile kernel with the sampled strides"""
    F = T.family(fam)
    n = F.n
    ctx.set_kernel("auto")
    ctx.set_patterns([F.P], F.k)
    d = ctx.device_alloc(n + 64)
    cnt = ctx.device_alloc(8)
    try:
        ctx.device_upload(d + 3, F.text)
        ctx.device_memset(cnt, 0, 8)
        _shard_count(ctx, d + 3, 0, n, n, 0, n, cnt)
        _check_count(F, int.from_bytes(ctx.device_download(cnt, 8), "little"), (T.family_id(fam), "pointer + 3"))
    finally:
        ctx.device_free(cnt)
        ctx.device_free(d)


@pytest.mark.parametrize("fam", [("dna", 64, 1), ("dna", 47, 2), ("dna", 120, 7)], ids=T.family_id)
def test_owner_ranges_cut_inside_plants(ctx, apm, fam):
    """own ranges cut 3 bytes into the intact piece of every seventh plant and 1 byte in front of its window, at positions
    that are no multiples of 16; each range with the halo m - 1 behind it and 3 bytes in front.  The ranges' counts add
    up to the whole text's."""
    F = T.family(fam)
    n, m = F.n, F.m
    cuts = set()
    for p in F.plants[::7]:
        cuts.update(c for c in (p["s"] + 3, p["j"] - 1) if 0 < c < n and c % 16)
    cuts = [0] + sorted(cuts) + [n]
    assert len(cuts) >= 3 * len(F.plants[::7]) // 2   # (one candidate in 16 is a multiple of 16 and left out)
    ctx.set_kernel("auto")
    ctx.set_patterns([F.P], F.k)
    cnt = ctx.device_alloc(8)
    d_text = ctx.device_alloc(max(e - b for b, e in zip(cuts[:-1], cuts[1:])) + m + 32)
    try:
        ctx.device_memset(cnt, 0, 8)
        for b, e in zip(cuts[:-1], cuts[1:]):
            lo, hi = max(0, b - 3), min(n, e + m - 1)
            ctx.device_upload(d_text, F.text[lo:hi])
            _shard_count(ctx, d_text, lo, hi - lo, n, b, e, cnt)
        _check_count(F, int.from_bytes(ctx.device_download(cnt, 8), "little"), (T.family_id(fam), "cuts", len(cuts)))
    finally:
        ctx.device_free(d_text)
        ctx.device_free(cnt)
