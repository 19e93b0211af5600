"""apm_find_all_buffer / apm_find_shard_device: the (pattern, position) records of EVERY pattern of the set in one pass of
the kernels the counting calls run.  The reference for positions is the CPU oracle (bisection over its range counts, or one
DP per window on small texts); every comparison is over the complete record set of every pattern of the case."""
import ctypes
import json
import os
import random
import subprocess

import pytest

import helpers as H

CASES = H.golden()["cases"]


# ---------------------------------------------------------------- CPU: the record's layout
def test_apm_match_layout_in_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "apm.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(apm_match), offsetof(apm_match, pos), '
                   'offsetof(apm_match, pattern), offsetof(apm_match, reserved)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(H.ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["16", "0", "8", "12"]


def test_apm_match_layout_in_ctypes():
    M = H.pkg().ApmMatch
    assert ctypes.sizeof(M) == 16
    assert (M.pos.offset, M.pattern.offset, M.reserved.offset) == (0, 8, 12)
    assert (M.pos.size, M.pattern.size, M.reserved.size) == (8, 4, 4)


def test_find_calls_are_declared_and_bound():
    apm = H.pkg()
    hdr = open(os.path.join(H.ROOT, "include", "apm.h")).read()
    for name in ("apm_find_all_buffer", "apm_find_shard_device"):
        assert name in apm.ABI_SYMBOLS and name + "(" in hdr
    assert "#define APM_ABI_VERSION 1" in hdr
    assert hasattr(apm.ApmContext, "find_all_buffer") and hasattr(apm.ApmContext, "find_shard_device")


# ---------------------------------------------------------------- reference positions
_ref_cache = {}


def ref_positions(text, pat, k):
    """matching window starts by bisection over the oracle's range counts (full DP for short patterns, its banded form
    -- exact for the predicate dist <= k -- where the band is a small part of the pattern)"""
    key = (hash(text), len(text), pat, k)
    if key in _ref_cache:
        return _ref_cache[key]
    banded = 8 * k <= len(pat)
    out = []

    def count(a, b):
        return H.oracle_counts(text, [pat], k, banded=banded, j_begin=a, j_end=b)[0]

    def descend(a, b, cnt):
        if cnt == 0:
            return
        if cnt == b - a:
            out.extend(range(a, b))
            return
        mid = (a + b) // 2
        left = count(a, mid)
        descend(a, mid, left)
        descend(mid, b, cnt - left)

    end = max(0, len(text) - k)
    if end:
        descend(0, end, count(0, end))
    _ref_cache[key] = out
    return out


def ref_records(text, pats, k):
    return [(i, j) for i, p in enumerate(pats) for j in ref_positions(text, p, k)]


def auto_kernel(p, k):
    """AUTO's rule (include/apm.h): 4 BANDED, 5 NFA, 3 BITPAR, 1 GENERIC, 0 for k >= m"""
    m = len(p)
    if k >= m:
        return 0
    if m <= 512 and k <= 7 and m // (k + 1) >= 4:
        return 4
    if k <= 7 and m + k // 2 <= 32 and len(set(p)) <= 16:
        return 5
    return 3 if m <= 4096 else 1


gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


@pytest.fixture(scope="module")
def ctx(apm):
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    c = apm.ApmContext(device=0)
    yield c
    c.close()


def check_complete(ctx, text, pats, k, capacity=None):
    """find_all_buffer == oracle, record for record; n_found == sum of the counts"""
    want = ref_records(text, pats, k)
    counts = ctx.count_buffer(text)
    got, total = ctx.find_all_buffer(text, capacity if capacity is not None else len(want) + 64)
    assert total == len(want) == sum(counts)
    assert got == want
    return want


# ---------------------------------------------------------------- 1. every kernel form
_FORM_WORKER = r"""
import json, random, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import helpers as H
apm = H.pkg()
rng = random.Random(20241)
lrng = random.Random(777)
out = {}
def run(key, pats, k, text, extra):
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        counts = ctx.count_buffer(bytes(text))
        rec, total = ctx.find_all_buffer(bytes(text), sum(counts) + 64)
        out[key] = dict(patterns=[p.decode("latin-1") for p in pats], counts=counts, records=rec, n_found=total,
                        kernels=[ctx.pattern_kernel(i) for i in range(len(pats))], **{s: ctx.stat(s) for s in extra})
for name, alphabet, n in (("dna", b"ACGT", 300000), ("prose", b"etaoin shrdlucETAOIN\n.,", 200000)):
    trng = random.Random(name)                              # the parent regenerates the text from this seed
    text = bytearray(trng.choice(alphabet) for _ in range(n))
    for k in (0, 1, 2, 3, 4, 5):
        pats = []
        for m in (16, 20, 27, 30, 40, 59, 64, 100, 128):
            o = rng.randrange(0, len(text) - m)
            p = bytearray(text[o:o + m])
            for _ in range(rng.randrange(0, k + 2)):          # substitutions
                p[rng.randrange(m)] = rng.choice(alphabet)
            if k >= 2 and rng.random() < 0.5:                  # one deletion + one insertion (keeps the length)
                i, j = sorted(rng.sample(range(1, m - 1), 2))
                del p[i]; p.insert(j, rng.choice(alphabet))
            pats.append(bytes(p))
        run("%s:%d" % (name, k), pats, k, text, ("sieve_clist",))
    for k in (2, 3, 4):   # long pieces only (>= 15 bytes): the sampled (stride-8) sieve, fused by default
        pats = []
        for m in (80, 96, 100, 128):
            o = lrng.randrange(0, len(text) - m)
            p = bytearray(text[o:o + m])
            for _ in range(lrng.randrange(0, k - 1)):
                p[lrng.randrange(m)] = lrng.choice(alphabet)
            if lrng.random() < 0.5:
                i, j = sorted(lrng.sample(range(1, m - 1), 2))
                del p[i]; p.insert(j, lrng.choice(alphabet))
            pats.append(bytes(p))
        run("%s:%d:long" % (name, k), pats, k, text, ("sieve_stride", "sieve_fused"))
print(json.dumps(out))
"""

FORM_ENVS = [{}, {"APM_FILTER_STREAM": "0"}, {"APM_FILTER_STREAM": "2"}, {"APM_FILTER_STREAM": "3"},
             {"APM_FILTER_DMA": "0"}, {"APM_FILTER_STREAM": "2", "APM_FILTER_DMA": "0"},
             {"APM_SIEVE": "0"}, {"APM_SIEVE": "0", "APM_FILTER_STREAM": "2"},
             {"APM_FUSED": "1"}, {"APM_FUSED": "0"}, {"APM_SIEVE_CF": "0"}, {"APM_FUSED_RC": "0"},
             {"APM_SIEVE_CLIST": "0"}, {"APM_CLIST_REGION_CAP": "1"}, {"APM_CLIST_REGION_CAP": "5"}]


@gpu
@pytest.mark.parametrize("env", FORM_ENVS, ids=lambda e: ",".join("%s=%s" % (k[4:], v) for k, v in e.items()) or "default")
def test_every_filter_kernel_form_records_equal_oracle(env):
    """The switch matrix of test_every_filter_kernel_form_agrees_with_oracle (list-driven verify, fused sampled and
    per-position, stream, tile with LDS-DMA and register staging, NFA and BITPAR beside them), its two texts, k = 0..5 and
    the long-piece sets: the sorted records equal the oracle's positions per pattern."""
    r = subprocess.run([os.sys.executable, "-c", _FORM_WORKER, H.ROOT, os.path.join(H.ROOT, "tests")],
                       capture_output=True, env=dict(os.environ, **env), timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = json.loads(r.stdout.decode().strip().splitlines()[-1])
    texts = {}
    for name, alphabet, n in (("dna", b"ACGT", 300000), ("prose", b"etaoin shrdlucETAOIN\n.,", 200000)):
        trng = random.Random(name)
        texts[name] = bytes(bytearray(trng.choice(alphabet) for _ in range(n)))
    assert len(got) == 18
    for key, res in got.items():
        name, k = key.split(":")[0], int(key.split(":")[1])
        if key.endswith(":long") and env.get("APM_SIEVE") != "0":
            assert res["sieve_stride"] == 8 and res["sieve_fused"] == (0 if env.get("APM_FUSED") == "0" else 1), (key, env)
        pats = [p.encode("latin-1") for p in res["patterns"]]
        assert res["kernels"] == [auto_kernel(p, k) for p in pats], key
        want = ref_records(texts[name], pats, k)
        assert [tuple(x) for x in res["records"]] == want, (key, env)
        assert res["n_found"] == sum(res["counts"]) == len(want), (key, env)
        assert len(want) >= 1, key


@gpu
@pytest.mark.parametrize("variant", ["bitpar", "wavefront", "generic", "nfa", "banded"])
def test_forced_variants_records_equal_oracle(ctx, variant):
    """the forced variant's kernels feed the sink too: BITPAR at 1-4 words, WAVEFRONT, GENERIC, NFA, BANDED on one text
    with occurrences planted at its very end (truncated tail windows match)"""
    rng = random.Random(99)
    k = 2
    pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in (12, 20, 29)]
    if variant not in ("nfa",):
        pats += [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in (40, 70, 100, 128)]
    text = bytearray(rng.choice(b"ACGT") for _ in range(30000))
    for i, p in enumerate(pats):
        for o in (1000 + 997 * i, 20001 + 313 * i):
            text[o:o + len(p)] = p
    text[len(text) - 9:] = pats[0][:9]           # truncated copies at the end of the text
    text = bytes(text)
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    ctx.set_kernel(variant)
    try:
        want = check_complete(ctx, text, pats, k)
        assert len(want) >= 2 * len(pats) and any(j + len(pats[i]) > len(text) for i, j in want)
    finally:
        ctx.set_kernel("auto")


# ---------------------------------------------------------------- 2. one mixed set, all families at once
def _mixed(k, lens, n, seed):
    rng = random.Random(seed)
    pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in lens]
    text = bytearray(rng.choice(b"ACGT") for _ in range(n))
    at = 500
    for p in pats:
        w = bytearray(p)
        if len(w) > 8 and k >= 1:
            w[len(w) // 2] = ord("A") if w[len(w) // 2] != ord("A") else ord("C")  # one substitution
        text[at:at + len(w)] = w
        at += len(w) + 211
    assert at < n - 5000
    cut = min(1200, len(pats[-1]) * 2 // 3)              # the text ends in a truncated copy of the last (longest) pattern
    text[n - cut:] = pats[-1][:cut]
    return pats, bytes(text)


@gpu
def test_mixed_set_routed_to_all_families(ctx):
    """One AUTO set at k = 3: BANDED-short (20), BANDED-long (300), NFA (13), a duplicate of the NFA pattern, a trivial
    pattern (m = 2 <= k: every window), BITPAR at 513-1024 (700) and 1025-4096 (1500), GENERIC (4200), with occurrences and
    truncated copies at the very end of the text.  AUTO sends no pattern of 129..512 bytes to BITPAR while k <= 7 (BANDED
    takes them), so that class runs in a second set at k = 8, beside BITPAR at 1-4 words."""
    k = 3
    pats, text = _mixed(k, (20, 300, 13, 700, 1500, 4200), 40000, 5)
    pats = pats[:3] + [pats[2], b"GA"] + pats[3:]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    assert [ctx.pattern_kernel(i) for i in range(len(pats))] == [auto_kernel(p, k) for p in pats] == [4, 4, 5, 5, 0, 3, 3, 1]
    want = check_complete(ctx, text, pats, k)
    per = [sum(1 for i, _ in want if i == q) for q in range(len(pats))]
    assert all(c >= 1 for c in per) and per[2] == per[3] and per[4] == len(text) - k
    assert any(j + len(pats[i]) > len(text) for i, j in want if i != 4)     # truncated tail windows among the records
    k = 8
    pats, text = _mixed(k, (40, 100, 200, 300, 512), 30000, 6)
    ctx.set_patterns(pats, k)
    assert [ctx.pattern_kernel(i) for i in range(len(pats))] == [3] * 5
    want = check_complete(ctx, text, pats, k)
    assert all(any(i == q for i, _ in want) for q in range(len(pats)))


# ---------------------------------------------------------------- 3. dense matches
def _dense_ref(text, pats, k):
    return [(i, j) for i, p in enumerate(pats) for j in H.oracle_positions(text, p, k)]


@gpu
@pytest.mark.parametrize("name,k,pats", [
    ("polyA-banded-nfa", 2, [b"A" * 20, b"A" * 9, b"AAAAAAAAAAAAAAAAAAAC"]),   # every window matches, three kernels
    ("polyA-bitpar", 9, [b"A" * 40, b"A" * 33 + b"CCCCCCC"]),
    ("tandem", 2, [b"ACGTACGTACGTACGTACGT", b"ACGTACGTA", b"CGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACG"]),
])
def test_dense_matches(ctx, name, k, pats):
    text = (b"A" * 12000) if name.startswith("polyA") else (b"ACGT" * 3000)
    want = _dense_ref(text, pats, k)
    if name.startswith("polyA"):                                            # a pattern that matches at every window start
        assert sum(1 for i, _ in want if i == 0) == len(text) - k
    assert len(want) > len(text) // 2
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    got, total = ctx.find_all_buffer(text, len(want) + 1000)               # ample capacity: the complete set
    assert total == len(want) == sum(ctx.count_buffer(text)) and got == want
    cap = 97                                                               # far below n_found
    got, total = ctx.find_all_buffer(text, cap)
    assert total == len(want) and len(got) == cap
    assert len(set(got)) == cap and set(got) <= set(want) and got == sorted(got)
    got, total = ctx.find_all_buffer(text, 0)                              # out == NULL, capacity == 0: a total count
    assert got == [] and total == len(want)


# ---------------------------------------------------------------- 4. the plan is untouched, one pass
@gpu
def test_plan_untouched_and_one_pass(ctx):
    c = next(c for c in CASES if c["name"] == "chrY_k3")
    text, pats, k = H.case_text(c), c["patterns"], c["k"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)

    def state():
        return (ctx.stat("sieve_on"), ctx.stat("sieve_stride"), [ctx.pattern_kernel(i) for i in range(len(pats))])

    before = ctx.count_buffer(text)
    t_count = ctx.timing()
    s0 = state()
    got, total = ctx.find_all_buffer(text, sum(before) + 8)
    t_find = ctx.timing()
    assert state() == s0
    assert ctx.count_buffer(text) == before == c["counts"]
    assert total == sum(before) and len(got) == total
    assert t_find["n_launches"] == t_count["n_launches"] >= 1            # the same launches: one pass
    assert t_find["text_bytes"] == t_count["text_bytes"] == ctx.timing()["text_bytes"]


# ---------------------------------------------------------------- 5. the shard API
def _shard_case(n, seed):
    """n bytes of random DNA, seven patterns of 16..128 bytes (BANDED at k = 3: the sieve pipeline on aligned text, the
    tile / stream kernels on unaligned), each planted a few times with one substitution; a truncated copy at the end"""
    rng = random.Random(seed)
    k = 3
    pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in (16, 24, 33, 50, 64, 100, 128)]
    text = bytearray(rng.choice(b"ACGT") for _ in range(n))
    for i, p in enumerate(pats):
        for o in range(1000 + 977 * i, n - 200, n // 5 + 131 * i):
            w = bytearray(p)
            w[len(w) // 3] = ord("A") if w[len(w) // 3] != ord("A") else ord("G")
            text[o:o + len(w)] = w
    text[n - 40:] = pats[-1][:40]
    return pats, k, bytes(text)


def _download_records(apm, ctx, d_out, d_n, cap):
    n = int.from_bytes(ctx.device_download(d_n, 8), "little")
    raw = ctx.device_download(d_out, 16 * min(n, cap)) if min(n, cap) else b""
    arr = (apm.ApmMatch * min(n, cap)).from_buffer_copy(raw)
    assert all(r.reserved == 0 for r in arr)
    return [(r.pattern, r.pos) for r in arr], n


@gpu
@pytest.mark.parametrize("misalign", [0, 3])
def test_shard_api_appends_into_one_buffer(apm, ctx, misalign):
    """owner ranges cut at positions that are no multiples of 16, every shard with its own device text (halo included),
    appended into ONE record buffer: the union is the whole-text set, nothing twice at a seam; d_counts is filled.
    misalign = 3: a text pointer off the 16-byte grid (the tile / stream fallback of the sieve pipeline)."""
    pats, k, text = _shard_case(200000, 17)
    n = len(text)
    want = ref_records(text, pats, k)
    assert all(sum(1 for q, _ in want if q == i) >= 3 for i in range(len(pats)))
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    halo = max(len(p) for p in pats) - 1
    cuts = [0, 4099, n // 4 + 1, n // 4 + 2, (2 * n // 3) | 3, n]        # (one shard of a single window start)
    assert cuts == sorted(set(cuts)) and all(c % 16 for c in cuts[1:-1])
    cap = len(want) + 16
    d_out, d_n, d_counts = ctx.device_alloc(16 * cap), ctx.device_alloc(16), ctx.device_alloc(8 * len(pats))
    ctx.device_memset(d_n, 0, 16)
    ctx.device_memset(d_counts, 0, 8 * len(pats))
    bufs = []
    try:
        for ob, oe in zip(cuts, cuts[1:]):
            hi = min(n, oe + halo)
            d = ctx.device_alloc(hi - ob + 32)
            bufs.append(d)
            ctx.device_upload(d + misalign, text[ob:hi])
            ctx.find_shard_device(d + misalign, ob, hi - ob, n, ob, oe, d_out, cap, d_n, d_counts)
        ctx.synchronize()
        got, total = _download_records(apm, ctx, d_out, d_n, cap)
        assert total == len(want) and len(set(got)) == len(got)             # no duplicate at any seam
        assert sorted(got) == want
        cnt = ctx.device_download(d_counts, 8 * len(pats))
        assert [int.from_bytes(cnt[8 * i:8 * i + 8], "little") for i in range(len(pats))] == [sum(1 for q, _ in want if q == i) for i in range(len(pats))]
        # without d_counts, appended behind what is there; capacity exhausted: the counter still counts
        ctx.find_shard_device(bufs[0] + misalign, 0, min(n, cuts[1] + halo), n, 0, cuts[1], d_out, cap, d_n, None)
        ctx.synchronize()
        got2, total2 = _download_records(apm, ctx, d_out, d_n, cap)
        first = [r for r in want if r[1] < cuts[1]]
        assert total2 == total + len(first) and got2[:len(got)] == got
        extra = got2[len(got):]
        assert len(got2) == min(cap, total2) and len(set(extra)) == len(extra) and set(extra) <= set(first)
    finally:
        for d in bufs + [d_out, d_n, d_counts]:
            ctx.device_free(d)


@gpu
def test_shard_beyond_4gib_has_64_bit_positions(apm, ctx):
    """only text_off is large: a 64 KiB shard of a (virtual) text of 5 GiB + 64 KiB"""
    rng = random.Random(4)
    pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in (24, 90, 14)]
    k = 3
    text = bytearray(rng.choice(b"ACGT") for _ in range(65536))
    for i, p in enumerate(pats):
        text[3000 + 7001 * i:3000 + 7001 * i + len(p)] = p
    text[-10:] = pats[0][:10]
    text = bytes(text)
    off = (5 << 30) + 48
    want = [(i, j + off) for i, j in ref_records(text, pats, k)]
    assert len(want) >= 4
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    d_text, d_out, d_n = ctx.device_alloc(len(text) + 16), ctx.device_alloc(16 * 256), ctx.device_alloc(16)
    try:
        ctx.device_upload(d_text, text)
        ctx.device_memset(d_n, 0, 16)
        ctx.find_shard_device(d_text, off, len(text), off + len(text), off, off + len(text), d_out, 256, d_n, None)
        ctx.synchronize()
        got, total = _download_records(apm, ctx, d_out, d_n, 256)
        assert total == len(want) and sorted(got) == want and all(pos > 1 << 32 for _, pos in got)
    finally:
        for d in (d_text, d_out, d_n):
            ctx.device_free(d)


@gpu
def test_shard_api_on_a_caller_stream(apm):
    import torch
    pats, k, text = _shard_case(150000, 18)
    want = ref_records(text, pats, k)
    assert len(want) >= 3 * len(pats)
    n = len(text)
    with apm.ApmContext(device=0) as cx:
        cx.set_patterns(pats, k)
        stream = torch.cuda.Stream(device="cuda:0")
        with torch.cuda.stream(stream):
            t = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
            t[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to("cuda:0")
            out = torch.zeros(2 * (len(want) + 8), dtype=torch.int64, device="cuda:0")
            nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
            cnt = torch.zeros(len(pats), dtype=torch.int64, device="cuda:0")
            cx.set_stream(stream.cuda_stream)
            cx.set_timing(False)
            for s in range(2):                                             # two shards, one buffer, stream order alone
                ob, oe = apm.shard_range(n, k, s, 2)
                cx.find_shard_device(t.data_ptr(), 0, n, n, ob, oe, out.data_ptr(), len(want) + 8, nf.data_ptr(), cnt.data_ptr())
        stream.synchronize()
        cx.set_stream(None)
        total = int(nf[0].item())
        rec = out.cpu().tolist()
        got = sorted((rec[2 * i + 1] & 0xffffffff, rec[2 * i]) for i in range(total))
        assert total == len(want) and got == want
        assert cnt.cpu().tolist() == [sum(1 for q, _ in want if q == i) for i in range(len(pats))]


# ---------------------------------------------------------------- 6. multi-device contexts, rehearsed on one GPU
@gpu
@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
@pytest.mark.parametrize("partition", ["text", "patterns"])
def test_multi_device_records_equal_single_device(apm, ctx, devices, partition):
    k = 3
    pats, text = _mixed(k, (20, 300, 13, 700, 1500), 50000, 8)
    pats.append(pats[0])
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    single, total1 = ctx.find_all_buffer(text, 4096)
    assert single == ref_records(text, pats, k) and total1 == len(single)
    os.environ["APM_DEVICES"] = devices
    try:
        m = apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]
    with m:
        m.set_partition(partition)
        m.set_patterns(pats, k)
        got, total = m.find_all_buffer(text, 4096)
        assert total == total1 and got == single                          # sorted, nothing twice at a seam
        assert len(set(got)) == len(got)
        assert m.count_buffer(text) == ctx.count_buffer(text)
        assert m.timing()["n_devices"] == len(devices.split(","))


# ---------------------------------------------------------------- 7. golden files
@gpu
@pytest.mark.parametrize("name", ["cfg1_basic_test", "chrY_k3"])
def test_golden_counts_and_find_buffer_positions(ctx, name):
    c = next(c for c in CASES if c["name"] == name)
    text, pats, k = H.case_text(c), c["patterns"], c["k"]
    ctx.set_kernel("auto")
    ctx.set_patterns(pats, k)
    got, total = ctx.find_all_buffer(text, sum(c["counts"]) + 8)
    assert total == sum(c["counts"])
    for i in range(len(pats)):
        mine = [pos for q, pos in got if q == i]
        assert len(mine) == c["counts"][i]
        old, old_total = ctx.find_buffer(text, i, capacity=max(1, c["counts"][i]) + 8)
        assert old_total == c["counts"][i] and mine == old
