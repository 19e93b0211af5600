"""The device-level entry points refuse what they refuse, in the words they use, and a refused call leaves the context
usable: apm_count_shard_device, apm_find_shard_device, apm_score_shard_device, apm_align_shard_device,
apm_map_positions_device and apm_normalize_device, each driven through every refusal it has -- status and, where one is
set, message -- and then one valid count, find, score and align on the same context against the oracle."""
import ctypes
import os
import random
import struct

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

OK, INVALID, STATE = 0, -1, -8
EQ, SUB, INS, DEL = range(4)
N, K = 256, 2
NO_PATTERNS = "apm_set_patterns has not been called"
NULL_PTR = "NULL device pointer"
SHARD = "inconsistent shard description"


def make_case():
    """256 bytes of ACGT with copies of two 12-byte patterns at 0, 1 and 2 edits, one of them cut by the end of the text"""
    rng = random.Random(2024)
    pats = [bytes(rng.choice(b"ACGT") for _ in range(12)) for _ in range(2)]
    text = bytearray(rng.choice(b"ACGT") for _ in range(N))
    for at, (i, edits) in zip((9, 40, 77, 120, 163, 201), ((0, 0), (1, 1), (0, 2), (1, 0), (0, 1), (1, 2))):
        w = bytearray(pats[i])
        for e in rng.sample(range(12), edits):
            w[e] = rng.choice([c for c in b"ACGT" if c != w[e]])
        text[at:at + 12] = w
    text[N - 7:] = pats[0][:7]
    return pats, bytes(text)


def window(text, p, j):
    size = min(len(p), len(text) - j)
    return p[:size], text[j:j + size]


def apply_script(p, t, ops):
    """the window the script makes of the pattern, and its number of edits"""
    out, x, y = bytearray(), 0, 0
    for op in ops:
        if op == EQ:
            assert p[y] == t[x]
        if op != DEL:
            out.append(t[x])
        x += op != DEL
        y += op != INS
    assert y == len(p) and x == len(t)
    return bytes(out), sum(1 for op in ops if op != EQ)


class Calls:
    """the six entry points over one context and one set of device buffers; every argument has its valid default, a
    refusal case overrides the one it is about"""

    def __init__(self, apm, ctx, bufs):
        self.lib, self.ctx, self.b = apm.load_library(), ctx, bufs
        self.stride = 8

    def last_error(self):
        return (self.lib.apm_last_error(self.ctx._ctx) or b"").decode()

    def _shard(self, a):
        return (ctypes.c_void_p(a.get("d_text", self.b["text"])), a.get("text_off", 0), a.get("text_len", N), a.get("n_total", N))

    def count(self, **a):
        return self.lib.apm_count_shard_device(a.get("ctx", self.ctx._ctx), *self._shard(a), a.get("own_begin", 0), a.get("own_end", N),
                                               ctypes.c_void_p(a.get("d_counts", self.b["counts"])))

    def find(self, **a):
        return self.lib.apm_find_shard_device(a.get("ctx", self.ctx._ctx), *self._shard(a), a.get("own_begin", 0), a.get("own_end", N),
                                              ctypes.c_void_p(a.get("d_rec", self.b["rec"])), a.get("capacity", N * 2),
                                              ctypes.c_void_p(a.get("d_n", self.b["n"])), ctypes.c_void_p(a.get("d_counts", self.b["counts"])))

    def score(self, **a):
        return self.lib.apm_score_shard_device(a.get("ctx", self.ctx._ctx), *self._shard(a), ctypes.c_void_p(a.get("d_rec", self.b["rec"])),
                                               a.get("capacity", N * 2), ctypes.c_void_p(a.get("d_n", self.b["n"])))

    def align(self, **a):
        return self.lib.apm_align_shard_device(a.get("ctx", self.ctx._ctx), *self._shard(a), ctypes.c_void_p(a.get("d_rec", self.b["rec"])),
                                               a.get("capacity", N * 2), ctypes.c_void_p(a.get("d_n", self.b["n"])),
                                               ctypes.c_void_p(a.get("d_ops", self.b["ops"])), a.get("stride", self.stride))

    def map_positions(self, **a):
        return self.lib.apm_map_positions_device(a.get("ctx", self.ctx._ctx), ctypes.c_void_p(a.get("d_rec", self.b["rec"])),
                                                 a.get("capacity", N * 2), ctypes.c_void_p(a.get("d_n", self.b["n"])))

    def normalize(self, **a):
        out_len = ctypes.c_uint64()
        return self.lib.apm_normalize_device(a.get("ctx", self.ctx._ctx), ctypes.c_void_p(a.get("d_src", self.b["text"])), a.get("src_len", N),
                                             a.get("flags", 3), ctypes.c_void_p(a.get("d_dst", self.b["dst"])), a.get("dst_capacity", N),
                                             None if a.get("no_out_len") else ctypes.byref(out_len))


def refused(calls, name, status, message, **args):
    rc = getattr(calls, name)(**args)
    assert rc == status, (name, args, rc, calls.last_error())
    if message is not None:
        assert calls.last_error() == message, (name, args)


SHARD_CALLS = ("count", "find", "score", "align")
ENTRY = {"count": "apm_count_shard_device", "find": "apm_find_shard_device", "score": "apm_score_shard_device",
         "align": "apm_align_shard_device", "map_positions": "apm_map_positions_device", "normalize": "apm_normalize_device"}


def test_refusals_then_one_valid_call_of_each():
    apm = H.pkg()
    assert apm.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    pats, text = make_case()
    with apm.ApmContext(device=0) as ctx:
        bufs = {"text": ctx.device_alloc(N + 16), "dst": ctx.device_alloc(N + 16), "counts": ctx.device_alloc(16),
                "rec": ctx.device_alloc(16 * N * 2 + 16), "n": ctx.device_alloc(16), "ops": ctx.device_alloc(4 * 64 * N * 2)}
        ctx.device_upload(bufs["text"], text)
        calls = Calls(apm, ctx, bufs)

        # ---- no context: the status alone
        for name in ENTRY:
            assert getattr(calls, name)(ctx=None) == INVALID, name

        # ---- patterns not set (the two text-mode calls take no pattern set)
        for name in SHARD_CALLS:
            refused(calls, name, STATE, NO_PATTERNS)
        refused(calls, "map_positions", STATE, "no text has been normalised on this context")

        # ---- a two-shard context (APM_DEVICES as test_multi_device_context_rehearsed_on_one_gpu sets it): the entry point's own name
        os.environ["APM_DEVICES"] = "0,0"
        try:
            two = apm.ApmContext(n_devices=0)
        finally:
            del os.environ["APM_DEVICES"]
        try:
            two.set_patterns(pats, K)
            for name, entry in ENTRY.items():
                refused(Calls(apm, two, bufs), name, STATE, entry + " needs a single-device context")
        finally:
            two.close()

        ctx.set_patterns(pats, K)
        calls.stride = ctx.align_row_words()
        assert calls.stride >= 2

        # ---- every required pointer NULL
        refused(calls, "count", INVALID, NULL_PTR, d_counts=None)
        for name in SHARD_CALLS:
            refused(calls, name, INVALID, NULL_PTR, d_text=None)
        for name in ("find", "score", "align", "map_positions"):
            refused(calls, name, INVALID, NULL_PTR, d_n=None)
            refused(calls, name, INVALID, NULL_PTR, d_rec=None)
        refused(calls, "align", INVALID, NULL_PTR, d_ops=None)
        refused(calls, "normalize", INVALID, "NULL pointer", no_out_len=True)
        refused(calls, "normalize", INVALID, "NULL pointer", d_src=None)
        refused(calls, "normalize", INVALID, "NULL pointer", d_dst=None)

        # ---- alignment of the record buffer and of the rows, the stride, the flags
        refused(calls, "find", INVALID, "d_out must be 16-byte aligned", d_rec=bufs["rec"] + 8)
        for name in ("score", "align", "map_positions"):
            refused(calls, name, INVALID, "d_rec must be 16-byte aligned", d_rec=bufs["rec"] + 8)
        refused(calls, "align", INVALID, "d_ops must be 4-byte aligned", d_ops=bufs["ops"] + 2)
        refused(calls, "align", INVALID, "stride_words %d is less than apm_align_row_words() = %d" % (calls.stride - 1, calls.stride),
                stride=calls.stride - 1)
        refused(calls, "normalize", INVALID, "text mode flags 0x0: need APM_TEXT_FASTA and / or APM_TEXT_UPPER", flags=0)
        refused(calls, "normalize", INVALID, "text mode flags 0x4: need APM_TEXT_FASTA and / or APM_TEXT_UPPER", flags=4)

        # ---- the shard description
        for name in SHARD_CALLS:
            refused(calls, name, INVALID, SHARD, text_off=1)                    # text_off + text_len > n_total
            refused(calls, name, INVALID, SHARD, n_total=N - 1)
        for name in ("count", "find"):
            refused(calls, name, INVALID, SHARD, own_begin=17, own_end=16)
            # (the scan's own: the call has begun when it refuses these)
            refused(calls, name, INVALID, "shard text starts after own_begin", text_off=16, text_len=N - 16, own_begin=0)
            refused(calls, name, INVALID, "shard text too short: halo of m_max-1 = 11 bytes required", text_len=100, own_end=100)
        refused(calls, "normalize", INVALID, "the normalised text has %d bytes, the destination holds 8" % N, dst_capacity=8)

        # ---- no capacity: no record pointer is needed
        ctx.device_memset(bufs["n"], 0, 16)
        ctx.device_memset(bufs["counts"], 0, 16)
        assert calls.find(d_rec=None, capacity=0) == OK, calls.last_error()
        assert calls.score(d_rec=None, capacity=0) == OK, calls.last_error()
        assert calls.align(d_rec=None, d_ops=None, capacity=0) == OK, calls.last_error()
        refused(calls, "map_positions", STATE, "no text has been normalised on this context", d_rec=None, capacity=0)
        assert calls.normalize() == OK, calls.last_error()
        assert calls.map_positions(d_rec=None, capacity=0) == OK, calls.last_error()
        ctx.synchronize()
        want_pos = [H.oracle_positions(text, p, K) for p in pats]
        want_counts = H.oracle_counts(text, pats, K)
        assert want_counts == [len(w) for w in want_pos] and min(want_counts) >= 3
        # (capacity 0 counts and numbers the matches, it stores none)
        assert list(struct.unpack("<2Q", ctx.device_download(bufs["counts"], 16))) == want_counts
        assert struct.unpack("<Q", ctx.device_download(bufs["n"], 8))[0] == sum(want_counts)

        # ---- after all of that: one valid call of each, against the oracle
        ctx.device_memset(bufs["counts"], 0, 16)
        assert calls.count() == OK, calls.last_error()
        ctx.synchronize()
        assert list(struct.unpack("<2Q", ctx.device_download(bufs["counts"], 16))) == want_counts
        ctx.device_memset(bufs["counts"], 0, 16)
        ctx.device_memset(bufs["n"], 0, 16)
        ctx.device_memset(bufs["ops"], 0x5A, 4 * 64 * N * 2)
        assert calls.find() == OK, calls.last_error()
        assert calls.score() == OK, calls.last_error()
        assert calls.align() == OK, calls.last_error()
        ctx.synchronize()
        total = struct.unpack("<Q", ctx.device_download(bufs["n"], 8))[0]
        assert total == sum(want_counts)
        assert list(struct.unpack("<2Q", ctx.device_download(bufs["counts"], 16))) == want_counts
        raw = ctx.device_download(bufs["rec"], 16 * total)
        rows = struct.unpack("<%dI" % (calls.stride * total), ctx.device_download(bufs["ops"], 4 * calls.stride * total))
        got = sorted((pat, pos, dist, apm.unpack_ops(rows[r * calls.stride:(r + 1) * calls.stride]))
                     for r, (pos, pat, dist) in enumerate(struct.unpack_from("<QII", raw, 16 * r) for r in range(total)))
        assert [(i, j) for i, j, _, _ in got] == [(i, j) for i, w in enumerate(want_pos) for j in w]
        for i, j, dist, ops in got:
            p, t = window(text, pats[i], j)
            assert dist == H.window_distance(p, t) <= K, (i, j)
            assert apply_script(p, t, ops) == (t, dist), (i, j)
        for d in bufs.values():
            ctx.device_free(d)
