"""Shared test helpers: package import, oracle binding, golden vectors.

The oracle (oracle/liboracle.so) is the CHECKER; it is only ever loaded here,
in __graft_entry__.smoke() and in bench.py's cpu_baseline leg.
"""
import base64
import ctypes
import hashlib
import importlib
import json
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "inf560-approximate-pattern-matching_amd"
PKG_DIR = os.path.join(ROOT, PKG_NAME)
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
REF_UTILS_SO = os.path.join(ROOT, "oracle", "_ref", "libref_utils.so")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "apm_sequential")


def pkg():
    return importlib.import_module(PKG_NAME)


def workloads():
    return importlib.import_module(PKG_NAME + ".workloads")


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        if not os.path.exists(ORACLE_SO):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "liboracle.so"], check=True)
        lib = ctypes.CDLL(ORACLE_SO)
        c = ctypes
        lib.oracle_window_distance.restype = c.c_int
        lib.oracle_window_distance.argtypes = [c.c_char_p, c.c_char_p, c.c_int, c.POINTER(c.c_int)]
        for name in ("oracle_count_range_mt", "oracle_count_range_banded_mt"):
            fn = getattr(lib, name)
            fn.restype = c.c_int64
            fn.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p, c.c_int, c.c_int, c.c_uint64, c.c_uint64, c.c_int]
        lib.oracle_count.restype = c.c_int64
        lib.oracle_count.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p, c.c_int, c.c_int]
        lib.oracle_count_range.restype = c.c_int64
        lib.oracle_count_range.argtypes = [c.c_char_p, c.c_uint64, c.c_char_p, c.c_int, c.c_int, c.c_uint64, c.c_uint64]
        lib.oracle_max_threads.restype = c.c_int
        _oracle = lib
    return _oracle


def oracle_counts(text, patterns, k, banded=False, threads=0, j_begin=0, j_end=None):
    lib = oracle()
    fn = lib.oracle_count_range_banded_mt if banded else lib.oracle_count_range_mt
    n = len(text)
    if j_end is None:
        j_end = n
    out = []
    for p in patterns:
        r = fn(text, n, p, len(p), k, j_begin, j_end, threads)
        assert r >= 0
        out.append(r)
    return out


def window_distance(p, t):
    m = len(p)
    col = (ctypes.c_int * (m + 1))()
    return oracle().oracle_window_distance(p, t, m, col)


def oracle_positions(text, p, k):
    """the matching window starts, one full DP per window (truncated at the end of the text like the reference's scan)"""
    n, m = len(text), len(p)
    out = []
    for j in range(0, max(0, n - k)):
        size = min(m, n - j)
        if window_distance(p[:size], text[j:j + size]) <= k:
            out.append(j)
    return out


def window_distance_pairs(seed=7, n=3000):
    """(pattern, window) pairs of tests/golden/window_distance.json: m in 1..140, three alphabets, up to 6
    substitutions and a rotation in 30 % of the windows."""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        m = rnd.randint(1, 140)
        alpha = rnd.choice([b"ab", b"ACGT", bytes(range(1, 256))])
        p = bytes(rnd.choice(alpha) for _ in range(m))
        t = bytearray(p)
        for _e in range(rnd.randint(0, 6)):
            t[rnd.randrange(m)] = rnd.choice(alpha)
        if rnd.random() < 0.3:
            s = rnd.randint(1, 3)
            t = t[s:] + t[:s]
        out.append((p, bytes(t)))
    return out


def pairs_digest(pairs):
    h = hashlib.sha256()
    for p, t in pairs:
        h.update(b"%d:" % len(p) + p + t)
    return h.hexdigest()


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(os.path.join(GOLDEN_DIR, "golden.json")) as f:
            g = json.load(f)
        for c in g["cases"]:
            c["patterns"] = [base64.b64decode(p) for p in c["patterns_b64"]]
            if "file" in c:
                c["path"] = os.path.join(GOLDEN_DIR, "dna", c["file"])
            else:
                c["text_bytes"] = base64.b64decode(c["text_b64"])
        _golden = g
    return _golden


def case_text(c):
    if "text_bytes" in c:
        return c["text_bytes"]
    with open(c["path"], "rb") as f:
        return f.read()


def case_cells(c):
    n = len(case_text(c)) if "text_bytes" in c else os.path.getsize(c["path"])
    return sum(max(0, n - c["k"]) * len(p) ** 2 for p in c["patterns"])


def plan_sets():
    """The pattern sets that pin the plan builder (tests/golden/plan_digests.json): (name, k, forced kernel, patterns)."""
    import numpy as np
    wl = workloads()
    K = pkg().KERNEL_IDS

    def rnd(seed, lens, alphabet=b"ACGT"):
        rs = np.random.RandomState(seed)
        a = np.frombuffer(alphabet, dtype=np.uint8)
        return [a[rs.randint(0, len(a), size=m)].tobytes() for m in lens]

    sets = []
    for name in ("cfg2", "cfg3", "cfg4", "cfg5"):  # as bench.py builds them on one GPU
        c = wl.CONFIGS[name]
        n = c["n"] // (8 if name in ("cfg4", "cfg5") else 1)
        sets.append((name, c["k"], K["auto"], wl.make_patterns(n, c["lens"], c["k"], wl.seed_of(c["cid"]))[0]))
    short = [8 + i % 7 for i in range(28)]
    sets.append(("short_k1", 1, K["auto"], rnd(101, short)))                      # window-DP slots
    sets.append(("short_k2", 2, K["auto"], rnd(102, short)))
    sets.append(("many20_k1", 1, K["auto"], rnd(103, [20] * 2000)))               # several verify launches, > 512 short tails
    sets.append(("alphabet_k2", 2, K["auto"], rnd(104, [16 + 3 * i for i in range(16)], b"0@P`")))  # bits 4..5 tell the letters apart: code_shift 4
    sets.append(("long_k8", 8, K["auto"], rnd(105, [129, 512, 513, 1024, 1025, 4096, 5000])))
    forced = rnd(106, [16, 20, 24, 28, 30])
    for v in ("wavefront", "nfa", "bitpar", "banded", "generic"):
        sets.append(("forced_" + v, 2, K[v], forced))
    sets.append(("k_ge_m", 5, K["auto"], rnd(107, [3, 5, 8, 40])))
    sets.append(("unsupported", 2, K["wavefront"], rnd(108, [20, 300])))
    return sets


def plan_sets_input():
    return "".join("%s %d %d %s\n" % (name, k, kern, " ".join(p.hex() for p in pats)) for name, k, kern, pats in plan_sets())
