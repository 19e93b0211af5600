"""Measurement aid (GPU box): what the best-hit pass costs against the scoring pass on the same records.

    python tools/best_probe.py [--runs 7] [--out FILE]

Two inputs, HIP-event times after a warm-up, median of --runs, the radius r = k:
  cfg3   cfg3's patterns on 1 GiB of synthetic text through the host calls: apm_find_all_dist_buffer against
         apm_find_best_buffer, kernel_ms of each, the "score" launch of the one and the "best" launch of the other
         (apm_get_launch_times).  About 10^4 records.
  dense  64 MiB of random DNA, 600 patterns of 20 bytes, k = 3 (tools/density_probe.py's set), records kept on the device:
         apm_find_shard_device, then apm_score_shard_device and apm_best_shard_device over its buffer, kernel_ms of each.
The pass walks at most 2 r + 1 windows per record where the scoring pass walks one, fewer with the early exit.
"""
import argparse
import ctypes
import importlib
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "inf560-approximate-pattern-matching_amd"
sys.path.insert(0, ROOT)


def med(v):
    return "%.4f [%.4f, %.4f]" % (statistics.median(v), min(v), max(v))


def probe_cfg3(apm, wl, runs, say):
    c = wl.CONFIGS["cfg3"]
    n, k, seed = 1 << 30, c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    buf = ctypes.create_string_buffer(n)
    apm.load_library().apm_synth_fill_host(ctypes.cast(buf, ctypes.c_void_p), 0, n, seed)
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    cap = 1 << 20
    out = (apm.ApmMatch * cap)()
    found, n_best = ctypes.c_uint64(), ctypes.c_uint64()
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        res = {"dist": [], "best": [], "score_launch": [], "best_launch": []}
        for it in range(2 + runs):                                # two warm-ups; the two calls alternate
            ctx._check(ctx._lib.apm_find_all_dist_buffer(ctx._ctx, ptr, n, out, cap, ctypes.byref(found)))
            if it >= 2:
                res["dist"].append(ctx.timing()["kernel_ms"])
                res["score_launch"] += [t for l, t in ctx.launch_times() if l == "score"]
            ctx._check(ctx._lib.apm_find_best_buffer(ctx._ctx, ptr, n, k, out, cap, ctypes.byref(n_best), ctypes.byref(found), None, 0))
            if it >= 2:
                res["best"].append(ctx.timing()["kernel_ms"])
                res["best_launch"] += [t for l, t in ctx.launch_times() if l == "best"]
        say("cfg3  1 GiB, %d patterns, k = %d, r = %d: %d records, %d best hits" % (len(pats), k, k, found.value, n_best.value))
        say("cfg3  apm_find_all_dist_buffer kernel_ms %s   of which the \"score\" launch %s" % (med(res["dist"]), med(res["score_launch"])))
        say("cfg3  apm_find_best_buffer     kernel_ms %s   of which the \"best\" launch  %s" % (med(res["best"]), med(res["best_launch"])))


def probe_dense(apm, runs, say):
    import torch
    P, m, k, n = 600, 20, 3, 64 << 20
    rnd = random.Random(7)
    g = torch.Generator().manual_seed(1)
    host = torch.tensor(list(b"ACGT"), dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]
    tb = host.numpy().tobytes()
    pats = []
    for _ in range(P):
        o = rnd.randrange(0, n - m)
        p = bytearray(tb[o:o + m])
        for _e in range(rnd.randrange(0, k + 1)):
            p[rnd.randrange(m)] = rnd.choice(b"ACGT")
        pats.append(bytes(p))
    text = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    text[:n] = host.to("cuda:0")
    cap = 1 << 20
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    kept = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    nk = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        res = {"find": [], "score": [], "best": []}
        for it in range(2 + runs):
            nf.zero_()
            nk.zero_()
            torch.cuda.synchronize()
            ctx.find_shard_device(text.data_ptr(), 0, n, n, 0, n, rec.data_ptr(), cap, nf.data_ptr(), None)
            ctx.synchronize()
            t_find = ctx.timing()["kernel_ms"]
            ctx.score_shard_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr())
            ctx.synchronize()
            t_score = ctx.timing()["kernel_ms"]
            ctx.best_shard_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr(), k, kept.data_ptr(), cap, nk.data_ptr())
            ctx.synchronize()
            t_best = ctx.timing()["kernel_ms"]
            if it >= 2:
                res["find"].append(t_find)
                res["score"].append(t_score)
                res["best"].append(t_best)
        say("dense 64 MiB, %d patterns of %d bytes, k = %d, r = %d: %d records, %d best hits" % (P, m, k, k, int(nf[0].item()), int(nk[0].item())))
        say("dense apm_find_shard_device    kernel_ms %s" % med(res["find"]))
        say("dense apm_score_shard_device   kernel_ms %s" % med(res["score"]))
        say("dense apm_best_shard_device    kernel_ms %s" % med(res["best"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    probe_cfg3(apm, wl, a.runs, say)
    probe_dense(apm, a.runs, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
