"""Measurement aid (GPU box): what the scoring pass costs on top of the plain find call.

    python tools/score_probe.py [--runs 7] [--out profiles/r04/score_probe.txt]

Two inputs, HIP-event times after a warm-up, median of --runs:
  cfg3   cfg3's patterns on 1 GiB of synthetic text through the host calls: apm_find_all_buffer against
         apm_find_all_dist_buffer, kernel_ms of each and the "score" launch of the latter (apm_get_launch_times).
         Matches are rare there (about 10^4): the pass should cost little more than an empty launch.
  polyA  the adversarial case, 64 MiB of 'A' against A*20 at k = 3: every window is a record (67 M of them), so the
         records stay on the device: apm_find_shard_device, then apm_score_shard_device over its buffer, kernel_ms of each
         (the scoring call's kernel_ms is its one launch).
"""
import argparse
import ctypes
import importlib
import os
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
    cap = 1 << 20
    out = (apm.ApmMatch * cap)()
    found = ctypes.c_uint64()
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        res = {"find": [], "dist": [], "score": []}
        for it in range(2 + runs):                                # two warm-ups; the two calls alternate
            for mode in ("find", "dist"):
                fn = ctx._lib.apm_find_all_dist_buffer if mode == "dist" else ctx._lib.apm_find_all_buffer
                ctx._check(fn(ctx._ctx, ctypes.cast(buf, ctypes.c_void_p), n, out, cap, ctypes.byref(found)))
                if it < 2:
                    continue
                res[mode].append(ctx.timing()["kernel_ms"])
                if mode == "dist":
                    res["score"] += [t for l, t in ctx.launch_times() if l == "score"]
        nonzero = sum(1 for i in range(min(found.value, cap)) if out[i].reserved)
        say("cfg3  1 GiB, %d patterns, k = %d, %d records (%d at distance >= 1)" % (len(pats), k, found.value, nonzero))
        say("cfg3  apm_find_all_buffer      kernel_ms %s" % med(res["find"]))
        say("cfg3  apm_find_all_dist_buffer kernel_ms %s   of which the \"score\" launch %s" % (med(res["dist"]), med(res["score"])))


def probe_polya(apm, runs, say):
    import torch
    n, k = 64 << 20, 3
    pats = [b"A" * 20]
    text = torch.full((n + 4096,), ord("A"), dtype=torch.uint8, device="cuda:0")
    cap = n
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        res = {"find": [], "score": []}
        for it in range(2 + runs):
            nf.zero_()
            torch.cuda.synchronize()
            ctx.find_shard_device(text.data_ptr(), 0, n, n, 0, n, rec.data_ptr(), cap, nf.data_ptr(), None)
            ctx.synchronize()
            t_find = ctx.timing()["kernel_ms"]
            ctx.score_shard_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr())
            ctx.synchronize()
            t_score = ctx.timing()["kernel_ms"]
            if it >= 2:
                res["find"].append(t_find)
                res["score"].append(t_score)
        records = int(nf[0].item())
        dist = rec.view(torch.int32)[3:4 * records:4]
        say("polyA 64 MiB of 'A', A*20, k = %d, %d records, distances all 0: %s" % (k, records, bool((dist == 0).all().item())))
        say("polyA apm_find_shard_device    kernel_ms %s" % med(res["find"]))
        say("polyA apm_score_shard_device   kernel_ms %s   (find + score %.4f)" % (
            med(res["score"]), statistics.median(res["find"]) + statistics.median(res["score"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04", "score_probe.txt"))
    a = ap.parse_args()
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    probe_cfg3(apm, wl, a.runs, say)
    probe_polya(apm, a.runs, say)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
