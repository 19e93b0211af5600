"""Measurement aid (GPU box): what the align pass costs next to the scoring pass and the scan of the same call.

    python tools/align_probe.py [--runs 7] [--out profiles/r05/align_probe.txt]

HIP-event times per launch (apm_get_launch_times) after two warm-ups, median [min, max] of --runs:
  chrY   golden chrY_k3 through apm_find_all_align_buffer: the scan launches, "score" and "align" of one call
  cfg3   cfg3's patterns (32 patterns, m = 16 .. 128, k = 3) on 64 MiB of synthetic DNA, the same call
  polyA  the dense case, 16 MiB of 'A' against A*20 at k = 3: every window is a record, so the records stay on the
         device: apm_find_shard_device, apm_score_shard_device and apm_align_shard_device over one buffer, kernel_ms of each
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(v):
    return "%.4f [%.4f, %.4f]" % (statistics.median(v), min(v), max(v))


def probe_host_call(apm, name, text, pats, k, cap, runs, say):
    n = len(text)
    buf = ctypes.create_string_buffer(text, n)
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        stride = ctx.align_row_words()
        out = (apm.ApmMatch * cap)()
        ops = (ctypes.c_uint32 * (cap * stride))()
        found = ctypes.c_uint64()
        res = {"scan": [], "score": [], "align": [], "kernel_ms": []}
        for it in range(2 + runs):
            ctx._check(ctx._lib.apm_find_all_align_buffer(ctx._ctx, ctypes.cast(buf, ctypes.c_void_p), n, out, cap,
                                                          ctypes.byref(found), ops, stride))
            if it < 2:
                continue
            lt = ctx.launch_times()
            res["scan"].append(sum(t for l, t in lt if l not in ("score", "align")))
            res["score"] += [t for l, t in lt if l == "score"]
            res["align"] += [t for l, t in lt if l == "align"]
            res["kernel_ms"].append(ctx.timing()["kernel_ms"])
        have = min(found.value, cap)
        edits = sum(1 for i in range(have) if out[i].reserved)
        indel = sum(1 for i in range(have) if ops[i * stride] > min(len(pats[out[i].pattern]), n - out[i].pos))
        say("%-5s %d bytes, %d patterns, k = %d, %d records (%d at distance >= 1, %d with an insertion), rows of %d dwords, align_rows %d"
            % (name, n, len(pats), k, found.value, edits, indel, stride, ctx.stat("align_rows")))
        say("%-5s scan launches %s   \"score\" %s   \"align\" %s   kernel_ms %s"
            % (name, med(res["scan"]), med(res["score"]), med(res["align"]), med(res["kernel_ms"])))


def probe_polya(apm, runs, say):
    import torch
    n, k = 16 << 20, 3
    pats = [b"A" * 20]
    text = torch.full((n + 4096,), ord("A"), dtype=torch.uint8, device="cuda:0")
    cap = n
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        stride = ctx.align_row_words()
        ops = torch.zeros(cap * stride, dtype=torch.int32, device="cuda:0")
        res = {"find": [], "score": [], "align": []}
        for it in range(2 + runs):
            nf.zero_()
            torch.cuda.synchronize()
            t = {}
            ctx.find_shard_device(text.data_ptr(), 0, n, n, 0, n, rec.data_ptr(), cap, nf.data_ptr(), None)
            ctx.synchronize()
            t["find"] = ctx.timing()["kernel_ms"]
            ctx.score_shard_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr())
            ctx.synchronize()
            t["score"] = ctx.timing()["kernel_ms"]
            ctx.align_shard_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr(), ops.data_ptr(), stride)
            ctx.synchronize()
            t["align"] = ctx.timing()["kernel_ms"]
            if it >= 2:
                for key in res:
                    res[key].append(t[key])
        records = int(nf[0].item())
        rows = ops.view(cap, stride)[:records]
        full = bool(((rows[:, 0] == 20) & (rows[:, 1] == 0) & (rows[:, 2] == 0)).sum().item() == records - 16)
        say("polyA 16 MiB of 'A', A*20, k = %d, %d records, rows of %d dwords, every full window 20 '=': %s, align_rows %d"
            % (k, records, stride, full, ctx.stat("align_rows")))
        say("polyA apm_find_shard_device kernel_ms %s   apm_score_shard_device %s   apm_align_shard_device %s"
            % (med(res["find"]), med(res["score"]), med(res["align"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05", "align_probe.txt"))
    a = ap.parse_args()
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    import helpers as H
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    c = next(c for c in H.golden()["cases"] if c["name"] == "chrY_k3")
    probe_host_call(apm, "chrY", H.case_text(c), c["patterns"], c["k"], sum(c["counts"]) + 8, a.runs, say)
    cfg = wl.CONFIGS["cfg3"]
    n, k, seed = 64 << 20, cfg["k"], wl.seed_of(cfg["cid"])
    pats, _ = wl.make_patterns(n, cfg["lens"], k, seed)
    probe_host_call(apm, "cfg3", apm.synth_fill_host(0, n, seed), pats, k, 1 << 16, a.runs, say)
    probe_polya(apm, a.runs, say)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
