"""Measurement aid (GPU box): what the nearest-occurrence search costs against the occurrence scan on the same input.

    python tools/nearest_probe.py [--runs 5] [--out FILE]

HIP-event times after a warm-up, median [min, max] of --runs, text resident on the device: cfg3's shape -- 1 GiB of
synthetic DNA, 32 patterns of 16..128 bytes.  The "nearest" launch (apm_nearest_shard_device: one walk per (segment,
pattern) at the bound m - 1, a key per pattern) and the "nspan" launch over its keys (apm_nearest_records_device); the
yardstick in the same run, on the same bytes: the "occ" launch (apm_occ_shard_device) at k = 3 under APM_OCC_ALL, whose
kernel the nearest-occurrence search leaves untouched (csrc/apm_occ.resources.txt is byte-identical to the parent
commit's).  The nearest walk is the occurrence walk's column step without the ballot per column, at a warm-up of 2 m - 1
bytes instead of m + k and S = 16 (2 m_max - 1).
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "inf560-approximate-pattern-matching_amd"
sys.path.insert(0, ROOT)


def med(v):
    return "%.4f [%.4f, %.4f]" % (statistics.median(v), min(v), max(v))


def timed(ctx, runs, call, before=None):
    """kernel_ms of `call` over `runs` runs behind two warm-ups"""
    out = []
    for it in range(2 + runs):
        if before:
            before()
        call()
        ctx.synchronize()
        if it >= 2:
            out.append(ctx.timing()["kernel_ms"])
    return out


def probe(apm, wl, runs, say):
    import torch
    c = wl.CONFIGS["cfg3"]
    n, k, seed = c["n"], c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    P = len(pats)
    text = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    cap = 1 << 20
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(P, dtype=torch.int64, device="cuda:0")
    keys = torch.empty(P, dtype=torch.int64, device="cuda:0")
    end = torch.zeros(2 * P, dtype=torch.int64, device="cuda:0")
    start = torch.zeros(2 * P, dtype=torch.int64, device="cuda:0")

    def zero():
        nf.zero_()
        counts.zero_()
        keys.fill_(-1)                                         # APM_NEAREST_NONE
        torch.cuda.synchronize()

    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        ctx.synth_fill_device(text.data_ptr(), 0, n, seed)
        ctx.synchronize()
        say("cfg3  %d bytes of synthetic DNA, %d patterns of %d..%d bytes" % (n, P, min(c["lens"]), max(c["lens"])))
        t_occ = timed(ctx, runs, lambda: ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, apm.APM_OCC_ALL, rec.data_ptr(), cap, nf.data_ptr(),
                                                              counts.data_ptr()), zero)
        say("cfg3  \"occ\"     APM_OCC_ALL, k = %d  kernel_ms %s   %d ends, S = %d, %d walks" % (k, med(t_occ), int(nf[0].item()), ctx.stat("occ_segment"),
                                                                                               ctx.stat("occ_lanes")))
        t_near = timed(ctx, runs, lambda: ctx.nearest_shard_device(text.data_ptr(), 0, n, n, 0, n, keys.data_ptr()), zero)
        say("cfg3  \"nearest\"                     kernel_ms %s   S = %d, %d walks" % (med(t_near), ctx.stat("nearest_segment"), ctx.stat("nearest_lanes")))
        k64 = [int(v) & ((1 << 64) - 1) for v in keys.cpu().tolist()]   # (the yardstick's second pass resets them)
        t = timed(ctx, runs, lambda: ctx.nearest_records_device(text.data_ptr(), 0, n, n, keys.data_ptr(), end.data_ptr(), start.data_ptr()))
        say("cfg3  \"nspan\"   over the %d keys    kernel_ms %s" % (P, med(t)))
        t_occ2 = timed(ctx, runs, lambda: ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, apm.APM_OCC_ALL, rec.data_ptr(), cap, nf.data_ptr(),
                                                               counts.data_ptr()), zero)
        say("cfg3  \"occ\"     again                kernel_ms %s" % med(t_occ2))
        ratio = statistics.median(t_near) / statistics.median(t_occ + t_occ2)
        say("cfg3  \"nearest\" / \"occ\" = %.3f" % ratio)
        say("cfg3  m:d of every pattern %s" % " ".join("%d:%d" % (len(p), v >> 56) for p, v in zip(pats, k64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    probe(apm, wl, a.runs, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
