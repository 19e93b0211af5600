"""Measurement aid (GPU box): what the occurrence search costs against the window scan on the same input.

    python tools/occ_probe.py [--runs 5] [--out FILE] [--skip-bitpar]

HIP-event times after a warm-up, median [min, max] of --runs, text resident on the device:
  cfg3   cfg3's shape: 1 GiB of synthetic DNA, 32 patterns of 16..128 bytes, k = 3.  The "occ" launch
         (apm_occ_shard_device) under both flags and the "span" launch over its ends (apm_occ_spans_device); the
         yardsticks on the same bytes: the forced-BITPAR counting call (apm_count_shard_device: the same bit-vector
         arithmetic at m columns per window start instead of about one per byte) and the window scan with distances
         (apm_find_shard_device + apm_score_shard_device, what apm_find_all_dist_buffer runs).  The yardsticks' kernels
         are untouched by the occurrence search (csrc/*.resources.txt are byte-identical to the parent commit's).
  dense  64 MiB of 'A', the pattern 'A' x 20, k = 3: every end from 16 on is reported under APM_OCC_ALL (the record buffer
         holds 2^22 of them, the counter stays exact), one under APM_OCC_LOCAL_MIN.
"""
import argparse
import importlib
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "inf560-approximate-pattern-matching_amd"
sys.path.insert(0, ROOT)


def med(v):
    return "%.4f [%.4f, %.4f]" % (statistics.median(v), min(v), max(v))


def timed(ctx, runs, call, before=None):
    """kernel_ms of `call` over `runs` runs behind two warm-ups, and the launch times of the last run"""
    out = []
    for it in range(2 + runs):
        if before:
            before()
        call()
        ctx.synchronize()
        if it >= 2:
            out.append(ctx.timing()["kernel_ms"])
    return out, ctx.launch_times()


def probe_cfg3(apm, wl, runs, say, skip_bitpar):
    import torch
    c = wl.CONFIGS["cfg3"]
    n, k, seed = c["n"], c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    P = len(pats)
    text = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    cap = 1 << 20
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    span = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(P, dtype=torch.int64, device="cuda:0")

    def zero():
        nf.zero_()
        counts.zero_()
        torch.cuda.synchronize()

    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        ctx.synth_fill_device(text.data_ptr(), 0, n, seed)
        ctx.synchronize()
        say("cfg3  %d bytes of synthetic DNA, %d patterns of %d..%d bytes, k = %d" % (n, P, min(c["lens"]), max(c["lens"]), k))
        for name, flags in (("APM_OCC_ALL", apm.APM_OCC_ALL), ("APM_OCC_LOCAL_MIN", apm.APM_OCC_LOCAL_MIN)):
            t, _ = timed(ctx, runs, lambda: ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, flags, rec.data_ptr(), cap, nf.data_ptr(),
                                                                  counts.data_ptr()), zero)
            say("cfg3  \"occ\"  %-18s kernel_ms %s   %d ends, S = %d, %d walks" % (name, med(t), int(nf[0].item()), ctx.stat("occ_segment"),
                                                                                  ctx.stat("occ_lanes")))
        t, _ = timed(ctx, runs, lambda: ctx.occ_spans_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr(), span.data_ptr()))
        say("cfg3  \"span\" over the %d LOCAL_MIN ends  kernel_ms %s" % (int(nf[0].item()), med(t)))
        t, _ = timed(ctx, runs, lambda: ctx.find_shard_device(text.data_ptr(), 0, n, n, 0, n, rec.data_ptr(), cap, nf.data_ptr(), counts.data_ptr()), zero)
        say("cfg3  window scan, AUTO, records (apm_find_shard_device)   kernel_ms %s   %d records" % (med(t), int(nf[0].item())))
        t, _ = timed(ctx, runs, lambda: ctx.score_shard_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr()))
        say("cfg3  their distances (apm_score_shard_device)            kernel_ms %s" % med(t))
        if not skip_bitpar:
            ctx.set_kernel("bitpar")
            t, _ = timed(ctx, max(1, min(runs, 3)), lambda: ctx.count_shard_device(text.data_ptr(), 0, n, n, 0, n, counts.data_ptr()), zero)
            say("cfg3  window scan, forced BITPAR (apm_count_shard_device) kernel_ms %s" % med(t))


def probe_dense(apm, runs, say):
    import torch
    n, k = 64 << 20, 3
    text = torch.full((n + 16,), ord("A"), dtype=torch.uint8, device="cuda:0")
    cap = 1 << 22
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    span = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")

    def zero():
        nf.zero_()
        torch.cuda.synchronize()

    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns([b"A" * 20], k)
        say("dense %d bytes of 'A', the pattern 'A' x 20, k = %d, a record buffer of %d" % (n, k, cap))
        t, _ = timed(ctx, runs, lambda: ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, apm.APM_OCC_ALL, rec.data_ptr(), cap, nf.data_ptr(), None), zero)
        say("dense \"occ\"  APM_OCC_ALL        kernel_ms %s   %d ends, S = %d" % (med(t), int(nf[0].item()), ctx.stat("occ_segment")))
        t, _ = timed(ctx, runs, lambda: ctx.occ_spans_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr(), span.data_ptr()))
        say("dense \"span\" over %d of them       kernel_ms %s" % (cap, med(t)))
        t, _ = timed(ctx, runs, lambda: ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, apm.APM_OCC_LOCAL_MIN, rec.data_ptr(), cap, nf.data_ptr(), None), zero)
        first = struct.unpack("<QII", rec[:2].cpu().numpy().tobytes())
        say("dense \"occ\"  APM_OCC_LOCAL_MIN  kernel_ms %s   %d end: %s" % (med(t), int(nf[0].item()), (first,)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-bitpar", action="store_true")
    a = ap.parse_args()
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    probe_cfg3(apm, wl, a.runs, say, a.skip_bitpar)
    probe_dense(apm, a.runs, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
