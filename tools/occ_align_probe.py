"""Measurement aid (GPU box): what the occurrence-script pass costs beside the span pass, on tools/occ_probe.py's cfg3 shape.

    python tools/occ_align_probe.py [--runs 5] [--out FILE]

cfg3's shape: 1 GiB of synthetic DNA resident on the device, 32 patterns of 16..128 bytes, k = 3.  One "occ" launch under
APM_OCC_LOCAL_MIN fills the record buffer; then the "span" launch over its ends (apm_occ_spans_device) and the "oalign" launch
over the (end, span) pairs (apm_occ_align_device) are timed in the same run: the launch times apm_get_launch_times reports,
median [min, max] of --runs after two warm-ups.  It also says how many rows hold a script and the longest one.
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


def launch_ms(ctx, label, runs, call):
    """the time of the launch `label` of `call` over `runs` runs behind two warm-ups"""
    out = []
    for it in range(2 + runs):
        call()
        ctx.synchronize()
        times = dict(ctx.launch_times())
        if it >= 2:
            out.append(times[label])
    return out


def main():
    import torch
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

    c = wl.CONFIGS["cfg3"]
    n, k, seed = c["n"], c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    cap = 1 << 20
    text = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    span = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(len(pats), dtype=torch.int64, device="cuda:0")
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        stride = ctx.occ_align_row_words()
        ops = torch.zeros(cap * stride, dtype=torch.int32, device="cuda:0")
        ctx.synth_fill_device(text.data_ptr(), 0, n, seed)
        ctx.synchronize()
        say("cfg3  %d bytes of synthetic DNA, %d patterns of %d..%d bytes, k = %d" % (n, len(pats), min(c["lens"]), max(c["lens"]), k))
        t = launch_ms(ctx, "occ", 1, lambda: (nf.zero_(), counts.zero_(), torch.cuda.synchronize(),
                                              ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, apm.APM_OCC_LOCAL_MIN, rec.data_ptr(), cap,
                                                                   nf.data_ptr(), counts.data_ptr())))
        n_rec = int(nf[0].item())
        say("cfg3  \"occ\"    APM_OCC_LOCAL_MIN  launch ms %s   %d ends" % (med(t), n_rec))
        t = launch_ms(ctx, "span", a.runs, lambda: ctx.occ_spans_device(text.data_ptr(), 0, n, n, rec.data_ptr(), cap, nf.data_ptr(), span.data_ptr()))
        say("cfg3  \"span\"   over the %d ends            launch ms %s" % (n_rec, med(t)))
        t = launch_ms(ctx, "oalign", a.runs, lambda: ctx.occ_align_device(text.data_ptr(), 0, n, n, rec.data_ptr(), span.data_ptr(), cap, nf.data_ptr(),
                                                                          ops.data_ptr(), stride))
        head = ops.view(cap, stride)[:n_rec, 0].cpu()
        say("cfg3  \"oalign\" over the %d (end, span) pairs launch ms %s   rows of %d dwords, %d hold a script, the longest %d ops" % (
            n_rec, med(t), stride, int((head > 0).sum().item()), int(head.max().item()) if n_rec else 0))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
