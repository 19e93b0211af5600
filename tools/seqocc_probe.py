"""Measurement aid (GPU box): what the occurrence search per sequence costs, by how long the sequences are.

    python tools/seqocc_probe.py [--runs 5] [--out FILE]

HIP-event times after a warm-up, median [min, max] of --runs, text resident on the device: cfg3's patterns (32 of 16..128
bytes, k = 3) on 1 GiB of synthetic DNA, so 1 GiB of ends and ms = ms per GiB -- the shape of profiles/r11/occ_probe.txt.
The "socc" launch (apm_occ_seq_shard_device, APM_OCC_LOCAL_MIN) and the "sspan" launch over its ends
(apm_occ_seq_spans_device) under three sequence tables: one sequence; sequences of 10 KB (genes, contigs); sequences of 150
bytes (reads).  Beside them, on the same bytes in the same run, the "occ" launch (apm_occ_shard_device), whose kernel this
search leaves untouched.  What the rows show: the boundary compare in the column loop (the one-sequence row against "occ"),
and the table searches and restarts at boundaries (the other two rows).
"""
import argparse
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "inf560-approximate-pattern-matching_amd"
sys.path.insert(0, ROOT)

CAP = 1 << 20  # records of room: cfg3 has some 23000 LOCAL_MIN ends


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
    flags = apm.APM_OCC_LOCAL_MIN
    text = torch.empty(n + 16, dtype=torch.uint8, device="cuda:0")
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        ctx.synth_fill_device(text.data_ptr(), 0, n, seed)
        ctx.synchronize()
        say("cfg3  %d bytes of synthetic DNA, %d patterns of %d..%d bytes, k = %d, APM_OCC_LOCAL_MIN; ms = ms per GiB of ends" %
            (n, P, min(c["lens"]), max(c["lens"]), k))
        out = torch.zeros(2 * CAP, dtype=torch.int64, device="cuda:0")
        span = torch.zeros(2 * CAP, dtype=torch.int64, device="cuda:0")
        seq = torch.zeros(CAP, dtype=torch.int32, device="cuda:0")
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda:0")
        counts = torch.zeros(P, dtype=torch.int64, device="cuda:0")

        def reset():
            cnt.zero_()
            counts.zero_()
            torch.cuda.synchronize()

        t_occ = timed(ctx, runs, lambda: ctx.occ_shard_device(text.data_ptr(), 0, n, n, 0, n, flags, out.data_ptr(), CAP, cnt.data_ptr(), counts.data_ptr()), reset)
        whole = sorted(map(tuple, out[:2 * int(cnt[0].item())].view(-1, 2).cpu().tolist()))
        say("cfg3  \"occ\"    this run                       kernel_ms %s   %d ends, S = %d, %d walks" %
            (med(t_occ), int(cnt[0].item()), ctx.stat("occ_segment"), ctx.stat("occ_lanes")))
        for what, length in (("one sequence", n), ("sequences of 10 KB", 10000), ("sequences of 150 bytes", 150)):
            begins = torch.arange(0, n, length, dtype=torch.int64, device="cuda:0")
            n_seq = int(begins.numel())
            table = torch.zeros((n_seq + 1, 2), dtype=torch.int64, device="cuda:0")    # {hdr_off, t_begin}; the sentinel n
            table[:n_seq, 1] = begins
            table[n_seq, 1] = n
            del begins
            t_scan = timed(ctx, runs, lambda: ctx.occ_seq_shard_device(text.data_ptr(), 0, n, n, 0, n, table.data_ptr(), n_seq, flags, out.data_ptr(), CAP,
                                                                     cnt.data_ptr(), counts.data_ptr()), reset)
            found = int(cnt[0].item())
            say("cfg3  \"socc\"   %-28s kernel_ms %s   %d sequences, %d ends, S = %d, %d walks, %.3f x \"occ\"" %
                (what, med(t_scan), n_seq, found, ctx.stat("seqocc_segment"), ctx.stat("seqocc_lanes"), statistics.median(t_scan) / statistics.median(t_occ)))
            t_span = timed(ctx, runs, lambda: ctx.occ_seq_spans_device(text.data_ptr(), 0, n, n, table.data_ptr(), n_seq, out.data_ptr(), CAP, cnt.data_ptr(),
                                                                     span.data_ptr(), seq.data_ptr()))
            say("cfg3  \"sspan\"  %-28s kernel_ms %s   over %d ends" % (what, med(t_span), min(found, CAP)))
            if n_seq == 1:
                got = sorted(map(tuple, out[:2 * found].view(-1, 2).cpu().tolist()))
                say("cfg3  one sequence: the records %s those of \"occ\"" % ("equal" if got == whole else "DIFFER FROM"))
            del table
            torch.cuda.empty_cache()


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
