"""Measurement aid (GPU box): what the nearest-occurrence search per sequence costs, by how long the sequences are.

    python tools/seqnear_probe.py [--runs 5] [--out FILE]

HIP-event times after a warm-up, median [min, max] of --runs, text resident on the device: cfg3's patterns (32 of 16..128
bytes) on 1 GiB of synthetic DNA, so 1 GiB of ends and ms = ms per GiB.  The "snear" launch (apm_nearest_seq_shard_device)
and the "snspan" launch over its keys (apm_nearest_seq_records_device) under three sequence tables: one sequence; sequences
of 150 bytes (reads); sequences of 10 KB (genes, contigs).  Beside them, on the same bytes in the same run, the "nearest"
launch (apm_nearest_shard_device), whose kernel this search leaves untouched, and the figure the parent commit recorded for
it in profiles/r15/nearest_probe.txt.  What the rows show: the boundary compare in the column loop (the one-sequence row
against "nearest"), and the flushes and restarts at boundaries (the other two rows).
"""
import argparse
import importlib
import os
import re
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
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        ctx.synth_fill_device(text.data_ptr(), 0, n, seed)
        ctx.synchronize()
        say("cfg3  %d bytes of synthetic DNA, %d patterns of %d..%d bytes; ms = ms per GiB of ends" % (n, P, min(c["lens"]), max(c["lens"])))
        keys = torch.empty(P, dtype=torch.int64, device="cuda:0")
        t_near = timed(ctx, runs, lambda: ctx.nearest_shard_device(text.data_ptr(), 0, n, n, 0, n, keys.data_ptr()), lambda: keys.fill_(-1))
        say("cfg3  \"nearest\"  this run                       kernel_ms %s   S = %d, %d walks" % (med(t_near), ctx.stat("nearest_segment"), ctx.stat("nearest_lanes")))
        whole = [int(v) & ((1 << 64) - 1) for v in keys.cpu().tolist()]
        parent = os.path.join(ROOT, "profiles", "r15", "nearest_probe.txt")
        if os.path.exists(parent):
            m = re.search(r'"nearest"\s+kernel_ms (\S+ \[[^\]]*\])', open(parent).read())
            say("cfg3  \"nearest\"  the parent's record            kernel_ms %s   (profiles/r15/nearest_probe.txt)" % (m.group(1) if m else "?"))
        del keys
        for what, length in (("one sequence", n), ("sequences of 150 bytes", 150), ("sequences of 10 KB", 10000)):
            begins = torch.arange(0, n, length, dtype=torch.int64, device="cuda:0")
            n_seq = int(begins.numel())
            table = torch.zeros((n_seq + 1, 2), dtype=torch.int64, device="cuda:0")    # {hdr_off, t_begin}; the sentinel n
            table[:n_seq, 1] = begins
            table[n_seq, 1] = n
            del begins
            rows = n_seq * P
            keys = torch.empty(rows, dtype=torch.int64, device="cuda:0")
            end = torch.zeros(2 * rows, dtype=torch.int64, device="cuda:0")
            start = torch.zeros(2 * rows, dtype=torch.int64, device="cuda:0")

            def reset():
                keys.fill_(-1)                                 # APM_NEAREST_NONE
                torch.cuda.synchronize()

            t_scan = timed(ctx, runs, lambda: ctx.nearest_seq_shard_device(text.data_ptr(), 0, n, n, 0, n, table.data_ptr(), n_seq, keys.data_ptr()), reset)
            say("cfg3  \"snear\"    %-28s kernel_ms %s   %d sequences, S = %d, %d walks, %.3f x \"nearest\"" %
                (what, med(t_scan), n_seq, ctx.stat("seqnear_segment"), ctx.stat("seqnear_lanes"), statistics.median(t_scan) / statistics.median(t_near)))
            t_span = timed(ctx, runs, lambda: ctx.nearest_seq_records_device(text.data_ptr(), 0, n, n, table.data_ptr(), n_seq, keys.data_ptr(),
                                                                            end.data_ptr(), start.data_ptr()))
            say("cfg3  \"snspan\"   %-28s kernel_ms %s   over %d keys" % (what, med(t_span), rows))
            if n_seq == 1:
                got = [int(v) & ((1 << 64) - 1) for v in keys.cpu().tolist()]
                say("cfg3  one sequence: the keys %s those of \"nearest\"" % ("equal" if got == whole else "DIFFER FROM"))
            else:
                none = int((keys == -1).sum().item())
                say("cfg3  %s: %d of %d pairs have no answer" % (what, none, rows))
            del keys, end, start, table
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
