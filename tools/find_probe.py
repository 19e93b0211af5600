"""Measurement aid (GPU box): the host-level find calls, for an A/B of two builds of the host path.

    python tools/find_probe.py [--runs 5] [--tag NAME]          (APM_LIB_PATH picks another build of the library)

256 MiB of synthetic DNA in host memory, cfg3's 32 patterns of 16..128 bytes, k = 3.  One call of each of the seven find
calls (the best-hit call with and without rows, the occurrence call with and without spans): its launch labels in stream
order (apm_get_launch_times), n_launches, windows, the records it returned and a digest of its whole result -- two builds
that compute the same print the same lines.  Then apm_find_all_align_buffer and apm_find_best_buffer timed: total_ms and
kernel_ms of apm_get_timing, and the "best_ms" statistic, median [min, max] of --runs behind two warm-ups."""
import argparse
import hashlib
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "inf560-approximate-pattern-matching_amd"
sys.path.insert(0, ROOT)


def med(v):
    return "%.4f [%.4f, %.4f]" % (statistics.median(v), min(v), max(v))


def digest(x):
    return hashlib.sha256(repr(x).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tag", default="?")
    a = ap.parse_args()
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    c = wl.CONFIGS["cfg3"]
    n, k, seed = 256 << 20, c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    text = apm.synth_fill_host(0, n, seed)
    cap = 1 << 16
    tag = a.tag
    print(tag, "n", n, "patterns", len(pats), "k", k, flush=True)
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        calls = [
            ("apm_find_buffer", lambda: ctx.find_buffer(text, 0, cap)),
            ("apm_find_all_buffer", lambda: ctx.find_all_buffer(text, cap)),
            ("apm_find_all_dist_buffer", lambda: ctx.find_all_dist_buffer(text, cap)),
            ("apm_find_all_align_buffer", lambda: ctx.find_all_align_buffer(text, cap)),
            ("apm_find_best_buffer", lambda: ctx.find_best_buffer(text, 4, cap)),
            ("apm_find_best_buffer+ops", lambda: ctx.find_best_buffer(text, 4, cap, align=True)),
            ("apm_find_occ_buffer", lambda: ctx.find_occ_buffer(text, apm.APM_OCC_LOCAL_MIN, cap)),
            ("apm_find_occ_buffer-spans", lambda: ctx.find_occ_buffer(text, apm.APM_OCC_LOCAL_MIN, cap, spans=False)),
            ("apm_find_occ_align_buffer", lambda: ctx.find_occ_align_buffer(text, apm.APM_OCC_LOCAL_MIN, cap)),
        ]
        for name, call in calls:
            res = call()
            t = ctx.timing()
            print(tag, "%-28s labels %s  n_launches %d  windows %d  records %d  digest %s" % (
                name, ",".join(l for l, _ in ctx.launch_times()), t["n_launches"], t["windows"], len(res[0]), digest(res)), flush=True)
        for name, call, stat in (("apm_find_all_align_buffer", calls[3][1], None), ("apm_find_best_buffer", calls[4][1], "best_ms")):
            tot, ker, st = [], [], []
            for it in range(2 + a.runs):
                call()
                if it >= 2:
                    t = ctx.timing()
                    tot.append(t["total_ms"])
                    ker.append(t["kernel_ms"])
                    if stat:
                        st.append(ctx.stat(stat))
            print(tag, "%-28s total_ms %s  kernel_ms %s%s" % (name, med(tot), med(ker), ("  %s %s" % (stat, med(st))) if stat else ""), flush=True)


if __name__ == "__main__":
    main()
