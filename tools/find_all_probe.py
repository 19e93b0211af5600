"""Measurement aid (GPU box): what the record calls (apm_find_all_buffer / apm_find_shard_device) cost.

    python tools/find_all_probe.py [--parent-root DIR] [--runs 5] [--out profiles/r04/find_all.txt]

All three questions in ONE call on one box (boxes differ by 5-10 %, tools/ab_libs.sh), the two trees alternating:
  (a) is the counting path unharmed?   bench.py's ms_per_step (cfg3) and the cfg5 shard time (1 GiB, device-resident
      synthetic text, HIP-event times after a warm-up), parent tree vs this tree, --runs alternating runs each; this tree's
      median must lie inside the parent's own spread.  --parent-root: a checkout of the parent commit, built (its bench.py
      and package are run from there); without it only this tree is measured.
  (b) what does locating cost?         apm_find_shard_device on cfg3 and cfg5 at 1 GiB against the counting time of (a),
      with the per-launch split of apm_get_launch_times.
  (c) how much faster than the old way? P calls of apm_find_buffer against one apm_find_all_buffer on a 64 MiB host text,
      identical record sets.
"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "inf560-approximate-pattern-matching_amd"


def worker_shard(root, cfg, mode, reps):
    """one process: cfg's patterns (planted for 1 GiB) on 1 GiB of device-resident synthetic text; median event ms"""
    sys.path.insert(0, root)
    import torch
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    c = wl.CONFIGS[cfg]
    n, k, seed = 1 << 30, c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    text = torch.empty(n + 4096, dtype=torch.uint8, device="cuda:0")
    cnt = torch.zeros(len(pats), dtype=torch.int64, device="cuda:0")
    cap = 1 << 20
    rec = torch.zeros(2 * cap, dtype=torch.int64, device="cuda:0")
    nf = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        ctx.synth_fill_device(text.data_ptr(), 0, n, seed)
        ctx.synchronize()

        def once():
            cnt.zero_()
            nf.zero_()
            torch.cuda.synchronize()
            if mode == "find":
                ctx.find_shard_device(text.data_ptr(), 0, n, n, 0, n, rec.data_ptr(), cap, nf.data_ptr(), cnt.data_ptr())
            else:
                ctx.count_shard_device(text.data_ptr(), 0, n, n, 0, n, cnt.data_ptr())
            ctx.synchronize()
            return ctx.timing()["kernel_ms"]

        for _ in range(3):
            once()
        ms = [once() for _ in range(reps)]
        lt = ctx.launch_times()
        print(json.dumps(dict(cfg=cfg, mode=mode, ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms),
                              launches=[(l, round(t, 4)) for l, t in lt], matches=int(cnt.sum()), records=int(nf[0]))))


def worker_old(root):
    """(c): 64 MiB of synthetic DNA on the host, cfg3's patterns planted for that size"""
    sys.path.insert(0, root)
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    c = wl.CONFIGS["cfg3"]
    n, k, seed = 64 << 20, c["k"], wl.seed_of(c["cid"])
    pats, _ = wl.make_patterns(n, c["lens"], k, seed)
    text = apm.synth_fill_host(0, n, seed)
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, k)
        ctx.count_buffer(text)                                   # warm-up: plan uploaded, text buffer allocated
        t0 = time.perf_counter()
        old = [(i, p) for i in range(len(pats)) for p in ctx.find_buffer(text, i, capacity=1 << 16)[0]]
        t_old = time.perf_counter() - t0
        ctx.find_all_buffer(text, 1 << 16)                       # warm-up: record buffer allocated
        t0 = time.perf_counter()
        new, total = ctx.find_all_buffer(text, 1 << 16)
        t_new = time.perf_counter() - t0
        print(json.dumps(dict(n=n, patterns=len(pats), records=total, identical=(old == new), old_ms=t_old * 1e3, new_ms=t_new * 1e3,
                              ratio=t_old / t_new)))


def run_json(cmd, cwd, timeout):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:                                        # nothing more on the GPU after a failure
        sys.exit("FAILED (%d): %s\n%s" % (r.returncode, " ".join(cmd), r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04", "find_all.txt"))
    a = ap.parse_args()
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(a.parent_root))] if a.parent_root else [])
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    bench = {t: [] for t, _ in trees}
    shard = {t: [] for t, _ in trees}
    for run in range(a.runs):                                    # (a): alternating, parent first
        for t, root in reversed(trees):
            b = run_json([sys.executable, "bench.py", "--gpus", "1"], root, 300)
            bench[t].append(b["ms_per_step"])
            s = run_json([sys.executable, os.path.abspath(__file__), "shard", root, "cfg5", "count", "10"], root, 300)
            shard[t].append(s["ms"])
            say("(a) run %d %-6s bench cfg3 ms_per_step %.4f   cfg5 count shard %.4f ms  %s" % (run, t, b["ms_per_step"], s["ms"], s["launches"]))
    for name, d in (("bench cfg3 ms_per_step", bench), ("cfg5 1 GiB count shard ms", shard)):
        for t, _ in trees:
            say("(a) %-28s %-6s median %.4f  min %.4f  max %.4f" % (name, t, statistics.median(d[t]), min(d[t]), max(d[t])))
        if "parent" in d:
            med = statistics.median(d["this"])
            say("(a) %-28s this tree's median inside the parent's spread: %s" % (name, min(d["parent"]) <= med <= max(d["parent"])))
    for cfg in ("cfg3", "cfg5"):                                 # (b)
        c = run_json([sys.executable, os.path.abspath(__file__), "shard", ROOT, cfg, "count", "10"], ROOT, 300)
        f = run_json([sys.executable, os.path.abspath(__file__), "shard", ROOT, cfg, "find", "10"], ROOT, 300)
        say("(b) %s 1 GiB  count %.4f ms [%.4f, %.4f]  find %.4f ms [%.4f, %.4f]  ratio %.3f  matches %d records %d" % (
            cfg, c["ms"], c["ms_min"], c["ms_max"], f["ms"], f["ms_min"], f["ms_max"], f["ms"] / c["ms"], f["matches"], f["records"]))
        say("(b) %s launches count %s" % (cfg, c["launches"]))
        say("(b) %s launches find  %s" % (cfg, f["launches"]))
    o = run_json([sys.executable, os.path.abspath(__file__), "old", ROOT], ROOT, 600)   # (c)
    say("(c) 64 MiB host text, %d patterns, %d records, identical sets: %s   %d x apm_find_buffer %.1f ms   apm_find_all_buffer %.1f ms   ratio %.1f" % (
        o["patterns"], o["records"], o["identical"], o["patterns"], o["old_ms"], o["new_ms"], o["ratio"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "shard":
        worker_shard(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]))
    elif len(sys.argv) > 1 and sys.argv[1] == "old":
        worker_old(sys.argv[2])
    else:
        main()
