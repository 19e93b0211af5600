#!/usr/bin/env python3
"""Build container: python3 tools/kernel_asm_diff.py <base tree> <new tree>   (base: a `git worktree` of the parent commit)
Compiles the device code of every kernel unit (the Makefile's KERNEL_FILES, with its flags; counting build and -DAPM_REC
build; and its ONCE_FILES, the units compiled once: counting build only) of both trees to assembly and compares it kernel
by kernel, comments dropped and labels renumbered.  Kernels are matched by symbol, whichever unit holds them.  A tree
whose Makefile does not name ONCE_FILES yet is compiled with the other tree's list.  Per kernel: `identical`, or instructions, VGPRs, SGPRs and scratch old -> new.
A diff of two builds, nothing else."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "inf560-approximate-pattern-matching_amd"
META = re.compile(r"^    \.(name|private_segment_fixed_size|sgpr_count|vgpr_count):\s+(\S+)")


def make_var(tree, name):
    return subprocess.check_output(["make", "-s", "-C", os.path.join(tree, PKG), "--eval=print-%: ; @echo $($*)", "print-" + name], text=True).split()


def kernels_of(tree, unit, rec, tmp):
    """{symbol: (normalised instruction stream, {resource: value})} of one unit's device code"""
    out = os.path.join(tmp, "%s_%s%s.s" % (os.path.basename(os.path.abspath(tree)), unit, "_rec" if rec else ""))
    flags = [f for f in make_var(tree, "HIPFLAGS") if f != "-fPIC"]
    subprocess.check_call(make_var(tree, "HIPCC") + flags + (["-DAPM_REC"] if rec else []) +
                          ["--cuda-device-only", "-S", "-w", os.path.join(tree, PKG, "csrc", unit + ".hip"), "-o", out])
    text = open(out).read()
    res, name = {}, None
    for line in text.split(".amdgpu_metadata", 1)[1].splitlines():
        m = META.match(line)
        if m and m.group(1) == "name":
            name = m.group(2)
            res[name] = {}
        elif m:
            res[name][m.group(1)] = int(m.group(2))
    found = {}
    for sym in res:
        body = text.split("\n%s:" % sym, 1)[1].split(".Lfunc_end", 1)[0]
        lines = [l.split(";", 1)[0].strip() for l in body.splitlines()]
        labels = {}
        found[sym] = ([re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l) for l in lines if l], res[sym])
    return found


def build(tree, once, tmp):
    jobs = [(tree, u, rec, tmp) for u in make_var(tree, "KERNEL_FILES") for rec in (False, True)]
    jobs += [(tree, u, False, tmp) for u in once if os.path.exists(os.path.join(tree, PKG, "csrc", u + ".hip"))]
    with ThreadPoolExecutor(int(os.environ.get("JOBS", "8"))) as pool:
        parts = list(pool.map(lambda j: kernels_of(*j), jobs))
    return {sym: k for part in parts for sym, k in part.items()}


def main(base, new):
    with tempfile.TemporaryDirectory() as tmp:
        once = sorted(set(make_var(base, "ONCE_FILES")) | set(make_var(new, "ONCE_FILES")))
        old, cur = build(base, once, tmp), build(new, once, tmp)
    n_insn = lambda k: sum(1 for l in k[0] if not l.endswith(":") and not l.startswith("."))
    for sym in sorted(set(old) | set(cur)):
        if sym not in old or sym not in cur:
            print("%-90s %s" % (sym, "only in the new tree" if sym in cur else "only in the base tree"))
        elif old[sym] == cur[sym]:
            print("%-90s identical (%d instructions)" % (sym, n_insn(cur[sym])))
        else:
            o, c = old[sym][1], cur[sym][1]
            print("%-90s instructions %d -> %d (%+.2f %%), vgpr %d -> %d, sgpr %d -> %d, scratch %d -> %d" % (
                sym, n_insn(old[sym]), n_insn(cur[sym]), 100.0 * (n_insn(cur[sym]) - n_insn(old[sym])) / n_insn(old[sym]),
                o["vgpr_count"], c["vgpr_count"], o["sgpr_count"], c["sgpr_count"], o["private_segment_fixed_size"], c["private_segment_fixed_size"]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
