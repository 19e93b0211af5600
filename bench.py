#!/usr/bin/env python3
"""bench.py -- the hot path (Levenshtein sliding-window DP + match count) on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N = 1)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one pass of the hot path over the rank's text shard (all patterns),
followed, for N > 1, by the RCCL all-reduce of the P partial counts.  Inputs are
resident in HBM before the timed region (device-side synthetic generator).

Workload at N = 1 (the headline): BASELINE.json configs[2] = cfg3, the largest
single-GPU configuration and the north_star workload: 1 GiB synthetic DNA, 32
patterns of mixed length 16..128, k = 3.  For N > 1 every GPU gets the same 1 GiB
cfg3 shard (weak scaling: a text of N GiB cut into owner-computes ranges with an
(m_max-1)-byte halo), so the N = 1 point of a scaling run IS the headline.
--config cfg2|cfg4|cfg5 selects another BASELINE workload (cfg4/cfg5: their
per-GPU shard, 2^33 / 8 bytes = 1 GiB).

A plain run sets up, warms up, times EXACTLY --steps steps in one region, writes
the counts of the last timed step if --dump-outputs DIR is given, and prints the
result line.  Everything else is measured only with --full: repeated timed
regions, the per-launch roofline and sieve statistics, the full-DP kernel
variants (`variants`, `counts_equal_bitpar`), the planted-occurrence and k = 0
closed-form checks, and at N = 1 cfg2, cfg4-per-GPU and cfg5-per-GPU
(`per_config`) and the reference's sequential path on the host cores
(`cpu_baseline`, 1 core, and `cpu_baseline_all_cores`); at N > 1 the whole
2^33-byte cfg4 / cfg5 texts sharded over the ranks (`per_config`).

--dump-outputs DIR writes DIR/counts.npy: the P per-pattern match counts the
timed path returned in its last timed step (float64, exact).  The inputs are
seeded, so the same arguments give the same inputs in every run.

Prints ONE JSON line (rank 0).  `value` = algorithmic window-DP cells per second,
sum_p (n-k) * m_p^2 / wall, with bit-exact counts; `config.kernel` names the kernel
variant that produced it ('banded' = exact shortcut, it does NOT evaluate every DP
cell); `variants` reports the full-DP kernels separately (cells really evaluated
per second and their VALU fraction) so that the shortcut number is never mistaken
for raw DP throughput.
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "inf560-approximate-pattern-matching_amd"

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s
# Integer VALU ceilings MEASURED on MI355X by tools/valu_probe.hip (profiles/r02/valu_probe.txt), chip-wide lane-ops/s
# at >= 2 waves per SIMD: the simple class (v_add/sub/and/or/xor_b32, v_lshrrev_b32, v_mov_b32, v_bitop3_b32) issues a
# wave64 instruction in 2 cycles per SIMD, everything else the scan kernels use (packed 16-bit v_pk_*, v_min*, DPP moves,
# v_alignbit/bfe/lshl_or/and_or/perm/mad24/dot4, v_lshlrev) in 4: 7.0e13 vs 3.8e13 lane-ops/s.
VALU_PEAK_LANE_OPS = 7.0e13          # simple class (the chip's integer VALU peak as measured)
VALU_PACKED_CLASS_LANE_OPS = 3.8e13  # packed / DPP / 3-operand / carry class
# Share of the 2-cycle class among the VALU instructions of the kernels' loops, from the gfx950 disassembly
# (tools/valu_mix.py -> profiles/r03/valu_mix.txt).  A kernel's VALU ceiling is the rate of ITS mix:
# 1 / (f2 / peak2 + (1 - f2) / peak4) lane-ops/s -- so no fraction can exceed 1 unless a count or a class is wrong.
VALU_MIX_F2 = {"wavefront": 0.280, "bitpar": 0.675}


def valu_ceiling(kernel):
    f2 = VALU_MIX_F2[kernel]
    return 1.0 / (f2 / VALU_PEAK_LANE_OPS + (1.0 - f2) / VALU_PACKED_CLASS_LANE_OPS)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=250, help="timed steps (default: ~0.1 s of timed region at the headline workload)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg3", help="workload: cfg3 (default, headline) | cfg2 | cfg4 | cfg5 "
                    "(cfg4/cfg5: per-GPU shard = their 8 GiB / 8)")
    ap.add_argument("--kernel", default="auto")
    ap.add_argument("--bytes-per-gpu", type=int, default=0, help="override the per-GPU text size")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) | gloo (CPU rehearsal of the N>1 path)")
    ap.add_argument("--full", action="store_true", help="also run every measurement and check beyond the headline "
                    "(repeated regions, roofline, variants, per_config, cpu_baseline); off by default")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-variants", action="store_true", help="with --full: skip variants")
    ap.add_argument("--no-per-config", action="store_true", help="with --full: skip per_config")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the counts of the last timed step to DIR/counts.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def per_gpu_bytes(cfg_name, wl):
    cfg = wl.CONFIGS[cfg_name]
    return cfg["n"] // (8 if cfg_name in ("cfg4", "cfg5") else 1)


def cpu_baseline(apm, pats, k, seed, gpu_slice_counts_fn):
    """The reference's sequential path timed on this box's host cores, on a bounded sample (a prefix of the same
    synthetic text, all patterns, ~8e9 DP cells = 15-25 s on one core): kind "reference" = oracle/_ref/apm_sequential
    (the reference's own sources compiled in the build container), else kind "port" = oracle/liboracle.so, 1 thread.
    Second leg: the same sample on ALL host cores (the oracle's position-parallel OpenMP form, the shape of
    /root/reference/src/patterns_over_ranks.c:353-375).  Returns (one_core, all_cores)."""
    per_pos = sum(len(p) ** 2 for p in pats)
    sample = max(4096, min(1 << 20, int(8.6e9 / per_pos) & ~4095))
    m_max = max(len(p) for p in pats)
    text = apm.synth_fill_host(0, sample + m_max - 1, seed)
    cells = float(sample) * per_pos
    ref_bin = os.path.join(ROOT, "oracle", "_ref", "apm_sequential")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    out = None
    if os.path.exists(ref_bin) and os.access(ref_bin, os.X_OK):
        with tempfile.NamedTemporaryFile(suffix=".fa", delete=False) as f:
            f.write(text[:sample])
            path = f.name
        try:
            r = subprocess.run([ref_bin, str(k), path] + [p.decode("latin-1") for p in pats],
                               capture_output=True, timeout=900)
            mt = re.search(rb"APM done in ([0-9.]+) s", r.stdout)
            if r.returncode == 0 and mt:
                secs = float(mt.group(1))
                n_pos = max(0, sample - k)
                out = dict(value=n_pos * per_pos / secs, unit="cells/s", cores=1, kind="reference", seconds=secs,
                           sample="first %d bytes of the bench text (as a file), all %d patterns, k=%d, oracle/_ref/apm_sequential" % (sample, len(pats), k))
        finally:
            os.unlink(path)
    import helpers as H                       # the oracle = checker (allowed here: cpu_baseline leg)
    if out is None:
        t0 = time.time()
        for p in pats:
            H.oracle().oracle_count_range(text, len(text), p, len(p), k, 0, sample)
        secs = time.time() - t0
        out = dict(value=cells / secs, unit="cells/s", cores=1, kind="port", seconds=secs,
                   sample="first %d bytes of the bench text, all %d patterns, k=%d, oracle/liboracle.so literal DP" % (sample, len(pats), k))
    # all host cores: literal DP, OpenMP over position chunks, 4x the sample so the run is not start-up bound
    cores = int(H.oracle().oracle_max_threads())
    big = min(1 << 22, sample * max(1, min(cores, 16) // 2))
    text_big = text if big == sample else apm.synth_fill_host(0, big + m_max - 1, seed)
    t0 = time.time()
    for p in pats:
        H.oracle().oracle_count_range_mt(text_big, len(text_big), p, len(p), k, 0, big, cores)
    secs = time.time() - t0
    allc = dict(value=float(big) * per_pos / secs, unit="cells/s", cores=cores, kind="port", seconds=secs,
                sample="first %d bytes of the bench text, all %d patterns, k=%d, oracle/liboracle.so literal DP, OpenMP over positions" % (big, len(pats), k))
    # checker: GPU counts on the same slice must equal the oracle's
    want = H.oracle_counts(text, pats, k, banded=True, j_end=sample)
    got = gpu_slice_counts_fn(text, sample)
    out["slice_counts_match_gpu"] = bool(got == want)
    return out, allc


def wavefront_wave_instr(lens, positions):
    """VALU wave-instructions the WAVEFRONT kernel issues (from the gfx950 disassembly of wf_scan: 10 per lane-step +
    6 per row of the lane, packed 16-bit = two windows per register; S = 64/Lm window pairs per sweep); within 3 % of
    SQ_INSTS_VALU measured on the cfg2 pass (profiles/r02/pmc_fulldp_cfg2.txt)."""
    total = 0.0
    for m in lens:
        best = None
        for r in (1, 2, 4):
            lm = (m + r - 1) // r
            if lm > 64:
                continue
            cost = (m + lm - 1) * (11.0 + 4.0 * r) / (64 // lm)       # the runtime's own choice of R (apm_runtime.hip)
            if best is None or cost < best[0]:
                best = (cost, r, lm)
        _, r, lm = best
        total += (m + lm - 1) * (10.0 + 6.0 * r) / (2 * (64 // lm)) * positions
    # wave-instructions for `positions` windows per pattern, one window pair per stream slot; scaled to the counter:
    # SQ_INSTS_VALU of the cfg2 pass = 1.72125e11 (profiles/r02/pmc_fulldp_cfg2.txt) against 1.77973e11 from this formula
    return total * (1.72125e11 / 1.77973e11)


def bitpar_wave_instr(lens, positions):
    """BITPAR: one window per lane; 13.7 VALU wave-instructions per column at one 32-row word (SQ_INSTS_VALU of the
    cfg2 pass, profiles/r02/pmc_fulldp_cfg2.txt), ~10.7 more per further word (apm_core.h bp_step)."""
    return sum(m * (10.7 * ((m + 31) // 32) + 3.0) for m in lens) * positions / 64.0


def main():
    args = parse()
    import torch
    import torch.distributed as dist
    apm = importlib.import_module(PKG)
    wl = importlib.import_module(PKG + ".workloads")
    sharding = importlib.import_module(PKG + ".sharding")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.gpus > 1 and world == 1:
        raise SystemExit("launch N>1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: this engine has no CPU fallback")
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)   # "nccl" IS RCCL on ROCm
        else:
            dist.init_process_group(backend=args.dist_backend)

    stream = torch.cuda.Stream(device=dev)                      # one explicit HIP stream for everything
    torch.cuda.set_stream(stream)
    ctx = apm.ApmContext(device=dev_index)
    ctx.set_stream(stream.cuda_stream)                          # the library launches on torch's stream

    # the true multi-GPU workloads (BASELINE.json configs[3..4]: ONE text of 2^33 bytes sharded over the ranks) run
    # beside the weak-scaled headline whenever there is more than one rank (--full)
    whole_cfgs = [c for c in ("cfg4", "cfg5") if args.full and world > 1 and not args.no_per_config and not args.bytes_per_gpu]
    per_gpu_max = max([args.bytes_per_gpu or per_gpu_bytes(args.config, wl)] +
                      ([] if (world > 1 or args.no_per_config or not args.full) else [per_gpu_bytes(c, wl) for c in ("cfg2", "cfg4", "cfg5")]) +
                      [wl.CONFIGS[c]["n"] // world + 4096 for c in whole_cfgs])
    text_buf = torch.empty(per_gpu_max + 512, dtype=torch.uint8, device=dev)   # one buffer, refilled per workload

    def measure(cfg_name, steps, warmup, full, with_variants, whole=False):
        """time `steps` steps of one workload; returns the result record (all ranks run it, rank 0 reports).
        full: also the repeated regions, roofline, sieve statistics and checks (and the variants if with_variants).
        whole: the workload's own text size (cfg4 / cfg5: 2^33 bytes) cut into `world` owner ranges -- the BASELINE
        configuration itself; otherwise every rank gets the per-GPU shard size (weak scaling)."""
        cfg = wl.CONFIGS[cfg_name]
        k, lens, seed = cfg["k"], cfg["lens"], wl.seed_of(cfg["cid"])
        per_gpu = args.bytes_per_gpu or per_gpu_bytes(cfg_name, wl)
        n_total = cfg["n"] if whole else per_gpu * world        # weak scaling unless `whole`
        if whole:
            per_gpu = (n_total + world - 1) // world
        pats, planted = wl.make_patterns(n_total, lens, k, seed)
        P = len(pats)
        m_max = max(lens)
        ctx.set_kernel("auto")
        ctx.set_patterns(pats, k)
        ctx.set_kernel(args.kernel)
        kernel_names = sorted({apm.KERNEL_NAMES[ctx.pattern_kernel(i)] for i in range(P)})

        ob, oe, lo, hi = sharding.rank_shard(n_total, k, m_max, rank, world)
        text = text_buf[: hi - lo + 16]
        ctx.synth_fill_device(text.data_ptr(), lo, hi - lo, seed)   # inputs resident in HBM
        # ring of count vectors: the all-reduce of step i (RCCL's own stream) overlaps the scans of the next steps
        RING = 4
        ring = [torch.zeros(P, dtype=torch.int64, device=dev) for _ in range(RING)]
        pending = [None] * RING
        counts = ring[0]
        torch.cuda.synchronize()

        def step(i):
            b = i % RING
            if pending[b] is not None:
                pending[b].wait()                                   # buffer free again (stream-level wait)
                pending[b] = None
            c = ring[b]
            c.zero_()
            ctx.count_shard_device(text.data_ptr(), lo, hi - lo, n_total, ob, oe, c.data_ptr())
            if world > 1:
                if args.dist_backend == "nccl":
                    pending[b] = dist.all_reduce(c, op=dist.ReduceOp.SUM, async_op=True)  # P x int64 over xGMI
                else:
                    h = c.cpu()
                    sharding.allreduce_counts(h)
                    c.copy_(h)
            return c

        def drain():
            for b in range(RING):
                if pending[b] is not None:
                    pending[b].wait()
                    pending[b] = None

        ctx.set_timing(False)       # no event records inside the timed region
        for i in range(warmup):
            step(i)
        drain()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        def timed_region():
            """EXACTLY `steps` steps between barrier + synchronize on both sides; (seconds, max over ranks; event ms)"""
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            ev0.record()
            c = None
            for i in range(steps):
                c = step(i)
            drain()
            ev1.record()
            torch.cuda.synchronize()
            if world > 1:
                dist.barrier()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            if world > 1:
                t = torch.tensor([el], dtype=torch.float64, device=dev if args.dist_backend == "nccl" else "cpu")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                el = float(t.item())
            return el, ev0.elapsed_time(ev1), c

        if whole:
            label = "%s: %s -- the whole text, sharded over %d ranks" % (cfg_name, cfg["desc"], world)
        elif cfg_name in ("cfg4", "cfg5") and not args.bytes_per_gpu:
            label = "%s per-GPU shard (1/8 of its text; %d such shards side by side): %s" % (cfg_name, world, cfg["desc"])
        else:
            label = "%s: %s" % (cfg_name, cfg["desc"])
        cells = wl.algorithmic_cells(n_total, lens, k)

        # The headline is ONE region of exactly `steps` steps: ms_per_step, value and the counts come from it.
        elapsed, ev_ms, counts = timed_region()
        final_counts = counts.cpu().tolist()
        sec_per_step = elapsed / steps
        rec = {
            "workload": label,
            "value": cells / sec_per_step, "unit": "cells/s", "ms_per_step": sec_per_step * 1e3,
            "event_ms_per_step": ev_ms / steps,
            "positions_x_patterns_per_s": float(max(0, n_total - k)) * P / sec_per_step,
            "text_bytes_total": n_total, "text_bytes_per_gpu": per_gpu, "patterns": P,
            "pattern_len": sorted(set(lens)), "k": k, "kernel": "+".join(kernel_names),
            "counts": final_counts,
        }
        if not full:
            return rec

        # --full: a region of K steps of this path is a few milliseconds (K = 20: 8 ms), and one clock ramp or one descheduled
        # host thread decides it.  The region is therefore timed REPEATEDLY -- every repeat is exactly K steps, bracketed as
        # the contract says -- until 0.25 s have been spent (at least 3, at most 15 regions counting the headline's; only a
        # FIRST region of >= 1 s stands alone: one of 75 ms -- 250 steps of cfg2, six times its kernel time -- was a host
        # stall, round 3); their MEDIAN is `median_ms_per_step`, all of them are listed in `timed_regions_ms_per_step`.
        # (All ranks take the same decisions: the elapsed time they see is the all-reduced maximum.)
        regions = [(elapsed, ev_ms)]
        spent = elapsed
        while not ((len(regions) == 1 and elapsed >= 1.0) or (spent >= 0.25 and len(regions) >= 3) or len(regions) >= 15):
            el, ev_ms_r, _ = timed_region()
            regions.append((el, ev_ms_r))
            spent += el
        regions.sort()
        rec["median_ms_per_step"] = regions[(len(regions) - 1) // 2][0] / steps * 1e3
        rec["timed_regions"] = len(regions)
        rec["timed_regions_ms_per_step"] = [r[0] / steps * 1e3 for r in regions]

        # per-launch kernel durations with HIP events on the launch stream (the library stamps the stream behind
        # every scan-kernel launch), averaged over `steps` calls
        ctx.set_timing(True)
        scratch = torch.zeros(P, dtype=torch.int64, device=dev)
        per_launch, step_ms = {}, []
        order = []
        for _ in range(steps):
            scratch.zero_()
            ctx.count_shard_device(text.data_ptr(), lo, hi - lo, n_total, ob, oe, scratch.data_ptr())
            tm = ctx.timing()
            step_ms.append(tm["main_kernel_ms"])
            seen = {}
            for label, ms in ctx.launch_times():
                idx = seen.get(label, 0)
                seen[label] = idx + 1
                key = "%s#%d" % (label, idx) if idx else label
                if key not in per_launch:
                    per_launch[key] = []
                    order.append(key)
                per_launch[key].append(ms)
        launches = [dict(kernel=key, ms_avg=sum(per_launch[key]) / len(per_launch[key])) for key in order]
        kernel_ms = sum(step_ms) / len(step_ms)
        shard_bytes = tm["text_bytes"]
        dom = max(launches, key=lambda d: d["ms_avg"]) if launches else dict(kernel="+".join(kernel_names), ms_avg=kernel_ms)
        for d in launches:
            d["gbs"] = shard_bytes / (d["ms_avg"] * 1e-3) / 1e9 if d["ms_avg"] > 0 else 0.0

        planted_found = all(c >= (1 if d <= k else 0) for c, (_, d) in zip(final_counts, planted))
        exact_k0 = None
        if k == 0 and min(lens) >= 24:
            exact_k0 = bool(final_counts == wl.expected_counts_k0(n_total, pats, planted, seed))

        # ROOFLINE, per STEP: algorithmic bytes (1 HBM byte per text position) over the sum of the step's scan
        # launches (HIP events on the launch stream) -- a step of the per-position pipeline is two launches, and the
        # fraction a reader takes for "how close to HBM" must price both.  The per-launch figures stay under `launches`,
        # the longest one under `dominant_kernel`.
        achieved = shard_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
        dom_gbs = shard_bytes / (dom["ms_avg"] * 1e-3) / 1e9 if dom["ms_avg"] > 0 else 0.0
        # HBM traffic of a step: NOT measured in this run -- PMC counters need rocprofv3 passes of their own (FETCH_SIZE and
        # WRITE_SIZE separately, profiles/run_profiles.sh); the committed summary of those passes is read here, and its
        # origin is stated in `traffic_source`.  null when there is no pass for this exact workload and kernel.
        traffic, traffic_source = None, None
        try:
            with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
                ent = json.load(f).get("%s:%s" % (cfg_name, "+".join(kernel_names)))
            if ent and world == 1 and not args.bytes_per_gpu:
                traffic = ent["step_traffic_bytes"]
                traffic_source = ("profiles/traffic.json, round %s: separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE) of `bench.py "
                                  "--config %s`, bytes = 2*FETCH_SIZE*1024 + WRITE_SIZE*1024 summed over the step's launches; committed "
                                  "beside profiles/%s/bench_%s_pmc_*.txt, not measured in this run" % (ent["round"], cfg_name, ent["round"], cfg_name))
        except Exception:
            traffic, traffic_source = None, None
        rec["planted_occurrences_found"] = bool(planted_found)
        rec["roofline"] = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                           "scope": "step: all scan launches of one pass over the shard",
                           "algorithmic_bytes_per_step": shard_bytes,
                           "step_kernel_ms": kernel_ms,
                           "launches_per_step": len(launches), "launches": launches,
                           "dominant_kernel": {"kernel": dom["kernel"], "ms_avg": dom["ms_avg"], "gbs": dom_gbs,
                                               "frac_of_peak_alone": dom_gbs / HBM_PEAK_GBS},
                           "note": "achieved = algorithmic bytes of the step (1 HBM byte per text position, SURVEY 8d) / sum of the "
                                   "average durations of the step's scan launches, HIP events on the launch stream; every launch's "
                                   "own rate is under `launches`"}
        if exact_k0 is not None:
            rec["counts_equal_closed_form_k0"] = exact_k0
        if ctx.stat("sieve_on"):
            rec["sieve"] = {key: ctx.stat(key) for key in ("sieve_rate", "sieve_clist", "sieve_mask_bytes", "sieve_candidates",
                                                            "sieve_stride", "sieve_fused", "verify_launches", "verify_image_bytes", "verify_blocks_per_cu", "verify_threads")}

        # full-DP kernel variants, reported under their own label (cells really evaluated)
        if with_variants and world == 1:
            variants = {}
            positions = float(max(0, n_total - k))
            if max(lens) <= 128:
                # BITPAR at FULL size: every window of every pattern through the bit-vector DP; its counts pin the headline's
                ctx.set_kernel("bitpar")
                ms = []
                for _ in range(2):
                    scratch.zero_()
                    ctx.count_shard_device(text.data_ptr(), lo, hi - lo, n_total, ob, oe, scratch.data_ptr())
                    ms.append(ctx.timing()["main_kernel_ms"])
                ok = scratch.cpu().tolist() == final_counts
                t_s = ms[-1] * 1e-3
                variants["bitpar"] = {"cells_evaluated_per_s": cells / t_s, "kernel_ms": ms[-1], "sample": "full size",
                                      "counts_equal_headline": bool(ok),
                                      "valu_lane_ops_per_s": bitpar_wave_instr(lens, positions) * 64 / t_s,
                                      "valu_frac": bitpar_wave_instr(lens, positions) * 64 / t_s / valu_ceiling("bitpar"),
                                      "hbm_frac": shard_bytes / t_s / 1e9 / HBM_PEAK_GBS}
                rec["counts_equal_bitpar"] = bool(ok)
            if max(lens) <= 256:
                # WAVEFRONT (the kernel north_star names) on a bounded prefix sized for ~1 s: same counts as AUTO there
                per_pos = float(sum(m * m for m in lens))
                sl = int(min(hi - lo - (m_max - 1), max(1 << 22, (int(8e12 / per_pos)) & ~4095)))
                ctx.set_kernel(args.kernel)
                scratch.zero_()
                ctx.count_shard_device(text.data_ptr(), lo, sl + m_max - 1, n_total, ob, ob + sl, scratch.data_ptr())
                torch.cuda.synchronize()
                ref_slice = scratch.cpu().tolist()
                ctx.set_kernel("wavefront")
                ms = []
                for _ in range(2):
                    scratch.zero_()
                    ctx.count_shard_device(text.data_ptr(), lo, sl + m_max - 1, n_total, ob, ob + sl, scratch.data_ptr())
                    ms.append(ctx.timing()["main_kernel_ms"])
                t_s = ms[-1] * 1e-3
                variants["wavefront"] = {"cells_evaluated_per_s": sl * per_pos / t_s, "kernel_ms": ms[-1],
                                         "sample": "first %d window starts of the shard" % sl,
                                         "counts_equal_headline": bool(scratch.cpu().tolist() == ref_slice),
                                         "valu_lane_ops_per_s": wavefront_wave_instr(lens, float(sl)) * 64 / t_s,
                                         "valu_frac": wavefront_wave_instr(lens, float(sl)) * 64 / t_s / valu_ceiling("wavefront"),
                                         "hbm_frac": sl / t_s / 1e9 / HBM_PEAK_GBS}
            ctx.set_kernel(args.kernel)
            rec["variants"] = variants
        rec["_ctx"] = dict(pats=pats, k=k, seed=seed, P=P, n_total=n_total)
        return rec

    head = measure(args.config, args.steps, args.warmup, args.full, args.full and not args.no_variants)
    hc = head.pop("_ctx", None)
    if args.dump_outputs and rank == 0:
        # what the timed path returned in its last timed step: the P per-pattern counts (all-reduced over the ranks)
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "counts.npy"), np.asarray(head["counts"], dtype=np.float64))

    cpu1 = cpu_all = None
    if args.full and not args.no_cpu_baseline and world == 1 and rank == 0:
        def gpu_slice(text_bytes, sample):
            t = torch.frombuffer(bytearray(text_bytes), dtype=torch.uint8).to(dev)
            c = torch.zeros(hc["P"], dtype=torch.int64, device=dev)
            ctx.count_shard_device(t.data_ptr(), 0, len(text_bytes), hc["n_total"], 0, sample, c.data_ptr())
            torch.cuda.synchronize()
            return c.cpu().tolist()
        cpu1, cpu_all = cpu_baseline(apm, hc["pats"], hc["k"], hc["seed"], gpu_slice)

    per_config = {}
    if args.full and world == 1 and not args.no_per_config and not args.bytes_per_gpu:
        for name in ("cfg2", "cfg3", "cfg4", "cfg5"):
            if name == args.config:
                continue
            r = measure(name, args.steps, args.warmup, True, not args.no_variants)
            r.pop("_ctx")
            r.pop("counts")
            per_config[name] = r

    for name in whole_cfgs:      # every rank takes part; rank 0 reports
        r = measure(name, args.steps, args.warmup, True, False, whole=True)
        r.pop("_ctx")
        r.pop("counts")
        per_config[name] = r

    if rank != 0:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    line = {
        "metric": "window-DP-cells/sec",
        "value": head["value"],
        "unit": "cells/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": head["ms_per_step"],
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u32",
        "data": "synthetic",
        "config": {"workload": head["workload"], "text_bytes_total": head["text_bytes_total"],
                   "text_bytes_per_gpu": head["text_bytes_per_gpu"], "patterns": head["patterns"],
                   "pattern_len": head["pattern_len"], "k": head["k"], "kernel": head["kernel"],
                   "partition": "text-sharded x%d, halo m_max-1, RCCL all-reduce of counts" % world},
        "note": "value = algorithmic window-DP cells (sum_p (n-k)*m_p^2) per second with bit-exact counts; "
                "config.kernel names the kernel that produced it ('banded' = exact shortcut: pigeonhole key filter + "
                "banded verification, it does NOT evaluate every DP cell); raw full-DP throughput is under variants (--full); "
                "counts_equal_bitpar (--full) = the headline's counts equal the full-DP BITPAR kernel's at full size",
        "positions_x_patterns_per_s": head["positions_x_patterns_per_s"],
        "counts": head["counts"],
        "event_ms_per_step": head["event_ms_per_step"],
        "timing_note": "ms_per_step / value = ONE region of exactly `steps` steps, bracketed by barrier + synchronize; with --full, "
                       "median_ms_per_step = the MEDIAN of `timed_regions` such regions (the first one included; at least 3 regions "
                       "and 0.25 s unless the first region alone takes 1 s)",
    }
    for key in ("planted_occurrences_found", "median_ms_per_step", "timed_regions", "timed_regions_ms_per_step", "roofline",
                "counts_equal_bitpar", "counts_equal_closed_form_k0", "sieve", "variants"):
        if key in head:
            line[key] = head[key]
    if cpu1 is not None:
        line["cpu_baseline"] = cpu1
        line["cpu_baseline_all_cores"] = cpu_all
    if per_config:
        line["per_config"] = per_config
    if args.full:
        line["valu_peak"] = {"lane_ops_per_s_2cycle_class": VALU_PEAK_LANE_OPS, "lane_ops_per_s_4cycle_class": VALU_PACKED_CLASS_LANE_OPS,
                             "share_of_2cycle_class": VALU_MIX_F2,
                             "ceiling_lane_ops_per_s": {kname: valu_ceiling(kname) for kname in VALU_MIX_F2},
                             "source": "class rates measured by tools/valu_probe.hip (profiles/r02/valu_probe.txt); class mix of each kernel's loops from "
                                       "the gfx950 disassembly (tools/valu_mix.py, profiles/r03/valu_mix.txt); valu_frac = VALU wave-instructions "
                                       "(per-column counts that matched SQ_INSTS_VALU within 3 %: profiles/r02/pmc_fulldp_cfg2.txt) x 64 lanes / "
                                       "kernel time / the ceiling of the kernel's own mix"}

    print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
