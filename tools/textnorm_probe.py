"""Measurement aid (GPU box): what the text-normalisation pass and the position map cost.
A 1 GiB device text laid out as 60-column FASTA (synthetic DNA, a '\\n' behind every 60 bytes, a header every 64 MiB) is
normalised with APM_TEXT_FASTA and with FASTA | UPPER; the same run times a device-to-device copy of 1 GiB (torch's
copy_ of a contiguous tensor: one hipMemcpyAsync), the floor for reading and writing the text once; then hand-made
records at random positions of the normalised text are mapped back, 10^4 and 10^6 of them.
    python tools/textnorm_probe.py [out.txt] [GiB, default 1]
Times are apm_get_stat's "norm_ms" / "map_ms" (HIP events around the launches; norm_ms includes the pass's one host
synchronisation) and, for the pass, the host clock around the call and a stream synchronise.  Not part of the product or
the test-suite."""
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

apm = importlib.import_module("inf560-approximate-pattern-matching_amd")

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(float(sys.argv[2]) * (1 << 30)) if len(sys.argv) > 2 else 1 << 30
REPS = 12
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = apm.ApmContext(device=0)
ctx.set_stream(stream.cuda_stream)

src = torch.empty(n + 16, dtype=torch.uint8, device=dev)
dst = torch.empty(n + 16, dtype=torch.uint8, device=dev)
ctx.synth_fill_device(src.data_ptr(), 0, n, 12345)
torch.cuda.synchronize()
src[60:n:61] = 10                                             # 60 sequence bytes and a '\n' per line
header = torch.tensor(list(b"\n>chrN synthetic record, sixty-four MiB of sequence behind it\n"), dtype=torch.uint8, device=dev)
n_headers = 0
for at in range(0, n - len(header), 64 << 20):
    src[at:at + len(header)] = header                         # (the '\n' in front makes the '>' a line start)
    n_headers += 1
torch.cuda.synchronize()
say("text: %d bytes, 60-column FASTA, %d headers" % (n, n_headers))


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def time_copy():
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        dst[:n].copy_(src[:n])
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms[2:]


def time_norm(flags):
    ev, wall, kept = [], [], 0
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept = ctx.normalize_device(src.data_ptr(), n, flags, dst.data_ptr(), n)
        ctx.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ctx.stat("norm_ms"))
    return ev[2:], wall[2:], kept


gib = n / float(1 << 30)
copy_a = time_copy()
results = {}
for name, flags in (("FASTA", apm.APM_TEXT_FASTA), ("FASTA|UPPER", apm.APM_TEXT_FASTA | apm.APM_TEXT_UPPER)):
    results[name] = time_norm(flags)
copy_b = time_copy()                                          # (the copy before and behind the passes: the spread of the floor)
copy_ms = med(copy_a + copy_b)
say("device-to-device copy: median %.3f ms, min %.3f ms per %.2f GiB (%.0f GB/s read + written)"
    % (copy_ms, min(copy_a + copy_b), gib, 2 * n / (copy_ms * 1e-3) / 1e9))
for name, (ev, wall, kept) in results.items():
    say("normalise %-11s: norm_ms median %.3f, min %.3f (%.3f ms per GiB); host clock median %.3f ms; kept %d of %d bytes; %.2f x the copy"
        % (name, med(ev), min(ev), med(ev) / gib, med(wall), kept, n, med(ev) / copy_ms))

kept = ctx.normalize_device(src.data_ptr(), n, apm.APM_TEXT_FASTA, dst.data_ptr(), n)
ctx.synchronize()
gen = torch.Generator(device=dev)
gen.manual_seed(7)
for n_rec in (10 ** 4, 10 ** 6):
    pristine = torch.zeros((n_rec, 2), dtype=torch.int64, device=dev)
    pristine[:, 0] = torch.randint(0, kept, (n_rec,), generator=gen, device=dev, dtype=torch.int64)
    rec = torch.empty_like(pristine)
    d_n = torch.tensor([n_rec, 0], dtype=torch.int64, device=dev)
    ms = []
    for _ in range(REPS):
        rec.copy_(pristine)
        ctx.map_positions_device(rec.data_ptr(), n_rec, d_n.data_ptr())
        ctx.synchronize()
        ms.append(ctx.stat("map_ms"))
    moved = rec[:, 0] - pristine[:, 0]
    assert bool((moved > 0).all()) and bool((rec[:, 0] < n).all())     # every position moved behind at least one header
    say("map %7d records: map_ms median %.3f, min %.3f (%.2f ns per record)" % (n_rec, med(ms[2:]), min(ms[2:]), med(ms[2:]) * 1e6 / n_rec))
ctx.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
