"""Measurement aid (GPU box): what the sequence index and the locate pass cost beside the normalisation pass.
A 1 GiB device text laid out as 60-column FASTA (synthetic DNA, a '\\n' behind every 60 bytes, a header every 256 KiB: a
few thousand sequences) is normalised with APM_TEXT_FASTA; IN THE SAME RUN the sequence table is built over it, and
hand-made records at random source offsets are located, 10^4 and 10^6 of them.
    python tools/seqindex_probe.py [out.txt] [GiB, default 1]
Times are apm_get_stat's "norm_ms", "seq_index_ms" and "locate_ms" (HIP events around the launches; the first two include
their pass's one host synchronisation), medians of the runs behind two warm-up runs.  Not part of the product or the
test-suite."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

apm = importlib.import_module("inf560-approximate-pattern-matching_amd")

out_path = sys.argv[1] if len(sys.argv) > 1 else None
n = int(float(sys.argv[2]) * (1 << 30)) if len(sys.argv) > 2 else 1 << 30
REPS = 12
EVERY = 256 << 10
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(device=dev)
torch.cuda.set_stream(stream)
ctx = apm.ApmContext(device=0)
ctx.set_stream(stream.cuda_stream)
ctx.set_patterns([b"ACGTACGTACGTACGTACGT", b"ACGT" * 75], 2)   # (the locate pass takes the pattern lengths from the set)

src = torch.empty(n + 16, dtype=torch.uint8, device=dev)
dst = torch.empty(n + 16, dtype=torch.uint8, device=dev)
ctx.synth_fill_device(src.data_ptr(), 0, n, 12345)
torch.cuda.synchronize()
src[60:n:61] = 10                                             # 60 sequence bytes and a '\n' per line
header = torch.tensor(list(b"\n>seqN synthetic sequence, a quarter MiB of lines behind it\n"), dtype=torch.uint8, device=dev)
n_headers = 0
for at in range(0, n - len(header), EVERY):
    src[at:at + len(header)] = header                         # (the '\n' in front makes the '>' a line start)
    n_headers += 1
torch.cuda.synchronize()
say("text: %d bytes, 60-column FASTA, %d headers" % (n, n_headers))
gib = n / float(1 << 30)

table = torch.empty((n_headers + 2, 2), dtype=torch.int64, device=dev)
norm, index = [], []
kept = n_seq = 0
for _ in range(REPS):
    kept = ctx.normalize_device(src.data_ptr(), n, apm.APM_TEXT_FASTA, dst.data_ptr(), n)
    ctx.synchronize()
    norm.append(ctx.stat("norm_ms"))
    n_seq = ctx.index_sequences_device(table.data_ptr(), n_headers + 2)
    ctx.synchronize()
    index.append(ctx.stat("seq_index_ms"))
assert n_seq == n_headers + 1 and int(table[n_seq, 0]) == n and int(table[n_seq, 1]) == kept
assert int(table[1, 0]) == 1 and int(table[2, 0]) == EVERY + 1
norm, index = norm[2:], index[2:]
say("normalise FASTA : norm_ms median %.3f, min %.3f (%.3f ms per GiB); kept %d of %d bytes" % (med(norm), min(norm), med(norm) / gib, kept, n))
say("index sequences : seq_index_ms median %.3f, min %.3f (%.3f ms per GiB); n_seq %d; %.2f x the normalisation pass"
    % (med(index), min(index), med(index) / gib, n_seq, med(index) / med(norm)))

gen = torch.Generator(device=dev)
gen.manual_seed(7)
for n_rec in (10 ** 4, 10 ** 6):
    rec = torch.zeros((n_rec, 2), dtype=torch.int64, device=dev)
    rec[:, 0] = torch.randint(0, n, (n_rec,), generator=gen, device=dev, dtype=torch.int64)     # (some fall on dropped bytes)
    loc = torch.empty((n_rec, 2), dtype=torch.int64, device=dev)
    d_n = torch.tensor([n_rec, 0], dtype=torch.int64, device=dev)
    ms = []
    for _ in range(REPS):
        ctx.locate_records_device(rec.data_ptr(), n_rec, d_n.data_ptr(), table.data_ptr(), n_seq, loc.data_ptr())
        ctx.synchronize()
        ms.append(ctx.stat("locate_ms"))
    seq = loc[:, 1] & 0xFFFFFFFF
    valid = seq != 0xFFFFFFFF
    assert bool((seq[valid] == rec[valid, 0] // EVERY + 1).all()) and 0.9 < float(valid.float().mean()) < 1.0
    say("locate %7d records: locate_ms median %.3f, min %.3f (%.2f ns per record); %.1f %% name a kept byte"
        % (n_rec, med(ms[2:]), min(ms[2:]), med(ms[2:]) * 1e6 / n_rec, 100.0 * float(valid.float().mean())))
ctx.close()
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
