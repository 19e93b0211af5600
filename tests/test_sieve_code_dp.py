"""The code-filter sieve's third stage -- the window DP on codes for units of short patterns (m + 2k <= 30), run on
a per-wave queue of entries -- must hand over every window the banded DP would count, and each candidate once: AUTO
(sieve + code filter + window DP + verify) against the forced full-DP BITPAR kernel, on short patterns planted with
edits at every offset around block seams, patterns that share key words, duplicate patterns, tandem repeats, and shard
cuts that are not block aligned.

The text here is 6 MiB = 1536 blocks of 4 KiB.  A sieve pass that fills the device runs several thousand waves, each
with the blocks w, w + W, ...: on a full device every wave of this test sees ONE block, starts with an empty queue and
flushes it at the end of its run.  The queue carried from one block into the next is the subject of
test_sieve_code_dp_queue.py, which sizes its text from the wave count the launch reports."""
import random

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

K = 3
SHORT = [16, 20, 21, 22, 23, 24]                     # DP slots go to the units of these (m + 2k <= 30)
LONG = [34, 41, 49, 56, 63, 70, 77, 85, 92, 99, 106, 114, 121, 128]


@pytest.fixture(scope="module")
def apm():
    return H.pkg()


def _edit(rnd, p, alpha, n_edits):
    p = bytearray(p)
    for _ in range(n_edits):
        r, pos = rnd.random(), rnd.randrange(len(p))
        if r < 0.4:
            p[pos] = rnd.choice(alpha)
        elif r < 0.7 and len(p) > 1:
            del p[pos]
        else:
            p.insert(pos, rnd.choice(alpha))
    return bytes(p)


def _case(seed, alpha):
    rnd = random.Random(seed)
    n = (6 << 20) + 1234
    text = bytearray(rnd.choice(alpha) for _ in range(n)) if len(alpha) > 4 else bytearray(
        alpha[b & 3] for b in random.Random(seed + 1).randbytes(n))
    pats = [bytes(rnd.choice(alpha) for _ in range(m)) for m in SHORT + LONG]
    pats.append(pats[1])                                       # a duplicate of a short pattern
    pats.append(pats[0][:-1] + bytes([alpha[(alpha.index(pats[0][-1]) + 1) % len(alpha)]]))  # shares most key words
    pats.append(pats[2][:8] + pats[3][8:22])                   # shares the first unit's words with another short one
    shorts = [p for p in pats if len(p) <= 24]
    # plants around the block seams (4 KiB from the text start and from the shard cuts below): every offset from
    # -(m + 8) to +8 of a seam, 0..k edits
    at = 4096 * 8
    for d in range(-40, 9):
        for p in shorts:
            w = _edit(rnd, p, alpha, rnd.randint(0, K))
            pos = at + d
            text[pos:pos + len(w)] = w
            at += 4096
    # tandem repeats of short patterns: bursts of entries (queue and list-region pressure) and of matches
    for i, p in enumerate(shorts[:4]):
        off = (5 << 20) + i * 40000
        rep = (p * (30000 // len(p) + 1))[:30000]
        text[off:off + len(rep)] = rep
    return bytes(text), pats


@pytest.mark.parametrize("seed,alpha", [(1, b"ACGT"), (2, b"ACGT"), (3, b"ACDEFGHIKLMNPQRSTVWY")])
def test_sieve_code_dp_vs_bitpar(apm, seed, alpha):
    import torch
    text, pats = _case(seed, alpha)
    n = len(text)
    host = torch.frombuffer(bytearray(text), dtype=torch.uint8)
    d_text = torch.zeros(n + 4096 + 64, dtype=torch.uint8, device="cuda:0")
    d_text[:n] = host.to("cuda:0")
    cnt = torch.zeros(len(pats), dtype=torch.int64, device="cuda:0")
    # (global shard begin, shard end): the whole text, and a cut 16-byte aligned but not block aligned with unaligned owners
    cuts = [(0, n, 0, n), (4096 * 9 + 48, n - 777, 4096 * 9 + 48 + 24, n - 777 - 131)]  # (a halo of m_max - 1 behind the owners)
    with apm.ApmContext(device=0) as c:
        c.set_patterns(pats, K)
        assert c.stat("sieve_on") == 1 and c.stat("sieve_stride") == 1
        for lo, hi, own_b, own_e in cuts:
            got = {}
            for variant in ("auto", "bitpar"):
                c.set_kernel(variant)
                cnt.zero_()
                torch.cuda.synchronize()
                c.count_shard_device(d_text.data_ptr() + lo, lo, hi - lo, n, own_b, own_e, cnt.data_ptr())
                c.synchronize()
                got[variant] = cnt.cpu().tolist()
                if variant == "auto":
                    assert c.stat("sieve_cf") > 0 and c.stat("sieve_cf_dp_slots") > 0, "the window-DP stage did not run"
            assert got["auto"] == got["bitpar"], (seed, lo, hi, [len(p) for p in pats])
            assert sum(got["auto"][:len(SHORT)]) >= 40 * len(SHORT)
