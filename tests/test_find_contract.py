"""The host-level find calls refuse what they refuse, in the words they use, and hand back what they found by one rule:
apm_find_buffer, apm_find_all_buffer, apm_find_all_dist_buffer, apm_find_all_align_buffer, apm_find_best_buffer,
apm_find_occ_buffer and apm_find_occ_align_buffer, each driven through every refusal it has -- status and message, with
nothing of the caller's written -- then through a capacity of 0 and of one record short, the row copy at a stride wider
than the row, and the agreement of the three window modes.  tests/test_entry_contract.py does the same for the device-level
calls.  Every call goes through the C ABI into buffers preset to a sentinel byte, so "untouched" can be seen."""
import ctypes
import os
import random
import types

import pytest

import helpers as H

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, STATE = 0, -1, -6, -8
N, K, RADIUS, CAP = 384, 2, 4, 96
ALL, LOCAL_MIN = 0, 1
FILL = 0xA5
SENT, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NO_PATTERNS = "apm_set_patterns has not been called"
ENTRY = {"find": "apm_find_buffer", "all": "apm_find_all_buffer", "dist": "apm_find_all_dist_buffer", "align": "apm_find_all_align_buffer",
         "best": "apm_find_best_buffer", "occ": "apm_find_occ_buffer", "occ_align": "apm_find_occ_align_buffer"}
ROW_CALLS = {"align": "apm_align_row_words", "best": "apm_align_row_words", "occ_align": "apm_occ_align_row_words"}


def make_case():
    """384 bytes of ACGT with an exact copy and a copy at one edit of each of three patterns of 8, 12 and 16 bytes"""
    rng = random.Random(560)
    pats = [bytes(rng.choice(b"ACGT") for _ in range(m)) for m in (8, 12, 16)]
    text = bytearray(rng.choice(b"ACGT") for _ in range(N))
    for at, (i, edits) in zip((20, 70, 130, 190, 250, 320), ((0, 0), (1, 1), (2, 0), (0, 1), (1, 0), (2, 1))):
        w = bytearray(pats[i])
        for e in rng.sample(range(len(w)), edits):
            w[e] = rng.choice([c for c in b"ACGT" if c != w[e]])
        text[at:at + len(w)] = w
    return pats, bytes(text)


def align_words(n_ops):
    """apm_align_words of include/apm.h: the count and 16 ops per dword"""
    return 1 + -(-n_ops // 16)


class Calls:
    """the seven calls over one context and one text; every argument has its valid default, a case overrides the one it
    is about.  `null` names the pointers handed over as NULL: ctx, text, found, matches (n_matches of the best-hit call), out,
    start, ops."""

    def __init__(self, apm, ctx, text, n_patterns):
        self.apm, self.lib, self.ctx, self.text, self.n_patterns = apm, apm.load_library(), ctx, text, n_patterns
        self.words = {"align": 0, "best": 0, "occ_align": 0}

    def set_words(self):
        self.words = {"align": self.ctx.align_row_words(), "best": self.ctx.align_row_words(), "occ_align": self.ctx.occ_align_row_words()}

    def last_error(self):
        return (self.lib.apm_last_error(self.ctx._ctx) or b"").decode()

    def call(self, name, cap=CAP, null=(), stride=None, flags=LOCAL_MIN, radius=RADIUS, index=0, rows=True):
        c, M = ctypes, self.apm.ApmMatch

        def preset(kind, n):
            buf = (kind * max(n, 1))()
            c.memset(buf, FILL, c.sizeof(buf))
            return buf

        def arg(key, v):
            return None if key in null else v

        rows = rows and name in self.words
        stride = (self.words[name] if rows else 0) if stride is None else stride
        out, start, pos, ops = preset(M, cap), preset(M, cap), preset(c.c_uint64, cap), preset(c.c_uint32, cap * stride)
        found, matches, counts = preset(c.c_uint64, 1), preset(c.c_uint64, 1), preset(c.c_uint64, self.n_patterns)
        head = (arg("ctx", self.ctx._ctx), arg("text", self.text), len(self.text))
        p_found = arg("found", c.cast(found, c.POINTER(c.c_uint64)))
        p_ops = arg("ops", ops) if rows else None
        L = self.lib
        if name == "find":
            rc = L.apm_find_buffer(*head, index, arg("out", pos), cap, p_found)
        elif name in ("all", "dist"):
            rc = getattr(L, ENTRY[name])(*head, arg("out", out), cap, p_found)
        elif name == "align":
            rc = L.apm_find_all_align_buffer(*head, arg("out", out), cap, p_found, p_ops, stride)
        elif name == "best":
            rc = L.apm_find_best_buffer(*head, radius, arg("out", out), cap, p_found, arg("matches", c.cast(matches, c.POINTER(c.c_uint64))), p_ops, stride)
        elif name == "occ":
            rc = L.apm_find_occ_buffer(*head, flags, arg("out", out), arg("start", start), cap, p_found, counts)
        else:
            rc = L.apm_find_occ_align_buffer(*head, flags, arg("out", out), arg("start", start), cap, p_found, counts, p_ops, stride)
        r = types.SimpleNamespace(rc=rc, name=name, cap=cap, stride=stride, found=found[0], matches=matches[0], counts=list(counts),
                                  pos=list(pos), rec=[(m.pattern, m.pos, m.reserved) for m in out],
                                  start=[(m.pattern, m.pos, m.reserved) for m in start],
                                  rows=[list(ops[q * stride:(q + 1) * stride]) for q in range(cap)] if stride else [], raw_ops=list(ops))
        # the call's total (the best-hit call counts its matches beside its best hits) and its records, slot by slot
        r.total = r.matches if name == "best" else r.found
        r.slots = r.pos if name == "find" else r.rec
        return r


def stored_nothing(r, from_slot=0):
    """the record, start, position and row slots from `from_slot` on are as they were handed over"""
    blank = (SENT, SENT64, SENT)
    return (all(p == SENT64 for p in r.pos[from_slot:]) and all(m == blank for m in r.rec[from_slot:]) and
            all(m == blank for m in r.start[from_slot:]) and all(w == SENT for w in r.raw_ops[from_slot * r.stride:]))


def refused(calls, name, status, message, **args):
    r = calls.call(name, **args)
    assert r.rc == status, (name, args, r.rc, calls.last_error())
    if message is not None:
        assert calls.last_error() == message, (name, args)
    assert stored_nothing(r) and r.found == SENT64 and r.matches == SENT64 and all(v == SENT64 for v in r.counts), (name, args)


def two_shard_context(apm):
    """APM_DEVICES=0,0 as tests/test_entry_contract.py builds one: two shards that share device 0"""
    os.environ["APM_DEVICES"] = "0,0"
    try:
        return apm.ApmContext(n_devices=0)
    finally:
        del os.environ["APM_DEVICES"]


@pytest.fixture(scope="module")
def apm():
    a = H.pkg()
    assert a.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return a


@pytest.fixture(scope="module")
def calls(apm):
    pats, text = make_case()
    with apm.ApmContext(device=0) as ctx:
        ctx.set_patterns(pats, K)
        c = Calls(apm, ctx, text, len(pats))
        c.pats = pats
        c.set_words()
        yield c


@pytest.fixture(scope="module")
def full(calls):
    """every call's whole answer at a capacity that holds it, computed once: name -> result"""
    out = {}
    for name in ENTRY:
        r = calls.call(name)
        assert r.rc == OK, (name, calls.last_error())
        assert 3 <= r.found <= CAP and r.found <= r.total <= CAP, (name, r.found, r.total)
        have = r.slots[:r.found]
        assert have == sorted(have) and len(set(have)) == len(have), name
        out[name] = r
    return out


def test_refusals(apm):
    pats, text = make_case()
    with apm.ApmContext(device=0) as ctx:
        calls = Calls(apm, ctx, text, len(pats))

        # ---- no context: the status alone
        for name in ENTRY:
            assert calls.call(name, null=("ctx",)).rc == INVALID, name

        # ---- patterns not set
        for name in ENTRY:
            refused(calls, name, STATE, NO_PATTERNS)

        ctx.set_patterns(pats, K)
        calls.set_words()

        # ---- a two-shard context: the calls that need the whole text on one device, each in its own words
        two = two_shard_context(apm)
        try:
            two.set_patterns(pats, K)
            c2 = Calls(apm, two, text, len(pats))
            c2.words = calls.words
            refused(c2, "best", UNSUPPORTED, "apm_find_best_buffer needs a single-device context: the resident shards' halo is m_max - 1, the pass needs "
                                             "the radius more on both sides")
            for name in ("occ", "occ_align"):
                refused(c2, name, UNSUPPORTED, ENTRY[name] + " needs a single-device context: the resident shards bring a right halo, the "
                                                             "occurrence scan needs a left one")
        finally:
            two.close()

        # ---- bad arguments: a NULL n_found, NULL records with a capacity, a NULL text with a length, NULL rows with a capacity
        for name, entry in ENTRY.items():
            bad = "bad argument to " + entry
            refused(calls, name, INVALID, bad, null=("found",))
            refused(calls, name, INVALID, bad, null=("out",))
            refused(calls, name, INVALID, bad, null=("text",))
        refused(calls, "find", INVALID, "bad argument to apm_find_buffer", index=-1)
        refused(calls, "find", INVALID, "bad argument to apm_find_buffer", index=len(pats))
        refused(calls, "best", INVALID, "bad argument to apm_find_best_buffer", null=("matches",))
        refused(calls, "align", INVALID, "bad argument to apm_find_all_align_buffer", null=("ops",))
        refused(calls, "occ_align", INVALID, "bad argument to apm_find_occ_align_buffer", null=("ops",))
        refused(calls, "occ_align", INVALID, "bad argument to apm_find_occ_align_buffer", null=("start",))

        # ---- a stride one short of a row, unknown occurrence flags, a radius beyond the largest
        for name, fn in ROW_CALLS.items():
            w = calls.words[name]
            assert w >= 2
            refused(calls, name, INVALID, "stride_words %d is less than %s() = %d" % (w - 1, fn, w), stride=w - 1)
        for name in ("occ", "occ_align"):
            refused(calls, name, INVALID, "unknown occurrence flags 0x2", flags=2)
            refused(calls, name, INVALID, "unknown occurrence flags 0xfffffffe", flags=0xFFFFFFFE)
        refused(calls, "best", INVALID, "radius %d is beyond APM_BEST_MAX_RADIUS = %d" % (apm.APM_BEST_MAX_RADIUS + 1, apm.APM_BEST_MAX_RADIUS),
                radius=apm.APM_BEST_MAX_RADIUS + 1)

        # ---- apm_find_buffer in a text mode
        ctx.set_text_mode(apm.APM_TEXT_UPPER)
        try:
            refused(calls, "find", UNSUPPORTED, "apm_find_buffer does not serve a text mode (apm_set_text_mode): use apm_find_all_buffer")
        finally:
            ctx.set_text_mode(0)

        # ---- after all of that the context still serves every call
        for name in ENTRY:
            r = calls.call(name)
            assert r.rc == OK and r.found >= 3, (name, calls.last_error())


def test_the_whole_answers(calls, full):
    """what the other tests compare against is the truth: the window calls find the oracle's windows at the oracle's
    distances, one position list is one pattern's, and the occurrence calls' counts are their records'"""
    want = [(i, j) for i, p in enumerate(calls.pats) for j in H.oracle_positions(calls.text, p, K)]
    assert [(i, j) for i, j, _ in full["all"].rec[:full["all"].found]] == want
    assert full["find"].pos[:full["find"].found] == [j for i, j in want if i == 0]
    for i, j, d in full["dist"].rec[:full["dist"].found]:
        p = calls.pats[i]
        size = min(len(p), N - j)
        assert d == H.window_distance(p[:size], calls.text[j:j + size]) <= K, (i, j)
    best = full["best"]
    assert best.total == len(want) and set((i, j) for i, j, _ in best.rec[:best.found]) <= set(want)
    for name in ("occ", "occ_align"):
        r = full[name]
        assert r.counts == [sum(1 for i, _, _ in r.rec[:r.found] if i == q) for q in range(len(calls.pats))], name
    assert full["occ"].rec == full["occ_align"].rec and full["occ"].start == full["occ_align"].start


def test_capacity_zero_counts_and_stores_nothing(calls, full):
    for name in ENTRY:
        for null in ((), ("out", "start", "ops")):                # (no capacity: no record pointer is needed)
            r = calls.call(name, cap=0, null=null)
            assert r.rc == OK, (name, null, calls.last_error())
            assert r.total == full[name].total, (name, null)
            assert stored_nothing(r), (name, null)
            if name in ("occ", "occ_align"):
                assert r.counts == full[name].counts, (name, null)


def test_capacity_one_short(calls, full):
    """the true total, and `capacity` records of the whole answer, sorted, each with its own start and row.  WHICH record
    is left out is the device's choice (include/apm.h: "an arbitrary subset"): the kernels append in no order, and on the
    MI355X this case lost (0, 21), the third of 19 windows, (0, 255), the second of 9 ends, and position 21 in one run and
    190 in the next of the one-pattern call -- not the last record.  So the records kept are not the first `capacity` of the
    sorted answer, and this does not ask that.  The best-hit call is one record short of its MATCHES: its best hits are
    those of the 18 records examined, all of the true ones or all but one."""
    for name in ENTRY:
        whole = full[name]
        cap = whole.total - 1
        r = calls.call(name, cap=cap)
        kept = min(r.found, cap)
        print(name, "capacity", cap, "found", r.found, "total", r.total, "left out", [s for s in whole.slots[:whole.found] if s not in r.slots[:kept]])
        assert r.rc == OK, (name, calls.last_error())
        assert r.total == whole.total, name
        if name == "best":
            assert whole.found - 1 <= r.found <= whole.found <= cap, name
        else:
            assert r.found == whole.total and kept == cap, name
        have = r.slots[:kept]
        assert have == sorted(have) and len(set(have)) == kept, name
        for q, s in enumerate(have):
            assert s in whole.slots[:whole.found], (name, s)
            at = whole.slots.index(s)
            if name in ("occ", "occ_align"):
                assert r.start[q] == whole.start[at], (name, s)
            if r.stride:
                assert r.rows[q] == whole.rows[at], (name, s)
        if name in ("occ", "occ_align"):
            assert r.counts == whole.counts, name
        assert stored_nothing(r, from_slot=kept), name


@pytest.mark.parametrize("name", ["align", "best"])
def test_row_copy_at_a_wider_stride(calls, full, name):
    """a row's defined words are those of a run at the row's own width; every word behind them, in the rows behind the last
    record too, stays the caller's (tests/test_occ_align_gpu.py does this for the occurrence scripts)"""
    tight = full[name]
    words = calls.words[name]
    assert tight.stride == words
    wide = calls.call(name, stride=words + 3)
    assert wide.rc == OK, calls.last_error()
    assert (wide.found, wide.total, wide.rec) == (tight.found, tight.total, tight.rec)
    for q in range(tight.found):
        used = align_words(tight.rows[q][0])
        assert 2 <= used <= words, (name, q)
        assert tight.rows[q][used:] == [SENT] * (words - used), (name, q)
        assert wide.rows[q] == tight.rows[q][:used] + [SENT] * (words + 3 - used), (name, q)
    assert all(row == [SENT] * (words + 3) for row in wide.rows[tight.found:]), "rows without a record were written"
    assert all(row == [SENT] * words for row in tight.rows[tight.found:]), "rows without a record were written"


def test_the_window_modes_agree(full):
    """plain, with distances, with scripts: the same (pattern, pos) list; the same distances in the two that report them"""
    plain, dist, align = (full[name] for name in ("all", "dist", "align"))
    assert plain.found == dist.found == align.found and plain.total == dist.total == align.total
    assert [m[:2] for m in plain.rec] == [m[:2] for m in dist.rec] == [m[:2] for m in align.rec]
    assert dist.rec == align.rec
    for q in range(align.found):                                  # (a script's ops that are not '=' are its distance)
        row = align.rows[q]
        ops = [(row[1 + j // 16] >> (2 * (j % 16))) & 3 for j in range(row[0])]
        assert sum(1 for op in ops if op) == align.rec[q][2], q
