"""ctypes binding of the C ABI in include/apm.h (libapm_hip.so).

This is glue for tests/ and bench.py only: the product is the C ABI and the C
host `host/apm_parallel`.  It mirrors the ABI one to one (same names, argument
meaning and error behaviour) and raises ApmError on any negative apm_status.
There is NO CPU fallback: if the HIP library is missing or no device is
visible, everything here fails loudly.

Load order matters in a process that also uses torch: torch bundles its own
libamdhip64.so.7; importing torch FIRST makes libapm_hip.so bind to that same
runtime instance (same SONAME), so torch device pointers and streams can be
handed to the C ABI.  The package therefore imports torch (if present) before
dlopen()ing the library.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("APM_LIB_PATH") or os.path.join(_HERE, "libapm_hip.so")  # APM_LIB_PATH: A/B builds

APM_KERNEL_AUTO, APM_KERNEL_GENERIC, APM_KERNEL_WAVEFRONT, APM_KERNEL_BITPAR, APM_KERNEL_BANDED, APM_KERNEL_NFA = range(6)
KERNEL_NAMES = {0: "auto", 1: "generic", 2: "wavefront", 3: "bitpar", 4: "banded", 5: "nfa"}
KERNEL_IDS = {v: k for k, v in KERNEL_NAMES.items()}
APM_TEXT_FASTA, APM_TEXT_UPPER = 1, 2  # text modes (apm_set_text_mode, apm_normalize_device), OR-able
APM_SEQ_NO_HEADER = (1 << 64) - 1      # hdr_off of entry 0 of a sequence table
APM_SEQ_INVALID = 0xFFFFFFFF           # seq of the location of a record that names no window
APM_LOC_SPANS, APM_LOC_TRUNCATED = 1, 2  # flags of a location, OR-able
APM_BEST_MAX_RADIUS = 64               # the largest radius of the best-hit pass
APM_OCC_ALL, APM_OCC_LOCAL_MIN = 0, 1  # flags of the occurrence search: every end within k / the first end of every local minimum
APM_OCC_MAX_PATTERN_LEN = 128          # the longest pattern the occurrence search serves
APM_OCC_NO_START = (1 << 64) - 1       # pos of the span record of an end that is no occurrence
APM_NEAREST_NONE = (1 << 64) - 1       # the key of a pattern no end of the text is nearer to than the empty substring


def nearest_key(dist, end):
    """the nearest-occurrence search's key (include/apm.h: "nearest occurrences"): the smaller key is the better answer"""
    return (dist << 56) | end


def nearest_dist(key):
    """APM_NEAREST_DIST"""
    return key >> 56


def nearest_end(key):
    """APM_NEAREST_END"""
    return key & ((1 << 56) - 1)

# every symbol include/apm.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "apm_device_count", "apm_abi_version", "apm_create", "apm_create_on_device", "apm_destroy",
    "apm_last_error", "apm_set_stream", "apm_set_patterns", "apm_set_kernel", "apm_set_partition", "apm_count_buffer",
    "apm_count_file", "apm_find_buffer", "apm_find_all_buffer", "apm_find_all_dist_buffer", "apm_find_all_align_buffer", "apm_find_best_buffer", "apm_best_shard_device", "apm_find_occ_buffer", "apm_occ_shard_device", "apm_occ_spans_device", "apm_occ_align_row_words", "apm_occ_align_device", "apm_find_occ_align_buffer", "apm_find_nearest_buffer", "apm_nearest_shard_device", "apm_nearest_records_device", "apm_find_nearest_seq_buffer", "apm_nearest_seq_shard_device", "apm_nearest_seq_records_device", "apm_find_occ_seq_buffer", "apm_occ_seq_shard_device", "apm_occ_seq_spans_device", "apm_find_shard_device", "apm_score_shard_device", "apm_align_shard_device", "apm_align_row_words", "apm_count_shard_device", "apm_shard_range", "apm_synth_fill_device",
    "apm_synth_fill_host", "apm_count_synthetic", "apm_set_timing", "apm_get_timing", "apm_get_launch_times", "apm_get_stat",
    "apm_pattern_kernel", "apm_set_text_mode", "apm_normalize_device", "apm_map_positions_device",
    "apm_index_sequences_device", "apm_locate_records_device", "apm_locate_buffer", "apm_get_sequences",
    "apm_device_alloc", "apm_device_free", "apm_device_upload", "apm_device_download",
    "apm_device_memset", "apm_synchronize",
]


class ApmError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("apm status %d: %s" % (status, message))
        self.status = status


class ApmTiming(ctypes.Structure):
    _fields_ = [("total_ms", ctypes.c_double), ("h2d_ms", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("reduce_ms", ctypes.c_double), ("main_kernel_ms", ctypes.c_double),
                ("text_bytes", ctypes.c_uint64), ("windows", ctypes.c_uint64),
                ("cells_algorithmic", ctypes.c_double), ("cells_evaluated", ctypes.c_double),
                ("n_devices", ctypes.c_int), ("n_launches", ctypes.c_int)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ApmMatch(ctypes.Structure):
    """apm_match of include/apm.h: 16 bytes"""
    _fields_ = [("pos", ctypes.c_uint64), ("pattern", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ApmSeq(ctypes.Structure):
    """apm_seq of include/apm.h: 16 bytes, one entry of a sequence table"""
    _fields_ = [("hdr_off", ctypes.c_uint64), ("t_begin", ctypes.c_uint64)]


class ApmLoc(ctypes.Structure):
    """apm_loc of include/apm.h: 16 bytes, where a record lies: sequence, offset inside it, flags"""
    _fields_ = [("off", ctypes.c_uint64), ("seq", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


_lib = None


def load_library():
    """dlopen libapm_hip.so (after torch, see module docstring)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ApmError(-2, "HIP extension %s is missing: run `make -C %s` (no CPU fallback exists)" % (LIB_PATH, _HERE))
    try:
        import torch  # noqa: F401  (binds libamdhip64.so.7 first)
    except Exception:
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    c = ctypes
    vp, u64, i32 = c.c_void_p, c.c_uint64, c.c_int
    sig = {
        "apm_device_count": (i32, []),
        "apm_abi_version": (i32, []),
        "apm_create": (i32, [c.POINTER(vp), i32]),
        "apm_create_on_device": (i32, [c.POINTER(vp), i32]),
        "apm_destroy": (None, [vp]),
        "apm_last_error": (c.c_char_p, [vp]),
        "apm_set_stream": (i32, [vp, vp]),
        "apm_set_patterns": (i32, [vp, i32, c.POINTER(c.c_char_p), c.POINTER(i32), i32]),
        "apm_set_kernel": (i32, [vp, i32]),
        "apm_set_partition": (i32, [vp, i32]),
        "apm_count_buffer": (i32, [vp, vp, u64, c.POINTER(u64)]),
        "apm_count_file": (i32, [vp, c.c_char_p, c.POINTER(u64)]),
        "apm_find_buffer": (i32, [vp, vp, u64, i32, c.POINTER(u64), u64, c.POINTER(u64)]),
        "apm_find_all_buffer": (i32, [vp, vp, u64, c.POINTER(ApmMatch), u64, c.POINTER(u64)]),
        "apm_find_all_dist_buffer": (i32, [vp, vp, u64, c.POINTER(ApmMatch), u64, c.POINTER(u64)]),
        "apm_find_shard_device": (i32, [vp, vp, u64, u64, u64, u64, u64, vp, u64, vp, vp]),
        "apm_score_shard_device": (i32, [vp, vp, u64, u64, u64, vp, u64, vp]),
        "apm_align_row_words": (i32, [vp]),
        "apm_align_shard_device": (i32, [vp, vp, u64, u64, u64, vp, u64, vp, vp, c.c_uint32]),
        "apm_find_all_align_buffer": (i32, [vp, vp, u64, c.POINTER(ApmMatch), u64, c.POINTER(u64), c.POINTER(c.c_uint32), c.c_uint32]),
        "apm_best_shard_device": (i32, [vp, vp, u64, u64, u64, vp, u64, vp, c.c_uint32, vp, u64, vp]),
        "apm_find_best_buffer": (i32, [vp, vp, u64, c.c_uint32, c.POINTER(ApmMatch), u64, c.POINTER(u64), c.POINTER(u64),
                                       c.POINTER(c.c_uint32), c.c_uint32]),
        "apm_occ_shard_device": (i32, [vp, vp, u64, u64, u64, u64, u64, c.c_uint, vp, u64, vp, vp]),
        "apm_occ_spans_device": (i32, [vp, vp, u64, u64, u64, vp, u64, vp, vp]),
        "apm_find_occ_buffer": (i32, [vp, vp, u64, c.c_uint, c.POINTER(ApmMatch), c.POINTER(ApmMatch), u64, c.POINTER(u64), c.POINTER(u64)]),
        "apm_occ_align_row_words": (i32, [vp]),
        "apm_find_nearest_buffer": (i32, [vp, vp, u64, c.POINTER(ApmMatch), c.POINTER(ApmMatch)]),
        "apm_nearest_shard_device": (i32, [vp, vp, u64, u64, u64, u64, u64, vp]),
        "apm_nearest_records_device": (i32, [vp, vp, u64, u64, u64, vp, vp, vp]),
        "apm_find_nearest_seq_buffer": (i32, [vp, vp, u64, c.POINTER(ApmMatch), c.POINTER(ApmMatch), u64, c.POINTER(u64)]),
        "apm_nearest_seq_shard_device": (i32, [vp, vp, u64, u64, u64, u64, u64, vp, u64, vp]),
        "apm_nearest_seq_records_device": (i32, [vp, vp, u64, u64, u64, vp, u64, vp, vp, vp]),
        "apm_find_occ_seq_buffer": (i32, [vp, vp, u64, c.c_uint, c.POINTER(ApmMatch), c.POINTER(ApmMatch), c.POINTER(c.c_uint32), u64, c.POINTER(u64),
                                           c.POINTER(u64), c.POINTER(c.c_uint32), c.c_uint32]),
        "apm_occ_seq_shard_device": (i32, [vp, vp, u64, u64, u64, u64, u64, vp, u64, c.c_uint, vp, u64, vp, vp]),
        "apm_occ_seq_spans_device": (i32, [vp, vp, u64, u64, u64, vp, u64, vp, u64, vp, vp, vp]),
        "apm_occ_align_device": (i32, [vp, vp, u64, u64, u64, vp, vp, u64, vp, vp, c.c_uint32]),
        "apm_find_occ_align_buffer": (i32, [vp, vp, u64, c.c_uint, c.POINTER(ApmMatch), c.POINTER(ApmMatch), u64, c.POINTER(u64), c.POINTER(u64),
                                            c.POINTER(c.c_uint32), c.c_uint32]),
        "apm_count_shard_device": (i32, [vp, vp, u64, u64, u64, u64, u64, vp]),
        "apm_set_text_mode": (i32, [vp, c.c_uint]),
        "apm_normalize_device": (i32, [vp, vp, u64, c.c_uint, vp, u64, c.POINTER(u64)]),
        "apm_map_positions_device": (i32, [vp, vp, u64, vp]),
        "apm_index_sequences_device": (i32, [vp, vp, u64, c.POINTER(u64)]),
        "apm_locate_records_device": (i32, [vp, vp, u64, vp, vp, u64, vp]),
        "apm_locate_buffer": (i32, [vp, c.POINTER(ApmMatch), u64, c.POINTER(ApmLoc)]),
        "apm_get_sequences": (i32, [vp, c.POINTER(ApmSeq), u64, c.POINTER(u64)]),
        "apm_shard_range": (i32, [u64, i32, i32, i32, c.POINTER(u64), c.POINTER(u64)]),
        "apm_synth_fill_device": (i32, [vp, vp, u64, u64, u64]),
        "apm_synth_fill_host": (None, [vp, u64, u64, u64]),
        "apm_count_synthetic": (i32, [vp, u64, u64, c.POINTER(u64)]),
        "apm_set_timing": (i32, [vp, i32]),
        "apm_get_timing": (i32, [vp, c.POINTER(ApmTiming)]),
        "apm_get_launch_times": (i32, [vp, i32, c.POINTER(c.c_double), c.POINTER(c.c_char_p)]),
        "apm_get_stat": (i32, [vp, c.c_char_p, c.POINTER(c.c_double)]),
        "apm_pattern_kernel": (i32, [vp, i32]),
        "apm_device_alloc": (i32, [vp, c.POINTER(vp), u64]),
        "apm_device_free": (i32, [vp, vp]),
        "apm_device_upload": (i32, [vp, vp, vp, u64]),
        "apm_device_download": (i32, [vp, vp, vp, u64]),
        "apm_device_memset": (i32, [vp, vp, i32, u64]),
        "apm_synchronize": (i32, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_count():
    n = load_library().apm_device_count()
    if n < 0:
        raise ApmError(n, (load_library().apm_last_error(None) or b"").decode())
    return n


def shard_range(n_total, k, shard, n_shards):
    b, e = ctypes.c_uint64(), ctypes.c_uint64()
    rc = load_library().apm_shard_range(n_total, k, shard, n_shards, ctypes.byref(b), ctypes.byref(e))
    if rc:
        raise ApmError(rc, "apm_shard_range: invalid argument")
    return b.value, e.value


def synth_fill_host(global_off, length, seed):
    """The synthetic DNA generator's bytes for [global_off, global_off+length) (host side)."""
    buf = ctypes.create_string_buffer(length)
    load_library().apm_synth_fill_host(ctypes.cast(buf, ctypes.c_void_p), global_off, length, seed)
    return buf.raw


OP_LETTERS = "=XID"  # include/apm.h's op codes 0..3: equal, substitution, text-only byte, pattern-only byte


def unpack_ops(row):
    """a record's row of dwords (word 0 = n_ops, 16 ops per dword behind it) as bytes, one op code per byte"""
    return bytes((row[1 + j // 16] >> (2 * (j % 16))) & 3 for j in range(row[0]))


def ops_to_script(ops_bytes):
    """the run-length string apm_parallel --alignments prints: bytes([0, 0, 1, 0]) -> 2=1X1="""
    out, i = [], 0
    while i < len(ops_bytes):
        j = i
        while j < len(ops_bytes) and ops_bytes[j] == ops_bytes[i]:
            j += 1
        out.append("%d%s" % (j - i, OP_LETTERS[ops_bytes[i]]))
        i = j
    return "".join(out)


def _text_arg(text):
    """text -> (keep-alive buffer, pointer, length) as the C ABI takes a host text; an empty one is a NULL pointer"""
    text = bytes(text)
    buf = ctypes.create_string_buffer(text, len(text)) if text else None
    return buf, ctypes.cast(buf, ctypes.c_void_p) if text else ctypes.c_void_p(), len(text)


def _tuples(rec, n, dist=True, starts=None, ops=None, stride=0, script=False):
    """the first n records as (pattern, pos[, dist][, start][, ops]): start None where the span record names none, ops one
    op code per byte out of the record's row of `stride` dwords, or (script) ops_to_script's string of them"""
    out = []
    for i in range(n):
        t = (rec[i].pattern, rec[i].pos) + ((rec[i].reserved,) if dist else ())
        if starts is not None:
            t += (None if starts[i].pos == APM_OCC_NO_START else starts[i].pos,)
        if ops is not None:
            row = unpack_ops(ops[i * stride:(i + 1) * stride])
            t += (ops_to_script(row) if script else row,)
        out.append(t)
    return out


class ApmContext:
    """Thin object wrapper over apm_ctx*.  device=None -> apm_create(n_devices)."""

    def __init__(self, n_devices=1, device=None):
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        if device is None:
            rc = self._lib.apm_create(ctypes.byref(self._ctx), n_devices)
        else:
            rc = self._lib.apm_create_on_device(ctypes.byref(self._ctx), device)
        if rc:
            raise ApmError(rc, (self._lib.apm_last_error(None) or b"").decode())
        self.n_patterns = 0

    # -- plumbing --
    def _check(self, rc):
        if rc:
            raise ApmError(rc, (self._lib.apm_last_error(self._ctx) or b"").decode())

    def close(self):
        if self._ctx:
            self._lib.apm_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- ABI mirror --
    def set_patterns(self, patterns, k):
        pats = [bytes(p) for p in patterns]
        n = len(pats)
        arr = (ctypes.c_char_p * max(n, 1))(*pats)
        lens = (ctypes.c_int * max(n, 1))(*[len(p) for p in pats])
        self._check(self._lib.apm_set_patterns(self._ctx, n, arr, lens, k))
        self.n_patterns = n

    def set_kernel(self, kernel):
        if isinstance(kernel, str):
            kernel = KERNEL_IDS[kernel]
        self._check(self._lib.apm_set_kernel(self._ctx, kernel))

    def set_partition(self, partition):
        """"text" (default: owner ranges of the text, counts summed) or "patterns" (slices of the pattern list, every
        device scans the whole text) -- multi-device contexts only"""
        self._check(self._lib.apm_set_partition(self._ctx, {"text": 0, "patterns": 1}.get(partition, partition)))

    def set_text_mode(self, flags):
        """APM_TEXT_FASTA | APM_TEXT_UPPER, or 0 (off): the host-level calls then search the normalised text and report
        source offsets -- single-device contexts only"""
        self._check(self._lib.apm_set_text_mode(self._ctx, flags))

    def normalize_device(self, d_src, src_len, flags, d_dst, dst_capacity):
        """one-to-one mirror: device pointers as integers; returns the kept length"""
        out_len = ctypes.c_uint64()
        self._check(self._lib.apm_normalize_device(self._ctx, ctypes.c_void_p(d_src), src_len, flags, ctypes.c_void_p(d_dst),
                                                   dst_capacity, ctypes.byref(out_len)))
        return out_len.value

    def map_positions_device(self, d_rec, capacity, d_n_rec):
        """one-to-one mirror: pos of the records goes from offsets in the last normalised text to offsets in its source"""
        self._check(self._lib.apm_map_positions_device(self._ctx, ctypes.c_void_p(d_rec), capacity, ctypes.c_void_p(d_n_rec)))

    def index_sequences_device(self, d_table, capacity):
        """one-to-one mirror: the sequence table of the last normalised source into d_table; returns n_seq"""
        n_seq = ctypes.c_uint64()
        self._check(self._lib.apm_index_sequences_device(self._ctx, ctypes.c_void_p(d_table), capacity, ctypes.byref(n_seq)))
        return n_seq.value

    def locate_records_device(self, d_rec, capacity, d_n_rec, d_table, n_seq, d_loc):
        """one-to-one mirror: d_loc[r] = the location of record r (pos a source offset) in the last normalised source"""
        self._check(self._lib.apm_locate_records_device(self._ctx, ctypes.c_void_p(d_rec), capacity, ctypes.c_void_p(d_n_rec),
                                                        ctypes.c_void_p(d_table), n_seq, ctypes.c_void_p(d_loc)))

    def locate(self, records):
        """[(off, seq, flags)] of the records [(pattern, pos, ...)] a find call of this context returned in a text mode"""
        n = len(records)
        rec = (ApmMatch * max(n, 1))()
        for i, r in enumerate(records):
            rec[i].pattern, rec[i].pos = r[0], r[1]
        loc = (ApmLoc * max(n, 1))()
        self._check(self._lib.apm_locate_buffer(self._ctx, rec, n, loc))
        return [(loc[i].off, loc[i].seq, loc[i].flags) for i in range(n)]

    def sequences(self, capacity=None):
        """([(hdr_off, t_begin)] with the sentinel, n_seq): the sequence table of the last host-level call in a text mode;
        capacity None: all of it"""
        n_seq = ctypes.c_uint64()
        if capacity is None:
            self._check(self._lib.apm_get_sequences(self._ctx, None, 0, ctypes.byref(n_seq)))
            capacity = n_seq.value + 1
        out = (ApmSeq * max(capacity, 1))()
        self._check(self._lib.apm_get_sequences(self._ctx, out, capacity, ctypes.byref(n_seq)))
        return [(out[i].hdr_off, out[i].t_begin) for i in range(min(capacity, n_seq.value + 1))], n_seq.value

    def set_stream(self, stream_ptr):
        self._check(self._lib.apm_set_stream(self._ctx, ctypes.c_void_p(stream_ptr)))

    def pattern_kernel(self, i):
        return self._lib.apm_pattern_kernel(self._ctx, i)

    def count_buffer(self, text):
        _keep, ptr, n = _text_arg(text)
        out = (ctypes.c_uint64 * max(self.n_patterns, 1))()
        self._check(self._lib.apm_count_buffer(self._ctx, ptr, n, out))
        return list(out)[: self.n_patterns]

    def find_buffer(self, text, pattern_index, capacity=1 << 16):
        """(positions ascending, total matches) of one pattern of the current set"""
        _keep, ptr, n = _text_arg(text)
        out = (ctypes.c_uint64 * max(capacity, 1))()
        found = ctypes.c_uint64()
        self._check(self._lib.apm_find_buffer(self._ctx, ptr, n, pattern_index, out, capacity,
                                              ctypes.byref(found)))
        return list(out)[: min(found.value, capacity)], found.value

    def find_all_buffer(self, text, capacity=1 << 16):
        """([(pattern, pos)] sorted, total matches) of every pattern of the current set, one pass; capacity 0: total only"""
        _keep, ptr, n = _text_arg(text)
        out = (ApmMatch * capacity)() if capacity else None
        found = ctypes.c_uint64()
        self._check(self._lib.apm_find_all_buffer(self._ctx, ptr, n, out, capacity, ctypes.byref(found)))
        return _tuples(out, min(found.value, capacity), dist=False), found.value

    def find_all_dist_buffer(self, text, capacity=1 << 16):
        """find_all_buffer with every match's edit distance: ([(pattern, pos, dist)] sorted, total matches)"""
        _keep, ptr, n = _text_arg(text)
        out = (ApmMatch * capacity)() if capacity else None
        found = ctypes.c_uint64()
        self._check(self._lib.apm_find_all_dist_buffer(self._ctx, ptr, n, out, capacity, ctypes.byref(found)))
        return _tuples(out, min(found.value, capacity)), found.value

    def align_row_words(self):
        """dwords of one record's row of ops for the current pattern set and k"""
        n = self._lib.apm_align_row_words(self._ctx)
        if n < 0:
            self._check(n)
        return n

    def find_all_align_buffer(self, text, capacity=1 << 16):
        """find_all_dist_buffer with every match's edit script: ([(pattern, pos, dist, ops_bytes)] sorted, total matches),
        ops_bytes one op code per byte (ops_to_script gives the letters)"""
        _keep, ptr, n = _text_arg(text)
        stride = self.align_row_words()
        out = (ApmMatch * capacity)() if capacity else None
        ops = (ctypes.c_uint32 * (capacity * stride))() if capacity else None
        found = ctypes.c_uint64()
        self._check(self._lib.apm_find_all_align_buffer(self._ctx, ptr, n, out, capacity, ctypes.byref(found), ops, stride))
        return _tuples(out, min(found.value, capacity), ops=ops, stride=stride), found.value

    def find_best_buffer(self, text, radius, capacity=1 << 16, align=False):
        """find_all_dist_buffer thinned to its best hits at `radius` (include/apm.h: "best hits"), one more launch on the
        device: ([(pattern, pos, dist)] sorted, n_best, total matches); align=True: [(pattern, pos, dist, ops_bytes)]"""
        _keep, ptr, n = _text_arg(text)
        stride = self.align_row_words() if align else 0
        out = (ApmMatch * capacity)() if capacity else None
        ops = (ctypes.c_uint32 * max(capacity * stride, 1))() if align else None
        n_best, total = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.apm_find_best_buffer(self._ctx, ptr, n, radius, out, capacity, ctypes.byref(n_best),
                                                   ctypes.byref(total), ops, stride))
        return _tuples(out, min(n_best.value, capacity), ops=ops, stride=stride), n_best.value, total.value

    def best_shard_device(self, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, radius, d_out, out_capacity,
                          d_n_out):
        """one-to-one mirror: device pointers as integers, the best hits of the records appended, scored, at *d_n_out"""
        self._check(self._lib.apm_best_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                    ctypes.c_void_p(d_rec), capacity, ctypes.c_void_p(d_n_rec), radius,
                                                    ctypes.c_void_p(d_out), out_capacity, ctypes.c_void_p(d_n_out)))

    def find_occ_buffer(self, text, flags=APM_OCC_LOCAL_MIN, capacity=1 << 16, spans=True):
        """the occurrence search (include/apm.h: "occurrence search"): ([(pattern, end, dist)] sorted, total, counts per
        pattern); spans=True: [(pattern, end, dist, start)], start None where the span pass found no occurrence"""
        _keep, ptr, n = _text_arg(text)
        ends = (ApmMatch * capacity)() if capacity else None
        starts = (ApmMatch * capacity)() if capacity and spans else None
        found = ctypes.c_uint64()
        counts = (ctypes.c_uint64 * max(self.n_patterns, 1))()
        self._check(self._lib.apm_find_occ_buffer(self._ctx, ptr, n, flags, ends, starts, capacity, ctypes.byref(found), counts))
        return _tuples(ends, min(found.value, capacity), starts=starts), found.value, list(counts)[: self.n_patterns]

    def occ_shard_device(self, d_text, text_off, text_len, n_total, own_begin, own_end, flags, d_out, capacity, d_n_found,
                         d_counts=None):
        """one-to-one mirror: device pointers as integers, the ends in [own_begin, own_end) appended at *d_n_found"""
        self._check(self._lib.apm_occ_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total, own_begin,
                                                   own_end, flags, ctypes.c_void_p(d_out), capacity,
                                                   ctypes.c_void_p(d_n_found), ctypes.c_void_p(d_counts)))

    def occ_spans_device(self, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, d_span):
        """one-to-one mirror: device pointers as integers, d_span[r] = the span record of the end d_rec[r]"""
        self._check(self._lib.apm_occ_spans_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                   ctypes.c_void_p(d_rec), capacity, ctypes.c_void_p(d_n_rec),
                                                   ctypes.c_void_p(d_span)))

    def occ_align_row_words(self):
        """dwords of one (end, span) pair's row of ops for the current pattern set and k"""
        n = self._lib.apm_occ_align_row_words(self._ctx)
        if n < 0:
            self._check(n)
        return n

    def occ_align_device(self, d_text, text_off, text_len, n_total, d_end, d_span, capacity, d_n_rec, d_ops, stride_words):
        """one-to-one mirror: device pointers as integers, row r of d_ops (stride_words dwords apart) gets the script of the
        pair (d_end[r], d_span[r])"""
        self._check(self._lib.apm_occ_align_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                   ctypes.c_void_p(d_end), ctypes.c_void_p(d_span), capacity,
                                                   ctypes.c_void_p(d_n_rec), ctypes.c_void_p(d_ops), stride_words))

    def find_occ_align_buffer(self, text, flags=APM_OCC_LOCAL_MIN, capacity=1 << 16):
        """find_occ_buffer with every occurrence's edit script (include/apm.h: "occurrence scripts"):
        ([(pattern, end, dist, start, script)] sorted, total, counts per pattern); script is ops_to_script's run-length
        string of the pattern against text[start : end + 1], "" (and start None) where the span pass found no occurrence"""
        _keep, ptr, n = _text_arg(text)
        stride = self.occ_align_row_words()
        ends = (ApmMatch * capacity)() if capacity else None
        starts = (ApmMatch * capacity)() if capacity else None
        ops = (ctypes.c_uint32 * (capacity * stride))() if capacity else None
        found = ctypes.c_uint64()
        counts = (ctypes.c_uint64 * max(self.n_patterns, 1))()
        self._check(self._lib.apm_find_occ_align_buffer(self._ctx, ptr, n, flags, ends, starts, capacity, ctypes.byref(found),
                                                        counts, ops, stride))
        rec = _tuples(ends, min(found.value, capacity), starts=starts, ops=ops, stride=stride, script=True)
        return rec, found.value, list(counts)[: self.n_patterns]

    def find_occ_seq_buffer(self, text, flags=APM_OCC_LOCAL_MIN, capacity=1 << 16, spans=True, scripts=False):
        """the occurrence search per sequence (include/apm.h: "occurrence search per sequence"; a text mode must be set): no
        occurrence crosses a sequence boundary.  ([(pattern, end, dist)] sorted, total, counts per pattern) -- positions
        are source offsets; spans=True: [(pattern, end, dist, start, seq)]; scripts=True (it implies spans):
        [(pattern, end, dist, start, seq, script)] with ops_to_script's run-length string"""
        _keep, ptr, n = _text_arg(text)
        spans = spans or scripts
        stride = self.occ_align_row_words() if scripts else 0
        ends = (ApmMatch * capacity)() if capacity else None
        starts = (ApmMatch * capacity)() if capacity and spans else None
        seqs = (ctypes.c_uint32 * capacity)() if capacity and spans else None
        ops = (ctypes.c_uint32 * (capacity * stride))() if capacity and scripts else None
        found = ctypes.c_uint64()
        counts = (ctypes.c_uint64 * max(self.n_patterns, 1))()
        self._check(self._lib.apm_find_occ_seq_buffer(self._ctx, ptr, n, flags, ends, starts, seqs, capacity, ctypes.byref(found),
                                                      counts, ops, stride))
        take = min(found.value, capacity)
        rec = _tuples(ends, take, starts=starts)
        if seqs is not None:
            rec = [t + (seqs[i],) for i, t in enumerate(rec)]
        if ops is not None:
            rec = [t + (ops_to_script(unpack_ops(ops[i * stride:(i + 1) * stride])),) for i, t in enumerate(rec)]
        return rec, found.value, list(counts)[: self.n_patterns]

    def occ_seq_shard_device(self, d_text, text_off, text_len, n_total, own_begin, own_end, d_table, n_seq, flags, d_out, capacity,
                             d_n_found, d_counts=None):
        """one-to-one mirror: device pointers as integers, the ends in [own_begin, own_end) under the sequence table d_table
        appended at *d_n_found"""
        self._check(self._lib.apm_occ_seq_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total, own_begin,
                                                       own_end, ctypes.c_void_p(d_table), n_seq, flags, ctypes.c_void_p(d_out),
                                                       capacity, ctypes.c_void_p(d_n_found), ctypes.c_void_p(d_counts)))

    def occ_seq_spans_device(self, d_text, text_off, text_len, n_total, d_table, n_seq, d_rec, capacity, d_n_rec, d_span, d_seq=None):
        """one-to-one mirror: device pointers as integers, d_span[r] = the span record of the end d_rec[r] clamped to its
        sequence and (d_seq given) d_seq[r] = that sequence"""
        self._check(self._lib.apm_occ_seq_spans_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                       ctypes.c_void_p(d_table), n_seq, ctypes.c_void_p(d_rec), capacity,
                                                       ctypes.c_void_p(d_n_rec), ctypes.c_void_p(d_span), ctypes.c_void_p(d_seq)))

    def find_nearest_buffer(self, text, spans=True):
        """every pattern's nearest occurrence (include/apm.h: "nearest occurrences"), whatever k is: one
        (pattern, end, dist) per pattern in pattern order, end None and dist m where there is none; spans=True:
        (pattern, end, dist, start)"""
        _keep, ptr, n = _text_arg(text)
        P = max(self.n_patterns, 1)
        ends = (ApmMatch * P)()
        starts = (ApmMatch * P)() if spans else None
        self._check(self._lib.apm_find_nearest_buffer(self._ctx, ptr, n, ends, starts))
        return [(t[0], None if t[1] == APM_OCC_NO_START else t[1]) + t[2:] for t in _tuples(ends, self.n_patterns, starts=starts)]

    def nearest_shard_device(self, d_text, text_off, text_len, n_total, own_begin, own_end, d_keys):
        """one-to-one mirror: device pointers as integers, the best key of the ends in [own_begin, own_end) merged into
        d_keys[pattern] (preset to APM_NEAREST_NONE)"""
        self._check(self._lib.apm_nearest_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                       own_begin, own_end, ctypes.c_void_p(d_keys)))

    def nearest_records_device(self, d_text, text_off, text_len, n_total, d_keys, d_end, d_start=None):
        """one-to-one mirror: device pointers as integers, d_end[i] and (d_start given) d_start[i] from d_keys[i]"""
        self._check(self._lib.apm_nearest_records_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                         ctypes.c_void_p(d_keys), ctypes.c_void_p(d_end),
                                                         ctypes.c_void_p(d_start)))

    def find_nearest_seq_buffer(self, text, spans=True):
        """every pattern's nearest occurrence in EVERY sequence of the text (include/apm.h: "nearest occurrences per
        sequence"; a text mode must be set), whatever k is: (n_seq, rows), row s * n_patterns + i the pair (sequence s,
        pattern i) as (pattern, end, dist) -- end a source offset, None and dist m where there is none; spans=True:
        (pattern, end, dist, start).  Sizes itself: the sequences of a first guess, one retry from the count the call left"""
        _keep, ptr, n = _text_arg(text)
        P = max(self.n_patterns, 1)
        n_seq = ctypes.c_uint64()
        cap = 64
        for attempt in (0, 1):
            ends = (ApmMatch * (cap * P))()
            starts = (ApmMatch * (cap * P))() if spans else None
            rc = self._lib.apm_find_nearest_seq_buffer(self._ctx, ptr, n, ends, starts, cap, ctypes.byref(n_seq))
            if rc == -1 and n_seq.value > cap and attempt == 0:  # APM_ERR_INVALID with the count set: too many sequences
                cap = n_seq.value
                continue
            self._check(rc)
            break
        rows = _tuples(ends, n_seq.value * self.n_patterns, starts=starts)
        return n_seq.value, [(t[0], None if t[1] == APM_OCC_NO_START else t[1]) + t[2:] for t in rows]

    def nearest_seq_shard_device(self, d_text, text_off, text_len, n_total, own_begin, own_end, d_table, n_seq, d_keys):
        """one-to-one mirror: device pointers as integers, the best key of the ends in [own_begin, own_end) of every
        (sequence, pattern) pair merged into d_keys[s * n_patterns + pattern] (preset to APM_NEAREST_NONE)"""
        self._check(self._lib.apm_nearest_seq_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                           own_begin, own_end, ctypes.c_void_p(d_table), n_seq, ctypes.c_void_p(d_keys)))

    def nearest_seq_records_device(self, d_text, text_off, text_len, n_total, d_table, n_seq, d_keys, d_end, d_start=None):
        """one-to-one mirror: device pointers as integers, d_end[r] and (d_start given) d_start[r] from d_keys[r]"""
        self._check(self._lib.apm_nearest_seq_records_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                             ctypes.c_void_p(d_table), n_seq, ctypes.c_void_p(d_keys),
                                                             ctypes.c_void_p(d_end), ctypes.c_void_p(d_start)))

    def align_shard_device(self, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec, d_ops, stride_words):
        """one-to-one mirror: device pointers as integers, row r of d_ops (stride_words dwords apart) gets record r's script"""
        self._check(self._lib.apm_align_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                     ctypes.c_void_p(d_rec), capacity, ctypes.c_void_p(d_n_rec),
                                                     ctypes.c_void_p(d_ops), stride_words))

    def score_shard_device(self, d_text, text_off, text_len, n_total, d_rec, capacity, d_n_rec):
        """one-to-one mirror: device pointers as integers, the fourth dword of the records becomes their capped distance"""
        self._check(self._lib.apm_score_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                     ctypes.c_void_p(d_rec), capacity, ctypes.c_void_p(d_n_rec)))

    def find_shard_device(self, d_text, text_off, text_len, n_total, own_begin, own_end, d_out, capacity, d_n_found,
                          d_counts=None):
        """one-to-one mirror: device pointers as integers, records appended at *d_n_found"""
        self._check(self._lib.apm_find_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len, n_total,
                                                    own_begin, own_end, ctypes.c_void_p(d_out), capacity,
                                                    ctypes.c_void_p(d_n_found), ctypes.c_void_p(d_counts)))

    def count_file(self, path):
        out = (ctypes.c_uint64 * max(self.n_patterns, 1))()
        self._check(self._lib.apm_count_file(self._ctx, os.fsencode(path), out))
        return list(out)[: self.n_patterns]

    def count_synthetic(self, n, seed):
        out = (ctypes.c_uint64 * max(self.n_patterns, 1))()
        self._check(self._lib.apm_count_synthetic(self._ctx, n, seed, out))
        return list(out)[: self.n_patterns]

    def count_shard_device(self, d_text, text_off, text_len, n_total, own_begin, own_end, d_counts):
        self._check(self._lib.apm_count_shard_device(self._ctx, ctypes.c_void_p(d_text), text_off, text_len,
                                                     n_total, own_begin, own_end, ctypes.c_void_p(d_counts)))

    def synth_fill_device(self, d_dst, global_off, length, seed):
        self._check(self._lib.apm_synth_fill_device(self._ctx, ctypes.c_void_p(d_dst), global_off, length, seed))

    def set_timing(self, enabled):
        self._check(self._lib.apm_set_timing(self._ctx, 1 if enabled else 0))

    def timing(self):
        t = ApmTiming()
        self._check(self._lib.apm_get_timing(self._ctx, ctypes.byref(t)))
        return t.as_dict()

    def launch_times(self, max_launches=32):
        """[(label, ms)] of the scan-kernel launches of the last counting call (HIP events on the launch stream)"""
        ms = (ctypes.c_double * max_launches)()
        labels = (ctypes.c_char_p * max_launches)()
        n = self._lib.apm_get_launch_times(self._ctx, max_launches, ms, labels)
        if n < 0:
            self._check(n)
        return [((labels[i] or b"?").decode(), ms[i]) for i in range(n)]

    def stat(self, name):
        v = ctypes.c_double()
        self._check(self._lib.apm_get_stat(self._ctx, name.encode(), ctypes.byref(v)))
        return v.value

    def synchronize(self):
        self._check(self._lib.apm_synchronize(self._ctx))

    def device_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self._lib.apm_device_alloc(self._ctx, ctypes.byref(p), nbytes))
        return p.value

    def device_free(self, ptr):
        self._check(self._lib.apm_device_free(self._ctx, ctypes.c_void_p(ptr)))

    def device_upload(self, d_dst, data):
        data = bytes(data)
        self._check(self._lib.apm_device_upload(self._ctx, ctypes.c_void_p(d_dst), data, len(data)))

    def device_download(self, d_src, nbytes):
        buf = ctypes.create_string_buffer(nbytes)
        self._check(self._lib.apm_device_download(self._ctx, ctypes.cast(buf, ctypes.c_void_p),
                                                  ctypes.c_void_p(d_src), nbytes))
        return buf.raw

    def device_memset(self, d_dst, value, nbytes):
        self._check(self._lib.apm_device_memset(self._ctx, ctypes.c_void_p(d_dst), value, nbytes))
