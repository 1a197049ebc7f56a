"""ctypes binding of include/pm_gpu.h and a PatternMatch-shaped host class."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_LIB = None

HIT_DTYPE = np.dtype([("end", "<i8"), ("pid", "<u4"), ("k", "u1"), ("aux", "u1", (3,))])
ALIGNMENT_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("editdist", "<i4"), ("value", "<i4")])
# pm_pcr_amplicon: the processed hit and its partner, their re-alignments, the amplicon length, pind and the N count
PCR_AMPLICON_DTYPE = np.dtype([("hit", HIT_DTYPE, (2,)), ("al", ALIGNMENT_DTYPE, (2,)), ("amplicon_len", "<i8"), ("pair", "<u4"), ("ncount", "<u4")])

SEM_AUTO, SEM_KEYWORD_TREE, SEM_SHIFT_AND, SEM_FILTER_BITVEC = 0, 2, 4, 5
SEM_EXACT_BASES, SEM_EXACT_HALVES, SEM_SHIFT_AND_INEXACT = 8, 12, 100
KERNEL_AUTO, KERNEL_BITPAR, KERNEL_SEED = 0, 16, 17
PM_E_OVERFLOW = -5

# every entry point include/pm_gpu.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "pm_create", "pm_add_pattern", "pm_init", "pm_init_device", "pm_scan", "pm_scan_view", "pm_scan_candidates",
    "pm_scan_candidates_async", "pm_scan_wait", "pm_candidates_device", "pm_set_capacity", "pm_finalize",
    "pm_finalize_device", "pm_finalize_device_owned", "pm_align_hits", "pm_align_hits_text",
    "pm_reset", "pm_destroy", "pm_last_error", "pm_selected_semantics", "pm_selected_kernel", "pm_describe",
    "pm_last_kernel_time", "pm_pick_semantics", "pm_measure_stream_read",
    "pm_final_hits_device", "pm_copy_records", "pm_pack_time", "pm_init_host", "pm_scan_stats", "pm_measure_pair_edit_floor", "pm_prepare_device",
    "pm_init_windowed", "pm_stream_residency", "pm_device_memory",
    "pm_init_packed", "pm_unpack_device", "pm_unpack_codes", "pm_pack_codes",
    "pm_align_hits_device", "pm_count_scan", "pm_counts",
    "pm_pcr_setup", "pm_pcr_feed", "pm_pcr_scan", "pm_pcr_pair", "pm_pcr_stats",
    "pm_comm_unique_id", "pm_comm_create", "pm_comm_gather", "pm_comm_destroy", "pm_comm_last_error",
]


class PmError(RuntimeError):
    def __init__(self, code, msg, required=0):
        super().__init__("pm_gpu error %d: %s" % (code, msg))
        self.code = code
        self.required = required          # PM_E_OVERFLOW: the record count the buffer must hold


class _Hit(C.Structure):
    _fields_ = [("end", C.c_int64), ("pid", C.c_uint32), ("k", C.c_uint8), ("aux", C.c_uint8 * 3)]


class _CountInfo(C.Structure):
    """pm_count_info"""
    _fields_ = [("tallied", C.c_uint64), ("skipped", C.c_uint64), ("aligned_device", C.c_uint64), ("aligned_host", C.c_uint64),
                ("bogus", C.c_uint64), ("record_bytes_to_host", C.c_uint64), ("first_bogus", _Hit)]


class _PcrParams(C.Structure):
    """pm_pcr_params"""
    _fields_ = [("any_orientation", C.c_int32), ("length_between", C.c_int32), ("amplicon_min", C.c_int64), ("amplicon_max", C.c_int64),
                ("size_slack", C.c_int32), ("reserved", C.c_int32), ("size_lb", C.c_void_p), ("size_ub", C.c_void_p),
                ("entry_starts", C.c_void_p), ("n_entries", C.c_int64)]


class _Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("semantics", C.c_int32), ("kernel", C.c_int32), ("k", C.c_int32),
                ("indels", C.c_int32), ("wildcards", C.c_int32), ("text_n", C.c_int32), ("eos", C.c_int32),
                ("device", C.c_int32), ("long_patterns", C.c_int32), ("reserved", C.c_int32 * 6)]


def library_path():
    """csrc/libpm_gpu.so.  A/B measurement builds of the same sources (csrc/Makefile VARIANT=...) are loaded only when the
    caller says so twice: PM_GPU_LIB names a libpm_gpu*.so inside csrc/ AND PM_GPU_LIB_AB=1 is set (scripts/sweep_pair2.sh);
    a stray environment variable cannot point the product at another file."""
    alt = os.environ.get("PM_GPU_LIB")
    if alt and os.environ.get("PM_GPU_LIB_AB") == "1":
        alt = os.path.abspath(alt)
        if os.path.dirname(alt) == _CSRC and os.path.basename(alt).startswith("libpm_gpu") and alt.endswith(".so"):
            return alt
        raise PmError(-1, "PM_GPU_LIB must name a libpm_gpu*.so inside %s" % _CSRC)
    return os.path.join(_CSRC, "libpm_gpu.so")


def build_library(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", _CSRC])
    return library_path()


def load_library():
    """Load csrc/libpm_gpu.so.  No fallback: a missing library is an error.

    Processes that also use PyTorch on the GPU should import torch first: torch ships its own HIP
    runtime, and whichever runtime is loaded first serves the process."""
    global _LIB
    if _LIB is None:
        path = library_path()
        if not os.path.exists(path):
            raise PmError(-4, "HIP extension %s is not built (run __graft_entry__.build())" % path)
        L = C.CDLL(path)
        L.pm_last_error.restype = C.c_char_p
        L.pm_last_error.argtypes = [C.c_void_p]
        L.pm_destroy.restype = None
        L.pm_destroy.argtypes = [C.c_void_p]
        for name in ABI_SYMBOLS:
            f = getattr(L, name)
            if name not in ("pm_last_error", "pm_destroy", "pm_comm_destroy", "pm_comm_last_error"):
                f.restype = C.c_int
        L.pm_create.argtypes = [C.POINTER(_Config), C.POINTER(C.c_void_p)]
        L.pm_add_pattern.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, C.c_int32, C.c_int32]
        L.pm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
        L.pm_init_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
        L.pm_init_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
        L.pm_init_windowed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64]
        L.pm_init_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64]
        L.pm_unpack_device.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pm_unpack_codes.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
        L.pm_pack_codes.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64]
        L.pm_stream_residency.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int]
        L.pm_device_memory.argtypes = [C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.pm_scan.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.pm_scan_view.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.pm_scan_candidates.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pm_scan_candidates_async.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        L.pm_scan_wait.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        L.pm_candidates_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.pm_set_capacity.argtypes = [C.c_void_p, C.c_size_t]
        L.pm_finalize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pm_finalize_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pm_finalize_device_owned.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                               C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.pm_align_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.pm_align_hits_text.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
        L.pm_reset.argtypes = [C.c_void_p]
        L.pm_selected_semantics.argtypes = [C.c_void_p]
        L.pm_selected_kernel.argtypes = [C.c_void_p]
        L.pm_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        L.pm_last_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.pm_pick_semantics.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.pm_measure_stream_read.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_float)]
        L.pm_final_hits_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.pm_copy_records.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.pm_scan_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pm_measure_pair_edit_floor.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        L.pm_pack_time.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.pm_align_hits_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.pm_count_scan.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_uint64]
        L.pm_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(_CountInfo)]
        L.pm_pcr_setup.argtypes = [C.c_void_p, C.POINTER(_PcrParams)]
        L.pm_pcr_feed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.pm_pcr_scan.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_size_t)]
        L.pm_pcr_pair.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                  C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.pm_pcr_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _LIB = L
    return _LIB


def pick_semantics(alphabet_size, acgt_normalized, k, patterns, esb=None, eeb=None, wildcards=False):
    """pick_pattern_index's automatic engine choice (reference select.cc:101-141)."""
    L = load_library()
    pl = np.array([len(p) for p in patterns], dtype=np.int32)
    a = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.int32).ctypes.data_as(C.c_void_p)
    return L.pm_pick_semantics(alphabet_size, int(acgt_normalized), k, int(wildcards), len(patterns),
                               pl.ctypes.data_as(C.c_void_p), a(esb), a(eeb))


def measure_stream_read(d_ptr, nbytes, reps=5, stream=0):
    """Streaming-read rate (GB/s) of this box over an HBM buffer (pm_measure_stream_read)."""
    g = C.c_float()
    rc = load_library().pm_measure_stream_read(C.c_void_p(d_ptr), C.c_size_t(nbytes), int(reps), C.c_void_p(stream), C.byref(g))
    if rc:
        raise PmError(rc, "pm_measure_stream_read failed")
    return g.value


def pack_codes(codes, bits):
    """pm_pack_codes: uint8 codes (< 2**bits) -> the bit-packed bytes of a <db>.sqz, MSB first, zero fill bits at the end."""
    arr = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros(max(0, (arr.size * int(bits) + 7) // 8), dtype=np.uint8)
    rc = load_library().pm_pack_codes(arr.ctypes.data_as(C.c_void_p), arr.size, int(bits), out.ctypes.data_as(C.c_void_p), out.size)
    if rc:
        raise PmError(rc, "pm_pack_codes: bits outside 1..8 or a code that does not fit %d bits" % bits)
    return out


def unpack_codes(packed, bits, first, n):
    """pm_unpack_codes: codes first .. first+n-1 of a bit-packed stream as a uint8 array."""
    arr = np.ascontiguousarray(packed, dtype=np.uint8)
    out = np.zeros(max(int(n), 0), dtype=np.uint8)
    rc = load_library().pm_unpack_codes(arr.ctypes.data_as(C.c_void_p), arr.size, int(bits), int(first), int(n), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise PmError(rc, "pm_unpack_codes: bits outside 1..8 or codes outside the packed bytes")
    return out


def unpack_device(d_packed, packed_bytes, bits, n, d_text, d_words=0, stream=0):
    """pm_unpack_device over raw device pointers (torch tensors' data_ptr()): n codes from bit 0 of d_packed into the bytes
    at d_text (room for n rounded up to 16) and, when d_words is given, the 2-bit words of the seed family."""
    rc = load_library().pm_unpack_device(C.c_void_p(d_packed), int(packed_bytes), int(bits), int(n), C.c_void_p(d_text),
                                         C.c_void_p(d_words or 0), C.c_void_p(stream or 0))
    if rc:
        raise PmError(rc, "pm_unpack_device failed (arguments, alignment or launch)")


def reverse_comp(p):
    comp = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N", "a": "t", "c": "g", "g": "c", "t": "a", "n": "n"}
    return "".join(comp.get(c, c) for c in reversed(p))


def sorted_tuples(hits):
    return sorted(zip(hits["end"].tolist(), hits["pid"].tolist(), hits["k"].tolist()))


class PatternMatch:
    """Host-side mirror of the reference's PatternMatch (pattern_match.h:84-156) over the GPU engine.

    k / indels / eos follow pick_pattern_index's arguments (select.cc:19-30): indels=True is the
    CLI's -k (edits), False is -K (substitutions only).  `semantics` forces a reference engine
    (-N), SEM_AUTO reproduces the automatic choice; `kernel` picks the GPU kernel family.
    long_patterns=True lets -K 1 / -K 2 patterns of 33..64 characters run on the pair plan (bit 0 of pm_config.long_patterns),
    long_exact=True lets k = 0 patterns of 33..64 characters run on the seed plan (bit 1), long_edits=True lets -k 1 / -k 2
    patterns of 33..64 characters run on the edit plan (bit 2), long_halves=True lets exact_halves -k 1 / -k 2 lists with
    patterns of 33..64 characters stay on the halves plan (bit 3); each acts on its own option sets.
    long_align=True (bit 4) changes no scan: with indels and k = 1 .. 3 the hits of patterns of 33..64 characters are re-aligned on
    the device by align_hits_device, count_scan and pcr_pair, not by host threads.
    wildcard primers: wild_class=True (bit 5) lets -w primers of 16..32 characters with more than 16 concrete variants run on
    pm_wild_sub_scan (k = 0 on keyword_tree / shift_and, -K 1 / -K 2 on filter_bitvec) and not on the bit-parallel residue.
    edit_pair=True (bit 6) lets the edit plan's first stage run on the pair geometry (pm_pair_edit_scan + pm_pair_edit_resolve)
    wherever its tables can be built, not only at -k 2 on one pattern tile: every tile of a larger list at -k 2, -k 1 under
    filter_bitvec / bare shift_and_inexact (two tests per window) and exact_bases -k 1 / -k 2.  The hits do not change.
    wild_long=True (bit 7) acts only together with wild_class: -w primers of 33..64 characters with more than 16 concrete
    variants join that class under the same rules (their keys are their last 16 characters'); a class that holds one is
    verified by pm_wild_sub_verify_wide on rows of 64 characters.  Alone it changes nothing.
    """

    def __init__(self, k=0, indels=True, eos="\n", semantics=SEM_AUTO, kernel=KERNEL_AUTO, device=0,
                 wildcards=False, text_n=False, long_patterns=False, long_exact=False, long_edits=False,
                 long_halves=False, long_align=False, wild_class=False, edit_pair=False, wild_long=False):
        self._L = load_library()
        cfg = _Config()
        cfg.abi_version, cfg.semantics, cfg.kernel, cfg.k = 1, semantics, kernel, k
        cfg.indels, cfg.wildcards, cfg.text_n = int(bool(indels)), int(bool(wildcards)), int(bool(text_n))
        cfg.eos = ord(eos) if isinstance(eos, str) else int(eos)
        cfg.device = device
        cfg.long_patterns = int(bool(long_patterns)) | (2 if long_exact else 0) | (4 if long_edits else 0) | (8 if long_halves else 0) | (16 if long_align else 0) | (32 if wild_class else 0) | (64 if edit_pair else 0) | (128 if wild_long else 0)
        self.long_patterns_bits = int(cfg.long_patterns)           # pm_config.long_patterns as handed to pm_create
        self._h = C.c_void_p()
        rc = self._L.pm_create(C.byref(cfg), C.byref(self._h))
        if rc:
            raise PmError(rc, (self._L.pm_last_error(None) or b"").decode())
        self._n = 0
        self._pos = 0
        self._keep = None
        self._k = k
        self._npat = 0
        self._maxlen = 0

    def _check(self, rc):
        if rc:
            raise PmError(rc, (self._L.pm_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._L.pm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- PatternMatch::add_pattern (pattern_match.h:116) --------------------------------------
    def add_pattern(self, pat, id=0, exact_start_bases=0, exact_end_bases=0):
        b = pat.encode() if isinstance(pat, str) else bytes(pat)
        self._check(self._L.pm_add_pattern(self._h, b, len(b), id, exact_start_bases, exact_end_bases))
        self._npat += 1
        self._maxlen = max(self._maxlen, len(b))
        return id

    # -- PatternMatch::init (pattern_match.h:130) -----------------------------------------------
    def init(self, text, table=None, window=None):
        """`text`: uint8 numpy array (host stream bytes as getnch() returns them).
        `table`: cp.ch(0..size-1) for a normalized stream, None for a raw one.
        `window`: bytes per window of pm_init_windowed -- the stream stays in host memory and the GPU holds a ring of
        windows of it; None uploads the whole stream (pm_init)."""
        arr = np.ascontiguousarray(text, dtype=np.uint8)
        self._keep = arr                      # pm_init borrows the host pointer
        tb = None if table is None else (C.c_uint8 * len(table)).from_buffer_copy(bytes(table))
        tl = 0 if table is None else len(table)
        if window is None:
            self._check(self._L.pm_init(self._h, arr.ctypes.data_as(C.c_void_p), arr.size, tb, tl))
        else:
            self._check(self._L.pm_init_windowed(self._h, arr.ctypes.data_as(C.c_void_p), arr.size, tb, tl, int(window)))
        self._n, self._pos = arr.size, 0

    def init_packed(self, packed, bits, n, table, window=None):
        """pm_init_packed: `packed` holds n codes of `bits` bits, MSB first (a <db>.sqz); it crosses PCIe packed and is
        unpacked on the GPU.  `window` as for init(): None keeps the whole stream resident."""
        arr = np.ascontiguousarray(packed, dtype=np.uint8)
        self._keep = arr                      # borrowed until close()
        tb = None if table is None else (C.c_uint8 * len(table)).from_buffer_copy(bytes(table))
        self._check(self._L.pm_init_packed(self._h, arr.ctypes.data_as(C.c_void_p), arr.size, int(bits), int(n), tb,
                                           0 if table is None else len(table), 0 if window is None else int(window)))
        self._n, self._pos = int(n), 0

    def init_host(self, text, table=None):
        """pm_init_host: a handle that runs the HOST stage only (finalize, align_hits) over the whole stream -- the merge
        rank of a position-sharded scan."""
        arr = np.ascontiguousarray(text, dtype=np.uint8)
        self._keep = arr
        tb = None if table is None else (C.c_uint8 * len(table)).from_buffer_copy(bytes(table))
        self._check(self._L.pm_init_host(self._h, arr.ctypes.data_as(C.c_void_p), arr.size, tb, 0 if table is None else len(table)))
        self._n, self._pos = arr.size, 0

    def init_device(self, data_ptr, n, table=None, stream=None, keepalive=None):
        """Stream already resident in HBM (e.g. a torch uint8 tensor's data_ptr())."""
        self._keep = keepalive
        tb = None if table is None else (C.c_uint8 * len(table)).from_buffer_copy(bytes(table))
        self._check(self._L.pm_init_device(self._h, C.c_void_p(data_ptr), n, tb, 0 if table is None else len(table),
                                           C.c_void_p(stream or 0)))
        self._n, self._pos = n, 0

    # -- PatternMatch::find_patterns (pattern_match.h:131) -------------------------------------
    def find_patterns(self, hits, minka=1, chunk=1 << 26):
        """Scan on from the current stream position until >= minka hits were produced or the end
        of the stream; appends (end, pid, k) tuples to `hits`; returns True if any were appended
        (the reference's `more`).  pos() afterwards is the scanned-to position."""
        got = 0
        buf = np.zeros(1 << 16, dtype=HIT_DTYPE)
        n_out, more = C.c_size_t(), C.c_int()
        while True:
            begin = self._pos
            end = min(self._n, begin + chunk)
            self._check(self._L.pm_scan(self._h, begin, end, buf.ctypes.data_as(C.c_void_p), buf.size,
                                        C.byref(n_out), C.byref(more)))
            self._pos = end
            while True:
                for i in range(n_out.value):
                    hits.append((int(buf["end"][i]), int(buf["pid"][i]), int(buf["k"][i])))
                got += n_out.value
                if not more.value:
                    break
                self._check(self._L.pm_scan(self._h, end, end, buf.ctypes.data_as(C.c_void_p), buf.size,
                                            C.byref(n_out), C.byref(more)))
            if got >= minka or self._pos >= self._n:
                return got > 0

    def find_all(self, chunk=1 << 26):
        """All hits over the whole stream as a structured array sorted by (end, pid)."""
        self.reset()
        hits = []
        while self.find_patterns(hits, minka=1 << 62, chunk=chunk):
            if self._pos >= self._n:
                break
        out = np.zeros(len(hits), dtype=HIT_DTYPE)
        if hits:
            a = np.array(hits, dtype=np.int64)
            out["end"], out["pid"], out["k"] = a[:, 0], a[:, 1], a[:, 2]
        return out

    def scan(self, begin, end, out):
        """pm_scan itself (PatternMatch::find_patterns over [begin,end), pattern_match.h:131): final hits, sorted by
        (end, pid), into the caller's array `out`; returns (count, more).  more: call again with begin == end."""
        n_out, more = C.c_size_t(), C.c_int()
        self._check(self._L.pm_scan(self._h, begin, end, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n_out), C.byref(more)))
        return n_out.value, more.value

    def scan_view(self, begin, end):
        """pm_scan_view: the range's final hits as a numpy view of the handle's own buffer (valid until the next call)."""
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pm_scan_view(self._h, begin, end, C.byref(p), C.byref(n)))
        if not n.value:
            return np.zeros(0, dtype=HIT_DTYPE)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value * 16,)).view(HIT_DTYPE)

    def pos(self):
        return self._pos

    # -- PatternMatch::reset (pattern_match.h:134) ----------------------------------------------
    def reset(self):
        self._check(self._L.pm_reset(self._h))
        self._pos = 0

    # -- device / host stages separately (multi-GPU path, bench) -------------------------------
    def set_capacity(self, n):
        self._check(self._L.pm_set_capacity(self._h, n))

    def scan_candidates(self, begin, end, to_host=True):
        """Device stage over (begin, end]; the record buffer grows (and the range is scanned again)
        when it was too small.  Returns the records (host array) or, with to_host=False, their count."""
        n_out = C.c_size_t()
        rc = self._L.pm_scan_candidates(self._h, begin, end, None, 0, C.byref(n_out))
        while rc == PM_E_OVERFLOW:
            self.set_capacity(int(n_out.value * 1.25) + 1024)
            rc = self._L.pm_scan_candidates(self._h, begin, end, None, 0, C.byref(n_out))
        self._check(rc)
        if not to_host:
            return n_out.value
        ptr, n = self.candidates_device()
        return self.copy_records(ptr, n)

    def copy_records(self, d_ptr, n):
        """n 16-byte records from HBM (pm_copy_records)."""
        out = np.zeros(n, dtype=HIT_DTYPE)
        if n:
            self._check(self._L.pm_copy_records(self._h, C.c_void_p(d_ptr), n, out.ctypes.data_as(C.c_void_p)))
        return out

    def scan_async(self, begin, end):
        self._check(self._L.pm_scan_candidates_async(self._h, begin, end))

    def scan_wait(self):
        """Raises PmError(PM_E_OVERFLOW) with .required set when the record buffer was too small:
        set_capacity(required * 1.25) and scan the range again."""
        n_out = C.c_size_t()
        rc = self._L.pm_scan_wait(self._h, C.byref(n_out))
        if rc == PM_E_OVERFLOW:
            raise PmError(rc, (self._L.pm_last_error(self._h) or b"").decode(), required=n_out.value)
        self._check(rc)
        return n_out.value

    def candidates_device(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pm_candidates_device(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def finalize(self, cands, scanned_to, last=True, sort=True):
        cands = np.ascontiguousarray(cands, dtype=HIT_DTYPE)
        out = np.empty(max(cands.size, 1), dtype=HIT_DTYPE)
        n_out = C.c_size_t()
        self._check(self._L.pm_finalize(self._h, cands.ctypes.data_as(C.c_void_p), cands.size, scanned_to,
                                        (1 if last else 0) | (2 if sort else 0),
                                        out.ctypes.data_as(C.c_void_p), out.size, C.byref(n_out)))
        return out[:n_out.value]

    def finalize_device(self, scanned_to, last=True, sort=True, d_cands=None, n=0, out=None, owned=None, keep=False):
        """GPU clustering of the records of the last scan (or of `d_cands`, a device pointer);
        returns the final hits (host array).  Raises PmError(-2) where only the host stage applies.
        owned=(own_lo, own_hi, guard_lo, guard_hi): this call is one shard of a position-sharded
        scan (pm_finalize_device_owned); guard_hi=None declares the true end of the stream.
        keep=True: the hits stay in HBM; returns (device pointer, count) (pm_final_hits_device)."""
        if keep:
            optr, ocap, sort = C.c_void_p(0), 0, False
        else:
            if out is None:
                cap = max(n if d_cands else self.candidates_device()[1], 1) + 1024
                out = np.empty(cap, dtype=HIT_DTYPE)
            optr, ocap = out.ctypes.data_as(C.c_void_p), out.size
        n_out = C.c_size_t()
        if owned is not None:
            own_lo, own_hi, guard_lo, guard_hi = owned
            self._check(self._L.pm_finalize_device_owned(self._h, C.c_void_p(d_cands or 0), n, own_lo, own_hi, guard_lo,
                                                         (1 << 63) - 1 if guard_hi is None else guard_hi, 2 if sort else 0,
                                                         optr, ocap, C.byref(n_out)))
        else:
            self._check(self._L.pm_finalize_device(self._h, C.c_void_p(d_cands or 0), n, scanned_to,
                                                   (1 if last else 0) | (2 if sort else 0), optr, ocap, C.byref(n_out)))
        if keep:
            p, cnt = C.c_void_p(), C.c_size_t()
            self._check(self._L.pm_final_hits_device(self._h, C.byref(p), C.byref(cnt)))
            return p.value or 0, cnt.value
        return out[:n_out.value]

    def align_hits(self, hits):
        """primer_match's per-hit re-alignment; returns a structured array (start, end, editdist, value)."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        out = np.zeros(hits.size, dtype=np.dtype([("start", "<i8"), ("end", "<i8"), ("editdist", "<i4"), ("value", "<i4")]))
        if hits.size:
            self._check(self._L.pm_align_hits(self._h, hits.ctypes.data_as(C.c_void_p), hits.size, out.ctypes.data_as(C.c_void_p)))
        return out

    def align_hits_device(self, d_hits, n, text=False, d_out=None, d_ops=None, d_text=None, stride=0):
        """pm_align_hits_device: re-align n 16-byte records that lie in HBM at `d_hits` (a device pointer); the results
        stay in HBM.  With the output pointers given they are used; otherwise torch tensors are allocated.  Returns
        (d_out, d_ops, d_text, stride, keepalive) -- device pointers (d_ops / d_text 0 without text=True) and the
        tensors that own them."""
        keep = []
        if d_out is None:
            import torch
            stride = max(int(stride), self._maxlen + self._k + 2) if text else 0
            out_t = torch.zeros(max(n, 1) * ALIGNMENT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            keep.append(out_t)
            d_out = out_t.data_ptr()
            if text:
                ops_t = torch.zeros(max(n, 1) * stride, dtype=torch.uint8, device="cuda")
                txt_t = torch.zeros(max(n, 1) * stride, dtype=torch.uint8, device="cuda")
                keep += [ops_t, txt_t]
                d_ops, d_text = ops_t.data_ptr(), txt_t.data_ptr()
        self._check(self._L.pm_align_hits_device(self._h, C.c_void_p(d_hits), n, C.c_void_p(d_out), C.c_void_p(d_ops or 0),
                                                 C.c_void_p(d_text or 0), stride))
        return d_out, d_ops or 0, d_text or 0, stride, keep

    def align_hits_device_numpy(self, hits, text=False):
        """Convenience for tests: upload `hits`, pm_align_hits_device, copy the results back.  Returns the alignment
        array, or (alignments, alignment strings, matching texts) with text=True."""
        import torch
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        n = hits.size
        if n == 0:
            empty = np.zeros(0, dtype=ALIGNMENT_DTYPE)
            return (empty, [], []) if text else empty
        d_hits = torch.from_numpy(hits.view(np.uint8).copy()).cuda()
        _, _, _, stride, keep = self.align_hits_device(d_hits.data_ptr(), n, text=text)
        al = keep[0].cpu().numpy().view(ALIGNMENT_DTYPE)[:n].copy()
        if not text:
            return al
        cut = lambda t: [bytes(row).split(b"\0", 1)[0].decode("latin-1") for row in t.cpu().numpy().reshape(n, stride)]
        return al, cut(keep[1]), cut(keep[2])

    def align_hits_text(self, hits, stride=0):
        """pm_align_hits_text: (alignments, alignment strings, matching texts) of host records."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        n = hits.size
        stride = max(int(stride), self._maxlen + self._k + 2)
        out = np.zeros(n, dtype=ALIGNMENT_DTYPE)
        ops, txt = C.create_string_buffer(max(n, 1) * stride), C.create_string_buffer(max(n, 1) * stride)
        if n:
            self._check(self._L.pm_align_hits_text(self._h, hits.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p), ops, txt, stride))
        cut = lambda b: [b.raw[i * stride:(i + 1) * stride].split(b"\0", 1)[0].decode("latin-1") for i in range(n)]
        return out, cut(ops), cut(txt)

    # -- the caller's tally loop on the device (primer_match -c) ----------------------------------
    def count_scan(self, begin, end, max_count=0):
        """pm_count_scan: the final hits of (begin, end] are re-aligned and tallied in HBM; nothing is handed out."""
        self._check(self._L.pm_count_scan(self._h, begin, end, int(max_count)))
        self._pos = min(self._n, max(self._pos, end))

    def counts(self):
        """pm_counts: (counts uint64[npatterns, k + 1] in add_pattern order, capped uint8[npatterns], info dict)"""
        counts = np.zeros((self._npat, self._k + 1), dtype=np.uint64)
        capped = np.zeros(self._npat, dtype=np.uint8)
        ci = _CountInfo()
        self._check(self._L.pm_counts(self._h, counts.ctypes.data_as(C.c_void_p), capped.ctypes.data_as(C.c_void_p), self._npat, C.byref(ci)))
        info = {name: int(getattr(ci, name)) for name in ("tallied", "skipped", "aligned_device", "aligned_host", "bogus", "record_bytes_to_host")}
        info["first_bogus"] = (int(ci.first_bogus.end), int(ci.first_bogus.pid)) if ci.bogus else None
        return counts, capped, info

    def count_all(self, max_count=0, chunk=1 << 30):
        """The tallies of `primer_match -c [-M max_count]` over the whole stream: (counts, capped, info) as counts()."""
        self.reset()
        pos = 0
        while pos < self._n:
            end = min(self._n, pos + chunk)
            self.count_scan(pos, end, max_count)
            pos = end
        return self.counts()

    # -- pcr_match's pairing stage on the device (pm_pcr_*) ----------------------------------------
    def pcr_setup(self, any_orientation=False, length_between=False, amplicon_min=0, amplicon_max=2000, size_slack=-1,
                  size_lb=None, size_ub=None, entry_starts=(0,)):
        """pm_pcr_setup, after init(): the options of pcr_match's pairing stage (-a, -b, -m, -M, -d), the UniSTS size
        bounds per primer pair (or None) and the stream positions where the FASTA entries start.  The patterns are the
        primers with ids 1..n (2j-1 forward, 2j reverse) and their reverse complements n+1..2n."""
        p = _PcrParams()
        p.any_orientation, p.length_between = int(bool(any_orientation)), int(bool(length_between))
        p.amplicon_min, p.amplicon_max, p.size_slack = int(amplicon_min), int(amplicon_max), int(size_slack)
        keep = []
        if size_lb is not None:
            lb = np.ascontiguousarray(np.asarray(size_lb, dtype=np.uint64))
            ub = np.ascontiguousarray(np.asarray(size_ub, dtype=np.uint64))
            if lb.size != self._npat // 4 or ub.size != lb.size:
                raise PmError(-1, "pcr_setup: one size_lb / size_ub per primer pair")
            keep += [lb, ub]
            p.size_lb, p.size_ub = lb.ctypes.data, ub.ctypes.data
        es = np.ascontiguousarray(np.asarray(entry_starts, dtype=np.int64))
        keep.append(es)
        p.entry_starts, p.n_entries = (es.ctypes.data if es.size else None), es.size
        self._check(self._L.pm_pcr_setup(self._h, C.byref(p)))

    def pcr_feed(self, hits):
        """pm_pcr_feed: append final hits (HIT_DTYPE) to the list the handle holds in HBM."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        self._check(self._L.pm_pcr_feed(self._h, hits.ctypes.data_as(C.c_void_p), hits.size))

    def pcr_scan(self, begin, end):
        """pm_pcr_scan: the final hits of (begin, end] join the held list in HBM; returns how many."""
        n = C.c_size_t()
        self._check(self._L.pm_pcr_scan(self._h, begin, end, C.byref(n)))
        self._pos = min(self._n, max(self._pos, end))
        return n.value

    def pcr_pair(self, scanned_to, more, text=False, stride=0):
        """pm_pcr_pair: one pairing round over the held hits.  Returns the surviving pairs as a PCR_AMPLICON_DTYPE array
        (a copy), or with text=True (survivors, alignment strings, matching texts), the strings as lists of (first hit's,
        partner's) per survivor.  stride: bytes per string (at least the longest pattern + k + 2, as align_hits_text)."""
        stride = max(int(stride), self._maxlen + self._k + 2)
        out, ops, txt, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._check(self._L.pm_pcr_pair(self._h, int(scanned_to), int(bool(more)), int(bool(text)), stride, C.byref(out), C.byref(n),
                                        C.byref(ops), C.byref(txt)))
        m = n.value
        if m:
            rec = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), shape=(m * PCR_AMPLICON_DTYPE.itemsize,)).view(PCR_AMPLICON_DTYPE).copy()
        else:
            rec = np.zeros(0, dtype=PCR_AMPLICON_DTYPE)
        if not text:
            return rec
        def cut(p):
            if not m:
                return []
            raw = C.string_at(p, 2 * m * stride)
            s = [raw[i * stride:(i + 1) * stride].split(b"\0", 1)[0].decode("latin-1") for i in range(2 * m)]
            return [(s[2 * i], s[2 * i + 1]) for i in range(m)]
        return rec, cut(ops), cut(txt)

    def pcr_stats(self):
        """pm_pcr_stats: hits held before / candidate pairs / survivors of the last round; hits re-aligned on the device / on
        the host and bytes copied device -> host since reset()"""
        v = (C.c_uint64 * 6)()
        self._check(self._L.pm_pcr_stats(self._h, v, 6))
        names = ("held", "candidates", "survivors", "aligned_device", "aligned_host", "bytes_to_host")
        return {k: int(v[i]) for i, k in enumerate(names)}

    def selected(self):
        return self._L.pm_selected_semantics(self._h), self._L.pm_selected_kernel(self._h)

    def describe(self):
        buf = C.create_string_buffer(512)
        self._check(self._L.pm_describe(self._h, buf, 512))
        return buf.value.decode()

    def scan_stats(self):
        """pm_scan_stats: counters of the last scan (see include/pm_gpu.h).  Waits for a look-ahead scan that scan() / scan_view()
        left in flight: polled between ranges it takes away the overlap of that scan with the caller's work."""
        v = (C.c_uint64 * 9)()
        self._check(self._L.pm_scan_stats(self._h, v, 9))
        names = ("candidates", "between_stages", "internal_rescans", "blocks", "rounds", "key_hits", "range_splits", "lookahead", "edit_suspects")
        return {k: int(v[i]) for i, k in enumerate(names)}

    def residency(self):
        """pm_stream_residency: the window size in use (0 = whole stream resident), HBM bytes held for the stream now and
        at peak, stream bytes that crossed PCIe and window loads since init, bits per code of the host form (0: bytes)"""
        v = (C.c_int64 * 6)()
        self._check(self._L.pm_stream_residency(self._h, v, 6))
        names = ("window", "held", "peak", "uploaded", "loads", "bits")
        return {k: int(v[i]) for i, k in enumerate(names)}

    def measure_pair_edit_floor(self, mode):
        """pm_measure_pair_edit_floor: (kernel ms, suspect records)"""
        ms, n = C.c_float(), C.c_uint64()
        self._check(self._L.pm_measure_pair_edit_floor(self._h, mode, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def pack_time(self):
        ms = C.c_float()
        self._check(self._L.pm_pack_time(self._h, C.byref(ms)))
        return ms.value

    def last_kernel_time(self):
        ms, n = C.c_float(), C.c_int()
        self._check(self._L.pm_last_kernel_time(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
