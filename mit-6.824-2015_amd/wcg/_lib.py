"""ctypes binding of libwcg.so (C ABI declared in include/wcg.h).

The product path has no CPU fallback: if libwcg.so is missing or no GPU is visible, opening an
engine raises.  Build the library with `python -c "import __graft_entry__ as g; g.build()"`.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# WCG_LIB: an alternative build of the same library (measurement variants only)
LIB_PATH = os.environ.get("WCG_LIB") or os.path.join(_HERE, "libwcg.so")

WCG_OK, WCG_EINVAL, WCG_ENOMEM, WCG_EHIP, WCG_EFULL, WCG_ESTATE = range(6)
RECORD_BYTES = 32

_lib: Optional[ctypes.CDLL] = None

# every symbol include/wcg.h declares (tests check the library exports them all)
EXPORTED = [
    "wcg_open", "wcg_close", "wcg_last_error", "wcg_set_stream", "wcg_reset", "wcg_map",
    "wcg_map_device", "wcg_reduce", "wcg_result_device", "wcg_result_copy", "wcg_partition",
    "wcg_export", "wcg_import", "wcg_timings", "wcg_enable_timing", "wcg_stats", "wcg_ihash",
    "wcg_version", "wcg_map_file", "wcg_partition_all", "wcg_map_json", "wcg_export_count",
    "wcg_export_write", "wcg_merge_runs", "wcg_result_copy_device", "wcg_sync", "wcg_free",
    "wcg_comm_id", "wcg_comm_init", "wcg_exchange", "wcg_gather_merge", "wcg_exchange_plan",
    "wcg_gather_plan", "wcg_exchange_local", "wcg_gather_merge_local", "wcg_reduce_path",
    "wcg_reduce_async", "wcg_reduce_wait", "wcg_ingest_stats", "wcg_top", "wcg_map_size_check",
    "wcg_lookup", "wcg_lookup_device", "wcg_range", "wcg_index_merged", "wcg_load_merged",
    "wcg_load_merged_device", "wcg_seed_stats", "wcg_import_json", "wcg_import_json_device",
    "wcg_by_count", "wcg_by_count_device", "wcg_count_rank", "wcg_by_count_stats",
]
COMM_ID_BYTES = 128
TOP_MAX = 1024                            # WCG_TOP_MAX
U64_MAX = (1 << 64) - 1
JSON_MAP, JSON_RES = 0, 1                 # WCG_JSON_MAP / WCG_JSON_RES: wcg_import_json's modes


class WcgError(RuntimeError):
    """Non-zero status from libwcg (the reference would log.Fatal at this point)."""

    def __init__(self, status: int, msg: str):
        super().__init__(f"wcg status {status}: {msg}")
        self.status = status


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc gfx950)")
    lib = ctypes.CDLL(LIB_PATH)
    P, U64, U32, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    PU64 = ctypes.POINTER(ctypes.c_uint64)
    sig = {
        "wcg_open": (I, [I, U64, U64, ctypes.POINTER(P)]),
        "wcg_close": (I, [P]),
        "wcg_last_error": (ctypes.c_char_p, [P]),
        "wcg_set_stream": (I, [P, P]),
        "wcg_reset": (I, [P]),
        "wcg_map": (I, [P, ctypes.c_char_p, U64]),
        "wcg_map_device": (I, [P, P, U64]),
        "wcg_reduce": (I, [P, PU64, PU64]),
        "wcg_result_device": (I, [P, ctypes.POINTER(P), PU64]),
        "wcg_result_copy": (I, [P, P, U64]),
        "wcg_partition": (I, [P, U32, U32, P, U64, PU64]),
        "wcg_export": (I, [P, U32, U32, ctypes.POINTER(P), PU64]),
        "wcg_import": (I, [P, P, U64]),
        "wcg_timings": (I, [P, ctypes.POINTER(ctypes.c_double), I, PU64]),
        "wcg_enable_timing": (I, [P, I]),
        "wcg_stats": (I, [P, PU64]),
        "wcg_ihash": (U32, [ctypes.c_char_p, U64]),
        "wcg_version": (ctypes.c_char_p, []),
        "wcg_map_file": (I, [P, ctypes.c_char_p, PU64, PU64]),
        "wcg_partition_all": (I, [P, U32, P, U64, PU64]),
        "wcg_map_json": (I, [P, ctypes.c_char_p, U64, U32, P, U64, PU64]),
        "wcg_export_count": (I, [P, U32, U32, PU64]),
        "wcg_export_write": (I, [P, P]),
        "wcg_merge_runs": (I, [P, P, PU64, U32, PU64, PU64]),
        "wcg_result_copy_device": (I, [P, P]),
        "wcg_sync": (I, [P]),
        "wcg_free": (I, [P, P]),
        "wcg_comm_id": (I, [P]),
        "wcg_comm_init": (I, [P, P, I, I]),
        "wcg_exchange": (I, [P, U32, PU64, PU64]),
        "wcg_gather_merge": (I, [P, I, PU64, PU64]),
        "wcg_exchange_plan": (I, [PU64, U32, U32, PU64, PU64, PU64, PU64, PU64]),
        "wcg_gather_plan": (I, [PU64, U32, U32, PU64, PU64]),
        "wcg_exchange_local": (I, [ctypes.POINTER(P), U32, U32, PU64, PU64]),
        "wcg_gather_merge_local": (I, [ctypes.POINTER(P), U32, U32, PU64, PU64]),
        "wcg_reduce_path": (I, [P, ctypes.POINTER(I)]),
        "wcg_reduce_async": (I, [P]),
        "wcg_reduce_wait": (I, [P, PU64, PU64]),
        "wcg_ingest_stats": (I, [P, ctypes.POINTER(ctypes.c_double), I]),
        "wcg_top": (I, [P, U32, P, U64, PU64, PU64]),
        "wcg_map_size_check": (I, [U64]),
        "wcg_lookup": (I, [P, ctypes.c_char_p, PU64, U64, PU64]),
        "wcg_lookup_device": (I, [P, P, P, U64, P]),
        "wcg_range": (I, [P, ctypes.c_char_p, U64, ctypes.c_char_p, U64, P, U64, PU64, PU64]),
        "wcg_index_merged": (I, [P, PU64]),
        "wcg_load_merged": (I, [P, ctypes.c_char_p, U64, PU64]),
        "wcg_load_merged_device": (I, [P, P, U64, PU64]),
        "wcg_import_json": (I, [P, ctypes.c_char_p, U64, I, PU64]),
        "wcg_import_json_device": (I, [P, P, U64, I, PU64]),
        "wcg_seed_stats": (I, [P, PU64]),
        "wcg_by_count": (I, [P, U64, U64, P, U64, PU64, PU64]),
        "wcg_by_count_device": (I, [P, U64, U64, ctypes.POINTER(P), PU64, PU64]),
        "wcg_count_rank": (I, [P, PU64, U64, PU64]),
        "wcg_by_count_stats": (I, [P, ctypes.POINTER(ctypes.c_double), I]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("WCG_LIB") and not hasattr(lib, name):
            continue                          # a measurement variant built from an older tree
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_hiprt = None


def _hip() -> ctypes.CDLL:
    """The HIP runtime (plain copies between host buffers and libwcg's device buffers)."""
    global _hiprt
    if _hiprt is None:
        for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
            try:
                h = ctypes.CDLL(name)
                break
            except OSError:
                continue
        else:
            raise ImportError("libamdhip64.so not found")
        h.hipMemcpy.restype = ctypes.c_int
        h.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        h.hipMalloc.restype = ctypes.c_int
        h.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        h.hipFree.restype = ctypes.c_int
        h.hipFree.argtypes = [ctypes.c_void_p]
        h.hipDeviceSynchronize.restype = ctypes.c_int
        _hiprt = h
    return _hiprt


def _hip_check(rc: int, what: str) -> None:
    if rc != 0:
        raise WcgError(WCG_EHIP, f"{what} failed: hipError {rc}")


def ihash(key: bytes) -> int:
    """FNV-1a 32 (mapreduce.go:185-189) via the library's host helper."""
    return load().wcg_ihash(key, len(key))


class Engine:
    """One GPU's word-count context (wraps wcg_ctx).

    Phase methods mirror the reference data plane: map_* = DoMap+Map over a split,
    reduce() = DoReduce x R + Merge, partition() = one DoReduce output file."""

    def __init__(self, device: int = 0, max_input_bytes: int = 0, max_keys: int = 1 << 20):
        self._lib = load()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.wcg_open(device, max_input_bytes, max_keys, ctypes.byref(self._ctx))
        if rc != WCG_OK:
            msg = self._lib.wcg_last_error(self._ctx).decode() if self._ctx else "open failed"
            if self._ctx:
                self._lib.wcg_close(self._ctx)
                self._ctx = ctypes.c_void_p()
            raise WcgError(rc, msg)
        self.device = device

    # -- plumbing
    def _chk(self, rc: int) -> None:
        if rc != WCG_OK:
            raise WcgError(rc, self._lib.wcg_last_error(self._ctx).decode())

    def close(self) -> None:
        if self._ctx:
            self._lib.wcg_close(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int) -> None:
        self._chk(self._lib.wcg_set_stream(self._ctx, ctypes.c_void_p(stream_ptr)))

    def enable_timing(self, on=True) -> None:
        """on = True/1: phase times of the last job; 2: summed over every job from now on (no
        timings() call, hence no host round trip, needed between jobs); 3: as 2, the map kernel
        only (each event is a ~5 us bubble between kernels); False/0: off."""
        mode = on if on in (2, 3) and on is not True else (1 if on else 0)
        self._chk(self._lib.wcg_enable_timing(self._ctx, mode))

    # -- phases
    def reset(self) -> None:
        self._chk(self._lib.wcg_reset(self._ctx))

    def map_host(self, data: bytes) -> None:
        self._chk(self._lib.wcg_map(self._ctx, data, len(data)))

    def map_device(self, dev_ptr: int, n: int) -> None:
        self._chk(self._lib.wcg_map_device(self._ctx, ctypes.c_void_p(dev_ptr), n))

    def map_file(self, path: str) -> Tuple[int, int]:
        """Split + DoMap of a whole file through the pinned double-buffered ingest; returns
        (bytes mapped, file size) - fewer bytes mapped when a 64 KiB+ line ended the scan (P1)."""
        mapped, size = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_map_file(self._ctx, os.fsencode(path), ctypes.byref(mapped), ctypes.byref(size)))
        return mapped.value, size.value

    def map_json(self, data: bytes, nreduce: int) -> List[bytes]:
        """DoMap's reference-exact JSON intermediate files (one per partition) for one split."""
        sizes = (ctypes.c_uint64 * nreduce)()
        self._chk(self._lib.wcg_map_json(self._ctx, data, len(data), nreduce, None, 0, sizes))
        total = sum(sizes)
        buf = ctypes.create_string_buffer(max(total, 1))
        self._chk(self._lib.wcg_map_json(self._ctx, data, len(data), nreduce, buf, total, sizes))
        return _slices(buf.raw, list(sizes))

    def reduce(self) -> Tuple[int, int]:
        nk, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_reduce(self._ctx, ctypes.byref(nk), ctypes.byref(nb)))
        return nk.value, nb.value

    def reduce_async(self) -> None:
        """wcg_reduce_async: queue the reduce (no host wait); reduce_wait() or any result call
        waits for it, the next reset()/map_*() drops it."""
        self._chk(self._lib.wcg_reduce_async(self._ctx))

    def reduce_wait(self) -> Tuple[int, int]:
        nk, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_reduce_wait(self._ctx, ctypes.byref(nk), ctypes.byref(nb)))
        return nk.value, nb.value

    def result_device(self) -> Tuple[int, int]:
        p, nb = ctypes.c_void_p(), ctypes.c_uint64()
        self._chk(self._lib.wcg_result_device(self._ctx, ctypes.byref(p), ctypes.byref(nb)))
        return p.value or 0, nb.value

    def result_copy_device(self, dev_ptr: int) -> None:
        """Async device copy of the formatted output into a caller's buffer (context stream)."""
        self._chk(self._lib.wcg_result_copy_device(self._ctx, ctypes.c_void_p(dev_ptr)))

    def sync(self) -> None:
        self._chk(self._lib.wcg_sync(self._ctx))

    def free(self, dev_ptr: int) -> None:
        """wcg_free: release the device buffer of result_device() or export() early."""
        self._chk(self._lib.wcg_free(self._ctx, dev_ptr))

    def result(self) -> bytes:
        _, nb = self.result_device()
        buf = ctypes.create_string_buffer(max(nb, 1))
        self._chk(self._lib.wcg_result_copy(self._ctx, buf, nb))
        return buf.raw[:nb]

    def partitions(self, nreduce: int) -> List[bytes]:
        """Every -res-<r> file of the last reduce (one device formatting pass for all)."""
        sizes = (ctypes.c_uint64 * nreduce)()
        self._chk(self._lib.wcg_partition_all(self._ctx, nreduce, None, 0, sizes))
        total = sum(sizes)
        buf = ctypes.create_string_buffer(max(total, 1))
        self._chk(self._lib.wcg_partition_all(self._ctx, nreduce, buf, total, sizes))
        return _slices(buf.raw, list(sizes))

    def partition(self, nreduce: int, r: int) -> bytes:
        nb = ctypes.c_uint64()
        self._chk(self._lib.wcg_partition(self._ctx, nreduce, r, None, 0, ctypes.byref(nb)))
        buf = ctypes.create_string_buffer(max(nb.value, 1))
        self._chk(self._lib.wcg_partition(self._ctx, nreduce, r, buf, nb.value, ctypes.byref(nb)))
        return buf.raw[:nb.value]

    def top_size(self, n: int) -> Tuple[int, int]:
        """wcg_top with host_out == NULL: (lines, bytes) of top(n); the lines stay on the device."""
        if not 0 <= n <= 0xFFFFFFFF:
            raise WcgError(WCG_EINVAL, "top: n out of range")
        nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_top(self._ctx, n, None, 0, ctypes.byref(nl), ctypes.byref(nb)))
        return nl.value, nb.value

    def top(self, n: int) -> bytes:
        """The n most frequent words of the last reduce (n <= TOP_MAX), selected on the device: the
        bytes `LC_ALL=C sort -n -k2 <merged file> | tail -n <n>` prints (test-wc.sh:2-3)."""
        _, nb = self.top_size(n)
        buf = ctypes.create_string_buffer(max(nb, 1))
        nl2, nb2 = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_top(self._ctx, n, buf, nb, ctypes.byref(nl2), ctypes.byref(nb2)))
        return buf.raw[:nb2.value]

    def lookup(self, words: Sequence[bytes]) -> List[int]:
        """The count of every word in the last reduce, 0 for a word that does not occur, in the
        order asked (wcg_lookup: binary searches on the device; only the counts come back).  Any
        bytes may be asked for."""
        nq = len(words)
        if nq == 0:
            self._chk(self._lib.wcg_lookup(self._ctx, None, None, 0, None))
            return []
        off = (ctypes.c_uint64 * (nq + 1))()
        total = 0
        for i, w in enumerate(words):
            total += len(w)
            off[i + 1] = total
        counts = (ctypes.c_uint64 * nq)()
        self._chk(self._lib.wcg_lookup(self._ctx, b"".join(words), off, nq, counts))
        return list(counts)

    def lookup_device(self, keys_ptr: int, off_ptr: int, nq: int, counts_ptr: int) -> None:
        """wcg_lookup_device: key bytes, nq + 1 u64 offsets and nq u64 counts in device memory;
        asynchronous on the engine's stream (sync() or a stream wait before the counts are read)."""
        self._chk(self._lib.wcg_lookup_device(self._ctx, ctypes.c_void_p(keys_ptr), ctypes.c_void_p(off_ptr), nq,
                                              ctypes.c_void_p(counts_ptr)))

    def range_size(self, lo: Optional[bytes] = None, hi: Optional[bytes] = None) -> Tuple[int, int]:
        """wcg_range with host_out == NULL: (lines, bytes) of range(lo, hi); the lines stay on the device."""
        nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_range(self._ctx, lo, len(lo) if lo is not None else 0, hi,
                                      len(hi) if hi is not None else 0, None, 0, ctypes.byref(nl), ctypes.byref(nb)))
        return nl.value, nb.value

    def range(self, lo: Optional[bytes] = None, hi: Optional[bytes] = None) -> bytes:
        """The merged file's lines with lo <= key < hi (bytewise; None: unbounded on that side),
        found and formatted on the device: what range_of_merged(result(), lo, hi) computes."""
        _, nb = self.range_size(lo, hi)
        buf = ctypes.create_string_buffer(max(nb, 1))
        nl2, nb2 = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_range(self._ctx, lo, len(lo) if lo is not None else 0, hi,
                                      len(hi) if hi is not None else 0, buf, nb, ctypes.byref(nl2), ctypes.byref(nb2)))
        return buf.raw[:nb2.value]

    def prefix(self, p: bytes) -> bytes:
        """The merged file's lines whose key starts with p: range(p, prefix_succ(p))."""
        return self.range(p, prefix_succ(p))

    @staticmethod
    def _window(first: int, n: Optional[int]) -> Tuple[int, int]:
        n = U64_MAX if n is None else n
        if not (0 <= first <= U64_MAX and 0 <= n <= U64_MAX):
            raise WcgError(WCG_EINVAL, "by_count: first or n out of range")
        return first, n

    def by_count_size(self, first: int = 0, n: Optional[int] = None) -> Tuple[int, int]:
        """wcg_by_count with host_out == NULL: (lines, bytes) of by_count(first, n); the lines stay
        on the device."""
        first, n = self._window(first, n)
        nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_by_count(self._ctx, first, n, None, 0, ctypes.byref(nl), ctypes.byref(nb)))
        return nl.value, nb.value

    def by_count(self, first: int = 0, n: Optional[int] = None) -> bytes:
        """The lines at ranks [first, first + n) of the merged file in count order (n = None: to the
        end), sorted and formatted on the device: what by_count_of_merged(result(), first, n)
        computes, the bytes of `LC_ALL=C sort -n -k2 <merged file>` from line `first` on."""
        first, n = self._window(first, n)
        _, nb = self.by_count_size(first, n)
        buf = ctypes.create_string_buffer(max(nb, 1))
        nl2, nb2 = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_by_count(self._ctx, first, n, buf, nb, ctypes.byref(nl2), ctypes.byref(nb2)))
        return buf.raw[:nb2.value]

    def by_count_device(self, first: int = 0, n: Optional[int] = None) -> Tuple[int, int, int]:
        """wcg_by_count_device: (device pointer, lines, bytes) of the same lines, left in the
        engine's window buffer (valid until the next by_count* call with another window, or the
        next job)."""
        first, n = self._window(first, n)
        p, nl, nb = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_by_count_device(self._ctx, first, n, ctypes.byref(p), ctypes.byref(nl), ctypes.byref(nb)))
        return p.value or 0, nl.value, nb.value

    def count_rank(self, counts: Sequence[int]) -> List[int]:
        """For every count c asked, the number of keys of the last reduce whose count is below c
        (wcg_count_rank: binary searches over the count order on the device).  The keys with a
        count >= c are the ranks [rank(c), keys) of by_count."""
        nq = len(counts)
        if nq == 0:
            self._chk(self._lib.wcg_count_rank(self._ctx, None, 0, None))
            return []
        if not all(0 <= int(c) <= U64_MAX for c in counts):
            raise WcgError(WCG_EINVAL, "count_rank: a count outside 0 .. 2^64-1")
        q = (ctypes.c_uint64 * nq)(*[int(c) for c in counts])
        r = (ctypes.c_uint64 * nq)()
        self._chk(self._lib.wcg_count_rank(self._ctx, q, nq, r))
        return list(r)

    def at_least(self, c: int) -> bytes:
        """The lines whose count is at least c, in count order: one rank, then one window."""
        return self.by_count(self.count_rank([c])[0], None)

    def by_count_stats(self) -> dict:
        """The last build of the count order (wcg_by_count_stats): whether the engine holds one, the
        digit passes it ran, and (with enable_timing on during the build) their device ms."""
        v = (ctypes.c_double * 11)()
        self._chk(self._lib.wcg_by_count_stats(self._ctx, v, 11))
        mask = int(v[1])
        return {"built": bool(v[0]), "digits": [d for d in range(8) if mask >> d & 1], "items_ms": v[2],
                "pass_ms": {d: v[3 + d] for d in range(8) if mask >> d & 1}}

    def export(self, nreduce: int, nranks: int) -> Tuple[int, List[int]]:
        """Bucket the local aggregate by owner rank; returns (device ptr, units per rank)."""
        p = ctypes.c_void_p()
        counts = (ctypes.c_uint64 * nranks)()
        self._chk(self._lib.wcg_export(self._ctx, nreduce, nranks, ctypes.byref(p), counts))
        return p.value or 0, list(counts)

    def export_count(self, nreduce: int, nranks: int) -> List[int]:
        """Units per destination rank of the local aggregate (one host synchronisation)."""
        counts = (ctypes.c_uint64 * nranks)()
        self._chk(self._lib.wcg_export_count(self._ctx, nreduce, nranks, counts))
        return list(counts)

    def export_write(self, dev_ptr: int) -> None:
        """Write the units counted by export_count into a caller's device buffer (async)."""
        self._chk(self._lib.wcg_export_write(self._ctx, ctypes.c_void_p(dev_ptr)))

    def import_records(self, dev_ptr: int, nunits: int) -> None:
        self._chk(self._lib.wcg_import(self._ctx, ctypes.c_void_p(dev_ptr), nunits))

    def merge_runs(self, dev_ptr: int, run_bytes: List[int]) -> Tuple[int, int]:
        """Merge sorted "key: count\n" runs held back to back at dev_ptr into this context's
        result (Merge, mapreduce.go:284-321); returns (keys, bytes)."""
        rb = (ctypes.c_uint64 * max(len(run_bytes), 1))(*run_bytes)
        nk, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_merge_runs(self._ctx, ctypes.c_void_p(dev_ptr), rb, len(run_bytes),
                                           ctypes.byref(nk), ctypes.byref(nb)))
        return nk.value, nb.value

    def index_merged(self) -> int:
        """wcg_index_merged: make the merged file this engine holds (after merge_runs, gather_merge
        on the root, load_merged) queryable by top / lookup / range / prefix; returns its lines.
        A file that breaks a rule of check_merged raises WcgError(WCG_EINVAL) naming line and rule."""
        nl = ctypes.c_uint64()
        self._chk(self._lib.wcg_index_merged(self._ctx, ctypes.byref(nl)))
        return nl.value

    def load_merged(self, data: bytes) -> int:
        """wcg_load_merged: one sorted "key: count\n" file (an mrtmp.<file> that already exists)
        becomes this engine's merged result, checked and indexed; returns its lines."""
        nl = ctypes.c_uint64()
        self._chk(self._lib.wcg_load_merged(self._ctx, data, len(data), ctypes.byref(nl)))
        return nl.value

    def load_merged_device(self, dev_ptr: int, n: int) -> int:
        """wcg_load_merged_device: the same for n bytes in device memory (synchronous)."""
        nl = ctypes.c_uint64()
        self._chk(self._lib.wcg_load_merged_device(self._ctx, ctypes.c_void_p(dev_ptr), n, ctypes.byref(nl)))
        return nl.value

    def import_json(self, data: bytes, mode: int) -> int:
        """wcg_import_json: one of the reference's JSON files (mode JSON_MAP: DoMap's per-occurrence
        intermediates; JSON_RES: a DoReduce -res file) decoded on the GPU and added to the tables, as
        map_host / import_host add; returns its lines.  A file that breaks a rule raises
        WcgError(WCG_EINVAL) naming line and rule, and leaves the engine as it was."""
        nl = ctypes.c_uint64()
        self._chk(self._lib.wcg_import_json(self._ctx, data if data else None, len(data), mode, ctypes.byref(nl)))
        return nl.value

    def import_json_device(self, dev_ptr: int, n: int, mode: int) -> int:
        """wcg_import_json_device: the same for n bytes in device memory (synchronous)."""
        nl = ctypes.c_uint64()
        self._chk(self._lib.wcg_import_json_device(self._ctx, ctypes.c_void_p(dev_ptr), n, mode, ctypes.byref(nl)))
        return nl.value

    # -- the shuffle and the final Merge over RCCL, inside the library
    @staticmethod
    def comm_id() -> bytes:
        """ncclGetUniqueId (made once, on rank 0, and handed to every rank by the host)."""
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        rc = load().wcg_comm_id(buf)
        if rc != WCG_OK:
            raise WcgError(rc, "wcg_comm_id: ncclGetUniqueId failed")
        return buf.raw

    def comm_init(self, comm_id: bytes, rank: int, world: int) -> None:
        """ncclCommInitRank for this engine (collective: every rank calls it)."""
        if len(comm_id) != COMM_ID_BYTES:
            raise WcgError(WCG_EINVAL, "comm_init: the id is 128 bytes")
        self._chk(self._lib.wcg_comm_init(self._ctx, comm_id, rank, world))

    def exchange(self, nreduce: int) -> Tuple[int, int]:
        """The ihash % nreduce shuffle (collective): afterwards this engine holds exactly the keys
        of the partitions its rank owns.  Returns (units sent, units received)."""
        snt, rcv = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_exchange(self._ctx, nreduce, ctypes.byref(snt), ctypes.byref(rcv)))
        return snt.value, rcv.value

    def gather_merge(self, root: int = 0) -> Tuple[int, int]:
        """Merge of every rank's sorted run at root (collective, after reduce()); (keys, bytes) of
        the merged file on root, (0, 0) elsewhere."""
        nk, nb = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._lib.wcg_gather_merge(self._ctx, root, ctypes.byref(nk), ctypes.byref(nb)))
        return nk.value, nb.value

    # -- host copies of the record units (the file-based shuffle of the config-5 workers)
    def export_host(self, nreduce: int, nranks: int) -> Tuple[bytes, List[int]]:
        """export() copied to host memory: (record units, units per rank)."""
        ptr, counts = self.export(nreduce, nranks)
        n = sum(counts) * RECORD_BYTES
        buf = ctypes.create_string_buffer(max(n, 1))
        if n:
            _hip_check(_hip().hipMemcpy(buf, ctypes.c_void_p(ptr), n, 2), "hipMemcpy D2H")
        return buf.raw[:n], counts

    def import_host(self, records: bytes) -> None:
        """import_records() from host memory (staged through a temporary device buffer)."""
        if len(records) % RECORD_BYTES:
            raise WcgError(WCG_EINVAL, "import_host: not a whole number of record units")
        n = len(records) // RECORD_BYTES
        if n == 0:
            return
        hip = _hip()
        dev = ctypes.c_void_p()
        _hip_check(hip.hipMalloc(ctypes.byref(dev), len(records)), "hipMalloc")
        try:
            _hip_check(hip.hipMemcpy(dev, records, len(records), 1), "hipMemcpy H2D")
            self.import_records(dev.value, n)
            _hip_check(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
        finally:
            hip.hipFree(dev)

    # -- diagnostics
    PHASES = ("map", "agg", "compact", "sort", "format", "export", "exchange", "import", "gather", "merge")

    def timings(self) -> Tuple[dict, int]:
        """Device ms per phase of the last job (needs enable_timing) and map launch count."""
        ms = (ctypes.c_double * 10)()
        nl = ctypes.c_uint64()
        self._chk(self._lib.wcg_timings(self._ctx, ms, 10, ctypes.byref(nl)))
        return dict(zip(self.PHASES, list(ms))), nl.value

    def reduce_path(self) -> int:
        """1 if the last reduce() ran the one-launch reduce (wcg_fused.h), 0 for the multi-launch one."""
        v = ctypes.c_int()
        self._chk(self._lib.wcg_reduce_path(self._ctx, ctypes.byref(v)))
        return v.value

    INGEST_STATS = ["host_issue_ms", "read_ms", "slot_wait_ms", "copy_ms", "copy_span_ms",
                    "copy_engine_idle_frac", "map_ms", "device_span_ms", "chunks"]

    def ingest_stats(self) -> dict:
        """The last map_file / map_host ingest's breakdown (wcg_ingest_stats): host reading and
        slot waits, the chunks' H2D copies and the copy engine's idle share of its span, the
        chunks' map kernels, and the device span from the first copy to the last map."""
        v = (ctypes.c_double * len(self.INGEST_STATS))()
        self._chk(self._lib.wcg_ingest_stats(self._ctx, v, len(self.INGEST_STATS)))
        return dict(zip(self.INGEST_STATS, list(v)))

    def seed_stats(self) -> dict:
        """The seed of k_map's LDS key tables (wcg_seed_stats): whether the context holds one, how
        many it has built, and whether the last finished job's map calls all ran seeded."""
        s = (ctypes.c_uint64 * 3)()
        self._chk(self._lib.wcg_seed_stats(self._ctx, s))
        return {"valid": bool(s[0]), "builds": int(s[1]), "last_job_seeded": bool(s[2])}

    def stats(self) -> dict:
        s = (ctypes.c_uint64 * 9)()
        self._chk(self._lib.wcg_stats(self._ctx, s))
        keys = ["tokens", "keys", "lds_hits", "global_ops", "long_tokens", "arena_bytes", "overflow",
                "spin_fail", "emitted"]
        return dict(zip(keys, list(s)))


def _slices(raw: bytes, sizes: List[int]) -> List[bytes]:
    out, off = [], 0
    for n in sizes:
        out.append(raw[off:off + n])
        off += n
    return out


def exchange_plan(counts: List[List[int]], rank: int) -> dict:
    """wcg_exchange_plan: counts[s][d] = units rank s sends to rank d -> this rank's send / receive
    offsets and counts (host arithmetic, no GPU)."""
    W = len(counts)
    flat = (ctypes.c_uint64 * (W * W))(*[int(x) for row in counts for x in row])
    so, sc, ro, rc = [(ctypes.c_uint64 * W)() for _ in range(4)]
    tot = (ctypes.c_uint64 * 2)()
    st = load().wcg_exchange_plan(flat, W, rank, so, sc, ro, rc, tot)
    if st != WCG_OK:
        raise WcgError(st, "wcg_exchange_plan: bad arguments")
    return {"send_off": list(so), "send_cnt": list(sc), "recv_off": list(ro), "recv_cnt": list(rc),
            "sent": tot[0], "received": tot[1]}


def gather_plan(sizes: List[int], root: int) -> Tuple[List[int], int]:
    """wcg_gather_plan: where each rank's run lands in root's receive buffer, and the total."""
    W = len(sizes)
    sz = (ctypes.c_uint64 * max(W, 1))(*sizes)
    off = (ctypes.c_uint64 * max(W, 1))()
    tot = ctypes.c_uint64()
    st = load().wcg_gather_plan(sz, W, root, off, ctypes.byref(tot))
    if st != WCG_OK:
        raise WcgError(st, "wcg_gather_plan: bad arguments")
    return list(off)[:W], tot.value


def _ctx_array(engines: List["Engine"]):
    return (ctypes.c_void_p * len(engines))(*[e._ctx.value for e in engines])


def exchange_local(engines: List["Engine"], nreduce: int) -> Tuple[List[int], List[int]]:
    """wcg_exchange_local: the shuffle across engines of this process (a world of len(engines)
    ranks, device copies for transport).  Returns (units sent, units received) per engine."""
    W = len(engines)
    snt, rcv = (ctypes.c_uint64 * W)(), (ctypes.c_uint64 * W)()
    st = load().wcg_exchange_local(_ctx_array(engines), W, nreduce, snt, rcv)
    if st != WCG_OK:
        msgs = "; ".join(load().wcg_last_error(e._ctx).decode() for e in engines)
        raise WcgError(st, f"wcg_exchange_local: {msgs}")
    return list(snt), list(rcv)


def gather_merge_local(engines: List["Engine"], root: int) -> Tuple[int, int]:
    """wcg_gather_merge_local: every engine's sorted run merged into engines[root]'s result."""
    nk, nb = ctypes.c_uint64(), ctypes.c_uint64()
    st = load().wcg_gather_merge_local(_ctx_array(engines), len(engines), root, ctypes.byref(nk), ctypes.byref(nb))
    if st != WCG_OK:
        msgs = "; ".join(load().wcg_last_error(e._ctx).decode() for e in engines)
        raise WcgError(st, f"wcg_gather_merge_local: {msgs}")
    return nk.value, nb.value


def _count_lines(merged: bytes) -> List[Tuple[int, bytes]]:
    """(count, key) of every "key: count\\n" line, in the file's order"""
    out = []
    for line in merged.split(b"\n"):
        if line:
            key, _, cnt = line.rpartition(b": ")
            out.append((int(cnt), key))
    return out


def _lines_of(items: List[Tuple[int, bytes]]) -> bytes:
    return b"".join(k + b": " + str(c).encode() + b"\n" for c, k in items)


def top_of_merged(merged: bytes, n: int) -> bytes:
    """What Engine.top(n) computes, stated on the host: the last n lines of the merged file
    ("key: count\\n" in bytewise key order) after a stable sort by count - the bytes of
    `LC_ALL=C sort -n -k2 <merged file> | tail -n <n>` (test-wc.sh:2-3).  Counts are Python
    integers (no width limit); lines of equal count stay in key order."""
    if n <= 0:
        return b""
    items = _count_lines(merged)
    items.sort(key=lambda it: it[0])                # stable: ties keep the file's key order
    return _lines_of(items[-n:])


def top_merge(parts: List[bytes], n: int) -> bytes:
    """The global top n from the tops of ranks that own disjoint keys (Engine.top(n) on every rank
    after exchange + reduce): at most len(parts) * n lines are parsed, no GPU.  The parts are not
    in one key order, so the order is (count, key bytes) outright."""
    if n <= 0:
        return b""
    items = [it for p in parts for it in _count_lines(p)]
    items.sort()
    return _lines_of(items[-n:])


def by_count_of_merged(merged: bytes, first: int = 0, n: Optional[int] = None) -> bytes:
    """What Engine.by_count(first, n) computes, stated on the host: the merged file's lines after a
    stable sort by count (the bytes of `LC_ALL=C sort -n -k2 <merged file>`: ascending counts, lines
    of equal count in the file's key order), from line `first` on, n lines at most (None: all)."""
    items = _count_lines(merged)
    items.sort(key=lambda it: it[0])                # stable: ties keep the file's key order
    first = max(0, first)
    return _lines_of(items[first:] if n is None else items[first:first + max(0, n)])


def count_rank_of_merged(merged: bytes, counts: Sequence[int]) -> List[int]:
    """What Engine.count_rank(counts) computes, stated on the host: for every count asked, the
    number of the merged file's lines whose count is below it."""
    import bisect
    have = sorted(c for c, _ in _count_lines(merged))
    return [bisect.bisect_left(have, int(c)) for c in counts]


def by_count_merge(parts: List[bytes]) -> bytes:
    """The whole job's count order from the count orders of ranks that own disjoint keys
    (Engine.by_count() on every rank after exchange + reduce), combined on the host.  The parts are
    not in one key order, so the order is (count, key bytes) outright, as in top_merge."""
    items = [it for p in parts for it in _count_lines(p)]
    items.sort()
    return _lines_of(items)


def _key_lines(merged: bytes) -> List[Tuple[bytes, bytes]]:
    """(key, line) of every "key: count\\n" line, in the file's order"""
    out = []
    for line in merged.split(b"\n"):
        if line:
            out.append((line.rpartition(b": ")[0], line + b"\n"))
    return out


def lookup_in_merged(merged: bytes, words: Sequence[bytes]) -> List[int]:
    """What Engine.lookup(words) computes, stated on the host: each word's count in the merged
    file ("key: count\\n" lines), 0 for a word that has no line; counts are Python integers."""
    counts = {k: c for c, k in _count_lines(merged)}
    return [counts.get(bytes(w), 0) for w in words]


def range_of_merged(merged: bytes, lo: Optional[bytes] = None, hi: Optional[bytes] = None) -> bytes:
    """What Engine.range(lo, hi) computes, stated on the host: the merged file's lines whose key k
    has lo <= k < hi as byte strings (Python's bytes order: bytewise, a prefix first), in the
    file's order; None leaves that side open."""
    return b"".join(line for k, line in _key_lines(merged)
                    if (lo is None or lo <= k) and (hi is None or k < hi))


KEY_BYTES_MAX = (1 << 23) - 1             # LONG_LEN_MAX: the longest key a record describes
MERGED_KINDS = ("count", "zero", "nul", "order", "newline")


def check_merged(merged: bytes) -> Optional[Tuple[int, str]]:
    """The rules Engine.index_merged / load_merged hold a merged file to, stated on the host: None
    for a valid file, else (index of the first bad line, rule), the rule being the word
    wcg_last_error uses.  A line's key ends at its first ':' (a line without one is all key).
    Per line, in this order:
      "count"  the line is key, ": ", a canonical decimal in 1 .. 2^64-1 (first digit 1-9, at most
               20 digits), newline, and the key has 1 .. KEY_BYTES_MAX bytes
      "zero"   the count is not "0"
      "nul"    the key holds no zero byte
      "order"  the key sorts strictly after the previous line's (Python's bytes order)
    and, for the file, "newline": a last line without its newline (load_merged looks at this
    first, so it is reported whatever the lines before hold)."""
    merged = bytes(merged)
    if merged and not merged.endswith(b"\n"):
        return merged.count(b"\n"), "newline"
    prev = None
    for i, line in enumerate(merged.split(b"\n")[:-1]):
        line += b"\n"
        klen = line.find(b":")
        if klen < 0:
            klen = len(line)
        key = line[:klen]
        body = line[:-1]
        nd = 0
        while nd < 21 and nd < len(body) and 0x30 <= body[len(body) - 1 - nd] <= 0x39:
            nd += 1
        digits = body[len(body) - nd:]
        bad = None
        if nd == 0 or nd > 20 or klen == 0 or klen > KEY_BYTES_MAX or len(line) != klen + 3 + nd or line[klen:klen + 2] != b": ":
            bad = "count"
        elif digits[:1] == b"0":
            bad = "zero" if nd == 1 else "count"
        elif int(digits) > 0xFFFFFFFFFFFFFFFF:
            bad = "count"
        elif b"\0" in key:
            bad = "nul"
        if bad is None and prev is not None and not prev < key:
            bad = "order"
        # a zero byte in the key, or a key out of order, of a line whose count is bad: "count" stands
        if bad is not None:
            return i, bad
        prev = key
    return None


def prefix_succ(p: bytes) -> Optional[bytes]:
    """The least byte string above every string that starts with p: p without its trailing 0xFF
    bytes and with its last byte incremented; None (no upper bound) when p is empty or all 0xFF."""
    q = bytes(p).rstrip(b"\xff")
    return q[:-1] + bytes([q[-1] + 1]) if q else None


def version() -> str:
    return load().wcg_version().decode()
