"""The MDSL garbage collector's data pass on the GPU (include/pom_gc.h).

Python mirror of what mdsl_gc_data_round does per ITB (mdsl/gc.c:945-993) and
mdsl_gc_data_stat with its range tree (mdsl/gc.c:1020-1113, lib/brtree.c):
  scan_dev   <- the bitmap walk with __add_to_brtree (mdsl/gc.c:968-993,
                :788-802) over decoded payloads in HBM
  scan_batch <- the decode switch and the walk over records in host memory;
                only counts and ranges come back from the GPU
  merge_dev  <- brt_add, brt_loop_on_ranges and gc_data_stat_cb over ranges in
                HBM: the merged map and its sums
  stat_batch <- all of it over records in host memory, with the extents of
                earlier rounds; only the merged map comes back from the GPU
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import numpy as np

from . import lzo

E_TRUNCATED = -4097
E_NOSPACE = -4098
EINVAL = -22

ADEPTH_OFF, ENTRIES_OFF = 3, 4
BITMAP_OFF, BITMAP_BYTES, INDEX_OFF, ITE_OFF = 3584, 128, 3712, 11904
ITE_SIZE, ITE_COLUMN_OFF, ITE_COLUMNS = 512, 368, 6
COLUMN_SIZE, COLUMN_LEN_OFF, COLUMN_OFFSET_OFF = 24, 8, 16

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_gc_scan_dev.restype = ctypes.c_int
        lib.pom_gc_scan_dev.argtypes = [_vp] * 5 + [ctypes.c_uint32, ctypes.c_int] + [_vp] * 4 + \
            [ctypes.c_uint64, _vp, _vp]
        lib.pom_gc_scan_batch.restype = ctypes.c_int
        lib.pom_gc_scan_batch.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t] + \
            [_vp] * 5
        lib.pom_gc_merge_scratch.restype = ctypes.c_size_t
        lib.pom_gc_merge_scratch.argtypes = [ctypes.c_uint32]
        lib.pom_gc_merge_dev.restype = ctypes.c_int
        lib.pom_gc_merge_dev.argtypes = [_vp, ctypes.c_uint32, _vp, ctypes.c_size_t, _vp, ctypes.c_uint64, _vp, _vp]
        lib.pom_gc_stat_batch.restype = ctypes.c_int
        lib.pom_gc_stat_batch.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t,
                                          _vp, ctypes.c_size_t] + [_vp] * 5
        _bound = True
    return lib


def scan_dev(payload: lzo.DeviceBatch, adepth, column: int, live, nranges, first, ranges, err,
             status=None, ranges_cap: "int | None" = None, stream=None) -> None:
    """Enqueue pom_gc_scan_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64, length int32 = the
    produced lengths, e.g. decompress_dev's out_len); adepth: uint8 per ITB;
    status: int32 per ITB or None.  Outputs, all on the GPU: live, nranges
    (int32, read as uint32), err (int32), first (int64, nblocks + 1), ranges
    (int64, shape [cap, 2]: low, high as uint64 bit patterns).  ranges_cap
    defaults to ranges' rows."""
    import torch
    n = payload.nblocks
    if first.numel() < n + 1:
        raise ValueError("first needs nblocks + 1 entries")
    cap = int(ranges.shape[0]) if ranges_cap is None else int(ranges_cap)
    if cap > (int(ranges.shape[0]) if ranges is not None else 0):
        raise ValueError("ranges_cap exceeds the ranges tensor")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_gc_scan_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth),
                                n, column, p(live), p(nranges), int(first.data_ptr()), p(ranges), cap, p(err),
                                lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_gc_scan_dev launch failed")


class ScanResult(NamedTuple):
    rc: int                 # 0 or E_NOSPACE
    ranges: np.ndarray      # uint64 [min(total, cap), 2]: low, high
    first: np.ndarray       # uint64 [n + 1]
    live: np.ndarray        # uint32 [n]
    err: np.ndarray         # int32 [n]
    len_ok: np.ndarray      # int32 [n]
    entries_ok: np.ndarray  # int32 [n]


def scan_batch(records: Sequence, column: int, ranges_cap: "int | None" = None) -> ScanResult:
    """pom_gc_scan_batch over ITB records (bytes-like, [itbh][payload], as
    stored).  ranges_cap None: sized for every ITE the records' lengths allow,
    so the call cannot run out of room; otherwise E_NOSPACE is returned in rc
    with first[n] the room needed.  Raises RuntimeError when the GPU path is
    unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    if ranges_cap is None:
        ranges_cap = 1024 * n
    ranges = np.zeros((max(ranges_cap, 1), 2), dtype=np.uint64)
    first = np.zeros(n + 1, dtype=np.uint64)
    live = np.zeros(max(n, 1), dtype=np.uint32)
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    entries_ok = np.zeros(max(n, 1), dtype=np.int32)
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    rc = lib.pom_gc_scan_batch(ptrs, lens, n, column, ranges.ctypes.data, ranges_cap, first.ctypes.data,
                               live.ctypes.data, err.ctypes.data, len_ok.ctypes.data, entries_ok.ctypes.data)
    if rc not in (0, E_NOSPACE):
        raise RuntimeError(f"pom_gc_scan_batch: {rc}")
    total = int(first[n])
    return ScanResult(rc, ranges[: min(total, ranges_cap)], first, live[:n], err[:n], len_ok[:n], entries_ok[:n])


MERGE_MAX = 1 << 30


def merge_scratch_bytes(n: int) -> int:
    """pom_gc_merge_scratch: bytes of device scratch merge_dev needs for n ranges."""
    if not 0 <= n <= MERGE_MAX:
        raise ValueError("n outside 0 ... 2^30")
    return int(_lib().pom_gc_merge_scratch(n))


def merge_dev(ranges, n: int, scratch, out, stat, out_cap: "int | None" = None, stream=None) -> None:
    """Enqueue pom_gc_merge_dev on the current (or the given) stream.

    ranges: int64 [>= n, 2] on the GPU (low, high as uint64 bit patterns), e.g.
    scan_dev's; it is not modified.  scratch: uint8, at least
    merge_scratch_bytes(n), 8-byte aligned; out: int64 [cap, 2]; stat: int64
    [5] = valid, max, nout, nin, nwrapped.  out_cap defaults to out's rows."""
    import torch
    cap = int(out.shape[0]) if out_cap is None else int(out_cap)
    if cap > (int(out.shape[0]) if out is not None else 0):
        raise ValueError("out_cap exceeds the out tensor")
    if n and int(ranges.shape[0]) < n:
        raise ValueError("fewer than n ranges")
    if stat.numel() * stat.element_size() < 40:
        raise ValueError("stat needs 40 bytes")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_gc_merge_dev(p(ranges), n, p(scratch), scratch.numel() * scratch.element_size(), p(out), cap,
                                 int(stat.data_ptr()), lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_gc_merge_dev refused or failed to launch")


class Stat(NamedTuple):
    valid: int
    max: int
    nout: int
    nin: int
    nwrapped: int


class StatResult(NamedTuple):
    rc: int                 # 0 or E_NOSPACE
    merged: np.ndarray      # uint64 [min(nout, cap), 2]: low, high
    stat: Stat
    live: np.ndarray        # uint32 [n]
    err: np.ndarray         # int32 [n]
    len_ok: np.ndarray      # int32 [n]
    entries_ok: np.ndarray  # int32 [n]


def stat_batch(records: Sequence, column: int, seed=None, merged_cap: "int | None" = None) -> StatResult:
    """pom_gc_stat_batch over ITB records (as scan_batch's).  seed: earlier
    rounds' extents, uint64 [k, 2], ascending and disjoint.  merged_cap None:
    room for every ITE the records can hold and the seed, so the call cannot
    run out of room; otherwise E_NOSPACE is returned in rc with stat.nout the
    room needed.  Raises ValueError for what the library answers with -EINVAL,
    RuntimeError when the GPU path is unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    seed = np.zeros((0, 2), dtype=np.uint64) if seed is None else np.ascontiguousarray(seed, dtype=np.uint64).reshape(-1, 2)
    if merged_cap is None:
        merged_cap = 1024 * n + len(seed)
    merged = np.zeros((max(merged_cap, 1), 2), dtype=np.uint64)
    stat = np.zeros(5, dtype=np.uint64)
    live = np.zeros(max(n, 1), dtype=np.uint32)
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    entries_ok = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib.pom_gc_stat_batch(ptrs, lens, n, column, seed.ctypes.data if len(seed) else None, len(seed),
                               merged.ctypes.data, merged_cap, stat.ctypes.data, live.ctypes.data, err.ctypes.data,
                               len_ok.ctypes.data, entries_ok.ctypes.data)
    if rc == EINVAL:
        raise ValueError("pom_gc_stat_batch: -EINVAL (column outside 0 ... 5, or a seed not ascending and disjoint)")
    if rc not in (0, E_NOSPACE):
        raise RuntimeError(f"pom_gc_stat_batch: {rc}")
    st = Stat(*[int(x) for x in stat])
    return StatResult(rc, merged[: min(st.nout, merged_cap)], st, live[:n], err[:n], len_ok[:n], entries_ok[:n])
