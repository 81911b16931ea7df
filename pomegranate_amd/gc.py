"""The MDSL garbage collector's data scan on the GPU (include/pom_gc.h).

Python mirror of what mdsl_gc_data_round does per ITB (mdsl/gc.c:945-993):
  scan_dev   <- the bitmap walk with __add_to_brtree (mdsl/gc.c:968-993,
                :788-802) over decoded payloads in HBM
  scan_batch <- the decode switch and the walk over records in host memory;
                only counts and ranges come back from the GPU
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
