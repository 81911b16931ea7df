"""The ITB sweep on the GPU (include/pom_sweep.h).

The loop of async_unlink_ite (mds/itb.c:2690-2800) over decoded ITBs in HBM:
the ITEs an asynchronous unlink left in state ITE_UNLINKED are cut out of their
chains and deleted, byte for byte as the reference's sequence leaves the table:
  sweep_dev     <- the check, then the sweep, over decoded payloads in HBM
  sweep_batch   <- the same over stored records: decoded, swept and encoded on
                   the GPU; only results and stored records come back
  sweep_header  <- the ITB's struct itbh from the old one and a result
  Result        <- a view over one result's 32 bytes
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import lzo
from .check import EINVAL, E_TRUNCATED, HDR_DTYPE, header_facts  # noqa: F401
from .itbsplit import SPLIT_E_DAMAGED, SPLIT_NO_STREAM  # noqa: F401

ITE_STATE_MASK = 7
ITE_UNLINKED = 1
SWEEP_NO_BUDGET = 0xFFFFFFFF

# struct pom_sweep_result
RESULT_DTYPE = np.dtype([("err", "<i4"), ("removed", "<u4"), ("dc", "<u4"), ("len", "<u4"), ("entries", "<i4"),
                         ("max_offset", "<i4"), ("pseudo_conflicts", "<i4"), ("itu", "<u2"), ("visited", "<u2")])
assert RESULT_DTYPE.itemsize == 32

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_itb_sweep_dev.restype = ctypes.c_int
        lib.pom_itb_sweep_dev.argtypes = [_vp] * 7 + [ctypes.c_uint32] + [_vp] * 3
        lib.pom_itb_sweep_scratch.restype = ctypes.c_size_t
        lib.pom_itb_sweep_scratch.argtypes = [ctypes.c_uint32]
        lib.pom_itb_sweep_header.restype = ctypes.c_int
        lib.pom_itb_sweep_header.argtypes = [_vp, _vp, ctypes.c_uint32, _vp]
        lib.pom_itb_sweep_batch.restype = ctypes.c_int
        lib.pom_itb_sweep_batch.argtypes = [_vp, _vp, ctypes.c_size_t] + [_vp] * 7
        _bound = True
    return lib


class Result(NamedTuple):
    """One struct pom_sweep_result."""
    err: int
    removed: int
    dc: int
    len: int
    entries: int
    max_offset: int
    pseudo_conflicts: int
    itu: int
    visited: int

    @classmethod
    def parse(cls, raw) -> "Result":
        raw = bytes(raw)
        if len(raw) != RESULT_DTYPE.itemsize:
            raise ValueError(f"a result has {RESULT_DTYPE.itemsize} bytes, not {len(raw)}")
        r = np.frombuffer(raw, dtype=RESULT_DTYPE)[0]
        return cls(*(int(r[name]) for name in RESULT_DTYPE.names))


def sweep_scratch_bytes(nitb: int) -> int:
    return int(_lib().pom_itb_sweep_scratch(nitb))


def sweep_dev(payload: lzo.DeviceBatch, adepth, hdr, result, scratch, budget=None, status=None, stream=None) -> None:
    """Enqueue pom_itb_sweep_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64 in multiples of 16,
    length int32), modified in place: of each only the bitmap and the index
    table may change; adepth: uint8 per ITB; hdr: the pom_check_hdr records as
    a uint8 tensor, 8-byte aligned; budget: uint32 per ITB (an int32 tensor's
    bits) or None (SWEEP_NO_BUDGET for each); status: int32 per ITB or None.
    result (uint8, 32 bytes per ITB) and scratch (uint8,
    sweep_scratch_bytes(n)) are on the GPU too.  The arena is 16-byte aligned.
    No two ITBs may share bytes."""
    import torch
    n = payload.nblocks
    nbytes = lambda t: t.numel() * t.element_size()
    if nbytes(result) < 32 * n or nbytes(hdr) < 32 * n or adepth.numel() < n:
        raise ValueError("an array is smaller than nitb entries")
    if budget is not None and nbytes(budget) < 4 * n:
        raise ValueError("budget is smaller than nitb entries")
    if nbytes(scratch) < sweep_scratch_bytes(n):
        raise ValueError("scratch is smaller than sweep_scratch_bytes(nitb)")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_itb_sweep_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth), p(hdr),
                                  p(budget), n, p(result), p(scratch), lzo._stream_handle(torch, stream))
    if rc == EINVAL:
        raise ValueError("pom_itb_sweep_dev: -EINVAL (hdr NULL, or an arena that is not 16-byte aligned)")
    if rc != 0:
        raise RuntimeError("pom_itb_sweep_dev launch failed")


def sweep_header(old_hdr, result, z: int = SPLIT_NO_STREAM) -> tuple:
    """pom_itb_sweep_header: (the ITB's struct itbh after the sweep, whether
    the record is stored compressed), from its header before it, one result
    (bytes-like, 32 bytes) and the size of the swept payload's LZO1X-1 stream
    (SPLIT_NO_STREAM: none).  Raises ValueError for what the library answers
    with -EINVAL: a result with err != 0 or with nothing removed."""
    old = np.frombuffer(bytes(old_hdr[:264]), dtype=np.uint8).copy()
    res = np.frombuffer(bytes(result), dtype=np.uint8).copy()
    if old.size != 264 or res.size != 32:
        raise ValueError("a header has 264 bytes, a result 32")
    out = np.zeros(264, dtype=np.uint8)
    rc = _lib().pom_itb_sweep_header(old.ctypes.data, res.ctypes.data, z, out.ctypes.data)
    if rc < 0:
        raise ValueError(f"pom_itb_sweep_header: {rc}")
    return out.tobytes(), rc


class SweepBatch(NamedTuple):
    err: np.ndarray                     # int32 [n]
    result: np.ndarray                  # RESULT_DTYPE [n]
    len_ok: np.ndarray                  # int32 [n]
    out: list                           # bytes per ITB: the swept stored record, b"" when none is produced


def sweep_batch(records: Sequence, budget: Optional[Sequence[int]] = None,
                out_cap: Optional[Sequence[int]] = None) -> SweepBatch:
    """pom_itb_sweep_batch over ITB records (bytes-like, [itbh][payload], as
    stored).  budget: one per record, or None (no budget); out_cap: the
    capacity of each record's output buffer, or None: the input's uncompressed
    record length, which always suffices.  Raises RuntimeError when the GPU
    path is unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    if out_cap is None:
        # (len or zlen, whichever a valid header of either kind makes the larger; a refused record needs none)
        out_cap = [min(max(int.from_bytes(bytes(r[240:244]), "little"), int.from_bytes(bytes(r[244:248]), "little"),
                           264), 1 << 20) if len(r) >= 264 else 264 for r in records]
    outs = [np.zeros(max(int(c), 1), dtype=np.uint8) for c in out_cap]
    arr = lambda items: (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in items])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    caps = (ctypes.c_size_t * max(n, 1))(*[int(c) for c in out_cap])
    out_len = (ctypes.c_size_t * max(n, 1))()
    bud = None if budget is None else np.asarray(budget, dtype=np.uint32)
    result = np.zeros(max(n, 1), dtype=RESULT_DTYPE)
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib.pom_itb_sweep_batch(arr(bufs), lens, n, None if bud is None else bud.ctypes.data, arr(outs), caps, out_len,
                                 result.ctypes.data, err.ctypes.data, len_ok.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"pom_itb_sweep_batch: {rc}")
    return SweepBatch(err[:n], result[:n], len_ok[:n], [outs[b][: out_len[b]].tobytes() for b in range(n)])
