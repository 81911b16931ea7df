"""The ITB split on the GPU (include/pom_split.h).

The loop of itb_split_local (mds/xtable.c:95-146) over decoded ITBs in HBM: the
ITEs whose hash has the split depth's bit move into a new ITB, the old one
keeps the rest, byte for byte as the reference's sequence leaves both:
  split_dev      <- the check, then the split, over decoded payloads in HBM
  split_batch    <- the same over stored records: decoded, split and both halves
                    encoded on the GPU; only results and stored records come back
  split_headers  <- both ITBs' struct itbh from the old one and a result
  Result         <- a view over one result's 48 bytes
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import lzo
from .check import EINVAL, E_TRUNCATED, HDR_DTYPE, header_facts  # noqa: F401

ITBH_STATE_OFF, ITBH_CONFLICTS_OFF, ITBH_TWIN_OFF, ITBH_SPLIT_RLINK_OFF = 1, 12, 208, 216
ITB_STATE_DIRTY = 1
SPLIT_DEPTH_MAX = 50
SPLIT_E_DAMAGED = -4103
SPLIT_NO_STREAM = 0xFFFFFFFF

# struct pom_split_result
RESULT_DTYPE = np.dtype([("err", "<i4"), ("moved", "<u4"), ("old_len", "<u4"), ("new_len", "<u4"),
                         ("old_entries", "<i4"), ("new_entries", "<i4"), ("old_max_offset", "<i4"),
                         ("new_max_offset", "<i4"), ("old_pseudo", "<i4"), ("new_pseudo", "<i4"),
                         ("old_inf", "<u2"), ("old_itu", "<u2"), ("new_inf", "<u2"), ("new_itu", "<u2")])
assert RESULT_DTYPE.itemsize == 48

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_itb_split_dev.restype = ctypes.c_int
        lib.pom_itb_split_dev.argtypes = [_vp] * 7 + [ctypes.c_uint32] + [_vp] * 6
        lib.pom_itb_split_scratch.restype = ctypes.c_size_t
        lib.pom_itb_split_scratch.argtypes = [ctypes.c_uint32]
        lib.pom_itb_split_headers.restype = ctypes.c_int
        lib.pom_itb_split_headers.argtypes = [_vp, ctypes.c_uint8, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]
        lib.pom_itb_split_batch.restype = ctypes.c_int
        lib.pom_itb_split_batch.argtypes = [_vp, _vp, ctypes.c_size_t] + [_vp] * 9
        _bound = True
    return lib


class Result(NamedTuple):
    """One struct pom_split_result."""
    err: int
    moved: int
    old_len: int
    new_len: int
    old_entries: int
    new_entries: int
    old_max_offset: int
    new_max_offset: int
    old_pseudo: int
    new_pseudo: int
    old_inf: int
    old_itu: int
    new_inf: int
    new_itu: int

    @classmethod
    def parse(cls, raw) -> "Result":
        raw = bytes(raw)
        if len(raw) != RESULT_DTYPE.itemsize:
            raise ValueError(f"a result has {RESULT_DTYPE.itemsize} bytes, not {len(raw)}")
        r = np.frombuffer(raw, dtype=RESULT_DTYPE)[0]
        return cls(*(int(r[name]) for name in RESULT_DTYPE.names))


def split_scratch_bytes(nitb: int) -> int:
    return int(_lib().pom_itb_split_scratch(nitb))


def split_dev(payload: lzo.DeviceBatch, adepth, hdr, new_payload: lzo.DeviceBatch, result, scratch,
              split_depth=None, status=None, stream=None) -> None:
    """Enqueue pom_itb_split_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64 in multiples of 16,
    length int32), modified in place: of each only the bitmap and the index
    table may change; adepth: uint8 per ITB; hdr: the pom_check_hdr records as
    a uint8 tensor, 8-byte aligned; new_payload: where the new ITBs' payloads
    go (off in multiples of 16, length = the capacities; an ITB's own
    payload length always suffices); split_depth: uint8 per ITB or None
    (hdr.depth + 1); status: int32 per ITB or None.  result (uint8, 48 bytes
    per ITB) and scratch (uint8, split_scratch_bytes(n)) are on the GPU too.
    Both arenas are 16-byte aligned.  No two ITBs may share bytes."""
    import torch
    n = payload.nblocks
    nbytes = lambda t: t.numel() * t.element_size()
    if new_payload.nblocks != n or nbytes(result) < 48 * n or nbytes(hdr) < 32 * n or adepth.numel() < n:
        raise ValueError("an array is smaller than nitb entries")
    if nbytes(scratch) < split_scratch_bytes(n):
        raise ValueError("scratch is smaller than split_scratch_bytes(nitb)")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_itb_split_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth), p(hdr),
                                  p(split_depth), n, p(new_payload.arena), p(new_payload.off), p(new_payload.length),
                                  p(result), p(scratch), lzo._stream_handle(torch, stream))
    if rc == EINVAL:
        raise ValueError("pom_itb_split_dev: -EINVAL (hdr NULL, or an arena that is not 16-byte aligned)")
    if rc != 0:
        raise RuntimeError("pom_itb_split_dev launch failed")


def split_headers(old_hdr, sd: int, result, old_z: int = SPLIT_NO_STREAM, new_z: int = SPLIT_NO_STREAM) -> tuple:
    """pom_itb_split_headers: (the old ITB's struct itbh after the split, the
    new ITB's, the bits that say which half is stored compressed), from the old
    ITB's header before it, one result (bytes-like, 48 bytes) and the sizes of
    the two payloads' LZO1X-1 streams (SPLIT_NO_STREAM: none).  Raises
    ValueError for what the library answers with -EINVAL: sd outside 1 ... 50,
    a result with err != 0 or with nothing moved."""
    old = np.frombuffer(bytes(old_hdr[:264]), dtype=np.uint8).copy()
    res = np.frombuffer(bytes(result), dtype=np.uint8).copy()
    if old.size != 264 or res.size != 48 or not 0 <= sd <= 255:
        raise ValueError("a header has 264 bytes, a result 48, a split depth 8 bits")
    o, n = np.zeros(264, dtype=np.uint8), np.zeros(264, dtype=np.uint8)
    rc = _lib().pom_itb_split_headers(old.ctypes.data, sd, res.ctypes.data, old_z, new_z, o.ctypes.data, n.ctypes.data)
    if rc < 0:
        raise ValueError(f"pom_itb_split_headers: {rc}")
    return o.tobytes(), n.tobytes(), rc


class SplitBatch(NamedTuple):
    err: np.ndarray                     # int32 [n]
    result: np.ndarray                  # RESULT_DTYPE [n]
    len_ok: np.ndarray                  # int32 [n]
    old: list                           # bytes per ITB: the old ITB's stored record, b"" when none is produced
    new: list                           # bytes per ITB: the new ITB's


def split_batch(records: Sequence, split_depth: Optional[Sequence[int]] = None,
                out_cap: Optional[Sequence[int]] = None) -> SplitBatch:
    """pom_itb_split_batch over ITB records (bytes-like, [itbh][payload], as
    stored).  split_depth: one per record, or None (h.depth + 1); out_cap: the
    capacity of each record's two output buffers, or None: the input's
    uncompressed record length, which always suffices.  Raises RuntimeError
    when the GPU path is unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    if out_cap is None:
        # (len or zlen, whichever a valid header of either kind makes the larger; a refused record needs none)
        out_cap = [min(max(int.from_bytes(bytes(r[240:244]), "little"), int.from_bytes(bytes(r[244:248]), "little"),
                           264), 1 << 20) if len(r) >= 264 else 264 for r in records]
    olds = [np.zeros(max(int(c), 1), dtype=np.uint8) for c in out_cap]
    news = [np.zeros(max(int(c), 1), dtype=np.uint8) for c in out_cap]
    arr = lambda items: (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in items])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    caps = (ctypes.c_size_t * max(n, 1))(*[int(c) for c in out_cap])
    old_len, new_len = (ctypes.c_size_t * max(n, 1))(), (ctypes.c_size_t * max(n, 1))()
    sd = None if split_depth is None else np.asarray(split_depth, dtype=np.uint8)
    result = np.zeros(max(n, 1), dtype=RESULT_DTYPE)
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib.pom_itb_split_batch(arr(bufs), lens, n, None if sd is None else sd.ctypes.data, arr(olds), arr(news), caps,
                                 old_len, new_len, result.ctypes.data, err.ctypes.data, len_ok.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"pom_itb_split_batch: {rc}")
    return SplitBatch(err[:n], result[:n], len_ok[:n], [olds[b][: old_len[b]].tobytes() for b in range(n)],
                      [news[b][: new_len[b]].tobytes() for b in range(n)])
