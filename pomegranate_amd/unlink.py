"""The ITB unlink on the GPU (include/pom_unlink.h).

The INDEX_UNLINK branch of itb_search (mds/itb.c:1769-1797, :1889-1911) with
ite_unlink (:676-735) and itb_del_ite (:602-671) over decoded ITBs in HBM: each
request finds its entry as the lookup does, gets the entry's MDU as it was, and
unlinks it; the requests of one ITB apply in the caller's order:
  unlink_dev     <- the check, then the requests, over decoded payloads in HBM
  unlink_batch   <- the same over stored records: decoded, unlinked and encoded
                    on the GPU; only results and stored records come back
  unlink_header  <- the ITB's struct itbh from the old one and a result
  Result         <- a view over one result's 32 bytes
Requests are lookup.REQ_DTYPE records (lookup.requests builds them).
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import lzo
from .check import EINVAL, E_TRUNCATED, HDR_DTYPE, header_facts  # noqa: F401
from .itbsplit import SPLIT_E_DAMAGED, SPLIT_NO_STREAM  # noqa: F401
from .lookup import (ENOENT, ESPLIT, LK_BY_NAME, LK_BY_UUID, LK_ITE_ACTIVE, LK_ITE_SHADOW, REC_SIZE,  # noqa: F401
                     REQ_DTYPE, requests)

UL_UNLINK = 0x00200000
ITE_FLAG_NORMAL, ITE_FLAG_LS, ITE_FLAG_SDT, ITE_FLAG_SYM, ITE_FLAG_KV = \
    0x80000000, 0x40000000, 0x10000000, 0x02000000, 0x01000000
ITE_NLINK_OFF = 38
UL_MODE_DIR = 0o040000
UL_NONE, UL_SHADOWED, UL_MARKED, UL_DELETED = 0, 1, 2, 3
UL_WHAT_MASK, UL_DELTA = 0xFF, 0x100

# struct pom_unlink_result
RESULT_DTYPE = np.dtype([("err", "<i4"), ("changed", "<u4"), ("removed", "<u4"), ("len", "<u4"), ("entries", "<i4"),
                         ("max_offset", "<i4"), ("pseudo_conflicts", "<i4"), ("itu", "<u2"), ("hits", "<u2")])
assert RESULT_DTYPE.itemsize == 32

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        u32 = ctypes.c_uint32
        lib.pom_itb_unlink_dev.restype = ctypes.c_int
        lib.pom_itb_unlink_dev.argtypes = [_vp] * 6 + [u32, ctypes.c_int, _vp, _vp, u32, _vp, u32] + [_vp] * 8
        lib.pom_itb_unlink_scratch.restype = ctypes.c_size_t
        lib.pom_itb_unlink_scratch.argtypes = [u32]
        lib.pom_itb_unlink_header.restype = ctypes.c_int
        lib.pom_itb_unlink_header.argtypes = [_vp, _vp, u32, _vp]
        lib.pom_itb_unlink_batch.restype = ctypes.c_int
        lib.pom_itb_unlink_batch.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, _vp,
                                             ctypes.c_size_t, _vp, ctypes.c_size_t] + [_vp] * 11
        _bound = True
    return lib


class Result(NamedTuple):
    """One struct pom_unlink_result."""
    err: int
    changed: int
    removed: int
    len: int
    entries: int
    max_offset: int
    pseudo_conflicts: int
    itu: int
    hits: int

    @classmethod
    def parse(cls, raw) -> "Result":
        raw = bytes(raw)
        if len(raw) != RESULT_DTYPE.itemsize:
            raise ValueError(f"a result has {RESULT_DTYPE.itemsize} bytes, not {len(raw)}")
        r = np.frombuffer(raw, dtype=RESULT_DTYPE)[0]
        return cls(*(int(r[name]) for name in RESULT_DTYPE.names))


def unlink_scratch_bytes(nitb: int) -> int:
    return int(_lib().pom_itb_unlink_scratch(nitb))


def unlink_dev(payload: lzo.DeviceBatch, adepth, hdr, async_unlink: bool, req, req_first, nreq: int, names,
               names_len: int, err, nr, depth, what, out, result, scratch, status=None, stream=None) -> None:
    """Enqueue pom_itb_unlink_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, 16-byte aligned, off int64 in
    multiples of 16, length int32), modified in place; adepth: uint8 per ITB;
    hdr: the pom_check_hdr records as a uint8 tensor, 8-byte aligned; req: the
    pom_lookup_req records as a uint8 tensor, 8-byte aligned, grouped by ITB:
    ITB b's are req_first[b] ... req_first[b + 1] (int32 tensor, nitb + 1
    entries), in application order; names: uint8 tensor holding the blob (None
    with names_len 0).  Outputs, all on the GPU: err, nr, depth, what (int32,
    nreq entries each), out (uint8, 136 * nreq bytes, 8-byte aligned), result
    (uint8, 32 bytes per ITB); scratch: uint8, unlink_scratch_bytes(n)."""
    import torch
    n = payload.nblocks
    nbytes = lambda t: t.numel() * t.element_size()
    if nbytes(result) < 32 * n or nbytes(hdr) < 32 * n or adepth.numel() < n or nbytes(req_first) < 4 * (n + 1):
        raise ValueError("an array is smaller than nitb entries")
    if nbytes(out) < REC_SIZE * nreq or min(nbytes(err), nbytes(nr), nbytes(depth), nbytes(what)) < 4 * nreq:
        raise ValueError("an output is smaller than nreq results")
    if nbytes(req) < REQ_DTYPE.itemsize * nreq or (names_len and names.numel() < names_len):
        raise ValueError("req or names is smaller than stated")
    if nbytes(scratch) < unlink_scratch_bytes(n):
        raise ValueError("scratch is smaller than unlink_scratch_bytes(nitb)")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_itb_unlink_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth), p(hdr), n,
                                   int(bool(async_unlink)), p(req), p(req_first), nreq, p(names), names_len, p(err),
                                   p(nr), p(depth), p(what), p(out), p(result), p(scratch),
                                   lzo._stream_handle(torch, stream))
    if rc == EINVAL:
        raise ValueError("pom_itb_unlink_dev: -EINVAL (hdr NULL, or an arena, req, out or scratch that is misaligned)")
    if rc != 0:
        raise RuntimeError("pom_itb_unlink_dev launch failed")


def unlink_header(old_hdr, result, z: int = SPLIT_NO_STREAM) -> tuple:
    """pom_itb_unlink_header: (the ITB's struct itbh after the unlinks, whether
    the record is stored compressed), from its header before them, one result
    (bytes-like, 32 bytes) and the size of the payload's LZO1X-1 stream
    (SPLIT_NO_STREAM: none).  Raises ValueError for what the library answers
    with -EINVAL: a result with err != 0 or with nothing changed."""
    old = np.frombuffer(bytes(old_hdr[:264]), dtype=np.uint8).copy()
    res = np.frombuffer(bytes(result), dtype=np.uint8).copy()
    if old.size != 264 or res.size != 32:
        raise ValueError("a header has 264 bytes, a result 32")
    out = np.zeros(264, dtype=np.uint8)
    rc = _lib().pom_itb_unlink_header(old.ctypes.data, res.ctypes.data, z, out.ctypes.data)
    if rc < 0:
        raise ValueError(f"pom_itb_unlink_header: {rc}")
    return out.tobytes(), rc


class UnlinkBatch(NamedTuple):
    err: np.ndarray                     # int32 [nreq]
    nr: np.ndarray                      # uint32 [nreq]
    depth: np.ndarray                   # uint32 [nreq]
    what: np.ndarray                    # uint32 [nreq]
    rec: np.ndarray                     # uint8 [nreq, 136]
    itb_err: np.ndarray                 # int32 [n]
    result: np.ndarray                  # RESULT_DTYPE [n]
    len_ok: np.ndarray                  # int32 [n]
    out: list                           # bytes per ITB: the stored record after the unlinks, b"" when none is produced


def unlink_batch(records: Sequence, req: np.ndarray, names: bytes = b"", async_unlink: bool = False,
                 itbid_check: bool = False, out_cap: Optional[Sequence[int]] = None) -> UnlinkBatch:
    """pom_itb_unlink_batch over ITB records (bytes-like, [itbh][payload], as
    stored) and a REQ_DTYPE array with its name blob, in the caller's order.
    out_cap: the capacity of each record's output buffer, or None: the input's
    uncompressed record length, which always suffices.  Raises RuntimeError
    when the GPU path is unusable."""
    lib = _lib()
    n, nreq = len(records), len(req)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    if out_cap is None:
        out_cap = [min(max(int.from_bytes(bytes(r[240:244]), "little"), int.from_bytes(bytes(r[244:248]), "little"),
                           264), 1 << 20) if len(r) >= 264 else 264 for r in records]
    outs = [np.zeros(max(int(c), 1), dtype=np.uint8) for c in out_cap]
    arr = lambda items: (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in items])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    caps = (ctypes.c_size_t * max(n, 1))(*[int(c) for c in out_cap])
    out_len = (ctypes.c_size_t * max(n, 1))()
    req = np.ascontiguousarray(req, dtype=REQ_DTYPE)
    blob = np.frombuffer(bytes(names) or b"\0", dtype=np.uint8)
    rec = np.zeros((max(nreq, 1), REC_SIZE), dtype=np.uint8)
    err = np.zeros(max(nreq, 1), dtype=np.int32)
    nr, depth, what = (np.zeros(max(nreq, 1), dtype=np.uint32) for _ in range(3))
    result = np.zeros(max(n, 1), dtype=RESULT_DTYPE)
    itb_err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib.pom_itb_unlink_batch(arr(bufs), lens, n, int(bool(itbid_check)), int(bool(async_unlink)),
                                  req.ctypes.data if nreq else None, nreq, blob.ctypes.data, len(names),
                                  rec.ctypes.data, err.ctypes.data, nr.ctypes.data, depth.ctypes.data, what.ctypes.data,
                                  arr(outs), caps, out_len, result.ctypes.data, itb_err.ctypes.data, len_ok.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"pom_itb_unlink_batch: {rc}")
    return UnlinkBatch(err[:nreq], nr[:nreq], depth[:nreq], what[:nreq], rec[:nreq], itb_err[:n], result[:n],
                       len_ok[:n], [outs[b][: out_len[b]].tobytes() for b in range(n)])
