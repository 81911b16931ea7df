"""The MDS key/value table listing on the GPU (include/pom_kvlist.h).

Python mirror of what itb_readdir's INDEX_KV branch does per ITB
(mds/itb.c:2472-2534 with __readdir_filter, :2422-2458):
  scan_dev   <- the bitmap walk, the filter and the key records over decoded
                payloads in HBM
  scan_batch <- the decode and the walk over records in host memory; only
                counts, the masks asked for and records come back from the GPU
  parse      <- the packed records as [key bytes]
"""
from __future__ import annotations

import ctypes
import struct
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import itb, lzo

E_TRUNCATED = -4097
E_NOSPACE = -4098
E_NAME = -4099
E_KEY = -4101
EINVAL = -22

OP_SCAN, OP_SCAN_CNT, OP_GREP, OP_GREP_CNT = 0, 1, 2, 3
KV_NORMAL, KV_STR = 0x8000, 0x4000
KV_FLAGS_OFF, KV_LEN_OFF, KV_KEY_OFF, KV_KLEN_OFF, KV_VALUE_OFF, KV_VALUE_MAX = 24, 28, 32, 40, 44, 320
NEEDLE_MAX = 255
MASK_WORDS = 16
REC_MAX = 4 + KV_VALUE_MAX

_vp = ctypes.c_void_p
_u32 = ctypes.c_uint32
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_kvlist_dev.restype = ctypes.c_int
        lib.pom_kvlist_dev.argtypes = [_vp] * 5 + [_u32, _u32, _vp, _u32] + [_vp] * 7 + [ctypes.c_uint64, _vp, _vp]
        lib.pom_kvlist_batch.restype = ctypes.c_int
        lib.pom_kvlist_batch.argtypes = [_vp, _vp, ctypes.c_size_t, _u32, _vp, _u32, _vp, ctypes.c_size_t] + [_vp] * 8
        _bound = True
    return lib


def scan_dev(payload: lzo.DeviceBatch, adepth, op: int, needle, live, dnum, nbytes, keybytes, mask, first, out, err,
             status=None, out_cap: "int | None" = None, needle_len: "int | None" = None, stream=None) -> None:
    """Enqueue pom_kvlist_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64, length int32 = the
    produced lengths); adepth: uint8 per ITB; needle: uint8 on the GPU at any
    alignment, or None (needle_len defaults to its size); status: int32 per
    ITB or None.  Outputs, all on the GPU: live, dnum, nbytes, keybytes (int32,
    read as uint32), err (int32), mask (int64, 16 per ITB, or None), first
    (int64, nblocks + 1), out (uint8, any alignment; None with out_cap 0).
    out_cap defaults to out's size."""
    import torch
    n = payload.nblocks
    if first.numel() < n + 1:
        raise ValueError("first needs nblocks + 1 entries")
    if mask is not None and mask.numel() < MASK_WORDS * n:
        raise ValueError("mask needs 16 words per ITB")
    room = int(out.numel()) if out is not None else 0
    cap = room if out_cap is None else int(out_cap)
    if cap > room:
        raise ValueError("out_cap exceeds the out tensor")
    nlen = (int(needle.numel()) if needle is not None else 0) if needle_len is None else int(needle_len)
    if nlen and (needle is None or nlen > needle.numel()):
        raise ValueError("needle_len exceeds the needle tensor")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_kvlist_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth), n, int(op),
                               p(needle), nlen, p(live), p(dnum), p(nbytes), p(keybytes), p(mask),
                               int(first.data_ptr()), p(out), cap, p(err), lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_kvlist_dev: bad op or needle length, or the launch failed")


class ScanResult(NamedTuple):
    rc: int                 # 0 or E_NOSPACE
    out: np.ndarray         # uint8 [min(total, cap)]: the records, packed (empty when count-only)
    first: np.ndarray       # uint64 [n + 1]: byte offsets
    live: np.ndarray        # uint32 [n]
    dnum: np.ndarray        # uint32 [n]
    keybytes: np.ndarray    # uint32 [n]
    mask: Optional[np.ndarray]  # uint64 [n, 16], or None when not asked for
    err: np.ndarray         # int32 [n]
    len_ok: np.ndarray      # int32 [n]
    entries_ok: np.ndarray  # int32 [n]


def _room(rec: np.ndarray) -> int:
    """The record bytes one stored ITB can yield: 324 for every whole ITE of
    its decoded payload, 1,024 ITEs at the most."""
    if rec.size < itb.ITBH_SIZE:
        return 0
    ln, zlen, algo = itb.header_fields(rec)
    payload = (zlen if algo == itb.COMPR_LZO else ln) - itb.ITBH_SIZE
    return REC_MAX * min(1024, max(0, (payload - 11904) // 512))


def scan_batch(records: Sequence, op: int = OP_SCAN, needle: bytes = b"", out_cap: "int | None" = None,
               count_only: bool = False, want_mask: bool = True) -> ScanResult:
    """pom_kvlist_batch over ITB records (bytes-like, [itbh][payload], as
    stored).  out_cap None: sized for the longest listing the records can
    hold, so the call cannot run out of room; otherwise E_NOSPACE is returned
    in rc with first[n] the room needed.  count_only: out == NULL, no record
    comes back.  Raises ValueError on -EINVAL (op, needle length) and
    RuntimeError when the GPU path is unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    if count_only:
        out_cap = 0
    elif out_cap is None:
        out_cap = sum(_room(b) for b in bufs)
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    first = np.zeros(n + 1, dtype=np.uint64)
    live = np.zeros(max(n, 1), dtype=np.uint32)
    dnum = np.zeros(max(n, 1), dtype=np.uint32)
    keybytes = np.zeros(max(n, 1), dtype=np.uint32)
    mask = np.zeros((max(n, 1), MASK_WORDS), dtype=np.uint64) if want_mask else None
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    entries_ok = np.zeros(max(n, 1), dtype=np.int32)
    nd = np.frombuffer(bytes(needle), dtype=np.uint8)
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    rc = lib.pom_kvlist_batch(ptrs, lens, n, int(op), nd.ctypes.data if nd.size else None, nd.size,
                              None if count_only else out.ctypes.data, out_cap, first.ctypes.data, live.ctypes.data,
                              dnum.ctypes.data, keybytes.ctypes.data, mask.ctypes.data if want_mask else None,
                              err.ctypes.data, len_ok.ctypes.data, entries_ok.ctypes.data)
    if rc == EINVAL:
        raise ValueError("pom_kvlist_batch: op above 3 or a needle longer than 255 bytes")
    if rc not in (0, E_NOSPACE):
        raise RuntimeError(f"pom_kvlist_batch: {rc}")
    total = int(first[n])
    return ScanResult(rc, out[: min(total, out_cap)], first, live[:n], dnum[:n], keybytes[:n],
                      mask[:n] if want_mask else None, err[:n], len_ok[:n], entries_ok[:n])


def parse(data) -> List[bytes]:
    """[key] of packed records; raises ValueError on a record that is cut
    short.  (The reference client's loop, api/api.c:3413-3415, stops at a
    zero-length key; this one goes on.)"""
    data = bytes(data)
    res, at = [], 0
    while at < len(data):
        if at + 4 > len(data):
            raise ValueError(f"length word cut at byte {at}")
        (klen,) = struct.unpack_from("<I", data, at)
        at += 4
        if at + klen > len(data):
            raise ValueError(f"key cut at byte {at}")
        res.append(data[at: at + klen])
        at += klen
    return res
