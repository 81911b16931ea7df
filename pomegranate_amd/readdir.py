"""The MDS directory listing on the GPU (include/pom_readdir.h).

Python mirror of what itb_readdir's FS branch does per ITB (mds/itb.c:2536-2589):
  scan_dev   <- the bitmap walk and the dentry_info records (mds/itb.c:2567-2585)
                over decoded payloads in HBM
  scan_batch <- the decode and the walk over records in host memory; only
                counts and records come back from the GPU
  parse      <- the packed records as [(uuid, mode, name)]
"""
from __future__ import annotations

import ctypes
import struct
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from . import itb, lzo

E_TRUNCATED = -4097
E_NOSPACE = -4098
E_NAME = -4099
EINVAL = -22

ITE_UUID_OFF, ITE_FLAG_OFF, ITE_NAMELEN_OFF, ITE_MODE_OFF, ITE_NAME_OFF, ITE_NAME_MAX = 8, 16, 20, 36, 104, 256
ITE_STATE_MASK, ITE_FLAG_KV = 7, 0x01000000
DENT_HDR, DENT_MODE_OFF, DENT_NAMELEN_OFF = 16, 8, 10
REC_MAX = DENT_HDR + ITE_NAME_MAX

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_readdir_dev.restype = ctypes.c_int
        lib.pom_readdir_dev.argtypes = [_vp] * 5 + [ctypes.c_uint32] + [_vp] * 5 + [ctypes.c_uint64, _vp, _vp]
        lib.pom_readdir_batch.restype = ctypes.c_int
        lib.pom_readdir_batch.argtypes = [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t] + [_vp] * 6
        _bound = True
    return lib


def scan_dev(payload: lzo.DeviceBatch, adepth, live, dnum, nbytes, first, out, err,
             status=None, out_cap: "int | None" = None, stream=None) -> None:
    """Enqueue pom_readdir_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64, length int32 = the
    produced lengths, e.g. decompress_dev's out_len); adepth: uint8 per ITB;
    status: int32 per ITB or None.  Outputs, all on the GPU: live, dnum, nbytes
    (int32, read as uint32), err (int32), first (int64, nblocks + 1), out
    (uint8, any alignment; None with out_cap 0).  out_cap defaults to out's
    size."""
    import torch
    n = payload.nblocks
    if first.numel() < n + 1:
        raise ValueError("first needs nblocks + 1 entries")
    room = int(out.numel()) if out is not None else 0
    cap = room if out_cap is None else int(out_cap)
    if cap > room:
        raise ValueError("out_cap exceeds the out tensor")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_readdir_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth), n,
                                p(live), p(dnum), p(nbytes), int(first.data_ptr()), p(out), cap, p(err),
                                lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_readdir_dev launch failed")


class ScanResult(NamedTuple):
    rc: int                 # 0 or E_NOSPACE
    out: np.ndarray         # uint8 [min(total, cap)]: the records, packed
    first: np.ndarray       # uint64 [n + 1]: byte offsets
    live: np.ndarray        # uint32 [n]
    dnum: np.ndarray        # uint32 [n]
    err: np.ndarray         # int32 [n]
    len_ok: np.ndarray      # int32 [n]
    entries_ok: np.ndarray  # int32 [n]


def _room(rec: np.ndarray) -> int:
    """The record bytes one stored ITB can yield: 272 for every whole ITE of
    its decoded payload, 1,024 ITEs at the most."""
    if rec.size < itb.ITBH_SIZE:
        return 0
    ln, zlen, algo = itb.header_fields(rec)
    payload = (zlen if algo == itb.COMPR_LZO else ln) - itb.ITBH_SIZE
    return REC_MAX * min(1024, max(0, (payload - 11904) // 512))


def scan_batch(records: Sequence, out_cap: "int | None" = None) -> ScanResult:
    """pom_readdir_batch over ITB records (bytes-like, [itbh][payload], as
    stored).  out_cap None: sized for the longest listing the records can hold
    (272 bytes for every ITE), so the call cannot run out of room;
    otherwise E_NOSPACE is returned in rc with first[n] the room needed.
    Raises RuntimeError when the GPU path is unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    if out_cap is None:
        out_cap = sum(_room(b) for b in bufs)
    out = np.zeros(max(out_cap, 1), dtype=np.uint8)
    first = np.zeros(n + 1, dtype=np.uint64)
    live = np.zeros(max(n, 1), dtype=np.uint32)
    dnum = np.zeros(max(n, 1), dtype=np.uint32)
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    entries_ok = np.zeros(max(n, 1), dtype=np.int32)
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    rc = lib.pom_readdir_batch(ptrs, lens, n, out.ctypes.data, out_cap, first.ctypes.data, live.ctypes.data,
                               dnum.ctypes.data, err.ctypes.data, len_ok.ctypes.data, entries_ok.ctypes.data)
    if rc not in (0, E_NOSPACE):
        raise RuntimeError(f"pom_readdir_batch: {rc}")
    total = int(first[n])
    return ScanResult(rc, out[: min(total, out_cap)], first, live[:n], dnum[:n], err[:n], len_ok[:n],
                      entries_ok[:n])


def parse(data) -> List[Tuple[int, int, bytes]]:
    """[(uuid, mode, name)] of packed records; raises ValueError on a record
    that is cut short."""
    data = bytes(data)
    res, at = [], 0
    while at < len(data):
        if at + DENT_HDR > len(data):
            raise ValueError(f"record header cut at byte {at}")
        uuid, mode, namelen, _ = struct.unpack_from("<QHHI", data, at)
        at += DENT_HDR
        if at + namelen > len(data):
            raise ValueError(f"name cut at byte {at}")
        res.append((uuid, mode, data[at: at + namelen]))
        at += namelen
    return res
