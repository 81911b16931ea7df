"""The MDS lookup on the GPU (include/pom_lookup.h).

Python mirror of the read-only INDEX_LOOKUP branch of itb_search
(mds/itb.c:1738-2053) for entries matched by name or by uuid:
  requests     <- hvfs_index fields as pom_lookup_req records and their name blob
  lookup_dev   <- the chain walk, ite_match and the MDU copy (mds/itb.c:1769-1814)
                  over decoded payloads in HBM
  lookup_batch <- the decode and the walk over records in host memory; only
                  codes and 136-byte records come back from the GPU
  parse        <- one record as (uuid, mdu bytes, (stored_itbid, len, offset))
"""
from __future__ import annotations

import ctypes
import struct
from typing import NamedTuple, Sequence, Tuple

import numpy as np

from . import lzo

E_TRUNCATED = -4097
E_LOOP = -4100
EINVAL = -22
ENOENT = -2
ESPLIT = -1028

ITB_INDEX_ENTRIES, ITB_INDEX_SIZE, IDX_ENTRY_BITS, IDX_FLAG_SHIFT = 2048, 4, 15, 30
IDX_FREE, IDX_UNIQUE, IDX_CONFLICT, IDX_OVERFLOW = 0, 1, 2, 3
ITE_HASH_OFF, ITE_MD_OFF, MDU_SIZE, MDU_DTIME_OFF = 0, 24, 104, 56
ITE_UNLINKED, ITE_SHADOW = 1, 3
ITBH_FLAG_OFF, ITBH_DEPTH_OFF, ITBH_ITBID_OFF, ITB_JUST_SPLIT = 0, 2, 136, 2
LK_BY_NAME, LK_BY_UUID, LK_LOOKUP, LK_COLUMN = 0x1, 0x2, 0x10, 0x40
LK_ITE_ACTIVE, LK_ITE_SHADOW = 0x01000000, 0x02000000
REC_SIZE = 136

# struct pom_lookup_req
REQ_DTYPE = np.dtype([("hash", "<u8"), ("uuid", "<u8"), ("itb", "<u4"), ("flag", "<u4"), ("name_off", "<u4"),
                      ("namelen", "<u2"), ("column", "<u2")])
assert REQ_DTYPE.itemsize == 32

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_lookup_dev.restype = ctypes.c_int
        lib.pom_lookup_dev.argtypes = [_vp] * 5 + [ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32] + \
            [_vp] * 5
        lib.pom_lookup_batch.restype = ctypes.c_int
        lib.pom_lookup_batch.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t, _vp,
                                         ctypes.c_size_t] + [_vp] * 4
        _bound = True
    return lib


def requests(items: Sequence[dict]) -> Tuple[np.ndarray, bytes]:
    """[{itb, hash, flag, uuid=0, name=b"", column=0}] -> (REQ_DTYPE array, name
    blob), the names packed one behind the other."""
    req = np.zeros(len(items), dtype=REQ_DTYPE)
    blob = bytearray()
    for r, it in enumerate(items):
        name = bytes(it.get("name", b""))
        req[r] = (it["hash"], it.get("uuid", 0), it["itb"], it["flag"], len(blob), len(name), it.get("column", 0))
        blob += name
    return req, bytes(blob)


def lookup_dev(payload: lzo.DeviceBatch, adepth, req, nreq: int, names, names_len: int, err, nr, depth, out,
               status=None, stream=None) -> None:
    """Enqueue pom_lookup_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64, length int32 = the
    produced lengths); adepth: uint8 per ITB; status: int32 per ITB or None;
    req: the pom_lookup_req records as a uint8 tensor, 8-byte aligned; names:
    uint8 tensor holding the blob at any alignment (None with names_len 0).
    Outputs, all on the GPU: err (int32), nr and depth (int32, read as uint32),
    nreq entries each, and out (uint8, 136 * nreq bytes, any alignment)."""
    import torch
    if out.numel() < REC_SIZE * nreq or min(err.numel(), nr.numel(), depth.numel()) < nreq:
        raise ValueError("an output is smaller than nreq results")
    if req.numel() < REQ_DTYPE.itemsize * nreq or (names_len and names.numel() < names_len):
        raise ValueError("req or names is smaller than stated")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_lookup_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth),
                               payload.nblocks, p(req), nreq, p(names), names_len, p(err), p(nr), p(depth), p(out),
                               lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_lookup_dev launch failed")


class LookupResult(NamedTuple):
    err: np.ndarray         # int32 [nreq]
    nr: np.ndarray          # uint32 [nreq]
    depth: np.ndarray       # uint32 [nreq]
    out: np.ndarray         # uint8 [nreq, 136]


def lookup_batch(records: Sequence, req: np.ndarray, names: bytes = b"", itbid_check: bool = False) -> LookupResult:
    """pom_lookup_batch over ITB records (bytes-like, [itbh][payload], as
    stored) and a REQ_DTYPE array with its name blob.  Raises RuntimeError when
    the GPU path is unusable."""
    lib = _lib()
    n, nreq = len(records), len(req)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    req = np.ascontiguousarray(req, dtype=REQ_DTYPE)
    blob = np.frombuffer(bytes(names) or b"\0", dtype=np.uint8)
    out = np.zeros((max(nreq, 1), REC_SIZE), dtype=np.uint8)
    err = np.zeros(max(nreq, 1), dtype=np.int32)
    nr = np.zeros(max(nreq, 1), dtype=np.uint32)
    depth = np.zeros(max(nreq, 1), dtype=np.uint32)
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    rc = lib.pom_lookup_batch(ptrs, lens, n, int(bool(itbid_check)), req.ctypes.data if nreq else None, nreq,
                              blob.ctypes.data, len(names), out.ctypes.data, err.ctypes.data, nr.ctypes.data,
                              depth.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"pom_lookup_batch: {rc}")
    return LookupResult(err[:nreq], nr[:nreq], depth[:nreq], out[:nreq])


def parse(record) -> Tuple[int, bytes, Tuple[int, int, int]]:
    """(uuid, the MDU_SIZE bytes from &ite.g, (stored_itbid, len, offset)) of
    one 136-byte record; the lease word is the u64 at mdu[MDU_DTIME_OFF:]."""
    record = bytes(record)
    if len(record) != REC_SIZE:
        raise ValueError(f"a record has {REC_SIZE} bytes, not {len(record)}")
    (uuid,) = struct.unpack_from("<Q", record, 0)
    return uuid, record[8: 8 + MDU_SIZE], struct.unpack_from("<QQQ", record, 8 + MDU_SIZE)
