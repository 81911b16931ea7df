"""The MDS key/value point get on the GPU (include/pom_kvget.h).

Python mirror of the INDEX_KV branches of itb_search (hvfs_get / hvfs_sget:
ite_match mds/itb.c:1095-1116, the copy :1808-1810, the reply mds/cbht.c:929-972):
  requests    <- hvfs_index fields as pom_kvget_req records and their key blob
  kvget_dev   <- the chain walk, the KV match and the record copy over decoded
                 payloads in HBM
  kvget_batch <- the decode and the get over records in host memory; only codes,
                 lengths, lease words and the packed records come back
  parse       <- one record as (flags, len, key, klen, value, column or None)
"""
from __future__ import annotations

import ctypes
import struct
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import lzo

E_TRUNCATED = -4097
E_NOSPACE = -4098
E_LOOP = -4100
E_VALUE = -4102
EINVAL = -22
ENOENT = -2
ESPLIT = -1028

KG_LOOKUP, KG_COLUMN, KG_KV = 0x10, 0x40, 0x40000000
KG_MAX_COLUMN, KG_KVFLAG_MASK, KG_LEASE_OFF, KG_REC_MAX = 0xFFF, 0xCFFF, 80, 364
KG_E_VALUE = E_VALUE
KV_NORMAL, KV_STR, KV_HEADER_LEN, KV_VALUE_MAX = 0x8000, 0x4000, 20, 320
COLUMN_SIZE = 24

# struct pom_kvget_req
REQ_DTYPE = np.dtype([("key", "<u8"), ("itb", "<u4"), ("flag", "<u4"), ("kvflag", "<u4"), ("skey_off", "<u4"),
                      ("sklen", "<u4"), ("reserved", "<u4")])
assert REQ_DTYPE.itemsize == 32

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_kvget_dev.restype = ctypes.c_int
        lib.pom_kvget_dev.argtypes = [_vp] * 5 + [ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32] + \
            [_vp] * 7 + [ctypes.c_uint64, _vp]
        lib.pom_kvget_batch.restype = ctypes.c_int
        lib.pom_kvget_batch.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp, ctypes.c_size_t, _vp,
                                        ctypes.c_size_t, _vp, ctypes.c_size_t] + [_vp] * 6
        _bound = True
    return lib


def requests(items: Sequence[dict]) -> Tuple[np.ndarray, bytes]:
    """[{itb, key, flag=KG_KV | KG_LOOKUP, kvflag=KV_NORMAL, skey=None}] ->
    (REQ_DTYPE array, key blob), the string keys packed one behind the other.
    An item with skey (bytes) is a string get unless it sets kvflag itself;
    sklen overrides len(skey)."""
    req = np.zeros(len(items), dtype=REQ_DTYPE)
    blob = bytearray()
    for r, it in enumerate(items):
        skey = it.get("skey")
        kvflag = it.get("kvflag", KV_NORMAL if skey is None else KV_STR)
        skey = bytes(skey or b"")
        req[r] = (it["key"], it["itb"], it.get("flag", KG_KV | KG_LOOKUP), kvflag, len(blob),
                  it.get("sklen", len(skey)), 0)
        blob += skey
    return req, bytes(blob)


def kvget_dev(payload: lzo.DeviceBatch, adepth, req, nreq: int, keys, keys_len: int, err, nr, depth, length, lease,
              first, out, out_cap: int, status=None, stream=None) -> None:
    """Enqueue pom_kvget_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64, length int32);
    adepth: uint8 per ITB; status: int32 per ITB or None; req: the
    pom_kvget_req records as a uint8 tensor, 8-byte aligned; keys: uint8 tensor
    holding the blob at any alignment (None with keys_len 0).  Outputs, all on
    the GPU: err, nr, depth, length (int32, nreq each), lease (int64, nreq),
    first (int64, nreq + 1) and out (uint8, any alignment, written below
    out_cap; None with out_cap 0)."""
    import torch
    if min(err.numel(), nr.numel(), depth.numel(), length.numel(), lease.numel()) < nreq or first.numel() < nreq + 1:
        raise ValueError("an output is smaller than nreq results")
    if out_cap and (out is None or out.numel() < out_cap):
        raise ValueError("out is smaller than out_cap")
    if req.numel() < REQ_DTYPE.itemsize * nreq or (keys_len and keys.numel() < keys_len):
        raise ValueError("req or keys is smaller than stated")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_kvget_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth),
                              payload.nblocks, p(req), nreq, p(keys), keys_len, p(err), p(nr), p(depth), p(length),
                              p(lease), p(first), p(out), out_cap, lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_kvget_dev launch failed")


class KvgetResult(NamedTuple):
    rc: int                 # 0 or E_NOSPACE
    err: np.ndarray         # int32 [nreq]
    nr: np.ndarray          # uint32 [nreq]
    depth: np.ndarray       # uint32 [nreq]
    len: np.ndarray         # uint32 [nreq]
    lease: np.ndarray       # uint64 [nreq]
    first: np.ndarray       # uint64 [nreq + 1]
    out: Optional[np.ndarray]   # uint8 [min(first[nreq], out_cap)], or None for a lengths-only call

    def record(self, r: int) -> bytes:
        return self.out[int(self.first[r]): int(self.first[r + 1])].tobytes()


def kvget_batch(records: Sequence, req: np.ndarray, keys: bytes = b"", itbid_check: bool = False,
                out_cap: Optional[int] = None, lengths_only: bool = False) -> KvgetResult:
    """pom_kvget_batch over ITB records (bytes-like, [itbh][payload], as
    stored) and a REQ_DTYPE array with its key blob.  out_cap None: room for
    every request's longest record.  Raises RuntimeError unless the call
    returns 0 or E_NOSPACE."""
    lib = _lib()
    n, nreq = len(records), len(req)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    req = np.ascontiguousarray(req, dtype=REQ_DTYPE)
    blob = np.frombuffer(bytes(keys) or b"\0", dtype=np.uint8)
    cap = KG_REC_MAX * nreq if out_cap is None else int(out_cap)
    out = None if lengths_only else np.zeros(max(cap, 1), dtype=np.uint8)
    err = np.zeros(max(nreq, 1), dtype=np.int32)
    nr, depth, length = (np.zeros(max(nreq, 1), dtype=np.uint32) for _ in range(3))
    lease = np.zeros(max(nreq, 1), dtype=np.uint64)
    first = np.zeros(nreq + 1, dtype=np.uint64)
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    rc = lib.pom_kvget_batch(ptrs, lens, n, int(bool(itbid_check)), req.ctypes.data if nreq else None, nreq,
                             blob.ctypes.data, len(keys), None if out is None else out.ctypes.data, cap,
                             first.ctypes.data, err.ctypes.data, nr.ctypes.data, depth.ctypes.data,
                             length.ctypes.data, lease.ctypes.data)
    if rc not in (0, E_NOSPACE):
        raise RuntimeError(f"pom_kvget_batch: {rc}")
    return KvgetResult(rc, err[:nreq], nr[:nreq], depth[:nreq], length[:nreq], lease[:nreq], first,
                       None if out is None else out[: min(int(first[nreq]), cap)])


def parse(record, column: bool = False):
    """(v.flags, v.len, v.key, v.klen, value bytes, (stored_itbid, len, offset)
    or None) of one record; column: the request had KG_COLUMN."""
    record = bytes(record)
    tail = COLUMN_SIZE if column else 0
    if len(record) < KV_HEADER_LEN + tail:
        raise ValueError(f"a record has at least {KV_HEADER_LEN + tail} bytes, not {len(record)}")
    flags, vlen, key, klen = struct.unpack_from("<IIQI", record, 0)
    if len(record) != KV_HEADER_LEN + vlen + tail:
        raise ValueError(f"v.len {vlen} does not agree with a record of {len(record)} bytes")
    value = record[KV_HEADER_LEN: KV_HEADER_LEN + vlen]
    return flags, vlen, key, klen, value, struct.unpack_from("<QQQ", record, KV_HEADER_LEN + vlen) if column else None
