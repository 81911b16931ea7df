"""Client column-data codec (include/pom_column.h): [u64 length][LZO1X-1 stream]
with raw fallback, as api/api.c:6509-6541 (hvfs_fwrite), :6652-6689
(hvfs_fwritev) and :6427-6446 (read side) use it; read_batch and slice_dev
add the read side's region copy (:6447-6460), so that only the requested bytes
leave the GPU."""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Tuple

from . import lzo

_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_col_zip_bound.restype = _sz
        lib.pom_col_zip_bound.argtypes = [_sz]
        lib.pom_col_zip_batch.restype = ctypes.c_int
        lib.pom_col_zip_batch.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp, _vp]
        lib.pom_col_zipv.restype = ctypes.c_int
        lib.pom_col_zipv.argtypes = [_vp, _vp, _sz, _vp, _sz, ctypes.POINTER(_sz),
                                     ctypes.POINTER(ctypes.c_int)]
        lib.pom_col_unzip_batch.restype = ctypes.c_int
        lib.pom_col_unzip_batch.argtypes = [_vp, _vp, _sz, _vp, _vp, _vp, _vp]
        lib.pom_col_read_batch.restype = ctypes.c_int
        lib.pom_col_read_batch.argtypes = [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp]
        lib.pom_col_slice_dev.restype = ctypes.c_int
        lib.pom_col_slice_dev.argtypes = [_vp] * 5 + [ctypes.c_uint32, _vp, ctypes.c_uint32] + [_vp] * 5
        _bound = True
    return lib


class Req(ctypes.Structure):
    """struct pom_col_req: size bytes from byte offset of decoded column col."""
    _fields_ = [("offset", ctypes.c_uint64), ("size", ctypes.c_uint64),
                ("col", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


def zip_bound(n: int) -> int:
    return int(_lib().pom_col_zip_bound(n))


def _arr(bufs):
    a = (_vp * len(bufs))()
    for i, b in enumerate(bufs):
        a[i] = ctypes.cast(b, _vp).value
    return a


def zip_batch(columns: Sequence[bytes], caps: Sequence[int] = None
              ) -> Tuple[List[bytes], List[int]]:
    """-> (zipped bytes or b"" when raw, compressed flags)."""
    lib = _lib()
    n = len(columns)
    caps = list(caps) if caps is not None else [zip_bound(len(c)) for c in columns]
    src = [ctypes.create_string_buffer(bytes(c), max(len(c), 1)) for c in columns]
    dst = [ctypes.create_string_buffer(max(c, 1)) for c in caps]
    ln = (_sz * n)(*[len(c) for c in columns])
    cp = (_sz * n)(*caps)
    zl = (_sz * n)()
    comp = (ctypes.c_int * n)()
    rc = lib.pom_col_zip_batch(_arr(src), ln, n, _arr(dst), cp, zl, comp)
    if rc != 0:
        raise RuntimeError(f"pom_col_zip_batch: {rc}")
    return [dst[i].raw[: zl[i]] for i in range(n)], list(comp)


def zipv(iov: Sequence[bytes], cap: int) -> Tuple[bytes, int]:
    lib = _lib()
    bufs = [ctypes.create_string_buffer(bytes(b), max(len(b), 1)) for b in iov]
    lens = (_sz * len(iov))(*[len(b) for b in iov])
    out = ctypes.create_string_buffer(max(cap, 1))
    zl = _sz(0)
    comp = ctypes.c_int(0)
    rc = lib.pom_col_zipv(_arr(bufs), lens, len(iov), out, cap, ctypes.byref(zl),
                          ctypes.byref(comp))
    if rc != 0:
        raise RuntimeError(f"pom_col_zipv: {rc}")
    return out.raw[: zl.value], comp.value


def unzip_batch(zipped: Sequence[bytes], caps: Sequence[int]) -> Tuple[List[bytes], List[int]]:
    """-> (decoded bytes, err codes: 0 = decoded to exactly the recorded length)."""
    lib = _lib()
    n = len(zipped)
    src = [ctypes.create_string_buffer(bytes(z), max(len(z), 1)) for z in zipped]
    out = [ctypes.create_string_buffer(max(c, 1)) for c in caps]
    zl = (_sz * n)(*[len(z) for z in zipped])
    cp = (_sz * n)(*caps)
    ol = (_sz * n)()
    err = (ctypes.c_int * n)()
    rc = lib.pom_col_unzip_batch(_arr(src), zl, n, _arr(out), cp, ol, err)
    if rc != 0:
        raise RuntimeError(f"pom_col_unzip_batch: {rc}")
    return [out[i].raw[: ol[i]] for i in range(n)], list(err)


def read_batch(zipped: Sequence[bytes], reqs: Sequence[Tuple[int, int, int]], room: Sequence[int] = None
               ) -> Tuple[List[bytes], List[int]]:
    """pom_col_read_batch: reqs are (col, offset, size) -> (the bytes read, err
    codes).  room[r]: the bytes allocated for request r (default: size, capped
    at 64 MiB for the sizes no buffer can have)."""
    lib = _lib()
    n, nr = len(zipped), len(reqs)
    src = [ctypes.create_string_buffer(bytes(z), max(len(z), 1)) for z in zipped]
    zl = (_sz * max(n, 1))(*[len(z) for z in zipped])
    rq = (Req * max(nr, 1))(*[Req(o, s, c, 0) for c, o, s in reqs])
    room = list(room) if room is not None else [min(s, 64 << 20) for _, _, s in reqs]
    out = [ctypes.create_string_buffer(max(k, 1)) for k in room]
    ol = (_sz * max(nr, 1))()
    err = (ctypes.c_int * max(nr, 1))()
    rc = lib.pom_col_read_batch(_arr(src), zl, n, rq, nr, _arr(out), ol, err)
    if rc != 0:
        raise RuntimeError(f"pom_col_read_batch: {rc}")
    return [out[i].raw[: ol[i]] for i in range(nr)], list(err)[:nr]


def slice_dev(data: "lzo.DeviceBatch", want, req, out, out_off, out_len, err, status=None,
              stream=None) -> None:
    """Enqueue pom_col_slice_dev on the current (or the given) stream.

    data: the decoded columns (arena uint8, off int64, length int32 = the
    produced lengths); want: int64 per column; status: int32 per column or
    None; req: int64 [nreq, 3] on the GPU, rows (offset, size, col) -- the bit
    pattern of struct pom_col_req; out: uint8; out_off: int64 per request.
    Outputs on the GPU: out_len, err (int32 per request)."""
    import torch
    nreq = int(req.shape[0])
    if req.dtype != torch.int64 or req.dim() != 2 or req.shape[1] != 3 or not req.is_contiguous():
        raise ValueError("req: a contiguous int64 [nreq, 3] tensor")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_col_slice_dev(p(data.arena), p(data.off), p(data.length), p(status), p(want),
                                  data.nblocks, p(req), nreq, p(out), p(out_off), p(out_len), p(err),
                                  lzo._stream_handle(torch, stream))
    if rc != 0:
        raise RuntimeError("pom_col_slice_dev launch failed")
