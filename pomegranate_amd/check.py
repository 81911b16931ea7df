"""The ITB check on the GPU (include/pom_check.h).

Whether the three views of one ITB agree -- the ITE bitmap, the index table's
hash chains and the header's counters, as __itb_add_index, itb_add_ite,
__ite_unlink and itb_del_ite keep them (mds/itb.c:215-322, :330-532, :567-671):
  check_dev   <- the check over decoded payloads in HBM
  check_batch <- the decode and the check over records in host memory; only
                 codes, 48-byte reports and, when asked for, the masks come
                 back from the GPU
  Report      <- a view over one report's 48 bytes
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import lzo

E_TRUNCATED = -4097
EINVAL = -22

ITBH_MAX_OFFSET_OFF, ITBH_PSEUDO_CONFLICTS_OFF, ITBH_INF_OFF, ITBH_ITU_OFF = 8, 16, 250, 252
ITB_SIZE = 12168
CK_ITBID = 0x1
CK_SLOT_MASK_WORDS, CK_ITE_MASK_WORDS = 32, 16

# The kinds: the bit number in `findings`, and the index into count[] below 16.
KINDS = ("S_OUTSIDE", "S_FLAG", "S_LINK_RANGE", "S_LINK_HOME", "S_LINK_FREE", "S_ENTRY_RANGE", "S_ENTRY_DEAD",
         "S_SHARED", "S_LEAKED", "S_ISLAND", "S_LOOP", "S_MISFILED", "E_STRAY", "E_DUP", "E_ORPHAN", "E_MISPLACED",
         "H_ENTRIES", "H_ITU", "H_PSEUDO", "H_MAXOFF", "H_LEN", "H_INF")
CK_KINDS = len(KINDS)
for _k, _name in enumerate(KINDS):
    globals()["CK_" + _name] = _k

# struct pom_check_hdr, struct pom_check_report
HDR_DTYPE = np.dtype([("entries", "<i4"), ("max_offset", "<i4"), ("pseudo_conflicts", "<i4"), ("ulen", "<u4"),
                      ("inf", "<u2"), ("itu", "<u2"), ("depth", "u1"), ("pad", "u1", (3,)), ("itbid", "<u8")])
REPORT_DTYPE = np.dtype([("findings", "<u4"), ("live", "<u4"), ("used_home", "<u2"), ("used_over", "<u2"),
                         ("reached", "<u2"), ("longest", "<u2"), ("count", "<u2", (16,))])
assert HDR_DTYPE.itemsize == 32 and REPORT_DTYPE.itemsize == 48

_vp = ctypes.c_void_p
_bound = False


def _lib() -> ctypes.CDLL:
    global _bound
    lib = lzo.load()
    if not _bound:
        lib.pom_itb_check_dev.restype = ctypes.c_int
        lib.pom_itb_check_dev.argtypes = [_vp] * 6 + [ctypes.c_uint32, ctypes.c_uint32] + [_vp] * 5
        lib.pom_itb_check_batch.restype = ctypes.c_int
        lib.pom_itb_check_batch.argtypes = [_vp, _vp, ctypes.c_size_t, ctypes.c_uint32] + [_vp] * 5
        _bound = True
    return lib


class Report(NamedTuple):
    """One struct pom_check_report."""
    findings: int
    live: int
    used_home: int
    used_over: int
    reached: int
    longest: int
    count: tuple

    @classmethod
    def parse(cls, raw) -> "Report":
        raw = bytes(raw)
        if len(raw) != REPORT_DTYPE.itemsize:
            raise ValueError(f"a report has {REPORT_DTYPE.itemsize} bytes, not {len(raw)}")
        r = np.frombuffer(raw, dtype=REPORT_DTYPE)[0]
        return cls(int(r["findings"]), int(r["live"]), int(r["used_home"]), int(r["used_over"]), int(r["reached"]),
                   int(r["longest"]), tuple(int(c) for c in r["count"]))

    @property
    def kinds(self) -> tuple:
        """The names of the kinds that occurred."""
        return tuple(name for k, name in enumerate(KINDS) if self.findings >> k & 1)


def header_facts(rec) -> np.ndarray:
    """One HDR_DTYPE row from a record's struct itbh, as pom_itb_check_batch
    fills it: ulen is h.zlen of a COMPR_LZO record, else h.len."""
    raw = np.frombuffer(bytes(rec[:264]), dtype=np.uint8)
    i32 = lambda o: int(raw[o: o + 4].view("<i4")[0])
    u16 = lambda o: int(raw[o: o + 2].view("<u2")[0])
    h = np.zeros(1, dtype=HDR_DTYPE)
    lzo_rec = u16(248) == 1
    h[0] = (i32(4), i32(ITBH_MAX_OFFSET_OFF), i32(ITBH_PSEUDO_CONFLICTS_OFF),
            int(raw[244 if lzo_rec else 240:][:4].view("<u4")[0]), u16(ITBH_INF_OFF), u16(ITBH_ITU_OFF),
            int(raw[2]), (0, 0, 0), int(raw[136:144].view("<u8")[0]))
    return h


def check_dev(payload: lzo.DeviceBatch, adepth, report, err, hdr=None, flags: int = 0, slot_mask=None,
              ite_mask=None, status=None, stream=None) -> None:
    """Enqueue pom_itb_check_dev on the current (or the given) stream.

    payload: the decoded payloads (arena uint8, off int64, length int32 = the
    produced lengths); adepth: uint8 per ITB; status: int32 per ITB or None;
    hdr: the pom_check_hdr records as a uint8 tensor, 8-byte aligned, or None.
    Outputs, all on the GPU: report (uint8, 48 bytes per ITB, 4-byte aligned),
    err (int32), and when given slot_mask (int64, 32 per ITB) and ite_mask
    (int64, 16 per ITB).  Raises ValueError for a flags bit other than
    CK_ITBID."""
    import torch
    n = payload.nblocks
    nbytes = lambda t: t.numel() * t.element_size()
    if nbytes(report) < 48 * n or err.numel() < n:
        raise ValueError("an output is smaller than nitb results")
    if (hdr is not None and nbytes(hdr) < 32 * n) or (slot_mask is not None and nbytes(slot_mask) < 256 * n) or \
            (ite_mask is not None and nbytes(ite_mask) < 128 * n):
        raise ValueError("hdr or a mask is smaller than stated")
    p = lambda t: int(t.data_ptr()) if t is not None and t.numel() else None
    rc = _lib().pom_itb_check_dev(p(payload.arena), p(payload.off), p(payload.length), p(status), p(adepth), p(hdr),
                                  n, flags, p(report), p(slot_mask), p(ite_mask), p(err),
                                  lzo._stream_handle(torch, stream))
    if rc == EINVAL:
        raise ValueError("pom_itb_check_dev: -EINVAL (a flags bit other than CK_ITBID)")
    if rc != 0:
        raise RuntimeError("pom_itb_check_dev launch failed")


class CheckResult(NamedTuple):
    err: np.ndarray                     # int32 [n]
    report: np.ndarray                  # REPORT_DTYPE [n]
    len_ok: np.ndarray                  # int32 [n]
    slot_mask: Optional[np.ndarray]     # uint64 [n, 32], with masks
    ite_mask: Optional[np.ndarray]      # uint64 [n, 16], with masks


def check_batch(records: Sequence, flags: int = 0, masks: bool = False) -> CheckResult:
    """pom_itb_check_batch over ITB records (bytes-like, [itbh][payload], as
    stored).  Raises ValueError for what the library answers with -EINVAL,
    RuntimeError when the GPU path is unusable."""
    lib = _lib()
    n = len(records)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in records]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * max(n, 1))(*[b.size for b in bufs])
    report = np.zeros(max(n, 1), dtype=REPORT_DTYPE)
    err = np.zeros(max(n, 1), dtype=np.int32)
    len_ok = np.zeros(max(n, 1), dtype=np.int32)
    slot_mask = np.zeros((max(n, 1), CK_SLOT_MASK_WORDS), dtype=np.uint64) if masks else None
    ite_mask = np.zeros((max(n, 1), CK_ITE_MASK_WORDS), dtype=np.uint64) if masks else None
    assert ctypes.sizeof(ctypes.c_size_t) == 8
    rc = lib.pom_itb_check_batch(ptrs, lens, n, flags, report.ctypes.data,
                                 slot_mask.ctypes.data if masks else None, ite_mask.ctypes.data if masks else None,
                                 err.ctypes.data, len_ok.ctypes.data)
    if rc == EINVAL:
        raise ValueError("pom_itb_check_batch: -EINVAL (a flags bit other than CK_ITBID)")
    if rc != 0:
        raise RuntimeError(f"pom_itb_check_batch: {rc}")
    return CheckResult(err[:n], report[:n], len_ok[:n], slot_mask[:n] if masks else None,
                       ite_mask[:n] if masks else None)
