#!/usr/bin/env python3
"""ITB check: decode-and-copy-back against decode-and-check-on-the-GPU.

Two paths over one seeded set of COMPR_LZO ITB records, in one process,
alternating, each warmed up first:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the host check
     (itb_check_one from tests/native/libitb_check_host.so, one C call over the
     batch): what a caller of the library could do before pom_itb_check_batch
     existed.  The decode alone is timed too (A without its check).
  B  pom_itb_check_batch: decode and check on the GPU; only codes and 48-byte
     reports come back (and, in a second measurement, the masks)
Both produce the same reports (checked once, outside the timing).  The record
set: `--records` records of 64 KiB payloads (105 ITEs) with an index table
built the way __itb_add_index builds it from the ITEs' hashes and header
counters to match, so that the check reports nothing.  Rates are GiB/s of
decoded payload, median and min ... max over `--rounds` alternating rounds;
the bytes each path copies each way are computed from the lengths.  Only the C
calls are timed (pointer arrays are built before).  Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import datetime
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pomegranate_amd import check, gc, itb, lzo  # noqa: E402
from lookup_rate import index_table  # noqa: E402

GIB = float(1 << 30)
H = itb.ITBH_SIZE


def make_records(n_ites_list, seed0):
    """Records as stored uncompressed, with adepth 10, the first n_ites bitmap
    bits set, the index table of their ITEs' hashes and the header counters
    itb_add_ite would have left."""
    recs = []
    for i, k in enumerate(n_ites_list):
        k = int(k)
        r = itb.make_record(seed0 + i, k)
        r = r[: itb.header_fields(r)[0]]
        r[2], r[3] = 0, 10                                  # depth 0: every hash belongs; adepth
        bm = bytearray(128)
        for nr in range(k):
            bm[nr // 8] |= 1 << (nr % 8)
        r[H + gc.BITMAP_OFF: H + gc.INDEX_OFF] = bm
        ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(k, gc.ITE_SIZE)
        hashes = ites[:, :8].copy().view("<u8")[:, 0].tolist()
        idx = index_table(hashes)
        r[H + gc.INDEX_OFF: H + gc.ITE_OFF] = idx.tobytes()
        over = int(((idx[1024:] >> 30) != 0).sum())
        struct.pack_into("<ii", r, 4, k, k - 1)             # entries, max_offset
        struct.pack_into("<i", r, check.ITBH_PSEUDO_CONFLICTS_OFF, over)
        struct.pack_into("<HH", r, check.ITBH_INF_OFF, over, over)
        struct.pack_into("<Q", r, 136, 0)
        recs.append(r)
    return recs


def build(n_ites_list, seed0):
    """make_records, compressed on the GPU: (COMPR_LZO records, decoded payload
    lengths)."""
    recs = make_records(n_ites_list, seed0)
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored]


def measure(stored, plain, rounds):
    lib = check._lib()
    itb._lib()
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_check_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    host.itb_check_batch_host.restype = None
    host.itb_check_batch_host.argtypes = [vp] * 6 + [u32, u32] + [vp] * 4
    n = len(stored)
    total_plain = float(sum(plain))
    z = [len(s) - H for s in stored]
    # B: read-only records
    keep_b = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep_b])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    rep_b = np.zeros(n, dtype=check.REPORT_DTYPE)
    sm_b, im_b = np.zeros((n, 32), np.uint64), np.zeros((n, 16), np.uint64)
    err_b, ok_b = np.zeros(n, np.int32), np.zeros(n, np.int32)
    # A: decoded in place in one arena, so every round starts from fresh copies (made outside the timing)
    offs = np.zeros(n, dtype=np.uint64)
    pos = 0
    for b, p in enumerate(plain):
        offs[b] = pos
        pos += (H + p + 15) // 16 * 16
    arena = np.zeros(pos, dtype=np.uint8)
    bufs = [arena[int(o): int(o) + H + p] for o, p in zip(offs, plain)]
    ptr_a = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    cap_a = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    err_a = (ctypes.c_int * n)()
    ok_a = (ctypes.c_int * n)()
    pay_off = offs + np.uint64(H)
    len_a = np.array(plain, dtype=np.uint32)
    adepth = np.full(n, 10, dtype=np.uint8)
    hdr = np.concatenate([check.header_facts(s) for s in stored])
    rep_a = np.zeros(n, dtype=check.REPORT_DTYPE)
    cerr_a = np.zeros(n, np.int32)

    def run_a():
        for b, s in zip(bufs, keep_b):
            b[: s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        host.itb_check_batch_host(arena.ctypes.data, pay_off.ctypes.data, len_a.ctypes.data, None, adepth.ctypes.data,
                                  hdr.ctypes.data, n, check.CK_ITBID, rep_a.ctypes.data, None, None,
                                  cerr_a.ctypes.data)
        t2 = time.perf_counter()
        assert rc == 0 and not any(err_a) and all(ok_a) and not cerr_a.any()
        return t2 - t0, t1 - t0

    def run_b(masks):
        t0 = time.perf_counter()
        rc = lib.pom_itb_check_batch(ptr_b, len_b, n, check.CK_ITBID, rep_b.ctypes.data,
                                     sm_b.ctypes.data if masks else None, im_b.ctypes.data if masks else None,
                                     err_b.ctypes.data, ok_b.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err_b.any() and ok_b.all()
        return dt

    run_a(), run_b(False), run_b(True), run_a(), run_b(False), run_b(True)   # warm-up: staging grown on every path
    assert rep_a.tobytes() == rep_b.tobytes(), "the two paths disagree"
    assert not rep_b["findings"].any(), "a table built as the MDS builds it reports something"
    ta, td, tb, tm = [], [], [], []
    for _ in range(rounds):
        both, decode = run_a()
        ta.append(both)
        td.append(decode)
        tb.append(run_b(False))
        tm.append(run_b(True))
    rate = lambda ts: {"median_ms": round(statistics.median(ts) * 1e3, 2),
                       "median_gibps": round(total_plain / statistics.median(ts) / GIB, 2),
                       "min_gibps": round(total_plain / max(ts) / GIB, 2),
                       "max_gibps": round(total_plain / min(ts) / GIB, 2)}
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    d2h_a = aligned(plain) + 8 * n
    res = {"date": datetime.date.today().isoformat(), "records": n, "decoded_bytes": int(total_plain),
           "compressed_bytes": int(sum(z)), "rounds": rounds,
           "A_decompress_batch_then_host_check": dict(rate(ta), h2d_bytes=aligned(z) + 48 * n, d2h_bytes=d2h_a),
           "A_decompress_batch_alone": rate(td),
           "B_check_batch": dict(rate(tb), h2d_bytes=aligned(z) + 73 * n, d2h_bytes=(12 + 48) * n),
           "B_check_batch_with_masks": dict(rate(tm), h2d_bytes=aligned(z) + 73 * n,
                                            d2h_bytes=(12 + 48 + 384) * n),
           "itbs_per_s_A": round(n / statistics.median(ta)), "itbs_per_s_B": round(n / statistics.median(tb)),
           "d2h_ratio": round(d2h_a / ((12 + 48) * n), 1)}
    res["B_over_A"] = round(statistics.median(ta) / statistics.median(tb), 2)
    res["B_over_A_decode_alone"] = round(statistics.median(td) / statistics.median(tb), 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="records of 64 KiB payloads")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    stored, plain = build([105] * args.records, 700000)
    measure(stored, plain, args.rounds)


if __name__ == "__main__":
    main()
