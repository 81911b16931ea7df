#!/usr/bin/env python3
"""GC data scan: decode-and-copy-back against decode-and-walk-on-the-GPU.

Two paths over one seeded set of COMPR_LZO ITB records, in one process,
alternating, each warmed up first:
  A  pom_itb_lzo_decompress_batch on copies of the records: what a GC linked
     against the library does today, WITHOUT its host-side bitmap walk (so A
     is a lower bound in A's favour)
  B  pom_gc_scan_batch: decode, walk and range gather on the GPU; only counts
     and ranges come back
Record sets: `--records` records of 64 KiB payloads (105 ITEs), and the C5
mix (bench.py run_c5: 1 ... 1024 ITEs, seed 5).  Rates are GiB/s of decoded
payload, median and min ... max over `--rounds` alternating rounds; the bytes
each path copies each way are computed from the lengths.  Only the C calls
are timed (pointer arrays are built before).  Prints one JSON line per set.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pomegranate_amd import gc, itb, lzo  # noqa: E402

GIB = float(1 << 30)
H = itb.ITBH_SIZE


def build(n_ites_list, seed0):
    """COMPR_LZO records (compressed on the GPU) with adepth 10 and the first
    n_ites bitmap bits set; returns (stored, decoded payload lengths)."""
    recs = []
    for i, k in enumerate(n_ites_list):
        r = itb.make_record(seed0 + i, int(k))
        r = r[: itb.header_fields(r)[0]]
        r[3] = 10
        r[4:8] = int(k).to_bytes(4, "little")
        bm = bytearray(128)
        for nr in range(int(k)):
            bm[nr // 8] |= 1 << (nr % 8)
        r[H + gc.BITMAP_OFF: H + gc.INDEX_OFF] = bm
        recs.append(r)
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored]


def measure(name, stored, plain, column, rounds):
    lib = gc._lib()
    itb._lib()
    n = len(stored)
    total_plain = float(sum(plain))
    z = [len(s) - H for s in stored]
    # B: read-only records
    keep_b = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep_b])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    cap = 1024 * n
    ranges = np.zeros((cap, 2), dtype=np.uint64)
    first = np.zeros(n + 1, dtype=np.uint64)
    live = np.zeros(n, dtype=np.uint32)
    err_b = np.zeros(n, dtype=np.int32)
    # A: decoded in place, so every round starts from fresh copies (made outside the timing)
    bufs = [np.zeros(H + p, dtype=np.uint8) for p in plain]
    ptr_a = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    cap_a = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    err_a = (ctypes.c_int * n)()
    ok_a = (ctypes.c_int * n)()

    def run_a():
        for b, s in zip(bufs, keep_b):
            b[: s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        dt = time.perf_counter() - t0
        assert rc == 0 and not any(err_a) and all(ok_a)
        return dt

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_gc_scan_batch(ptr_b, len_b, n, column, ranges.ctypes.data, cap, first.ctypes.data,
                                   live.ctypes.data, err_b.ctypes.data, None, None)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err_b.any()
        return dt

    run_a(), run_b(), run_a(), run_b()                           # warm-up: staging grown on both paths
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(run_a())
        tb.append(run_b())
    nr = int(first[n])
    rate = lambda ts: {"median_gibps": round(total_plain / statistics.median(ts) / GIB, 2),
                       "min_gibps": round(total_plain / max(ts) / GIB, 2),
                       "max_gibps": round(total_plain / min(ts) / GIB, 2)}
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    res = {"set": name, "records": n, "decoded_bytes": int(total_plain), "compressed_bytes": int(sum(z)),
           "live_ites": int(live.sum()), "ranges": nr, "rounds": rounds, "column": column,
           "A_decompress_batch": dict(rate(ta), h2d_bytes=aligned(z) + 48 * n, d2h_bytes=aligned(plain) + 8 * n),
           "B_gc_scan_batch": dict(rate(tb), h2d_bytes=aligned(z) + 61 * n, d2h_bytes=20 * n + 16 * nr)}
    res["B_over_A"] = round(statistics.median(ta) / statistics.median(tb), 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="records of 64 KiB payloads")
    ap.add_argument("--c5-records", type=int, default=1024, help="records of the C5 mix")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--column", type=int, default=0)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    if args.records:
        stored, plain = build([105] * args.records, 700000)
        measure("64KiB", stored, plain, args.column, args.rounds)
    if args.c5_records:
        ites = np.random.default_rng(5).integers(1, 1025, args.c5_records)
        stored, plain = build(ites, 100000)
        measure("C5", stored, plain, args.column, args.rounds)


if __name__ == "__main__":
    main()
