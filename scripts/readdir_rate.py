#!/usr/bin/env python3
"""Directory listing: decode-and-copy-back against decode-and-list-on-the-GPU.

Two paths over one seeded set of COMPR_LZO ITB records, in one process,
alternating, each warmed up first:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the host walk
     (itb_dents_one from tests/native/libitb_dents_host.so, one C call over the
     batch): what an MDS linked against the library does today for a cold
     listing.  The decode alone is timed too (A without its walk).
  B  pom_readdir_batch: decode, walk and record packing on the GPU; only counts
     and records come back
Both produce the same bytes (checked once, outside the timing).  Record sets:
`--records` records of 64 KiB payloads (105 ITEs), and the C5 mix (bench.py
run_c5: 1 ... 1024 ITEs, seed 5); names are the generator's 17 bytes.  Rates
are GiB/s of decoded payload, median and min ... max over `--rounds`
alternating rounds; the bytes each path copies each way are computed from the
lengths.  Only the C calls are timed (pointer arrays are built before).
Prints one JSON line per set.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pomegranate_amd import gc, itb, lzo, readdir  # noqa: E402

GIB = float(1 << 30)
H = itb.ITBH_SIZE


def build(n_ites_list, seed0, name_len=None):
    """COMPR_LZO records (compressed on the GPU) with adepth 10 and the first
    n_ites bitmap bits set; returns (stored, decoded payload lengths).
    name_len: every name becomes that many seeded random letters (default:
    the generator's 17-byte names)."""
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
        if name_len is not None:
            ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(int(k), gc.ITE_SIZE)
            ites[:, readdir.ITE_NAMELEN_OFF: readdir.ITE_NAMELEN_OFF + 4] = np.frombuffer(
                int(name_len).to_bytes(4, "little"), dtype=np.uint8)
            ites[:, readdir.ITE_NAME_OFF: readdir.ITE_NAME_OFF + name_len] = np.random.default_rng(seed0 + i).integers(
                97, 123, (int(k), name_len), dtype=np.uint8)
        recs.append(r)
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored]


def measure(name, stored, plain, rounds, alt=False, name_len=None):
    lib = readdir._lib()
    itb._lib()
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_dents_host.so"))
    host.itb_dents_host_batch.restype = ctypes.c_int
    host.itb_dents_host_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                          ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    n = len(stored)
    total_plain = float(sum(plain))
    z = [len(s) - H for s in stored]
    cap = sum(readdir.REC_MAX * min(1024, (p - 11904) // 512) for p in plain)
    # B: read-only records
    keep_b = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep_b])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    out_b = np.zeros(cap, dtype=np.uint8)
    first_b = np.zeros(n + 1, dtype=np.uint64)
    live = np.zeros(n, dtype=np.uint32)
    dnum = np.zeros(n, dtype=np.uint32)
    err_b = np.zeros(n, dtype=np.int32)
    # A: decoded in place, so every round starts from fresh copies (made outside the timing)
    bufs = [np.zeros(H + p, dtype=np.uint8) for p in plain]
    ptr_a = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    cap_a = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    err_a = (ctypes.c_int * n)()
    ok_a = (ctypes.c_int * n)()
    pay_a = (ctypes.c_void_p * n)(*[b.ctypes.data + H for b in bufs])
    len_a = np.array(plain, dtype=np.uint32)
    adepth = np.full(n, 10, dtype=np.uint8)
    out_a = np.zeros(cap, dtype=np.uint8)
    first_a = np.zeros(n + 1, dtype=np.uint64)

    def run_a():
        for b, s in zip(bufs, keep_b):
            b[: s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        rw = host.itb_dents_host_batch(pay_a, len_a.ctypes.data, adepth.ctypes.data, n, out_a.ctypes.data, cap,
                                       first_a.ctypes.data)
        t2 = time.perf_counter()
        assert rc == 0 and rw == 0 and not any(err_a) and all(ok_a)
        return t2 - t0, t1 - t0

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_readdir_batch(ptr_b, len_b, n, out_b.ctypes.data, cap, first_b.ctypes.data, live.ctypes.data,
                                   dnum.ctypes.data, err_b.ctypes.data, None, None)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err_b.any()
        return dt

    run_a(), run_b(), run_a(), run_b()                           # warm-up: staging grown on both paths
    nbytes = int(first_b[n])
    assert (first_a == first_b).all() and (out_a[:nbytes] == out_b[:nbytes]).all(), "the two paths disagree"
    def run_alt():
        # the same call with every emitting lane copying its own record (itb_dents.hip, dents_copy=1)
        os.environ["POM_LZO_DEBUG"] = "dents_copy=1"
        lzo.debug_reload()
        try:
            return run_b()
        finally:
            del os.environ["POM_LZO_DEBUG"]
            lzo.debug_reload()

    if alt:
        run_alt()
        assert (first_a == first_b).all() and (out_a[:nbytes] == out_b[:nbytes]).all(), "the per-lane copy disagrees"
    ta, td, tb, tl = [], [], [], []
    for k in range(rounds):
        both, decode = run_a()
        ta.append(both)
        td.append(decode)
        if alt and k % 2:                       # B and its alternative take turns behind A
            tl.append(run_alt())
        tb.append(run_b())
        if alt and not k % 2:
            tl.append(run_alt())
    rate = lambda ts: {"median_gibps": round(total_plain / statistics.median(ts) / GIB, 2),
                       "min_gibps": round(total_plain / max(ts) / GIB, 2),
                       "max_gibps": round(total_plain / min(ts) / GIB, 2)}
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    d2h_a = aligned(plain) + 8 * n
    d2h_b = 24 * n + nbytes
    res = {"set": name, "records": n, "name_len": name_len if name_len is not None else 17, "decoded_bytes": int(total_plain), "compressed_bytes": int(sum(z)),
           "live_ites": int(live.sum()), "dentries": int(dnum.sum()), "record_bytes": nbytes, "rounds": rounds,
           "A_decompress_batch_then_host_walk": dict(rate(ta), h2d_bytes=aligned(z) + 48 * n, d2h_bytes=d2h_a),
           "A_decompress_batch_alone": rate(td),
           "B_readdir_batch": dict(rate(tb), h2d_bytes=aligned(z) + 61 * n, d2h_bytes=d2h_b),
           "d2h_ratio": round(d2h_a / d2h_b, 1)}
    res["B_over_A"] = round(statistics.median(ta) / statistics.median(tb), 2)
    res["B_over_A_decode_alone"] = round(statistics.median(td) / statistics.median(tb), 2)
    if alt:
        res["B_per_lane_copy"] = rate(tl)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="records of 64 KiB payloads")
    ap.add_argument("--c5-records", type=int, default=1024, help="records of the C5 mix")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--name-len", type=int, default=None, help="0 ... 256: every name this long (default: 17, the generator's)")
    ap.add_argument("--alt", action="store_true", help="also time B with the per-lane byte copy (dents_copy=1)")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    if args.records:
        stored, plain = build([105] * args.records, 700000, args.name_len)
        measure("64KiB", stored, plain, args.rounds, args.alt, args.name_len)
    if args.c5_records:
        ites = np.random.default_rng(5).integers(1, 1025, args.c5_records)
        stored, plain = build(ites, 100000, args.name_len)
        measure("C5", stored, plain, args.rounds, args.alt, args.name_len)


if __name__ == "__main__":
    main()
