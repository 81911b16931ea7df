#!/usr/bin/env python3
"""Lookups: decode-and-copy-back against decode-and-search-on-the-GPU.

Two paths over one seeded set of COMPR_LZO ITB records, in one process,
alternating, each warmed up first:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the host walk
     (itb_find_one from tests/native/libitb_find_host.so, one C call over the
     batch): what an MDS linked against the library does today for cold
     lookups.  The decode alone is timed too (A without its walk).
  B  pom_lookup_batch: decode, chain walk and MDU copy on the GPU; only codes
     and 136-byte records come back
Both produce the same results (checked once, outside the timing).  Record sets:
`--records` records of 64 KiB payloads (105 ITEs), and the C5 mix (bench.py
run_c5: 1 ... 1024 ITEs, seed 5), each with an index table built the way
__itb_add_index builds it from the ITEs' hashes, at 1 and at 64 lookups by
name per ITB (the `ls -l` that follows a listing).  Rates are GiB/s of decoded
payload, median and min ... max over `--rounds` alternating rounds; the bytes
each path copies each way are computed from the lengths.  Only the C calls are
timed (pointer arrays are built before).  Prints one JSON line per set and
lookup count.
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

from pomegranate_amd import gc, itb, lookup, lzo  # noqa: E402

GIB = float(1 << 30)
H = itb.ITBH_SIZE


def index_table(hashes):
    """The table __itb_add_index (mds/itb.c:261-303) leaves after adding ITE 0,
    1, ... with these hashes to an empty adepth-10 ITB: overflow slots are
    handed out in order from 1024 (h.inf starts at 0 and nothing is freed)."""
    idx = [0] * 2048
    free = 1024
    for nr, hsh in enumerate(hashes):
        off = hsh & 1023
        w = idx[off]
        flag = w >> 30
        if flag == lookup.IDX_FREE:
            idx[off] = nr | lookup.IDX_UNIQUE << 30
        elif flag == lookup.IDX_UNIQUE:
            idx[off] = (w & 0x7FFF) | free << 15 | lookup.IDX_CONFLICT << 30
            idx[free] = nr | lookup.IDX_UNIQUE << 30
            free += 1
        else:
            idx[free] = w
            idx[off] = nr | free << 15 | lookup.IDX_CONFLICT << 30
            free += 1
    return np.array(idx, dtype="<u4")


def build(n_ites_list, seed0):
    """COMPR_LZO records (compressed on the GPU) with adepth 10, the first
    n_ites bitmap bits set and the index table of their ITEs' hashes; returns
    (stored, decoded payload lengths, per record the ITEs' (hash, name))."""
    recs, keys = [], []
    for i, k in enumerate(n_ites_list):
        k = int(k)
        r = itb.make_record(seed0 + i, k)
        r = r[: itb.header_fields(r)[0]]
        r[lookup.ITBH_FLAG_OFF], r[lookup.ITBH_DEPTH_OFF], r[3] = 0, 0, 10
        r[4:8] = k.to_bytes(4, "little")
        bm = bytearray(128)
        for nr in range(k):
            bm[nr // 8] |= 1 << (nr % 8)
        r[H + gc.BITMAP_OFF: H + gc.INDEX_OFF] = bm
        ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(k, gc.ITE_SIZE)
        hashes = ites[:, :8].copy().view("<u8")[:, 0].tolist()
        namelens = ites[:, 20:24].copy().view("<u4")[:, 0].tolist()
        r[H + gc.INDEX_OFF: H + gc.ITE_OFF] = index_table(hashes).tobytes()
        keys.append([(hashes[nr], ites[nr, 104: 104 + min(namelens[nr], 255)].tobytes()) for nr in range(k)])
        recs.append(r)
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored], keys


def measure(name, stored, plain, keys, per_itb, rounds):
    lib = lookup._lib()
    itb._lib()
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_find_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    host.itb_find_batch_host.restype = ctypes.c_int
    host.itb_find_batch_host.argtypes = [vp] * 5 + [u32, vp, u32, vp, u32] + [vp] * 4 + [ctypes.c_int]
    n = len(stored)
    total_plain = float(sum(plain))
    z = [len(s) - H for s in stored]
    items = []
    for b, ks in enumerate(keys):
        for j in range(per_itb):
            hsh, nm = ks[(j * 37) % len(ks)]
            items.append(dict(itb=b, hash=hsh, flag=lookup.LK_BY_NAME | lookup.LK_LOOKUP, name=nm))
    req, names = lookup.requests(items)
    nreq = len(req)
    blob = np.frombuffer(names, dtype=np.uint8)
    # B: read-only records
    keep_b = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep_b])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    out_b = np.zeros((nreq, lookup.REC_SIZE), dtype=np.uint8)
    err_b, nr_b, depth_b = np.zeros(nreq, np.int32), np.zeros(nreq, np.uint32), np.zeros(nreq, np.uint32)
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
    out_a = np.zeros((nreq, lookup.REC_SIZE), dtype=np.uint8)
    res_a = np.zeros((3, nreq), dtype=np.uint32)

    def run_a():
        for b, s in zip(bufs, keep_b):
            b[: s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        rw = host.itb_find_batch_host(arena.ctypes.data, pay_off.ctypes.data, len_a.ctypes.data, None,
                                      adepth.ctypes.data, n, req.ctypes.data, nreq, blob.ctypes.data, len(names),
                                      res_a[0].ctypes.data, res_a[1].ctypes.data, res_a[2].ctypes.data,
                                      out_a.ctypes.data, 0)
        t2 = time.perf_counter()
        assert rc == 0 and rw == 0 and not any(err_a) and all(ok_a)
        return t2 - t0, t1 - t0

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_lookup_batch(ptr_b, len_b, n, 0, req.ctypes.data, nreq, blob.ctypes.data, len(names),
                                  out_b.ctypes.data, err_b.ctypes.data, nr_b.ctypes.data, depth_b.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err_b.any()
        return dt

    run_a(), run_b(), run_a(), run_b()                           # warm-up: staging grown on both paths
    assert (res_a[0].view(np.int32) == err_b).all() and (res_a[1] == nr_b).all() and (res_a[2] == depth_b).all() \
        and (out_a == out_b).all(), "the two paths disagree"
    ta, td, tb = [], [], []
    for _ in range(rounds):
        both, decode = run_a()
        ta.append(both)
        td.append(decode)
        tb.append(run_b())
    rate = lambda ts: {"median_gibps": round(total_plain / statistics.median(ts) / GIB, 2),
                       "min_gibps": round(total_plain / max(ts) / GIB, 2),
                       "max_gibps": round(total_plain / min(ts) / GIB, 2)}
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    d2h_a = aligned(plain) + 8 * n
    d2h_b = (12 + lookup.REC_SIZE) * nreq
    res = {"set": name, "records": n, "lookups_per_itb": per_itb, "lookups": nreq,
           "decoded_bytes": int(total_plain), "compressed_bytes": int(sum(z)), "name_bytes": len(names),
           "mean_depth": round(float(depth_b.mean()), 2), "max_depth": int(depth_b.max()), "rounds": rounds,
           "A_decompress_batch_then_host_walk": dict(rate(ta), h2d_bytes=aligned(z) + 48 * n, d2h_bytes=d2h_a),
           "A_decompress_batch_alone": rate(td),
           "B_lookup_batch": dict(rate(tb), h2d_bytes=aligned(z) + 41 * n + 32 * nreq + len(names), d2h_bytes=d2h_b),
           "lookups_per_s_A": round(nreq / statistics.median(ta)), "lookups_per_s_B": round(nreq / statistics.median(tb)),
           "d2h_ratio": round(d2h_a / d2h_b, 1)}
    res["B_over_A"] = round(statistics.median(ta) / statistics.median(tb), 2)
    res["B_over_A_decode_alone"] = round(statistics.median(td) / statistics.median(tb), 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="records of 64 KiB payloads")
    ap.add_argument("--c5-records", type=int, default=1024, help="records of the C5 mix")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-itb", type=int, nargs="+", default=[1, 64], help="lookups per ITB")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    if args.records:
        stored, plain, keys = build([105] * args.records, 700000)
        for per in args.per_itb:
            measure("64KiB", stored, plain, keys, per, args.rounds)
    if args.c5_records:
        ites = np.random.default_rng(5).integers(1, 1025, args.c5_records)
        stored, plain, keys = build(ites, 100000)
        for per in args.per_itb:
            measure("C5", stored, plain, keys, per, args.rounds)


if __name__ == "__main__":
    main()
