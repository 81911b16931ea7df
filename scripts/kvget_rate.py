#!/usr/bin/env python3
"""Key/value point gets: decode-and-copy-back against decode-and-get-on-the-GPU.

Two paths over one seeded set of COMPR_LZO ITB records of an xTable (105
entries each, NORMAL keys, values of `--vlen` bytes), in one process,
alternating, each warmed up first:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the host's own
     walk (itb_kvget.h from tests/native/libitb_kvget_host.so, one C call over
     the batch): what a caller does without pom_kvget_batch.  The decode alone
     is timed too (A without its walk).
  B  pom_kvget_batch: decode, chain walk, match and record copy on the GPU;
     only the fixed-size results and the packed records come back
Both produce the same results (checked once, outside the timing).  At 1, 8 and
64 gets per ITB (`--per-itb`), with or without a column (`--column`).  Rates are
requests per second, median and min ... max over `--rounds` alternating rounds;
the bytes each path copies each way are computed from the lengths: B's D2H is
first[nreq] record bytes plus 24 bytes a request (err, nr, depth, len, lease)
plus one 8-byte total a chunk.  Only the C calls are timed.  Prints one JSON
line per gets-per-ITB count.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pomegranate_amd import gc, itb, kvget, lookup, lzo  # noqa: E402
from lookup_rate import index_table  # noqa: E402

H = itb.ITBH_SIZE


def build(n_records, n_ites, vlen, seed0):
    """COMPR_LZO records (compressed on the GPU) with adepth 10 whose ITEs are
    NORMAL key/value entries: v.key = the ITE's hash, v.len = vlen, the value
    what the generator left there; the index table is the one __itb_add_index
    builds from the keys.  Returns (stored, decoded payload lengths, keys)."""
    recs, keys = [], []
    for i in range(n_records):
        r = itb.make_record(seed0 + i, n_ites)
        r = r[: itb.header_fields(r)[0]]
        r[lookup.ITBH_FLAG_OFF], r[lookup.ITBH_DEPTH_OFF], r[3] = 0, 0, 10
        r[4:8] = n_ites.to_bytes(4, "little")
        bm = bytearray(128)
        for nr in range(n_ites):
            bm[nr // 8] |= 1 << (nr % 8)
        r[H + gc.BITMAP_OFF: H + gc.INDEX_OFF] = bm
        ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(n_ites, gc.ITE_SIZE)
        ites[:, 24:28] = np.frombuffer(np.uint32(kvget.KV_NORMAL).tobytes(), dtype=np.uint8)
        ites[:, 28:32] = np.frombuffer(np.uint32(vlen).tobytes(), dtype=np.uint8)
        ites[:, 32:40] = ites[:, 0:8]
        ks = ites[:, :8].copy().view("<u8")[:, 0].tolist()
        r[H + gc.INDEX_OFF: H + gc.ITE_OFF] = index_table(ks).tobytes()
        keys.append(ks)
        recs.append(r)
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored], keys, recs


def device_launches(recs, keys, per_itb, column, launches):
    """pom_kvget_dev over the decoded payloads in HBM, every request in ONE
    launch of each kernel (the host batch cuts a call into chunks): for a
    kernel trace of find, prefix and emit at the full request count."""
    import torch
    dev = torch.device("cuda:0")
    n = len(recs)
    flag = kvget.KG_KV | kvget.KG_LOOKUP | (kvget.KG_COLUMN if column else 0)
    items = [dict(itb=b, key=ks[(j * 37) % len(ks)], flag=flag, kvflag=kvget.KV_NORMAL | (j % 6 if column else 0))
             for b, ks in enumerate(keys) for j in range(per_itb)]
    req, _ = kvget.requests(items)
    nreq = len(req)
    sizes = np.array([len(r) - H for r in recs], dtype=np.int64)
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum((sizes[:-1] + 15) // 16 * 16)
    arena = np.zeros(int(off[-1] + sizes[-1]), dtype=np.uint8)
    for o, r in zip(off, recs):
        arena[int(o): int(o) + len(r) - H] = np.frombuffer(r, dtype=np.uint8)[H:]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    src = lzo.DeviceBatch(t(arena), t(off), t(sizes.astype(np.int32)))
    adepth = torch.full((n,), 10, dtype=torch.uint8, device=dev)
    dreq = t(req.view(np.uint8))
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device=dev)
    err, nr, depth, ln, lease, first = i32(nreq), i32(nreq), i32(nreq), i32(nreq), i64(nreq), i64(nreq + 1)
    cap = kvget.KG_REC_MAX * nreq
    out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    for _ in range(launches):
        kvget.kvget_dev(src, adepth, dreq, nreq, None, 0, err, nr, depth, ln, lease, first, out, cap)
    torch.cuda.synchronize()
    assert not err.any().item()
    print(json.dumps({"device_launches": launches, "gets": nreq, "record_bytes": int(first[-1].item()) // nreq}),
          flush=True)


def measure(stored, plain, keys, per_itb, column, rounds):
    lib = kvget._lib()
    itb._lib()
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_kvget_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    host.itb_kvget_batch_host.restype = ctypes.c_int
    host.itb_kvget_batch_host.argtypes = [vp] * 5 + [u32, vp, u32, vp, u32] + [vp] * 7 + [ctypes.c_uint64, ctypes.c_int]
    n = len(stored)
    z = [len(s) - H for s in stored]
    flag = kvget.KG_KV | kvget.KG_LOOKUP | (kvget.KG_COLUMN if column else 0)
    items = [dict(itb=b, key=ks[(j * 37) % len(ks)], flag=flag, kvflag=kvget.KV_NORMAL | (j % 6 if column else 0))
             for b, ks in enumerate(keys) for j in range(per_itb)]
    req, _ = kvget.requests(items)
    nreq = len(req)
    cap = kvget.KG_REC_MAX * nreq
    mk = lambda: (np.zeros(nreq, np.int32), np.zeros(nreq, np.uint32), np.zeros(nreq, np.uint32),
                  np.zeros(nreq, np.uint32), np.zeros(nreq, np.uint64), np.zeros(nreq + 1, np.uint64),
                  np.zeros(cap, np.uint8))
    res_a, res_b = mk(), mk()
    keep_b = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep_b])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
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
    p = lambda a: a.ctypes.data

    def run_a():
        for b, s in zip(bufs, keep_b):
            b[: s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        e, nr, d, ln, ls, first, out = res_a
        rw = host.itb_kvget_batch_host(p(arena), p(pay_off), p(len_a), None, p(adepth), n, p(req), nreq, None, 0,
                                       p(e), p(nr), p(d), p(ln), p(ls), p(first), p(out), cap, 0)
        t2 = time.perf_counter()
        assert rc == 0 and rw == 0 and not any(err_a) and all(ok_a)
        return t2 - t0, t1 - t0

    def run_b():
        e, nr, d, ln, ls, first, out = res_b
        t0 = time.perf_counter()
        rc = lib.pom_kvget_batch(ptr_b, len_b, n, 0, p(req), nreq, None, 0, p(out), cap, p(first), p(e), p(nr), p(d),
                                 p(ln), p(ls))
        dt = time.perf_counter() - t0
        assert rc == 0 and not e.any()
        return dt

    run_a(), run_b(), run_a(), run_b()                           # warm-up: staging grown on both paths
    assert all((a == b).all() for a, b in zip(res_a, res_b)), "the two paths disagree"
    ta, td, tb = [], [], []
    for _ in range(rounds):
        both, decode = run_a()
        ta.append(both)
        td.append(decode)
        tb.append(run_b())
    rate = lambda ts: {"median_req_per_s": round(nreq / statistics.median(ts)),
                       "min_req_per_s": round(nreq / max(ts)), "max_req_per_s": round(nreq / min(ts)),
                       "median_ms": round(1e3 * statistics.median(ts), 3)}
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    total = int(res_b[5][nreq])
    d2h_a = aligned(plain) + 8 * n
    d2h_b = total + 24 * nreq
    res = {"records": n, "gets_per_itb": per_itb, "gets": nreq, "record_bytes": total // max(nreq, 1),
           "decoded_bytes": int(sum(plain)), "compressed_bytes": int(sum(z)),
           "mean_depth": round(float(res_b[2].mean()), 2), "rounds": rounds,
           "A_decompress_batch_then_host_walk": dict(rate(ta), h2d_bytes=aligned(z) + 48 * n, d2h_bytes=d2h_a),
           "A_decompress_batch_alone": rate(td),
           "B_kvget_batch": dict(rate(tb), h2d_bytes=aligned(z) + 41 * n + 32 * nreq,
                                 d2h_bytes=d2h_b, d2h_note="first[nreq] + 24 a request (+ 8 a chunk)"),
           "d2h_ratio": round(d2h_a / d2h_b, 1),
           "B_over_A": round(statistics.median(ta) / statistics.median(tb), 2),
           "B_over_A_decode_alone": round(statistics.median(td) / statistics.median(tb), 2)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="ITBs of 105 entries")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--per-itb", type=int, nargs="+", default=[1, 8, 64], help="gets per ITB")
    ap.add_argument("--vlen", type=int, default=40, help="v.len of every entry (0 ... 320)")
    ap.add_argument("--column", action="store_true", help="every get asks for a column")
    ap.add_argument("--dev", type=int, default=0, metavar="LAUNCHES",
                    help="instead: this many pom_kvget_dev calls over the decoded payloads, all gets in one launch")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    stored, plain, keys, recs = build(args.records, 105, args.vlen, 700000)
    if args.dev:
        for per in args.per_itb:
            device_launches(recs, keys, per, args.column, args.dev)
        return
    for per in args.per_itb:
        measure(stored, plain, keys, per, args.column, args.rounds)


if __name__ == "__main__":
    main()
