#!/usr/bin/env python3
"""ITB sweep over stored records: one batch on the GPU against what a caller
had before it.

Two paths over one seeded set of `--records` COMPR_LZO ITB records of 64 KiB
payloads (105 ITEs, adepth 10, built as check_rate.py builds them; a seeded
half of the ITEs is in state ITE_UNLINKED, the rest in states that never
sweep), in one process, alternating, each warmed up:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the sweep by
     itb_sweep.h's serial loop compiled for the host
     (tests/native/libitb_sweep_host.so) on `--threads` threads, then
     pom_itb_lzo_compress_batch: the three calls are timed; the header fields
     the codec reads (len, compress_algo) are set between them, outside the
     timing
  B  pom_itb_sweep_batch: decode, check, sweep and encode on the GPU; only
     results and stored records come back
Both produce the same results and the same stored payloads (checked once,
outside the timing).  Medians and min ... max over `--rounds` alternating
rounds; the bytes each path copies each way are computed from the lengths.
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import ctypes
import datetime
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from pomegranate_amd import check, gc, itb, itbsweep, lzo  # noqa: E402
from check_rate import make_records  # noqa: E402

H = itb.ITBH_SIZE
ITE_FLAG_OFF = 16
OTHER_STATES = np.array([0, 2, 3, 5, 7], dtype=np.uint32)


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="payloads of 64 KiB")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--fraction", type=float, default=0.5, help="of the ITEs in state ITE_UNLINKED")
    return ap.parse_args()


def build(n, k, fraction, seed0):
    """make_records with every ITE's state bits set (the other 29 flag bits
    stay), compressed on the GPU: (COMPR_LZO records, decoded payload lengths,
    marked ITEs)."""
    recs = make_records([k] * n, seed0)
    rng = np.random.default_rng(seed0)
    marked = 0
    for r in recs:
        ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(k, gc.ITE_SIZE)
        flags = ites[:, ITE_FLAG_OFF: ITE_FLAG_OFF + 4].copy().view("<u4")[:, 0]
        mark = rng.random(k) < fraction
        state = np.where(mark, np.uint32(itbsweep.ITE_UNLINKED), rng.choice(OTHER_STATES, k))
        flags = (flags & ~np.uint32(itbsweep.ITE_STATE_MASK)) | state.astype(np.uint32)
        ites[:, ITE_FLAG_OFF: ITE_FLAG_OFF + 4] = flags.astype("<u4").view(np.uint8).reshape(k, 4)
        marked += int(mark.sum())
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored], marked


def main():
    args = parse()
    lib = itbsweep._lib()
    itb._lib()
    n, threads = args.records, args.threads
    stored, plain, marked = build(n, 105, args.fraction, 700000)
    assert len(set(plain)) == 1
    pl = plain[0]
    P = 8                               # a record's place in its row, so that its payload lies at a multiple of 16
    slot = (P + H + pl + 15) // 16 * 16
    assert (P + H) % 16 == 0
    z = [len(s) - H for s in stored]
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_sweep_host.so"))
    host.itb_sweep_batch_host.restype = None
    host.itb_sweep_batch_host.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint32, ctypes.c_int] + [ctypes.c_void_p] * 2
    keep = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    # B
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    out_b = np.zeros((n, slot), np.uint8)
    po = (ctypes.c_void_p * n)(*[out_b[b].ctypes.data for b in range(n)])
    caps = (ctypes.c_size_t * n)(*([H + pl] * n))
    ol = (ctypes.c_size_t * n)()
    res_b = np.zeros(n, dtype=itbsweep.RESULT_DTYPE)
    err_b, ok_b = np.zeros(n, np.int32), np.zeros(n, np.int32)
    # A: records decoded in place, swept there, then through the codec
    a = np.zeros((n, slot), np.uint8)
    tmp = np.zeros((n, H + lzo.worst_compress(pl)), np.uint8)
    ptr_a = (ctypes.c_void_p * n)(*[a[b].ctypes.data + P for b in range(n)])
    cap_a = (ctypes.c_size_t * n)(*([H + pl] * n))
    err_a, ok_a = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    ptmp = (ctypes.c_void_p * n)(*[tmp[b].ctypes.data for b in range(n)])
    ctmp = (ctypes.c_size_t * n)(*([tmp.shape[1]] * n))
    oi, cerr = (ctypes.c_void_p * n)(), (ctypes.c_int * n)()
    offs = np.arange(n, dtype=np.uint64) * np.uint64(slot) + np.uint64(P + H)
    lens = np.full(n, pl, np.uint32)
    adepth = np.full(n, 10, np.uint8)
    hdr = np.concatenate([check.header_facts(s) for s in stored])
    res_a, steps = np.zeros(n, dtype=itbsweep.RESULT_DTYPE), np.zeros(n, np.uint32)
    cut = [(i * n // threads, (i + 1) * n // threads) for i in range(threads)]

    def part(lo_hi):
        lo, hi = lo_hi
        host.itb_sweep_batch_host(a.ctypes.data, offs[lo:].ctypes.data, lens[lo:].ctypes.data, None,
                                  adepth[lo:].ctypes.data, hdr[lo:].ctypes.data, None, hi - lo, 0,
                                  res_a[lo:].ctypes.data, steps[lo:].ctypes.data)

    def run_a(pool):
        for b, s in enumerate(keep):
            a[b, P: P + s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        assert rc == 0 and not any(err_a) and all(ok_a)
        t2 = time.perf_counter()
        list(pool.map(part, cut))
        t3 = time.perf_counter()
        assert not res_a["err"].any() and (res_a["removed"].all() or args.fraction == 0)
        # (untimed) what the codec reads of the header: len, COMPR_NONE
        a[:, P + 240: P + 244] = np.where(res_a["removed"] > 0, res_a["len"], H + pl).astype("<u4").view(np.uint8).reshape(n, 4)
        a[:, P + 248: P + 250] = 0
        t4 = time.perf_counter()
        rc = lib.pom_itb_lzo_compress_batch(ptr_a, ptmp, ctmp, oi, cerr, n)
        t5 = time.perf_counter()
        assert rc == 0 and not any(cerr)
        return (t1 - t0) + (t3 - t2) + (t5 - t4), t1 - t0, t3 - t2, t5 - t4

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_itb_sweep_batch(ptr_b, len_b, n, None, po, caps, ol, res_b.ctypes.data, err_b.ctypes.data,
                                     ok_b.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err_b.any() and ok_b.all()
        return dt

    with ThreadPoolExecutor(threads) as pool:
        run_a(pool), run_b(), run_a(pool), run_b()                                  # warm-up
        assert res_a.tobytes() == res_b.tobytes(), "the two paths' results disagree"
        assert int(res_b["removed"].sum()) == marked
        for b in range(0, n, max(1, n // 64)):                                      # a sample of the stored payloads
            if res_b["removed"][b] == 0:
                continue
            rec = tmp[b] if oi[b] == ptmp[b] else a[b][P:]
            assert int.from_bytes(rec[240:244].tobytes(), "little") == ol[b], "the two paths' record lengths disagree"
            assert (rec[H:ol[b]] == out_b[b][H:ol[b]]).all(), "the two paths' stored payloads disagree"
        ta, tb, parts = [], [], []
        for _ in range(args.rounds):
            r = run_a(pool)
            ta.append(r[0])
            parts.append(r[1:])
            tb.append(run_b())
    ms = lambda ts: {"median_ms": round(statistics.median(ts) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2),
                     "max_ms": round(max(ts) * 1e3, 2)}
    al = lambda v: int(sum((int(x) + 15) // 16 * 16 for x in v))
    u = np.where(res_b["removed"] > 0, res_b["len"].astype(np.int64) - H, 0)
    s = np.maximum(np.array(list(ol), np.int64) - H, 0)
    out = {"date": datetime.date.today().isoformat(), "records": n, "decoded_bytes": int(n * pl),
           "compressed_bytes": int(sum(z)), "marked": marked, "removed": int(res_b["removed"].sum()),
           "dc": int(res_b["dc"].sum()), "rounds": args.rounds, "host_threads": threads,
           "A_decode_hostsweep_encode": dict(ms(ta), decode=ms([p[0] for p in parts]),
                                             host_sweep=ms([p[1] for p in parts]), encode=ms([p[2] for p in parts]),
                                             h2d_bytes=al(z) + al(u) + 48 * 2 * n,
                                             d2h_bytes=al(plain) + al(s) + 8 * 2 * n),
           "B_sweep_batch": dict(ms(tb), h2d_bytes=al(z) + (32 + 1 + 8 * 6 + 4 * 7 + 20) * n,
                                 d2h_bytes=(8 + 32 + 8) * n + al(s)),
           "A_over_B": round(statistics.median(ta) / statistics.median(tb), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
