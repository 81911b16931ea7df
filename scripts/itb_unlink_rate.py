#!/usr/bin/env python3
"""ITB unlink over stored records: one batch on the GPU against what a caller
had before it.

Two paths over one seeded set of `--records` COMPR_LZO ITB records of 64 KiB
payloads (105 ITEs, adepth 10, built as check_rate.py builds them; every ITE an
active ITE_FLAG_NORMAL file with nlink 1) and `--requests` unlinks by uuid of
distinct ITEs of each, in one process, alternating, each warmed up, for
async_unlink 0 and 1:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the unlinks by
     itb_unlink.h's serial form compiled for the host
     (tests/native/libitb_unlink_host.so) on `--threads` threads, then
     pom_itb_lzo_compress_batch: the three calls are timed; the header fields
     the codec reads (len, compress_algo) are set between them, outside the
     timing
  B  pom_itb_unlink_batch: decode, check, unlink and encode on the GPU; only
     the requests' answers, the results and the stored records come back
Both produce the same answers, results and stored payloads (checked once,
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

from pomegranate_amd import check, gc, itb, lookup, lzo, unlink  # noqa: E402
from check_rate import make_records  # noqa: E402

H = itb.ITBH_SIZE


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="payloads of 64 KiB")
    ap.add_argument("--requests", type=int, default=8, help="per record")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    return ap.parse_args()


def build(n, k, per, seed0):
    """make_records with every ITE an active NORMAL file of nlink 1 and mode
    0100644, compressed on the GPU, and `per` requests by uuid for distinct
    ITEs of each record, grouped by record: (COMPR_LZO records, decoded payload
    lengths, REQ_DTYPE requests)."""
    recs = make_records([k] * n, seed0)
    rng = np.random.default_rng(seed0)
    req = np.zeros(n * per, dtype=lookup.REQ_DTYPE)
    for b, r in enumerate(recs):
        ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(k, gc.ITE_SIZE)
        ites[:, 16:20] = np.frombuffer(np.uint32(unlink.ITE_FLAG_NORMAL).tobytes(), np.uint8)
        ites[:, 36:40] = np.frombuffer(np.array([0o100644, 1], "<u2").tobytes(), np.uint8)
        ites[:, 8:16] = (np.arange(k, dtype="<u8") + 1000).view(np.uint8).reshape(k, 8)
        picks = rng.choice(k, per, replace=False)
        rows = req[b * per: (b + 1) * per]
        rows["hash"] = ites[picks, :8].copy().view("<u8")[:, 0]
        rows["uuid"] = picks.astype(np.uint64) + 1000
        rows["itb"] = b
        rows["flag"] = lookup.LK_BY_UUID | unlink.UL_UNLINK
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored], req


def main():
    args = parse()
    lib = unlink._lib()
    itb._lib()
    n, per, threads = args.records, args.requests, args.threads
    stored, plain, req = build(n, 105, per, 710000)
    assert len(set(plain)) == 1
    pl, nreq = plain[0], n * per
    P = 8                               # a record's place in its row, so that its payload lies at a multiple of 16
    slot = (P + H + pl + 15) // 16 * 16
    assert (P + H) % 16 == 0
    z = [len(s) - H for s in stored]
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_unlink_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    host.itb_unlink_batch_host.restype = None
    host.itb_unlink_batch_host.argtypes = [vp] * 6 + [u32, ctypes.c_int, vp, vp, vp, u32, ctypes.c_int] + [vp] * 6
    keep = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    blob = np.zeros(1, np.uint8)
    # B
    ptr_b = (vp * n)(*[k.ctypes.data for k in keep])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    out_b = np.zeros((n, slot), np.uint8)
    po = (vp * n)(*[out_b[b].ctypes.data for b in range(n)])
    caps = (ctypes.c_size_t * n)(*([H + pl] * n))
    ol = (ctypes.c_size_t * n)()
    res_b = np.zeros(n, dtype=unlink.RESULT_DTYPE)
    ierr_b, ok_b = np.zeros(n, np.int32), np.zeros(n, np.int32)
    words_b = np.zeros((4, nreq), np.uint32)
    rec_b = np.zeros((nreq, 136), np.uint8)
    # A: records decoded in place, unlinked there, then through the codec
    a = np.zeros((n, slot), np.uint8)
    tmp = np.zeros((n, H + lzo.worst_compress(pl)), np.uint8)
    ptr_a = (vp * n)(*[a[b].ctypes.data + P for b in range(n)])
    cap_a = (ctypes.c_size_t * n)(*([H + pl] * n))
    err_a, ok_a = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    ptmp = (vp * n)(*[tmp[b].ctypes.data for b in range(n)])
    ctmp = (ctypes.c_size_t * n)(*([tmp.shape[1]] * n))
    oi, cerr = (vp * n)(), (ctypes.c_int * n)()
    offs = np.arange(n, dtype=np.uint64) * np.uint64(slot) + np.uint64(P + H)
    lens = np.full(n, pl, np.uint32)
    adepth = np.full(n, 10, np.uint8)
    hdr = np.concatenate([check.header_facts(s) for s in stored])
    res_a = np.zeros(n, dtype=unlink.RESULT_DTYPE)
    words_a = np.zeros((4, nreq), np.uint32)
    rec_a = np.zeros((nreq, 136), np.uint8)
    cut = [(i * n // threads, (i + 1) * n // threads) for i in range(threads)]
    # (a thread's part is a call of its own: its ITBs and groups are numbered from 0)
    req_part, first_part = [], []
    for lo, hi in cut:
        q = req[lo * per: hi * per].copy()
        q["itb"] -= lo
        req_part.append(q)
        first_part.append(np.arange(hi - lo + 1, dtype=np.uint32) * per)

    def part(i, async_):
        lo, hi = cut[i]
        w = [words_a[k, lo * per:].ctypes.data for k in range(4)]
        host.itb_unlink_batch_host(a.ctypes.data, offs[lo:].ctypes.data, lens[lo:].ctypes.data, None,
                                   adepth[lo:].ctypes.data, hdr[lo:].ctypes.data, hi - lo, async_,
                                   req_part[i].ctypes.data, first_part[i].ctypes.data, blob.ctypes.data, 0, 0, *w,
                                   rec_a[lo * per:].ctypes.data, res_a[lo:].ctypes.data)

    def run_a(pool, async_):
        for b, s in enumerate(keep):
            a[b, P: P + s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        assert rc == 0 and not any(err_a) and all(ok_a)
        t2 = time.perf_counter()
        list(pool.map(lambda i: part(i, async_), range(threads)))
        t3 = time.perf_counter()
        assert not res_a["err"].any() and res_a["changed"].all()
        # (untimed) what the codec reads of the header: len, COMPR_NONE
        a[:, P + 240: P + 244] = res_a["len"].astype("<u4").view(np.uint8).reshape(n, 4)
        a[:, P + 248: P + 250] = 0
        t4 = time.perf_counter()
        rc = lib.pom_itb_lzo_compress_batch(ptr_a, ptmp, ctmp, oi, cerr, n)
        t5 = time.perf_counter()
        assert rc == 0 and not any(cerr)
        return (t1 - t0) + (t3 - t2) + (t5 - t4), t1 - t0, t3 - t2, t5 - t4

    def run_b(async_):
        t0 = time.perf_counter()
        rc = lib.pom_itb_unlink_batch(ptr_b, len_b, n, 0, async_, req.ctypes.data, nreq, blob.ctypes.data, 0,
                                      rec_b.ctypes.data, *(words_b[k].ctypes.data for k in range(4)), po, caps, ol,
                                      res_b.ctypes.data, ierr_b.ctypes.data, ok_b.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0 and not ierr_b.any() and ok_b.all() and not words_b[0].any()
        return dt

    ms = lambda ts: {"median_ms": round(statistics.median(ts) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2),
                     "max_ms": round(max(ts) * 1e3, 2)}
    al = lambda v: int(sum((int(x) + 15) // 16 * 16 for x in v))
    out = {"date": datetime.date.today().isoformat(), "records": n, "requests": nreq, "decoded_bytes": int(n * pl),
           "compressed_bytes": int(sum(z)), "rounds": args.rounds, "host_threads": threads}
    with ThreadPoolExecutor(threads) as pool:
        for async_ in (0, 1):
            run_a(pool, async_), run_b(async_), run_a(pool, async_), run_b(async_)      # warm-up
            assert res_a.tobytes() == res_b.tobytes(), "the two paths' results disagree"
            assert words_a.tobytes() == words_b.tobytes() and rec_a.tobytes() == rec_b.tobytes(), \
                "the two paths' answers disagree"
            assert int(res_b["removed"].sum()) == (0 if async_ else nreq)
            for b in range(0, n, max(1, n // 64)):                                      # a sample of the stored payloads
                rec = tmp[b] if oi[b] == ptmp[b] else a[b][P:]
                assert int.from_bytes(rec[240:244].tobytes(), "little") == ol[b], "the two paths' record lengths disagree"
                assert (rec[H:ol[b]] == out_b[b][H:ol[b]]).all(), "the two paths' stored payloads disagree"
            ta, tb, parts = [], [], []
            for _ in range(args.rounds):
                r = run_a(pool, async_)
                ta.append(r[0])
                parts.append(r[1:])
                tb.append(run_b(async_))
            u = res_b["len"].astype(np.int64) - H
            s = np.maximum(np.array(list(ol), np.int64) - H, 0)
            out[f"async_{async_}"] = {
                "removed": int(res_b["removed"].sum()), "changed": int(res_b["changed"].sum()),
                "A_decode_hostunlink_encode": dict(ms(ta), decode=ms([p[0] for p in parts]),
                                                   host_unlink=ms([p[1] for p in parts]),
                                                   encode=ms([p[2] for p in parts]),
                                                   h2d_bytes=al(z) + al(u) + 48 * 2 * n,
                                                   d2h_bytes=al(plain) + al(s) + 8 * 2 * n),
                "B_unlink_batch": dict(ms(tb), h2d_bytes=al(z) + (32 + 1 + 8 * 6 + 4 * 7 + 20) * n + 4 * (n + 1) + 32 * nreq,
                                       d2h_bytes=(8 + 32 + 8) * n + (16 + 136) * nreq + al(s)),
                "A_over_B": round(statistics.median(ta) / statistics.median(tb), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
