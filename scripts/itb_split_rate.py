#!/usr/bin/env python3
"""ITB split over stored records: one batch on the GPU against what a caller
had before it.

Two paths over one seeded set of `--records` COMPR_LZO ITB records of 64 KiB
payloads (105 ITEs, adepth 10, built as check_rate.py builds them; about half
the ITEs move at split depth 1), in one process, alternating, each warmed up:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the split by
     itb_split.h compiled for the host (tests/native/libitb_split_host.so) on
     `--threads` threads, then pom_itb_lzo_compress_batch of both halves: the
     three calls are timed; the header fields the codec reads (len,
     compress_algo) are set between them, outside the timing
  B  pom_itb_split_batch: decode, check, split and encode of both halves on the
     GPU; only results and stored records come back
Both produce the same results and the same stored payloads (checked once,
outside the timing).  Medians and min ... max over `--rounds` alternating
rounds; the bytes each path copies each way are computed from the lengths.

--dev-entry is a side measurement, labelled as such in its output: the device
entry pom_itb_split_dev alone over payloads already decoded in HBM, in three
variants that differ in hash bit 10 alone (nothing, about half, everything
moves), against itb_split_one on the host; nothing crosses PCIe there and
neither decode nor encode is in it.  Prints one JSON line.
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

from pomegranate_amd import check, gc, itb, itbsplit, lzo  # noqa: E402
from check_rate import make_records  # noqa: E402

H = itb.ITBH_SIZE
VARIANTS = ("none", "half", "all")


def variant(arena, offs, n_ites, which):
    """A copy of the payload arena with hash bit 10 of every ITE cleared, kept or set."""
    out = arena.copy()
    if which != "half":
        for o in offs:
            at = int(o) + gc.ITE_OFF + 1                        # bits 8 ... 15 of the little-endian hash
            col = out[at: at + gc.ITE_SIZE * n_ites: gc.ITE_SIZE]
            col[:] = (col & 0xFB) if which == "none" else (col | 0x04)
    return out


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="payloads of 64 KiB")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dev-entry", action="store_true", help="the side measurement of pom_itb_split_dev alone")
    return ap.parse_args()


def dev_entry(args):
    import torch
    assert torch.cuda.is_available(), "the rate script needs a GPU"
    dev = torch.device("cuda:0")
    n, k = args.records, 105
    recs = make_records([k] * n, 700000)
    plen = len(recs[0]) - H
    assert all(len(r) - H == plen for r in recs) and plen % 16 == 0
    offs = np.arange(n, dtype=np.uint64) * np.uint64(plen)
    base = np.concatenate([np.frombuffer(r, dtype=np.uint8)[H:] for r in recs])
    hdr = np.concatenate([check.header_facts(r) for r in recs])
    lens = np.full(n, plen, dtype=np.uint32)
    adepth = np.full(n, 10, dtype=np.uint8)
    sd = np.full(n, 1, dtype=np.uint8)

    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_split_host.so"))
    host.itb_split_batch_host.restype = None
    host.itb_split_batch_host.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint32] + [ctypes.c_void_p] * 5

    def run_host(payload, new, result, steps):
        """-> seconds; slices of the batch on the pool's threads (ctypes drops the
        GIL).  result: RESULT_DTYPE per ITB, so that a slice starts at its ITB."""
        cut = [(i * n // args.threads, (i + 1) * n // args.threads) for i in range(args.threads)]

        def part(lo_hi):
            lo, hi = lo_hi
            host.itb_split_batch_host(payload.ctypes.data, offs[lo:].ctypes.data, lens[lo:].ctypes.data, None,
                                      adepth[lo:].ctypes.data, hdr[lo:].ctypes.data, sd[lo:].ctypes.data, hi - lo,
                                      new.ctypes.data, offs[lo:].ctypes.data, lens[lo:].ctypes.data,
                                      result[lo:].ctypes.data, steps[lo:].ctypes.data)
        t0 = time.perf_counter()
        list(pool.map(part, cut))
        return time.perf_counter() - t0

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_off, d_len, d_ad, d_sd = t(offs.view(np.int64)), t(lens.view(np.int32)), t(adepth), t(sd)
    d_hdr = t(hdr.view(np.uint8))
    d_new = torch.zeros(n * plen, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(48 * n, dtype=torch.uint8, device=dev)
    d_rep = torch.zeros(48 * n, dtype=torch.uint8, device=dev)
    d_err = torch.zeros(n, dtype=torch.int32, device=dev)
    d_scr = torch.empty(itbsplit.split_scratch_bytes(n), dtype=torch.uint8, device=dev)
    d_work = torch.zeros(n * plen, dtype=torch.uint8, device=dev)
    work = lzo.DeviceBatch(d_work, d_off, d_len)
    newb = lzo.DeviceBatch(d_new, d_off, d_len)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run_dev(pristine, split):
        d_work.copy_(pristine)
        torch.cuda.synchronize()
        e0.record()
        if split:
            itbsplit.split_dev(work, d_ad, d_hdr, newb, d_res, d_scr, split_depth=d_sd)
        else:
            check.check_dev(work, d_ad, d_rep, d_err, hdr=d_hdr)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    out = {"what": "side measurement: pom_itb_split_dev alone, payloads resident in HBM, no decode, encode or PCIe",
           "date": datetime.date.today().isoformat(), "records": n, "ites": k, "payload_bytes": int(n * plen),
           "rounds": args.rounds, "host_threads": args.threads}
    with ThreadPoolExecutor(args.threads) as pool:
        for which in VARIANTS:
            image = variant(base, offs, k, which)
            pristine = t(image)
            h_new, h_res = np.zeros(n * plen, np.uint8), np.zeros(n, dtype=itbsplit.RESULT_DTYPE)
            h_steps = np.zeros(n, np.uint32)
            h_pay = image.copy()
            run_host(h_pay, h_new, h_res, h_steps)
            run_dev(pristine, True), run_dev(pristine, False), run_dev(pristine, True)        # warm-up
            res = np.frombuffer(d_res.cpu().numpy().tobytes(), dtype=itbsplit.RESULT_DTYPE)
            assert d_res.cpu().numpy().tobytes() == h_res.tobytes(), f"{which}: the two paths' results disagree"
            assert not res["err"].any()
            assert (d_work.cpu().numpy() == h_pay).all(), f"{which}: the two paths' old payloads disagree"
            moved = int(res["moved"].sum())
            if moved:
                got_new = d_new.cpu().numpy()
                for b in range(0, n, max(1, n // 64)):                                        # a sample of the new payloads
                    m = int(res["new_len"][b]) - H
                    o = int(offs[b])
                    assert (got_new[o: o + m] == h_new[o: o + m]).all(), "the two paths' new payloads disagree"
            td, tc, th = [], [], []
            for _ in range(args.rounds):
                td.append(run_dev(pristine, True))
                tc.append(run_dev(pristine, False))
                h_pay[:] = image
                th.append(run_host(h_pay, h_new, h_res, h_steps))
            ms = lambda ts: {"median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3),
                             "max_ms": round(max(ts) * 1e3, 3)}
            out[which] = {"moved": moved, "live": n * k,
                          "ite_bytes_copied": 512 * moved, "table_bytes": (8320 * 2 + 11904) * n if moved else 8320 * n,
                          "D_split_dev": ms(td), "D_check_dev_alone": ms(tc), "H_host_threads": ms(th),
                          "H_over_D": round(statistics.median(th) / statistics.median(td), 2)}
    print(json.dumps(out), flush=True)


def batch(args):
    from check_rate import build
    lib = itbsplit._lib()
    itb._lib()
    n, threads = args.records, args.threads
    stored, plain = build([105] * n, 700000)
    assert len(set(plain)) == 1
    pl = plain[0]
    P = 8                               # a record's place in its row, so that its payload lies at a multiple of 16
    slot = (P + H + pl + 15) // 16 * 16
    assert (P + H) % 16 == 0
    z = [len(s) - H for s in stored]
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_split_host.so"))
    host.itb_split_batch_host.restype = None
    host.itb_split_batch_host.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_uint32] + [ctypes.c_void_p] * 5
    keep = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    # B
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    out_o, out_n = np.zeros((n, slot), np.uint8), np.zeros((n, slot), np.uint8)
    po = (ctypes.c_void_p * n)(*[out_o[b].ctypes.data for b in range(n)])
    pn = (ctypes.c_void_p * n)(*[out_n[b].ctypes.data for b in range(n)])
    caps = (ctypes.c_size_t * n)(*([H + pl] * n))
    ol, nl = (ctypes.c_size_t * n)(), (ctypes.c_size_t * n)()
    res_b = np.zeros(n, dtype=itbsplit.RESULT_DTYPE)
    err_b, ok_b = np.zeros(n, np.int32), np.zeros(n, np.int32)
    # A: records decoded in place, new ITBs beside them, then 2n records through the codec
    a_o, a_n = np.zeros((n, slot), np.uint8), np.zeros((n, slot), np.uint8)
    tmp = np.zeros((2 * n, H + lzo.worst_compress(pl)), np.uint8)
    ptr_a = (ctypes.c_void_p * n)(*[a_o[b].ctypes.data + P for b in range(n)])
    cap_a = (ctypes.c_size_t * n)(*([H + pl] * n))
    err_a, ok_a = (ctypes.c_int * n)(), (ctypes.c_int * n)()
    pin = (ctypes.c_void_p * (2 * n))(*([a_o[b].ctypes.data + P for b in range(n)] +
                                       [a_n[b].ctypes.data + P for b in range(n)]))
    ptmp = (ctypes.c_void_p * (2 * n))(*[tmp[b].ctypes.data for b in range(2 * n)])
    ctmp = (ctypes.c_size_t * (2 * n))(*([tmp.shape[1]] * (2 * n)))
    oi, cerr = (ctypes.c_void_p * (2 * n))(), (ctypes.c_int * (2 * n))()
    offs = np.arange(n, dtype=np.uint64) * np.uint64(slot) + np.uint64(P + H)
    lens = np.full(n, pl, np.uint32)
    adepth, sd = np.full(n, 10, np.uint8), np.full(n, 1, np.uint8)
    hdr = np.concatenate([check.header_facts(s) for s in stored])
    res_a, steps = np.zeros(n, dtype=itbsplit.RESULT_DTYPE), np.zeros(n, np.uint32)
    cut = [(i * n // threads, (i + 1) * n // threads) for i in range(threads)]

    def part(lo_hi):
        lo, hi = lo_hi
        host.itb_split_batch_host(a_o.ctypes.data, offs[lo:].ctypes.data, lens[lo:].ctypes.data, None,
                                  adepth[lo:].ctypes.data, hdr[lo:].ctypes.data, sd[lo:].ctypes.data, hi - lo,
                                  a_n.ctypes.data, offs[lo:].ctypes.data, lens[lo:].ctypes.data,
                                  res_a[lo:].ctypes.data, steps[lo:].ctypes.data)

    def run_a(pool):
        for b, s in enumerate(keep):
            a_o[b, P: P + s.size] = s
        t0 = time.perf_counter()
        rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
        t1 = time.perf_counter()
        assert rc == 0 and not any(err_a) and all(ok_a)
        t2 = time.perf_counter()
        list(pool.map(part, cut))
        t3 = time.perf_counter()
        assert not res_a["err"].any() and res_a["moved"].all()
        # (untimed) what the codec reads of the two headers: len, COMPR_NONE
        a_n[:, P: P + H] = a_o[:, P: P + H]
        a_o[:, P + 240: P + 244] = res_a["old_len"].astype("<u4").view(np.uint8).reshape(n, 4)
        a_n[:, P + 240: P + 244] = res_a["new_len"].astype("<u4").view(np.uint8).reshape(n, 4)
        a_o[:, P + 248: P + 250] = 0
        a_n[:, P + 248: P + 250] = 0
        t4 = time.perf_counter()
        rc = lib.pom_itb_lzo_compress_batch(pin, ptmp, ctmp, oi, cerr, 2 * n)
        t5 = time.perf_counter()
        assert rc == 0 and not any(cerr)
        return (t1 - t0) + (t3 - t2) + (t5 - t4), t1 - t0, t3 - t2, t5 - t4

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_itb_split_batch(ptr_b, len_b, n, None, po, pn, caps, ol, nl, res_b.ctypes.data,
                                     err_b.ctypes.data, ok_b.ctypes.data)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err_b.any() and ok_b.all()
        return dt

    with ThreadPoolExecutor(threads) as pool:
        run_a(pool), run_b(), run_a(pool), run_b()                                  # warm-up
        assert res_a.tobytes() == res_b.tobytes(), "the two paths' results disagree"
        for b in range(0, n, max(1, n // 64)):                                      # a sample of the stored payloads
            for k, (mine, ln) in enumerate(((out_o[b], ol[b]), (out_n[b], nl[b]))):
                rec = tmp[k * n + b] if oi[k * n + b] == ptmp[k * n + b] else (a_o, a_n)[k][b][P:]
                assert int.from_bytes(rec[240:244].tobytes(), "little") == ln, "the two paths' record lengths disagree"
                assert (rec[H:ln] == mine[H:ln]).all(), "the two paths' stored payloads disagree"
        ta, tb, parts = [], [], []
        for _ in range(args.rounds):
            r = run_a(pool)
            ta.append(r[0])
            parts.append(r[1:])
            tb.append(run_b())
    ms = lambda ts: {"median_ms": round(statistics.median(ts) * 1e3, 2), "min_ms": round(min(ts) * 1e3, 2),
                     "max_ms": round(max(ts) * 1e3, 2)}
    al = lambda v: int(sum((int(x) + 15) // 16 * 16 for x in v))
    uo, un = res_b["old_len"].astype(np.int64) - H, res_b["new_len"].astype(np.int64) - H
    so, sn = np.array(list(ol), np.int64) - H, np.array(list(nl), np.int64) - H
    out = {"date": datetime.date.today().isoformat(), "records": n, "decoded_bytes": int(n * pl),
           "compressed_bytes": int(sum(z)), "moved": int(res_b["moved"].sum()), "rounds": args.rounds,
           "host_threads": threads,
           "A_decode_hostsplit_encode": dict(ms(ta), decode=ms([p[0] for p in parts]), host_split=ms([p[1] for p in parts]),
                                             encode=ms([p[2] for p in parts]),
                                             h2d_bytes=al(z) + al(uo) + al(un) + 48 * 3 * n,
                                             d2h_bytes=al(plain) + al(so) + al(sn) + 8 * 3 * n),
           "B_split_batch": dict(ms(tb), h2d_bytes=al(z) + (32 + 1 + 1 + 8 * 5 + 4 * 5 + 56) * n,
                                 d2h_bytes=(8 + 48 + 16) * n + al(so) + al(sn)),
           "A_over_B": round(statistics.median(ta) / statistics.median(tb), 2)}
    print(json.dumps(out), flush=True)


def main():
    args = parse()
    dev_entry(args) if args.dev_entry else batch(args)


if __name__ == "__main__":
    main()
