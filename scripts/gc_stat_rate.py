#!/usr/bin/env python3
"""GC data stat: merge-on-the-GPU against scan-and-merge-on-the-host.

Two paths over one seeded set of COMPR_LZO ITB records whose columns are an
append log's (each ITE's offset is where the one before ended, a gap now and
then), in one process, alternating, each warmed up first:
  A  pom_gc_stat_batch: decode, walk, sort and merge on the GPU, only each
     chunk's merged map comes back, the chunks' maps folded on the host
  B  pom_gc_scan_batch: decode and walk on the GPU, every range comes back;
     then the merge on the host in numpy (argsort, maximum.accumulate, heads),
     checked equal to A
Record sets: `--records` records of 64 KiB payloads (105 ITEs), and the C5 mix
(1 ... 1024 ITEs, seed 5).  Times are milliseconds a call, median and min ...
max over `--rounds` alternating rounds; B's merge is timed apart as well.  The
D2H bytes of each path are read from one extra, untimed call with the
host_timing debug key.  Only the C calls and the numpy merge are timed
(pointer arrays are built before).  Prints one JSON line per set.

`--merge-dev N [N ...]`: pom_gc_merge_dev alone on N random ranges, for a
kernel trace (rocprofv3 --kernel-trace --stats -- python scripts/gc_stat_rate.py
--merge-dev 262144), with device-event times of the whole call.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pomegranate_amd import gc, itb, lzo  # noqa: E402

H = itb.ITBH_SIZE
U64 = np.uint64


def build(n_ites_list, seed0, column):
    """COMPR_LZO records (compressed on the GPU) with adepth 10, the first
    n_ites bitmap bits set and `column` of every ITE a piece of one append
    log; the records are shuffled.  Returns (stored, decoded lengths)."""
    rng = np.random.default_rng(seed0)
    recs, at = [], 4096
    for i, k in enumerate(n_ites_list):
        k = int(k)
        r = itb.make_record(seed0 + i, k)
        r = r[: itb.header_fields(r)[0]]
        r[3] = 10
        r[4:8] = k.to_bytes(4, "little")
        bm = bytearray(128)
        for nr in range(k):
            bm[nr // 8] |= 1 << (nr % 8)
        r[H + gc.BITMAP_OFF: H + gc.INDEX_OFF] = bm
        ln = rng.integers(1, 8192, k, dtype=U64)
        gap = (rng.integers(0, 50, k) == 0) * rng.integers(1, 4096, k, dtype=U64)
        off = U64(at) + np.concatenate([np.zeros(1, dtype=U64), np.cumsum(ln + U64(1) + gap, dtype=U64)[:-1]])
        at = int(off[-1] + ln[-1] + U64(1) + gap[-1])
        raw = np.stack([ln, off], axis=1).tobytes()
        for nr in range(k):
            o = H + gc.ITE_OFF + gc.ITE_SIZE * nr + gc.ITE_COLUMN_OFF + gc.COLUMN_SIZE * column + gc.COLUMN_LEN_OFF
            r[o: o + 16] = raw[16 * nr: 16 * nr + 16]
        recs.append(r)
    recs = [recs[i] for i in rng.permutation(len(recs))]
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored]


def host_merge(ranges):
    """The model's merge in numpy: (extents [k, 2], valid, max)."""
    keep = ranges[:, 1] > ranges[:, 0]
    k = ranges[keep]
    k = k[np.argsort(k[:, 0], kind="stable")]
    if len(k) == 0:
        return np.zeros((0, 2), dtype=U64), 0, 0
    runmax = np.maximum.accumulate(k[:, 1])
    head = np.ones(len(k), dtype=bool)
    head[1:] = k[1:, 0] > runmax[:-1]
    last = np.ones(len(k), dtype=bool)
    last[:-1] = head[1:]
    out = np.stack([k[head, 0], runmax[last]], axis=1)
    return out, int((out[:, 1] - out[:, 0]).sum(dtype=U64)), int(out[-1, 1])


def d2h_bytes(call, first_copy_per_block, first_copy_per_chunk):
    """One untimed call with host_timing=1: the chunks and the bytes of their
    second D2H copy are on stderr; the first copy's size follows from the
    chunk's blocks."""
    old = os.environ.get("POM_LZO_DEBUG")
    os.environ["POM_LZO_DEBUG"] = "host_timing=1"
    lzo.debug_reload()
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            if old is None:
                del os.environ["POM_LZO_DEBUG"]
            else:
                os.environ["POM_LZO_DEBUG"] = old
            lzo.debug_reload()
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    chunks = [(int(a), int(b)) for a, b in re.findall(r"deliver n=(\d+): wait [\d.]+ \((\d+) B\)", text)]
    assert chunks, "no chunk was reported"
    return {"chunks": len(chunks),
            "d2h_bytes": sum(first_copy_per_block * n + first_copy_per_chunk + b for n, b in chunks)}


def measure(name, stored, plain, column, rounds):
    lib = gc._lib()
    n = len(stored)
    keep = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
    lens = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    cap = 1024 * n
    ranges = np.zeros((cap, 2), dtype=U64)
    first = np.zeros(n + 1, dtype=U64)
    merged = np.zeros((cap, 2), dtype=U64)
    stat = np.zeros(5, dtype=U64)
    live = np.zeros(n, dtype=np.uint32)
    err = np.zeros(n, dtype=np.int32)
    b_out = {}

    def run_a():
        t0 = time.perf_counter()
        rc = lib.pom_gc_stat_batch(ptr, lens, n, column, None, 0, merged.ctypes.data, cap, stat.ctypes.data,
                                   live.ctypes.data, err.ctypes.data, None, None)
        dt = time.perf_counter() - t0
        assert rc == 0 and not err.any()
        return dt

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_gc_scan_batch(ptr, lens, n, column, ranges.ctypes.data, cap, first.ctypes.data,
                                   live.ctypes.data, err.ctypes.data, None, None)
        t1 = time.perf_counter()
        b_out["m"] = host_merge(ranges[: int(first[n])])
        t2 = time.perf_counter()
        assert rc == 0 and not err.any()
        return t2 - t0, t2 - t1

    run_a(), run_b(), run_a(), run_b()                           # warm-up: staging grown on both paths
    ta, tb, tm = [], [], []
    for _ in range(rounds):
        ta.append(run_a())
        b, m = run_b()
        tb.append(b)
        tm.append(m)
    out_b, valid_b, max_b = b_out["m"]
    nout = int(stat[2])
    assert (nout, int(stat[0]), int(stat[1])) == (len(out_b), valid_b, max_b), "A and B disagree"
    assert (merged[:nout] == out_b).all(), "A and B disagree"
    ms = lambda ts: {"median_ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3),
                     "max_ms": round(1e3 * max(ts), 3)}
    res = {"set": name, "records": n, "decoded_bytes": int(sum(plain)), "ranges": int(first[n]), "extents": nout,
           "wrapped": int(stat[4]), "rounds": rounds, "column": column,
           "A_gc_stat_batch": dict(ms(ta), **d2h_bytes(run_a, 20, 40)),
           "B_gc_scan_batch_plus_host_merge": dict(ms(tb), host_merge=ms(tm), **d2h_bytes(run_b, 20, 0))}
    res["B_over_A"] = round(statistics.median(tb) / statistics.median(ta), 2)
    print(json.dumps(res), flush=True)
    return res


def merge_dev_alone(sizes, rounds):
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    for n in sizes:
        low = rng.integers(0, 1 << 40, n, dtype=U64)
        r = np.stack([low, low + rng.integers(1, 1 << 22, n, dtype=U64)], axis=1)
        want, valid, mx = host_merge(r)
        d_in = torch.from_numpy(r.view(np.int64)).to(dev)
        scratch = torch.zeros(gc.merge_scratch_bytes(n), dtype=torch.uint8, device=dev)
        out = torch.zeros((n, 2), dtype=torch.int64, device=dev)
        stat = torch.zeros(5, dtype=torch.int64, device=dev)
        for _ in range(3):
            gc.merge_dev(d_in, n, scratch, out, stat)
        torch.cuda.synchronize()
        ts = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gc.merge_dev(d_in, n, scratch, out, stat)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        st = stat.cpu().numpy().view(U64)
        assert (int(st[0]), int(st[1]), int(st[2])) == (valid, mx, len(want))
        assert (out.cpu().numpy().view(U64)[: len(want)] == want).all()
        t0 = time.perf_counter()
        host_merge(r)
        host_ms = 1e3 * (time.perf_counter() - t0)
        print(json.dumps({"merge_dev_ranges": n, "extents": len(want), "rounds": rounds,
                          "median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
                          "max_ms": round(max(ts), 4), "numpy_merge_ms": round(host_ms, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="records of 64 KiB payloads")
    ap.add_argument("--c5-records", type=int, default=1024, help="records of the C5 mix")
    ap.add_argument("--small", type=int, nargs="*", default=[16, 128], help="smaller sets of 64 KiB records")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--column", type=int, default=0)
    ap.add_argument("--merge-dev", type=int, nargs="*", default=None, help="pom_gc_merge_dev alone on N ranges")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    if args.merge_dev is not None:
        merge_dev_alone(args.merge_dev, args.rounds)
        return
    for k in args.small:
        stored, plain = build([105] * k, 710000, args.column)
        measure(f"64KiB x {k}", stored, plain, args.column, args.rounds)
    if args.records:
        stored, plain = build([105] * args.records, 700000, args.column)
        measure("64KiB", stored, plain, args.column, args.rounds)
    if args.c5_records:
        ites = np.random.default_rng(5).integers(1, 1025, args.c5_records)
        stored, plain = build(ites, 100000, args.column)
        measure("C5", stored, plain, args.column, args.rounds)


if __name__ == "__main__":
    main()
