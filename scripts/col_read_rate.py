#!/usr/bin/env python3
"""Column reads by offset and size: unzip-and-slice against read-on-the-GPU.

Paths over one seeded set of zipped columns (ITB-family synth, zipped on the
GPU), in one process, alternating, each warmed up first:
  A   pom_col_unzip_batch of every column once, then the requested regions
      copied out on the host: what a caller of the library does today
  A1  (workload b only) pom_col_unzip_batch of the column once per request,
      the reference's behaviour (api/api.c:6427-6460 decodes the whole column
      for every read): one batch over the columns per request round
  B   pom_col_read_batch: decode and region copy on the GPU; only the slices
      come back
Workloads:
  a   `--columns` columns of 64 KiB, one 4 KiB request each at a random offset
  b   `--big-columns` columns of 4 MiB, each read sequentially by 32 requests
      of 128 KiB in one call
Rates are GiB/s of requested bytes, median and min ... max over `--rounds`
alternating rounds; the D2H bytes of each side are computed from the lengths.
Only the C calls and the host-side region copies are timed (pointer arrays are
built before).  Prints one JSON line per workload.
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

from pomegranate_amd import column, synth  # noqa: E402

GIB = float(1 << 30)
_sz = ctypes.c_size_t


def build(n, size, seed0):
    cols = [bytes(synth.block(synth.ITB, seed0 + i, size)) for i in range(n)]
    zips, comp = column.zip_batch(cols)
    assert all(comp), "a column did not compress"
    return cols, zips


def measure(name, cols, zips, reqs, rounds, per_request_unzip):
    """reqs: (col, offset, size), every region inside its column."""
    lib = column._lib()
    n, nr = len(zips), len(reqs)
    keep = [np.frombuffer(z, dtype=np.uint8) for z in zips]
    zptr = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
    zlen = (_sz * n)(*[len(z) for z in zips])
    # A: whole columns come back
    full = [np.zeros(len(c), dtype=np.uint8) for c in cols]
    fptr = (ctypes.c_void_p * n)(*[f.ctypes.data for f in full])
    fcap = (_sz * n)(*[f.size for f in full])
    flen = (_sz * n)()
    ferr = (ctypes.c_int * n)()
    outs_a = [np.zeros(s, dtype=np.uint8) for _, _, s in reqs]
    # B: only the slices
    rq = (column.Req * nr)(*[column.Req(o, s, c, 0) for c, o, s in reqs])
    outs_b = [np.zeros(s, dtype=np.uint8) for _, _, s in reqs]
    optr = (ctypes.c_void_p * nr)(*[o.ctypes.data for o in outs_b])
    olen = (_sz * nr)()
    oerr = (ctypes.c_int * nr)()

    def unzip_all():
        rc = lib.pom_col_unzip_batch(zptr, zlen, n, fptr, fcap, flen, ferr)
        assert rc == 0 and not any(ferr)

    def run_a():
        t0 = time.perf_counter()
        unzip_all()
        for out, (c, o, s) in zip(outs_a, reqs):
            out[:] = full[c][o: o + s]
        return time.perf_counter() - t0

    by_round, nth = {}, {}                                  # a column's k-th request is in round k
    for r, (c, _, _) in enumerate(reqs):
        nth[c] = nth.get(c, -1) + 1
        by_round.setdefault(nth[c], []).append(r)

    def run_a1():
        t0 = time.perf_counter()
        for rs in by_round.values():                       # every column decoded again for its next request
            unzip_all()
            for r in rs:
                c, o, s = reqs[r]
                outs_a[r][:] = full[c][o: o + s]
        return time.perf_counter() - t0

    def run_b():
        t0 = time.perf_counter()
        rc = lib.pom_col_read_batch(zptr, zlen, n, rq, nr, optr, olen, oerr)
        dt = time.perf_counter() - t0
        assert rc == 0 and not any(oerr)
        return dt

    paths = {"A_unzip_and_slice": run_a, "B_read_batch": run_b}
    if per_request_unzip:
        paths["A1_unzip_per_request"] = run_a1
    for fn in paths.values():                              # warm-up: staging grown on every path
        fn(), fn()
    for r, (c, o, s) in enumerate(reqs):
        assert outs_b[r].tobytes() == cols[c][o: o + s] == outs_a[r].tobytes(), r
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            times[k].append(fn())
    requested = float(sum(s for _, _, s in reqs))
    rate = lambda ts: {"median_gibps": round(requested / statistics.median(ts) / GIB, 3),
                       "min_gibps": round(requested / max(ts) / GIB, 3),
                       "max_gibps": round(requested / min(ts) / GIB, 3),
                       "median_ms": round(statistics.median(ts) * 1e3, 2)}
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    d2h_a = aligned(len(c) for c in cols) + 8 * n
    res = {"workload": name, "columns": n, "requests": nr, "requested_bytes": int(requested),
           "decoded_bytes": sum(len(c) for c in cols), "compressed_bytes": sum(len(z) for z in zips), "rounds": rounds,
           "A_unzip_and_slice": dict(rate(times["A_unzip_and_slice"]), d2h_bytes=d2h_a),
           "B_read_batch": dict(rate(times["B_read_batch"]),
                                d2h_bytes=aligned(s for _, _, s in reqs) + 8 * n + 8 * nr + 16)}
    if per_request_unzip:
        res["A1_unzip_per_request"] = dict(rate(times["A1_unzip_per_request"]), d2h_bytes=d2h_a * len(by_round))
        res["B_over_A1"] = round(statistics.median(times["A1_unzip_per_request"]) /
                                 statistics.median(times["B_read_batch"]), 2)
    res["B_over_A"] = round(statistics.median(times["A_unzip_and_slice"]) / statistics.median(times["B_read_batch"]), 2)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--columns", type=int, default=4096, help="workload a: columns of 64 KiB")
    ap.add_argument("--big-columns", type=int, default=64, help="workload b: columns of 4 MiB")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    rng = np.random.default_rng(11)
    if args.columns:
        cols, zips = build(args.columns, 64 << 10, 300000)
        reqs = [(c, int(rng.integers(0, (64 << 10) - 4096 + 1)), 4096) for c in range(args.columns)]
        measure("a_64KiB_one_4KiB_read", cols, zips, reqs, args.rounds, False)
    if args.big_columns:
        cols, zips = build(args.big_columns, 4 << 20, 400000)
        reqs = [(c, k * (128 << 10), 128 << 10) for c in range(args.big_columns) for k in range(32)]
        measure("b_4MiB_32_sequential_128KiB_reads", cols, zips, reqs, args.rounds, True)


if __name__ == "__main__":
    main()
