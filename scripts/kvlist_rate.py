#!/usr/bin/env python3
"""Key/value table listing: decode-and-copy-back against decode-and-list-on-the-GPU.

Two paths over one seeded set of COMPR_LZO ITB records of an xTable key/value
table, in one process, alternating, each warmed up twice first:
  A  pom_itb_lzo_decompress_batch on copies of the records, then the host walk
     (itb_keys_one from tests/native/libitb_keys_host.so, one C call over the
     batch, one thread): what a caller of the library could do before
     pom_kvlist_batch.  The decode alone is timed too (A0).
  B  pom_kvlist_batch: decode, filter, walk and record packing on the GPU; only
     counts and records come back
for four operations: scan, grep with a needle planted in about 1% of the
values, grep with no match, and count-only (the 1% grep with out == NULL).
Both paths produce the same bytes (checked once per operation, outside the
timing).  Record sets: `--records` records of 64 KiB payloads (105 ITEs) and
the C5 mix (1 ... 1024 ITEs, seed 5); half of the entries NORMAL with 40-byte
values, half STR with 24-byte keys and 40-byte values (`--str-klen L`: every
entry STR with an L-byte key, for the copy plans at other record lengths).
`--adversarial`: every value 320 x 'a', grepped for 159 x 'a' + 'b'.  `--alt`
also times B with the per-lane copy (keys_copy=1) and with the plain search
(keys_search=1).  Rates are GiB/s of decoded payload, median and min ... max
over `--rounds` alternating rounds; the bytes each path copies each way are
computed from the lengths.  Only the C calls are timed.  Prints one JSON line
per set and operation.
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

from pomegranate_amd import gc, itb, kvlist, lzo  # noqa: E402

GIB = float(1 << 30)
H = itb.ITBH_SIZE
NEEDLE = b"Needle#1"
ABSENT = b"Absent#2"
ADVERSARIAL = b"a" * 159 + b"b"


def build(n_ites_list, seed0, str_klen=None, adversarial=False):
    """COMPR_LZO records (compressed on the GPU) with adepth 10 and the first
    n_ites bitmap bits set; returns (stored, decoded payload lengths)."""
    recs = []
    for i, k in enumerate(n_ites_list):
        k = int(k)
        r = itb.make_record(seed0 + i, k)
        r = r[: itb.header_fields(r)[0]]
        r[3] = 10
        r[4:8] = k.to_bytes(4, "little")
        bm = np.zeros(128, dtype=np.uint8)
        full = np.unpackbits(bm, bitorder="little")
        full[:k] = 1
        r[H + gc.BITMAP_OFF: H + gc.INDEX_OFF] = np.packbits(full, bitorder="little").tobytes()
        rng = np.random.default_rng(seed0 + i)
        ites = np.frombuffer(r, dtype=np.uint8)[H + gc.ITE_OFF:].reshape(k, gc.ITE_SIZE)
        is_str = (np.arange(k) % 2 == 1) if str_klen is None else np.ones(k, dtype=bool)
        klen = 24 if str_klen is None else str_klen
        ites[:, kvlist.KV_FLAGS_OFF: kvlist.KV_FLAGS_OFF + 4] = np.where(is_str, kvlist.KV_STR, kvlist.KV_NORMAL).astype(
            "<u4").view(np.uint8).reshape(k, 4)
        ites[:, kvlist.KV_KEY_OFF: kvlist.KV_KEY_OFF + 8] = rng.integers(0, 1 << 40, k).astype("<u8").view(
            np.uint8).reshape(k, 8)
        ites[:, kvlist.KV_KLEN_OFF: kvlist.KV_KLEN_OFF + 4] = np.where(is_str, klen, 0).astype("<u4").view(
            np.uint8).reshape(k, 4)
        value = np.zeros((k, kvlist.KV_VALUE_MAX), dtype=np.uint8)
        if adversarial:
            value[:] = ord("a")
        else:
            used = min(kvlist.KV_VALUE_MAX - 1, klen + 40)
            value[:, :used] = rng.integers(97, 123, (k, used), dtype=np.uint8)
            value[~is_str, 40:] = 0
            hit = np.flatnonzero(rng.random(k) < 0.01)
            at = np.where(is_str[hit], klen, 0) + 3
            for j, a in zip(hit, at):
                if a + len(NEEDLE) < used:
                    value[j, a: a + len(NEEDLE)] = np.frombuffer(NEEDLE, dtype=np.uint8)
        ites[:, kvlist.KV_VALUE_OFF: kvlist.KV_VALUE_OFF + kvlist.KV_VALUE_MAX] = value
        recs.append(r)
    tmps = [bytearray(H + lzo.worst_compress(len(r) - H)) for r in recs]
    which, err = itb.compress_batch(recs, tmps)
    assert not any(err) and all(which), "a record did not compress"
    stored = [bytes(t[: itb.header_fields(t)[0]]) for t in tmps]
    return stored, [itb.header_fields(s)[1] - H for s in stored]


def measure(name, stored, plain, rounds, ops, alt=False):
    lib = kvlist._lib()
    itb._lib()
    host = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libitb_keys_host.so"))
    host.itb_keys_host_batch.restype = ctypes.c_int
    host.itb_keys_host_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    n = len(stored)
    total_plain = float(sum(plain))
    z = [len(s) - H for s in stored]
    cap = sum(kvlist.REC_MAX * min(1024, (p - 11904) // 512) for p in plain)
    keep_b = [np.frombuffer(s, dtype=np.uint8) for s in stored]
    ptr_b = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep_b])
    len_b = (ctypes.c_size_t * n)(*[len(s) for s in stored])
    out_b = np.zeros(cap, dtype=np.uint8)
    first_b = np.zeros(n + 1, dtype=np.uint64)
    live = np.zeros(n, dtype=np.uint32)
    dnum_b = np.zeros(n, dtype=np.uint32)
    kb = np.zeros(n, dtype=np.uint32)
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
    dnum_a = np.zeros(n, dtype=np.uint32)
    aligned = lambda v: sum((x + 15) // 16 * 16 for x in v)
    rate = lambda ts: {"median_gibps": round(total_plain / statistics.median(ts) / GIB, 2),
                       "min_gibps": round(total_plain / max(ts) / GIB, 2),
                       "max_gibps": round(total_plain / min(ts) / GIB, 2)}
    for label, op, needle, count_only in ops:
        nd = np.frombuffer(needle, dtype=np.uint8)
        ndp = nd.ctypes.data if nd.size else None

        def run_a():
            for b, s in zip(bufs, keep_b):
                b[: s.size] = s
            t0 = time.perf_counter()
            rc = lib.pom_itb_lzo_decompress_batch(ptr_a, cap_a, err_a, ok_a, n)
            t1 = time.perf_counter()
            rw = host.itb_keys_host_batch(pay_a, len_a.ctypes.data, adepth.ctypes.data, n, op, ndp, nd.size,
                                          None if count_only else out_a.ctypes.data, cap, first_a.ctypes.data,
                                          dnum_a.ctypes.data)
            t2 = time.perf_counter()
            assert rc == 0 and rw == 0 and not any(err_a) and all(ok_a)
            return t2 - t0, t1 - t0

        def run_b(debug=None):
            if debug:
                os.environ["POM_LZO_DEBUG"] = debug
                lzo.debug_reload()
            try:
                t0 = time.perf_counter()
                rc = lib.pom_kvlist_batch(ptr_b, len_b, n, op, ndp, nd.size, None if count_only else out_b.ctypes.data,
                                          cap, first_b.ctypes.data, live.ctypes.data, dnum_b.ctypes.data,
                                          kb.ctypes.data, None, err_b.ctypes.data, None, None)
                dt = time.perf_counter() - t0
            finally:
                if debug:
                    del os.environ["POM_LZO_DEBUG"]
                    lzo.debug_reload()
            assert rc == 0 and not err_b.any()
            return dt

        def same():
            nbytes = int(first_b[n])
            return (first_a == first_b).all() and (dnum_a == dnum_b).all() and \
                (count_only or (out_a[:nbytes] == out_b[:nbytes]).all())

        run_a(), run_b(), run_a(), run_b()                       # warm-up: staging grown on both paths
        assert same(), "the two paths disagree"
        alts = {"B_per_lane_copy": "keys_copy=1", "B_plain_search": "keys_search=1"} if alt else {}
        for dbg in alts.values():
            run_b(dbg)
            assert same(), f"{dbg} disagrees"
        ta, td, tb, tl = [], [], [], {k: [] for k in alts}
        for k in range(rounds):
            both, decode = run_a()
            ta.append(both)
            td.append(decode)
            order = [None] + list(alts) if k % 2 else list(alts) + [None]     # B and its alternatives take turns
            for which in order:
                if which is None:
                    tb.append(run_b())
                else:
                    tl[which].append(run_b(alts[which]))
        nbytes = 0 if count_only else int(first_b[n])
        d2h_a = aligned(plain) + 8 * n
        d2h_b = 28 * n + nbytes
        res = {"set": name, "op": label, "records": n, "decoded_bytes": int(total_plain),
               "compressed_bytes": int(sum(z)), "live_ites": int(live.sum()), "emitted": int(dnum_b.sum()),
               "record_bytes": int(first_b[n]), "rounds": rounds,
               "A_decompress_batch_then_host_walk": dict(rate(ta), h2d_bytes=aligned(z) + 48 * n, d2h_bytes=d2h_a),
               "A0_decompress_batch_alone": rate(td),
               "B_kvlist_batch": dict(rate(tb), h2d_bytes=aligned(z) + 65 * n + 256, d2h_bytes=d2h_b),
               "d2h_ratio": round(d2h_a / d2h_b, 1),
               "B_over_A": round(statistics.median(ta) / statistics.median(tb), 2),
               "B_over_A0": round(statistics.median(td) / statistics.median(tb), 2)}
        for which in alts:
            res[which] = rate(tl[which])
        print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=4096, help="records of 64 KiB payloads")
    ap.add_argument("--c5-records", type=int, default=1024, help="records of the C5 mix")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--str-klen", type=int, default=None, help="0 ... 279: every entry STR with a key this long")
    ap.add_argument("--adversarial", action="store_true", help="only the adversarial set: 320 x 'a' values")
    ap.add_argument("--op", default=None, help="only this operation: scan, grep_1pct, grep_none or count_only")
    ap.add_argument("--alt", action="store_true", help="also time B with keys_copy=1 and with keys_search=1")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least 5 alternating rounds"
    ops = [("scan", kvlist.OP_SCAN, b"", False), ("grep_1pct", kvlist.OP_GREP, NEEDLE, False),
           ("grep_none", kvlist.OP_GREP, ABSENT, False), ("count_only", kvlist.OP_GREP_CNT, NEEDLE, True)]
    if args.op:
        ops = [o for o in ops if o[0] == args.op]
        assert ops, "no such operation"
    if args.adversarial:
        stored, plain = build([105] * args.records, 900000, adversarial=True)
        measure("adversarial", stored, plain, args.rounds, [("grep_adversarial", kvlist.OP_GREP, ADVERSARIAL, False)],
                args.alt)
        return
    if args.records:
        stored, plain = build([105] * args.records, 700000, args.str_klen)
        measure("64KiB", stored, plain, args.rounds, ops, args.alt)
    if args.c5_records:
        ites = np.random.default_rng(5).integers(1, 1025, args.c5_records)
        stored, plain = build(ites, 100000, args.str_klen)
        measure("C5", stored, plain, args.rounds, ops, args.alt)


if __name__ == "__main__":
    main()
