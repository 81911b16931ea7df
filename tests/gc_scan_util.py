"""The garbage-collector scan's test oracle and record builders (shared by
test_gc_scan.py and test_gpu_gc_scan.py).

walk() restates mdsl/gc.c:968-993 (the find_next_bit loop) and :788-802
(__add_to_brtree) in Python; it does not look at the product's itb_scan.h.
Where the reference is undefined (a bad adepth, a payload that ends early) it
follows the rules of include/pom_gc.h."""
from __future__ import annotations

import struct

import numpy as np

from pomegranate_amd import itb

EINVAL, E_TRUNCATED, E_NOSPACE = -22, -4097, -4098
BITMAP_OFF, INDEX_OFF, ITE_OFF, ITE_SIZE, COLUMN_OFF = 3584, 3712, 11904, 512, 368
M64 = (1 << 64) - 1


def find_next_bit(bitmap: bytes, size: int, offset: int) -> int:
    """lib/bitmap.c:163 over little-endian unsigned long: the first set bit at
    or after offset, or a value >= size."""
    for nr in range(offset, (size + 63) // 64 * 64):
        if bitmap[nr // 8] >> (nr % 8) & 1:
            return nr
    return max(size, offset)


def walk(payload: bytes, adepth: int, column: int):
    """(err, live, [(low, high), ...]) of one decoded payload."""
    if adepth < 1 or adepth > 10:
        return EINVAL, 0, []
    if len(payload) < INDEX_OFF:
        return E_TRUNCATED, 0, []
    bitmap = payload[BITMAP_OFF:INDEX_OFF]
    limit = 1 << adepth
    live, ranges, cut = 0, [], False
    nr = -1
    while nr < limit:                                           # mdsl/gc.c:971
        nr = find_next_bit(bitmap, limit, nr + 1)
        if nr < limit:
            live += 1                                           # itenr++
            ite = ITE_OFF + ITE_SIZE * nr
            if ite + ITE_SIZE > len(payload):
                cut = True
                continue
            _, ln, off = struct.unpack_from("<QQQ", payload, ite + COLUMN_OFF + 24 * column)
            if ln > 0:                                          # mdsl/gc.c:792
                ranges.append((off, (off + ln + 1) & M64))
    if cut:
        return E_TRUNCATED, live, []
    return 0, live, ranges


def set_itb(buf, base: int, bits, columns=None, seed: int = 0):
    """Writes the bitmap (set bits `bits`) and, for every ITE that fits the
    payload at buf[base:], six columns: random {itbid, len, offset} with about
    a quarter of the lens 0, or columns[nr] = [(len, offset)] * 6."""
    bm = bytearray(128)
    for nr in bits:
        bm[nr // 8] |= 1 << (nr % 8)
    buf[base + BITMAP_OFF: base + INDEX_OFF] = bm
    n_ites = max(0, (len(buf) - base - ITE_OFF) // ITE_SIZE)
    n_ites = min(n_ites, 1024)
    if n_ites:
        rng = np.random.default_rng(seed ^ 0x6C)
        cols = rng.integers(0, 1 << 40, (n_ites, 6, 3), dtype=np.uint64)
        cols[:, :, 1] *= rng.integers(0, 4, (n_ites, 6), dtype=np.uint64) > 0
        if columns:
            for nr, six in columns.items():
                if nr < n_ites:
                    for c, (ln, off) in enumerate(six):
                        cols[nr, c, 1], cols[nr, c, 2] = ln, off
        raw = cols.tobytes()
        for nr in range(n_ites):
            at = base + ITE_OFF + ITE_SIZE * nr + COLUMN_OFF
            buf[at: at + 144] = raw[144 * nr: 144 * (nr + 1)]


def make_record(seed: int, n_ites: int, adepth: int, bits, entries=None, columns=None) -> bytearray:
    """itb.make_record (random header bytes, synthetic payload) with adepth,
    entries, the bitmap and the columns set explicitly; trimmed to h.len."""
    rec = itb.make_record(seed, n_ites)
    ln = itb.header_fields(rec)[0]
    rec = rec[:ln]
    bits = list(bits)
    rec[3] = adepth
    live = sum(1 for b in bits if b < (1 << adepth)) if 1 <= adepth <= 10 else 0
    struct.pack_into("<i", rec, 4, live if entries is None else entries)
    set_itb(rec, itb.ITBH_SIZE, bits, columns, seed)
    return rec


def lzo_record(oracle, rec, zlen_delta: int = 0) -> bytearray:
    """rec as itb_lzo_compress stores it (mds/itb.c:2904-2945): zlen = len,
    len = 264 + compressed size, COMPR_LZO; compressed by the fixture oracle."""
    ln = itb.header_fields(rec)[0]
    z = oracle.compress(bytes(rec[itb.ITBH_SIZE:ln]))
    out = bytearray(rec[:itb.ITBH_SIZE]) + z
    struct.pack_into("<II", out, itb.LEN_OFF, itb.ITBH_SIZE + len(z), ln + zlen_delta)
    struct.pack_into("<H", out, itb.ALGO_OFF, itb.COMPR_LZO)
    return out


def expect_batch(payloads, adepths, column):
    """Per-ITB oracle results and the concatenated ranges in ITB order:
    (err[], live[], first[n + 1], ranges [total, 2] uint64).  payloads[b] None:
    an ITB that yields nothing (its err is the caller's business)."""
    errs, lives, first, rows = [], [], [0], []
    for p, ad in zip(payloads, adepths):
        e, lv, rg = (None, 0, []) if p is None else walk(p, ad, column)
        errs.append(e)
        lives.append(lv)
        rows.extend(rg)
        first.append(len(rows))
    arr = np.array(rows, dtype=np.uint64).reshape(-1, 2)
    return errs, lives, np.array(first, dtype=np.uint64), arr
