"""The directory listing's test oracle and record builders (shared by
test_readdir.py and test_gpu_readdir.py).

listing() restates the FS branch of itb_readdir (mds/itb.c:2536-2589: the
test_bit loop, the state and KV test, the dentry_info it fills) in Python; it
does not look at the product's itb_dents.h.  Where the reference is undefined
(a bad adepth, a payload that ends early, a name longer than s.name) it follows
the rules of include/pom_readdir.h."""
from __future__ import annotations

import struct

import numpy as np

import gc_scan_util
from gc_scan_util import BITMAP_OFF, EINVAL, E_NOSPACE, E_TRUNCATED, INDEX_OFF, ITE_OFF, ITE_SIZE, lzo_record  # noqa: F401

E_NAME = -4099
ITE_ACTIVE, ITE_STATE_MASK, ITE_FLAG_KV, ITE_FLAG_NORMAL = 0, 7, 0x01000000, 0x80000000
NAME_MAX = 256


def listing(payload: bytes, adepth: int):
    """(err, live, dnum, records) of one decoded payload."""
    if adepth < 1 or adepth > 10:
        return EINVAL, 0, 0, b""
    if len(payload) < INDEX_OFF:
        return E_TRUNCATED, 0, 0, b""
    bitmap = payload[BITMAP_OFF:INDEX_OFF]
    live, dnum, out, cut, long_name = 0, 0, bytearray(), False, False
    for idx in range(1 << adepth):                              # mds/itb.c:2567
        if not bitmap[idx // 8] >> (idx % 8) & 1:               # test_bit
            continue
        live += 1
        ite = ITE_OFF + ITE_SIZE * idx
        if ite + ITE_SIZE > len(payload):
            cut = True
            continue
        _, uuid, flag, namelen = struct.unpack_from("<QQII", payload, ite)
        if (flag & ITE_STATE_MASK) != ITE_ACTIVE or flag & ITE_FLAG_KV:      # :2569-2574
            continue
        if namelen > NAME_MAX:
            long_name = True
            continue
        (mode,) = struct.unpack_from("<H", payload, ite + 36)                # s.mdu.mode
        out += struct.pack("<QHHI", uuid, mode, namelen, 0)                  # struct dentry_info, zeroed buffer
        out += payload[ite + 104: ite + 104 + namelen]                       # s.name
        dnum += 1
    if cut:
        return E_TRUNCATED, live, 0, b""
    if long_name:
        return E_NAME, live, 0, b""
    return 0, live, dnum, bytes(out)


def set_ite(buf, base: int, nr: int, flag=None, name=None, namelen=None, uuid=None, mode=None):
    """Overwrites fields of ITE nr of the payload at buf[base:]; namelen
    defaults to len(name) and may lie (257 and up)."""
    ite = base + ITE_OFF + ITE_SIZE * nr
    assert ite + ITE_SIZE <= len(buf)
    if uuid is not None:
        struct.pack_into("<Q", buf, ite + 8, uuid)
    if flag is not None:
        struct.pack_into("<I", buf, ite + 16, flag)
    if name is not None:
        assert len(name) <= NAME_MAX
        buf[ite + 104: ite + 104 + len(name)] = name
        if namelen is None:
            namelen = len(name)
    if namelen is not None:
        struct.pack_into("<I", buf, ite + 20, namelen)
    if mode is not None:
        struct.pack_into("<H", buf, ite + 36, mode)


def name_of(seed: int, nr: int, n: int) -> bytes:
    """n name bytes, none of them 0, different for every (seed, nr)."""
    rng = np.random.default_rng((seed << 12) ^ nr ^ 0xD1E)
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


def fill_ites(buf, base: int, seed: int, n_ites: int, namelens=None, flags=None):
    """Every ITE of the payload gets a random uuid and mode, the flag
    flags[nr] (default: active, ITE_FLAG_NORMAL) and a random name of
    namelens[nr] bytes (default: 0 ... 40, seeded), the rest of s.name random
    too, so that a byte copied from behind a name shows."""
    rng = np.random.default_rng(seed ^ 0xDE27)
    lens = rng.integers(0, 41, n_ites)
    for nr in range(n_ites):
        ite = base + ITE_OFF + ITE_SIZE * nr
        buf[ite + 104: ite + 360] = rng.integers(0, 256, 256, dtype=np.uint8).tobytes()
        n = int(lens[nr]) if namelens is None or nr not in namelens else namelens[nr]
        set_ite(buf, base, nr, flag=(flags or {}).get(nr, ITE_FLAG_NORMAL | int(rng.integers(0, 1 << 20)) << 3),
                name=name_of(seed, nr, min(n, NAME_MAX)), namelen=n, uuid=int(rng.integers(0, 1 << 63)),
                mode=int(rng.integers(0, 1 << 16)))


def make_record(seed: int, n_ites: int, adepth: int, bits, entries=None, namelens=None, flags=None) -> bytearray:
    """gc_scan_util.make_record (adepth, entries and the bitmap set
    explicitly) with the ITEs' listing fields from fill_ites."""
    rec = gc_scan_util.make_record(seed, n_ites, adepth, bits, entries)
    fill_ites(rec, 264, seed, min(n_ites, 1024), namelens, flags)
    return rec


def expect_batch(payloads, adepths):
    """Per-ITB oracle results and the concatenated records in ITB order:
    (err[], live[], dnum[], first[n + 1] in bytes, data).  payloads[b] None: an
    ITB that yields nothing (its err is the caller's business)."""
    errs, lives, dnums, first, data = [], [], [], [0], bytearray()
    for p, ad in zip(payloads, adepths):
        e, lv, dn, rec = (None, 0, 0, b"") if p is None else listing(p, ad)
        errs.append(e)
        lives.append(lv)
        dnums.append(dn)
        data += rec
        first.append(len(data))
    return errs, lives, dnums, np.array(first, dtype=np.uint64), bytes(data)
