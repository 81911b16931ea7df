"""The key/value point get's test oracle and case families (shared by
test_kvget.py and test_gpu_kvget.py).

get() restates the INDEX_KV branch of ite_match (mds/itb.c:1095-1116), the
chain walk and the copy of itb_search (:1769-1814), __data_column_hook
(:1650-1661) and the reply of mds/cbht.c:929-977 in Python, on tables built by
lookup_util's add_index / set_slot / make_record and entries set by
kvlist_util's set_ite.  It does not look at the product's itb_kvget.h.  Where
the reference is undefined (a bad adepth, a payload that ends early, a cyclic
chain, a value or a key longer than its field, a column past the ITE, a request
the ABI refuses) it follows the rules of include/pom_kvget.h."""
from __future__ import annotations

import struct

import numpy as np

import kvlist_util
import lookup_util as L
from gc_scan_util import EINVAL, E_NOSPACE, E_TRUNCATED, ITE_OFF, ITE_SIZE, lzo_record  # noqa: F401
from kvlist_util import KV_NORMAL, KV_STR, set_ite
from lookup_util import (E_LOOP, ENOENT, ESPLIT, H, IDX_CONFLICT, IDX_FREE, IDX_OVERFLOW, IDX_UNIQUE,  # noqa: F401
                         INDEX_ENTRIES, ITB_JUST_SPLIT, get_slot, payload_of, set_slot)

E_VALUE = -4102
F_LOOKUP, F_COLUMN, F_KV = 0x10, 0x40, 0x40000000
ALL_FLAGS = F_LOOKUP | F_COLUMN | F_KV
KVFLAG_MASK, MAX_COLUMN = 0xCFFF, 0xFFF
KV_OFF, KV_HEADER_LEN, VALUE_OFF, VALUE_MAX, COLUMN_OFF, LEASE_OFF = 24, 20, 44, 320, 368, 80
REC_MAX = 364
NONE = (0, 0, 0, b"")

VLENS = (0, 1, 11, 12, 13, 27, 28, 29, 43, 44, 319, 320, 321)
SKLENS = (0, 1, 7, 8, 9, 16, 17, 255, 256, 320, 321)


# ---------------------------------------------------------------------------
# The oracle
# ---------------------------------------------------------------------------
def ite_match(payload, ite: int, q: dict, keys: bytes) -> bool:
    """mds/itb.c:1095-1116, the INDEX_KV branch."""
    vkey, vklen = struct.unpack_from("<QI", payload, ite + 32)
    if q["kvflag"] & KV_STR:
        if q["key"] != vkey:
            return False
        if vklen != q["sklen"]:                         # (hi->data is never NULL here)
            return False
        if q["sklen"] > VALUE_MAX:                      # include/pom_kvget.h rule 6
            return False
        skey = keys[q["skey_off"]: q["skey_off"] + q["sklen"]]
        return bytes(payload[ite + VALUE_OFF: ite + VALUE_OFF + q["sklen"]]) == skey
    return q["key"] == vkey                             # defaults to KV_NORMAL


def get(payload, adepth: int, q: dict, keys: bytes):
    """(err, nr, depth, lease, record) of one request {key, flag, kvflag,
    skey_off, sklen} against one decoded payload."""
    if adepth < 1 or adepth > 10:
        return (EINVAL,) + NONE
    if len(payload) < ITE_OFF:
        return (E_TRUNCATED,) + NONE
    if (q["flag"] & ~ALL_FLAGS or q["kvflag"] & ~KVFLAG_MASK
            or (q["flag"] & F_COLUMN and q["kvflag"] & MAX_COLUMN > 5)
            or (q["kvflag"] & KV_STR and q["sklen"] <= VALUE_MAX and q["skey_off"] + q["sklen"] > len(keys))):
        return (EINVAL,) + NONE
    offset = q["key"] & ((1 << adepth) - 1)                             # mds/itb.c:1769
    depth = 0
    while offset < INDEX_ENTRIES:                                       # :1780
        entry, conflict, flag = get_slot(payload, 0, offset)
        if flag == IDX_FREE:
            break
        if depth == INDEX_ENTRIES:
            return E_LOOP, 0, depth, 0, b""
        depth += 1
        ite = ITE_OFF + ITE_SIZE * entry
        if ite + ITE_SIZE > len(payload):
            return E_TRUNCATED, 0, depth, 0, b""
        hit = ite_match(payload, ite, q, keys)
        if flag == IDX_UNIQUE:
            if not hit:
                break
        elif not hit:                                                   # CONFLICT & OVERFLOW
            offset = conflict
            continue
        vflags, vlen = struct.unpack_from("<II", payload, ite + KV_OFF)
        if not vflags & (KV_NORMAL | KV_STR):                           # mds/cbht.c:974-977
            return EINVAL, 0, depth, 0, b""
        if vlen > VALUE_MAX:
            return E_VALUE, 0, depth, 0, b""
        rec = bytes(payload[ite + KV_OFF: ite + KV_OFF + KV_HEADER_LEN + vlen])     # :1808-1810
        if q["flag"] & F_COLUMN:                                        # __data_column_hook, cbht.c:935-953
            at = ite + COLUMN_OFF + 24 * (q["kvflag"] & MAX_COLUMN)
            rec += bytes(payload[at: at + 24])
        (lease,) = struct.unpack_from("<Q", payload, ite + LEASE_OFF)   # e->s.mdu.dtime
        return 0, entry, depth, lease, rec
    return ENOENT, 0, depth, 0, b""


def as_dicts(req: np.ndarray):
    return [{k: int(row[k]) for k in ("key", "itb", "flag", "kvflag", "skey_off", "sklen")} for row in req]


class Want:
    """The oracle over a whole call."""

    def __init__(self, payloads, adepths, req, keys, status=None):
        n = len(req)
        self.err, self.nr, self.depth, self.len = (np.zeros(n, t) for t in (np.int32, np.uint32, np.uint32, np.uint32))
        self.lease = np.zeros(n, np.uint64)
        self.recs = []
        for r, q in enumerate(as_dicts(req)):
            b = q["itb"]
            if b >= len(payloads):
                res = (EINVAL,) + NONE
            elif status is not None and status[b]:
                res = (status[b],) + NONE
            else:
                res = get(payloads[b], adepths[b], q, keys)
            self.err[r], self.nr[r], self.depth[r], self.lease[r] = res[:4]
            self.len[r] = len(res[4])
            self.recs.append(res[4])
        self.first = np.zeros(n + 1, np.uint64)
        self.first[1:] = np.cumsum(self.len.astype(np.uint64))
        self.data = b"".join(self.recs)

    def pick(self, idx):
        """The oracle's answer for the requests idx, in that order."""
        w = Want.__new__(Want)
        w.err, w.nr, w.depth, w.len, w.lease = (a[idx] for a in (self.err, self.nr, self.depth, self.len, self.lease))
        w.recs = [self.recs[int(i)] for i in idx]
        w.first = np.zeros(len(idx) + 1, np.uint64)
        w.first[1:] = np.cumsum(w.len.astype(np.uint64))
        w.data = b"".join(w.recs)
        return w


def same(got, want: Want, out_cap=None):
    """got: (err, nr, depth, len, lease, first, data) with data the bytes of
    out[0, min(first[nreq], out_cap))."""
    for g, w, what in zip(got[:6], (want.err, want.nr, want.depth, want.len, want.lease, want.first),
                          ("err", "nr", "depth", "len", "lease", "first")):
        g = np.asarray(g)
        assert g.shape == w.shape, what
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, f"{what}: request {int(bad[0])}: {g[bad[0]]} != {w[bad[0]]}"
    data = want.data if out_cap is None else want.data[:out_cap]
    g = bytes(got[6])
    if g != data:
        at = next(i for i, (x, y) in enumerate(zip(g, data)) if x != y) if len(g) == len(data) else min(len(g), len(data))
        r = int(np.searchsorted(want.first, at, side="right")) - 1
        raise AssertionError(f"out: byte {at} (request {r}, its byte {at - int(want.first[r])}) differs; "
                             f"{len(g)} bytes, want {len(data)}")


# ---------------------------------------------------------------------------
# Builders
# ---------------------------------------------------------------------------
def set_kv(rec, nr: int, flags=None, vlen=None, key=None, klen=None, value=None):
    """Fields of ITE nr's struct kv in a record [itbh][payload]."""
    set_ite(rec, H, nr, flags=flags, key=key, klen=klen, value=value)
    if vlen is not None:
        struct.pack_into("<I", rec, H + ITE_OFF + ITE_SIZE * nr + 28, vlen)


def make_table(seed: int, n_ites: int, adepth: int, keys, kv=None) -> bytearray:
    """lookup_util.make_record's table (built by add_index in ascending nr from
    keys[nr] & mask) over ITEs whose every byte is random and non-zero
    (kvlist_util.fill_ites; the columns too), then v.key = keys[nr] and
    kv[nr] = set_kv's keyword arguments.  Without kv[nr]: a NORMAL entry with a
    seeded v.len of 0 ... 60."""
    rec = L.make_record(seed, n_ites, adepth, keys)
    kvlist_util.fill_ites(rec, H, seed, min(n_ites, 1024))
    rng = np.random.default_rng(seed ^ 0x6E7)
    lens = rng.integers(0, 61, n_ites)
    items = keys.items() if isinstance(keys, dict) else enumerate(keys)
    for nr, key in items:
        set_kv(rec, nr, flags=KV_NORMAL, vlen=int(lens[nr]), key=key)
    for nr, kw in (kv or {}).items():
        set_kv(rec, nr, **kw)
    return rec


def kv_fields(rec, nr: int):
    """(flags, len, key, klen, value[320]) of ITE nr of a record."""
    ite = H + ITE_OFF + ITE_SIZE * nr
    return struct.unpack_from("<IIQI", rec, ite + KV_OFF) + (bytes(rec[ite + VALUE_OFF: ite + VALUE_OFF + VALUE_MAX]),)


class Blob:
    """The key blob, keys put at chosen residues mod 8 of their offset."""

    def __init__(self):
        self.bytes = bytearray()

    def put(self, key: bytes, residue=None, after=None) -> int:
        while residue is not None and len(self.bytes) % 8 != residue:
            self.bytes.append(0xEE)
        at = len(self.bytes)
        self.bytes.extend(key)
        if after is not None:
            self.bytes.append(after)
        return at


def rows_to_req(rows):
    from pomegranate_amd import kvget
    return np.array([(key, itb, flag, kvflag, off, sklen, 0xDEAD0000 + i) for i, (key, itb, flag, kvflag, off, sklen)
                     in enumerate(rows)], dtype=kvget.REQ_DTYPE)


GET = F_KV | F_LOOKUP


# ---------------------------------------------------------------------------
# Case families: (records as stored uncompressed, adepths, req, key blob)
# ---------------------------------------------------------------------------
def family_values():
    """One ITB of 13 NORMAL entries, v.len = VLENS[nr] (321: POM_KG_E_VALUE);
    each without a column, with columns 0 ... 5, and column 6 for the refusal.
    Records of 20, 32 and 48 bytes meet the granule edges; the column follows
    values of every length."""
    keys = [0x7000 + 0x40 * nr + nr for nr in range(len(VLENS))]
    rec = make_table(8000, len(VLENS), 4, keys, {nr: dict(vlen=v) for nr, v in enumerate(VLENS)})
    rows = []
    for nr, key in enumerate(keys):
        rows.append((key, 0, GET, KV_NORMAL, 0, 0))
        for column in range(7):
            rows.append((key, 0, GET | F_COLUMN, KV_NORMAL | column, 0, 0))
    rows.append((keys[3], 0, GET, KV_NORMAL | 6, 0, 0))                 # the column is not read without the flag
    rows.append((keys[3], 0, F_COLUMN, 2, 0, 0))                        # neither kind: NORMAL; neither LOOKUP nor KV
    return [rec], [4], rows_to_req(rows), b""


def family_strkeys():
    """ITE nr is a STR entry with klen = SKLENS[nr] (321: no request can match
    it) and the rest of v.value random.  The blob holds every key at every
    residue 0 ... 7 of its offset, each followed by a byte that differs from
    what follows in v.value; at residue 3 also the key with its last and with
    its first byte changed.  Then the refusals: stray flag bits, kvflag bits
    outside 0xCFFF, keys outside the blob; sklen above 320 walks and misses."""
    n = len(SKLENS)
    keys = [0x9000 + 0x100 * nr + nr for nr in range(n)]
    rec = make_table(8100, n, 4, keys, {nr: dict(flags=KV_STR | 0x33, klen=k, vlen=k + 5 if k + 5 <= 320 else 320)
                                         for nr, k in enumerate(SKLENS)})
    blob, rows = Blob(), []
    for nr, k in enumerate(SKLENS):
        value = kv_fields(rec, nr)[4]
        skey = value[:min(k, 320)]
        after = value[k] ^ 0xFF if k < 320 else 0x77
        for residue in range(8):
            at = blob.put(skey, residue, after) if k <= 320 else 0
            rows.append((keys[nr], 0, GET, KV_STR, at, k))
        if 0 < k <= 320:
            rows.append((keys[nr], 0, GET, KV_STR, blob.put(skey[:-1] + bytes([skey[-1] ^ 1]), 3, after), k))
            rows.append((keys[nr], 0, GET, KV_STR, blob.put(bytes([skey[0] ^ 0x80]) + skey[1:], 3, after), k))
            rows.append((keys[nr], 0, GET, KV_STR, blob.put(skey, 5, after), k - 1))        # klen differs
            rows.append((keys[nr] ^ (1 << 50), 0, GET, KV_STR, blob.put(skey, 6, after), k))   # v.key differs
    at = blob.put(kv_fields(rec, 4)[4][:9], 2, 0)
    good = (keys[4], 0, GET, KV_STR, at, 9)
    rows.append(good)
    for stray in (0x1, 0x2, 0x4, 0x8, 0x20, 0x80, 0x100, 0x01000000, 0x02000000, 0x20000000, 0x80000000):
        rows.append((keys[4], 0, GET | stray, KV_STR, at, 9))
    for bad in (0x1000, 0x2000, 0x10000, 0x80000000):
        rows.append((keys[4], 0, GET, KV_STR | bad, at, 9))
        rows.append((keys[4], 0, GET, KV_NORMAL | bad, at, 9))
    rows.append((keys[4], 0, GET, KV_STR | KV_NORMAL, at, 9))           # both kinds: STR is tested first
    end = len(blob.bytes)
    rows.append((keys[4], 0, GET, KV_STR, end - 3, 4))                  # one byte past the blob
    rows.append((keys[0], 0, GET, KV_STR, end, 0))                      # empty, at the end: allowed
    rows.append((keys[0], 0, GET, KV_STR, end + 1, 0))
    rows.append((keys[4], 0, GET, KV_STR, 0xFFFFFFFF, 9))
    rows.append((keys[4], 0, GET, KV_NORMAL, 0xFFFFFFFF, 0xFFFFFFFF))   # a NORMAL get reads neither field
    rows.append((keys[10], 0, GET, KV_STR, 0xFFFFFFFF, 321))            # walks, misses; the blob is not read
    rows.append((keys[10], 0, GET, KV_STR, 0, 0xFFFFFFFF))
    return [rec], [4], rows_to_req(rows), bytes(blob.bytes)


def family_corners():
    """ITB 0 (adepth 3): a NORMAL get that hits a STR entry with the same
    v.key, and a STR get that hits a NORMAL entry; three entries with one v.key
    and klen 3, 5, 3 on one chain (add_index leaves it as 4, 2, 3: the first wins); a
    hit on an entry with neither kind flag; one with v.len 321.  ITBs 1 and 2:
    every entry hashed to one home slot, chains of 8 and of 1,024 hops."""
    k_str, k_nrm, k_dup, k_none, k_long = 0xA001, 0xA002, 0xA003, 0xA004, 0xA005
    kv = {0: dict(flags=KV_STR, key=k_str, klen=4, vlen=30), 1: dict(flags=KV_NORMAL, key=k_nrm, klen=6, vlen=44),
          2: dict(key=k_dup, flags=KV_STR, klen=3, vlen=10, value=b"abcZ"),
          3: dict(key=k_dup, flags=KV_STR, klen=5, vlen=11, value=b"abcdeZ"),
          4: dict(key=k_dup, flags=KV_STR, klen=3, vlen=12, value=b"abcY"),
          5: dict(flags=0x3FFF, key=k_none, vlen=8), 6: dict(flags=0xFFFF0000, key=k_none + 8, vlen=8),
          7: dict(flags=KV_NORMAL, key=k_long, vlen=321)}
    a = make_table(8200, 8, 3, [k_str, k_nrm, k_dup, k_dup, k_dup, k_none, k_none + 8, k_long], kv)
    blob = Blob()
    v0, v1 = kv_fields(a, 0)[4], kv_fields(a, 1)[4]
    rows = [(k_str, 0, GET, KV_NORMAL, 0, 0), (k_str, 0, GET, KV_STR, blob.put(v0[:4]), 4),
            (k_nrm, 0, GET, KV_STR, blob.put(v1[:6]), 6), (k_nrm, 0, GET, KV_STR, blob.put(v1[:5]), 5),
            (k_nrm, 0, GET | F_COLUMN, KV_STR | 3, blob.put(v1[:6], 1), 6),
            (k_dup, 0, GET, KV_NORMAL, 0, 0), (k_dup, 0, GET, KV_STR, blob.put(b"abc", 7), 3),
            (k_dup, 0, GET, KV_STR, blob.put(b"abcde", 3), 5), (k_dup, 0, GET, KV_STR, blob.put(b"abcd"), 4),
            (k_none, 0, GET, KV_NORMAL, 0, 0), (k_none + 8, 0, GET | F_COLUMN, KV_NORMAL | 1, 0, 0),
            (k_long, 0, GET, KV_NORMAL, 0, 0), (k_long, 0, GET | F_COLUMN, KV_NORMAL, 0, 0)]
    short_keys = [5 + 8 * (nr + 1) for nr in range(8)]
    short = make_table(8201, 8, 3, short_keys)
    long_keys = [77 + 1024 * (nr + 1) for nr in range(1024)]
    long_ = make_table(8202, 1024, 10, long_keys)
    rows += [(k, 1, GET, KV_NORMAL, 0, 0) for k in short_keys] + [(5 + 8 * 99, 1, GET, KV_NORMAL, 0, 0)]
    picks = sorted(set(range(0, 1024, 37)) | {0, 1, 1022, 1023})
    rows += [(long_keys[nr], 2, GET | (F_COLUMN if nr % 2 else 0), KV_NORMAL | nr % 6, 0, 0) for nr in picks]
    rows.append((77 + 1024 * 5000, 2, GET, KV_NORMAL, 0, 0))
    return [a, short, long_], [3, 3, 10], rows_to_req(rows), bytes(blob.bytes)


def family_handmade():
    """One adepth-3 record of 8 ITEs whose table is set slot by slot, one home
    slot a case (as lookup_util.family_handmade; v.key's low bits name the
    slot):
      1  a UNIQUE slot that misses, with a populated conflict: nothing past it is found
      2  flag OVERFLOW, followed like CONFLICT
      3  conflict 2048: the loop ends as a miss
      4  a self-loop;  5: a 2-cycle -- POM_LK_E_LOOP with depth 2048 on a miss
      6  entry 8, whose ITE ends past the payload;  7: entry 32,767
    and the same record one byte short, where ITE 7 no longer fits."""
    slot_of = {0: 1, 1: 1, 2: 2, 3: 2, 4: 3, 5: 4, 6: 5, 7: 5}
    keys = {nr: 0xB000 + 0x100 * nr + slot for nr, slot in slot_of.items()}
    rec = make_table(8300, 8, 3, {}, {nr: dict(flags=KV_NORMAL, key=k, vlen=9 + nr) for nr, k in keys.items()})
    set_slot(rec, H, 1, 0, 9, IDX_UNIQUE)
    set_slot(rec, H, 9, 1, 0, IDX_UNIQUE)
    set_slot(rec, H, 2, 2, 10, IDX_OVERFLOW)
    set_slot(rec, H, 10, 3, 0, IDX_UNIQUE)
    set_slot(rec, H, 3, 4, 2048, IDX_CONFLICT)
    set_slot(rec, H, 4, 5, 4, IDX_CONFLICT)
    set_slot(rec, H, 5, 6, 13, IDX_CONFLICT)
    set_slot(rec, H, 13, 7, 5, IDX_OVERFLOW)
    set_slot(rec, H, 6, 8, 0, IDX_UNIQUE)
    set_slot(rec, H, 7, 32767, 9, IDX_CONFLICT)
    (ln,) = struct.unpack_from("<I", rec, 240)
    short = bytearray(rec[: ln - 1])
    struct.pack_into("<I", short, 240, ln - 1)
    set_slot(short, H, 6, 7, 0, IDX_UNIQUE)             # ITE 7 is cut, ITE 6 (slot 5) is whole
    rows = []
    for itb in (0, 1):
        rows += [(keys[0], itb, GET, KV_NORMAL, 0, 0), (keys[1], itb, GET, KV_NORMAL, 0, 0),         # 1: hit, ENOENT at depth 1
                 (keys[2], itb, GET, KV_NORMAL, 0, 0), (keys[3], itb, GET | F_COLUMN, KV_NORMAL | 5, 0, 0),
                 (0xC002, itb, GET, KV_NORMAL, 0, 0),                                                  # 2: miss at depth 2
                 (keys[4], itb, GET, KV_NORMAL, 0, 0), (0xC003, itb, GET, KV_NORMAL, 0, 0),            # 3
                 (keys[5], itb, GET, KV_NORMAL, 0, 0), (0xC004, itb, GET, KV_NORMAL, 0, 0),            # 4: the head hits; a miss loops
                 (keys[6], itb, GET, KV_NORMAL, 0, 0), (keys[7], itb, GET, KV_NORMAL, 0, 0),
                 (0xC005, itb, GET, KV_NORMAL, 0, 0), (0xC005, itb, GET, KV_STR, 0, 0),               # 5
                 (0xC006, itb, GET, KV_NORMAL, 0, 0), (keys[7] + 1, itb, GET, KV_NORMAL, 0, 0),       # 6
                 (0xC007, itb, GET, KV_NORMAL, 0, 0)]                                                  # 7
    return [rec, short], [3, 3], rows_to_req(rows), b""


def family_mixed(n: int = 24):
    """n records with adepth 1 ... 10 and 1 ... 40 ITEs, seeded keys, so chains
    of every short length form; NORMAL and STR entries with v.len over VLENS's
    legal values and seeded ones; every entry by its key (a column now and
    then), and runs of misses between the hits: an absent key of the same home
    slot, a string key with its last byte changed, a klen that differs."""
    rng = np.random.default_rng(0x4B47)
    recs, adepths, rows, blob = [], [], [], Blob()
    for b in range(n):
        adepth = 1 + b % 10
        n_ites = min(1 << adepth, (1, 2, 5, 13, 40, 24, 31, 17, 8, 3, 40, 11)[b % 12])
        keys = L.spread_hashes(0x600 + b, n_ites)
        kv = {}
        for nr in range(n_ites):
            vlen = int(rng.choice(VLENS[:-1])) if rng.random() < 0.5 else int(rng.integers(0, 90))
            if nr % 3 == 1:
                kv[nr] = dict(flags=KV_STR, klen=int(rng.integers(0, 24)), vlen=vlen)
            else:
                kv[nr] = dict(flags=KV_NORMAL | (KV_STR if nr % 5 == 0 else 0), vlen=vlen)
        rec = make_table(8400 + b, n_ites, adepth, keys, kv)
        recs.append(rec)
        adepths.append(adepth)
        for nr in range(n_ites):
            flags, _, key, klen, value = kv_fields(rec, nr)
            col = (F_COLUMN, int(rng.integers(0, 6))) if rng.random() < 0.3 else (0, 0)
            if nr % 3 == 1:
                rows.append((key, b, GET | col[0], KV_STR | col[1], blob.put(value[:klen]), klen))
                if klen:
                    for _ in range(int(rng.integers(0, 4))):
                        rows.append((key, b, GET, KV_STR, blob.put(value[:klen - 1] + bytes([value[klen - 1] ^ 4])), klen))
                rows.append((key, b, GET, KV_STR, blob.put(value[:klen + 1]), klen + 1))
            else:
                rows.append((key, b, GET | col[0], KV_NORMAL | col[1], 0, 0))
            for _ in range(int(rng.integers(0, 5)) if nr % 4 == 0 else 0):
                rows.append((key ^ (1 << int(rng.integers(11, 60))), b, GET | col[0], KV_NORMAL | col[1], 0, 0))
    return recs, adepths, rows_to_req(rows), bytes(blob.bytes)


FAMILIES = {"values": family_values, "strkeys": family_strkeys, "corners": family_corners,
            "handmade": family_handmade, "mixed": family_mixed}


def rule_order_case():
    """itb >= nitb, then status, adepth, the index table's presence, then the
    request's own checks: (records, adepths, status, req, keys)."""
    recs, _, req, _ = family_corners()
    rec = recs[1]
    key = 5 + 8 * 3
    rows = [(key, b, flag, KV_NORMAL, 0, 0) for b in (0, 1, 2, 3, 4, 5, 0xFFFFFFFF) for flag in (GET, GET | 0x4)]
    short = bytearray(rec[: H + ITE_OFF - 1])
    struct.pack_into("<I", short, 240, len(short))
    return [rec, rec, rec, short, rec], [3, 3, 0, 3, 11], [0, -6, -5, 0, 0], rows_to_req(rows), b""
