"""The ITB split's test oracle and table builders (shared by test_itb_split.py
and test_gpu_itb_split.py).

split_tables() restates the loop of itb_split_local (mds/xtable.c:103-146) in
Python on check_util.Table, whose add() and delete() already restate
itb_add_ite / __itb_add_index and itb_del_ite / __ite_unlink; add_blob() is the
__itb_add_ite_blob wrapper (mds/itb.c:501-532), headers() the two struct itbh a
split leaves, expect() the rules of include/pom_split.h around them.  Nothing
here reads the product's itb_split.h.

The loop cannot be pinned by a golden fixture: a driver for it would have to
carry the reference's loop, and calling itb_split_local itself needs the MDS's
locks, txg and CBHT.  So this restatement is reviewed against the cited lines,
and the tests hold it to the invariants a CPU study of it found (invariants()):
the moved set is exactly the ITEs with the bit set, N's ITEs are numbered
0 ... moved - 1, O's ITE area and lock region do not change, neither record is
longer than O's was, both tables are clean under check() with the header facts
and POM_CK_ITBID, and the loop takes at most live + moved + 1 chain steps."""
from __future__ import annotations

import struct

import numpy as np

import check_util as C
from check_util import (BITMAP_OFF, EINVAL, H, IDX_CONFLICT, IDX_FREE, IDX_UNIQUE, INDEX_OFF, ITB_SIZE,  # noqa: F401
                        ITBH_ENTRIES, ITBH_INF, ITBH_ITU, ITBH_LEN, ITBH_MAX_OFFSET, ITBH_PSEUDO, ITE_OFF, ITE_SIZE,
                        Table, add_index, get_slot, set_hash)

E_DAMAGED = -4103
E_OUTPUT_OVERRUN = -5
DEPTH_MAX = 50
ITBH_FLAG, ITBH_STATE, ITBH_DEPTH, ITBH_ADEPTH, ITBH_CONFLICTS, ITBH_ITBID = 0, 1, 2, 3, 12, 136
ITBH_TWIN, ITBH_SPLIT_RLINK, ITBH_ZLEN, ITBH_ALGO = 208, 216, 244, 248
ITB_JUST_SPLIT, ITB_STATE_DIRTY = 2, 1
RESULT = struct.Struct("<iIIIiiiiiiHHHH")
RESULT_FIELDS = ("err", "moved", "old_len", "new_len", "old_entries", "new_entries", "old_max_offset",
                 "new_max_offset", "old_pseudo", "new_pseudo", "old_inf", "old_itu", "new_inf", "new_itu")
assert RESULT.size == 48


def result_fields(raw) -> dict:
    return dict(zip(RESULT_FIELDS, RESULT.unpack(bytes(raw))))


def moves(hsh: int, sd: int) -> bool:
    """(e.hash >> ITB_DEPTH) & (1UL << (depth - 1)), in u64."""
    return bool((hsh >> 10) & (1 << (sd - 1)) & C.M64)


# ---------------------------------------------------------------------------
# The loop
# ---------------------------------------------------------------------------
def table_of(payload, adepth: int, hdr: dict) -> Table:
    """A Table over a decoded payload and its header facts."""
    t = Table(adepth)
    t.rec[H: H + len(payload)] = payload
    for off, key in ((ITBH_ENTRIES, "entries"), (ITBH_MAX_OFFSET, "max_offset"), (ITBH_PSEUDO, "pseudo_conflicts")):
        struct.pack_into("<i", t.rec, off, hdr[key])
    struct.pack_into("<I", t.rec, ITBH_LEN, hdr["ulen"])
    struct.pack_into("<HH", t.rec, ITBH_INF, hdr["inf"], hdr["itu"])
    t.hashes = {nr: struct.unpack_from("<Q", t.rec, H + ITE_OFF + ITE_SIZE * nr)[0]
                for nr in range(t.d) if t._bit(nr)}
    return t


def add_blob(n: Table, ite: bytes) -> int:
    """__itb_add_ite_blob (mds/itb.c:501-532) with __itb_add_index's tail (:309-316)."""
    nr = next(k for k in range(n.d) if not n._bit(k))                  # find_first_zero_bit
    n._bit(nr, 1)
    at = H + ITE_OFF + ITE_SIZE * nr
    n.rec[at: at + ITE_SIZE] = ite
    (hsh,) = struct.unpack_from("<Q", ite, 0)
    offset = hsh & (n.d - 1)
    if get_slot(n.rec, H, offset)[2] in (IDX_UNIQUE, IDX_CONFLICT):
        n._i32(ITBH_PSEUDO, +1)
    add_index(n.rec, offset, nr)
    if n._i32(ITBH_MAX_OFFSET) <= nr:
        n._i32(ITBH_MAX_OFFSET, value=nr)
        n._i32(ITBH_LEN, value=ITB_SIZE + (nr + 1) * ITE_SIZE)
    n._i32(ITBH_ENTRIES, +1)
    n.hashes[nr] = hsh
    return nr


def split_tables(o: Table, sd: int):
    """mds/xtable.c:103-146 on O, into a fresh N (get_free_itb: everything
    zero, len = sizeof(struct itb), O's adepth).  For an adepth below 10 only
    the home half is scanned.  -> (N, [(old nr, new nr)] in move order, steps)"""
    n = Table(o.adepth)
    d = o.d
    pairs, steps, need_rescan = [], 0, False
    j = 0
    while j < d:                                                    # for (j = 0; ...) { rescan:
        if get_slot(o.rec, H, j)[2] == IDX_FREE:
            j += 1
            continue
        offset, rescan = j, False
        while True:                                                 # do {
            steps += 1
            assert steps <= 4 * d, "the loop does not end"
            entry, c, flag = get_slot(o.rec, H, offset)
            assert flag in (IDX_UNIQUE, IDX_CONFLICT), "a chain the check would have refused"
            done = flag == IDX_UNIQUE
            conflict = c if flag == IDX_CONFLICT else 0
            at = H + ITE_OFF + ITE_SIZE * entry
            (hsh,) = struct.unpack_from("<Q", o.rec, at)
            if moves(hsh, sd):
                assert (hsh & (d - 1)) == j
                pairs.append((entry, add_blob(n, bytes(o.rec[at: at + ITE_SIZE]))))
                o.delete(entry)                                     # itb_del_ite(oi, e, offset, j)
                if offset == j:
                    need_rescan = True
            if done:
                break
            if need_rescan:
                need_rescan, rescan = False, True
                break
            offset = conflict                                       # } while (1);
        if not rescan:
            j += 1
    return n, pairs, steps


# ---------------------------------------------------------------------------
# The rules of include/pom_split.h
# ---------------------------------------------------------------------------
class Split:
    """What one ITB's split must leave: result (48 bytes), the payload after
    it, N's payload (None when nothing is produced), and the loop's facts."""

    def __init__(self, result, payload, new_payload=None, pairs=(), steps=0, o=None, n=None):
        self.result, self.payload, self.new_payload = result, payload, new_payload
        self.pairs, self.steps, self.o, self.n = list(pairs), steps, o, n

    @property
    def fields(self):
        return result_fields(self.result)


def _only(err: int, moved: int = 0) -> bytes:
    return RESULT.pack(err, moved, *([0] * 12))


def expect_one(payload, adepth: int, hdr: dict, sd=None, payload_off: int = 0, new_off: int = 0, new_cap=None,
               status: int = 0) -> Split:
    payload = bytes(payload)
    new_cap = len(payload) if new_cap is None else new_cap
    sd = hdr["depth"] + 1 if sd is None else sd
    if status:
        return Split(_only(status), payload)
    err, report, _, _ = C.check(payload, adepth, hdr, 0)
    if err:
        return Split(_only(err), payload)
    if not 1 <= sd <= DEPTH_MAX:
        return Split(_only(EINVAL), payload)
    if payload_off % 16 or new_off % 16:
        return Split(_only(EINVAL), payload)
    if C.report_fields(report)["findings"] & ~(1 << C.E_MISPLACED):
        return Split(_only(E_DAMAGED), payload)
    o = table_of(payload, adepth, hdr)
    moved = sum(moves(h, sd) for h in o.hashes.values())
    if new_cap < ITE_OFF + ITE_SIZE * moved:
        return Split(_only(E_OUTPUT_OVERRUN, moved), payload)
    if moved == 0:
        return Split(_only(0), payload)
    n, pairs, steps = split_tables(o, sd)
    assert len(pairs) == moved
    i32 = lambda t, off: struct.unpack_from("<i", t.rec, off)[0]
    u16 = lambda t, off: struct.unpack_from("<H", t.rec, off)[0]
    result = RESULT.pack(0, moved, i32(o, ITBH_LEN), i32(n, ITBH_LEN), i32(o, ITBH_ENTRIES), i32(n, ITBH_ENTRIES),
                         i32(o, ITBH_MAX_OFFSET), i32(n, ITBH_MAX_OFFSET), i32(o, ITBH_PSEUDO), i32(n, ITBH_PSEUDO),
                         u16(o, ITBH_INF), u16(o, ITBH_ITU), u16(n, ITBH_INF), u16(n, ITBH_ITU))
    return Split(result, bytes(o.rec[H: H + len(payload)]), bytes(n.rec[H: i32(n, ITBH_LEN)]), pairs, steps, o, n)


def expect(payloads, adepths, hdrs, sds=None, payload_offs=None, new_offs=None, new_caps=None, status=None):
    n = len(payloads)
    pick = lambda a, b, default: default if a is None else a[b]
    return [expect_one(payloads[b], adepths[b], hdrs[b], pick(sds, b, None), pick(payload_offs, b, 0),
                       pick(new_offs, b, 0), pick(new_caps, b, None), pick(status, b, 0)) for b in range(n)]


def assert_same(got, want, payloads, names=None):
    """got: [(result, the payload after, the new payload's whole room after,
    steps or None)] against expect()'s answers: result, the payload, the new
    payload and the room behind it, which keeps its fill of 0x5A; for a split
    that produced something the step count too, where the caller has it."""
    for b, ((res, after, room, steps), w) in enumerate(zip(got, want)):
        what = names[b] if names else f"ITB {b}"
        assert result_fields(res) == w.fields, what
        assert after == w.payload, f"{what}: the payload"
        produced = w.new_payload or b""
        assert room[: len(produced)] == produced, f"{what}: the new payload"
        assert room[len(produced):] == b"\x5A" * (len(room) - len(produced)), f"{what}: bytes past the new payload"
        if w.new_payload is None:
            assert after == bytes(payloads[b]), f"{what}: nothing produced, yet the payload changed"
        elif steps is not None:
            assert steps == w.steps, f"{what}: steps"


def invariants(payload, adepth: int, hdr: dict, sd: int, s: Split, itbid: bool = True):
    """What the contract relies on, for a split that produced something.
    itbid=False: the halves are checked without POM_CK_ITBID (a table whose
    hashes do not carry its itbid below the split bit)."""
    f = s.fields
    before = table_of(payload, adepth, hdr)
    want = sorted(nr for nr, h in before.hashes.items() if moves(h, sd))
    assert f["err"] == 0 and f["moved"] == len(want) > 0
    assert sorted(old for old, _ in s.pairs) == want                            # the moved set
    assert [new for _, new in s.pairs] == list(range(len(want)))                # N numbered 0 ... moved - 1
    assert s.payload[:BITMAP_OFF] == bytes(payload[:BITMAP_OFF]) and s.payload[ITE_OFF:] == bytes(payload[ITE_OFF:])
    assert len(s.payload) == len(payload)
    assert f["old_len"] <= H + len(payload) and f["new_len"] <= H + len(payload)
    assert f["new_len"] == H + len(s.new_payload) == ITB_SIZE + ITE_SIZE * f["moved"]
    assert s.steps <= len(before.hashes) + f["moved"] + 1
    for old, new in s.pairs:
        assert s.new_payload[ITE_OFF + ITE_SIZE * new:][:ITE_SIZE] == bytes(payload[ITE_OFF + ITE_SIZE * old:][:ITE_SIZE])
    # both halves are clean, kind 15 included, under the headers the split leaves
    ohdr = dict(hdr, depth=sd, entries=f["old_entries"], max_offset=f["old_max_offset"],
                pseudo_conflicts=f["old_pseudo"], itu=f["old_itu"], ulen=f["old_len"])
    nhdr = dict(hdr, depth=sd, itbid=hdr["itbid"] | 1 << (sd - 1), entries=f["new_entries"],
                max_offset=f["new_max_offset"], pseudo_conflicts=f["new_pseudo"], inf=f["new_inf"], itu=f["new_itu"],
                ulen=f["new_len"])
    for p, h in ((s.payload[: f["old_len"] - H], ohdr), (s.new_payload, nhdr)):
        e, report, _, _ = C.check(p, adepth, h, C.CK_ITBID if itbid else 0)
        assert e == 0 and C.report_fields(report)["findings"] == 0, C.report_fields(report)


def _stored_as(h: bytearray, ulen: int, z):
    """itb_lzo_compress's rule (mds/itb.c:2904-2945): the stream is kept when it
    is smaller than the payload."""
    lzo = z is not None and z < ulen - H
    struct.pack_into("<IIH", h, ITBH_LEN, H + z if lzo else ulen, ulen if lzo else 0, 1 if lzo else 0)
    return lzo


def headers(old_hdr, sd: int, result, old_z=None, new_z=None):
    """pom_itb_split_headers: (O's struct itbh, N's, which of them is stored
    compressed as bits 0 and 1); old_z, new_z: the streams' sizes, None: none."""
    f = result_fields(result)
    o = bytearray(old_hdr[:H])
    o[ITBH_DEPTH] = sd
    struct.pack_into("<ii", o, ITBH_ENTRIES, f["old_entries"], f["old_max_offset"])
    struct.pack_into("<i", o, ITBH_PSEUDO, f["old_pseudo"])
    struct.pack_into("<H", o, ITBH_ITU, f["old_itu"])
    n = bytearray(o)
    bits = int(_stored_as(o, f["old_len"], old_z))
    n[ITBH_FLAG], n[ITBH_STATE] = ITB_JUST_SPLIT, ITB_STATE_DIRTY
    (itbid,) = struct.unpack_from("<Q", n, ITBH_ITBID)
    struct.pack_into("<Q", n, ITBH_ITBID, itbid | 1 << (sd - 1))
    struct.pack_into("<iii", n, ITBH_ENTRIES, f["new_entries"], f["new_max_offset"], 0)
    struct.pack_into("<i", n, ITBH_PSEUDO, f["new_pseudo"])
    struct.pack_into("<HH", n, ITBH_INF, f["new_inf"], f["new_itu"])
    struct.pack_into("<QQ", n, ITBH_TWIN, 0, 0)
    bits |= int(_stored_as(n, f["new_len"], new_z)) << 1
    return bytes(o), bytes(n), bits


def stored_records(oracle, old_hdr, sd: int, s: "Split"):
    """Both halves of a split that produced something as itb_lzo_compress
    stores them: lzo_record(oracle, record) where the oracle's stream is
    smaller than the payload, else the record uncompressed."""
    f = s.fields
    old_p, new_p = s.payload[: f["old_len"] - H], s.new_payload
    zo, zn = oracle.compress(old_p), oracle.compress(new_p)
    o, n, bits = headers(old_hdr, sd, s.result, len(zo), len(zn))
    return o + (zo if bits & 1 else old_p), n + (zn if bits & 2 else new_p)


# ---------------------------------------------------------------------------
# Tables.  Every hash carries the ITB's itbid below the split bit, so a table is
# clean under POM_CK_ITBID before the split and both halves are after it.
# ---------------------------------------------------------------------------
def random_split_table(seed: int, adepth: int, depth: int) -> Table:
    """check_util.random_table at `depth` (itbid: the low `depth` bits of the
    seed), run to about three quarters full: the bit above the itbid is random,
    so about half the ITEs move at sd = depth + 1."""
    d = 1 << adepth
    return C.random_table(seed, adepth, 2 * d + 3, depth=depth, itbid=seed & ((1 << depth) - 1))


def _built(adepth: int, seed: int, hashes) -> Table:
    t = Table(adepth, seed)
    for h in hashes:
        assert t.add(h) is not None
    return t


def _mark(t: Table, nr: int, sd: int):
    """ITE nr gets the move bit (its home slot stays: the bit lies above bit 9)."""
    t.hashes[nr] |= 1 << (9 + sd)
    set_hash(t.rec, nr, t.hashes[nr])


def _chain(t: Table, home: int):
    """The ITEs on home's chain, head first."""
    out, offset = [], home
    while True:
        entry, conflict, flag = get_slot(t.rec, H, offset)
        assert flag in (IDX_UNIQUE, IDX_CONFLICT)
        out.append(entry)
        if flag == IDX_UNIQUE:
            return out
        offset = conflict


def directed(adepth: int):
    """[(name, record, sd)]: one table per piece of the loop's machinery.
      none        nothing moves: a result, nothing produced
      all         everything moves: O ends empty, len 12168 and max_offset 0
      alternate   one chain of d ITEs with alternating move bits: head swaps
                  and rescans
      head, tail  one chain where only the head, only the tail moves
      stale       a moved UNIQUE head just before a chain whose head stays: the
                  need_rescan left set across the `done` break
      one_home    every moved ITE shares one home slot in N: N's overflow half
                  fills in inf order
      maxoff      the highest ITE moves while the one below it is dead:
                  __ite_unlink's max_offset-- lands on a dead ITE
      sd1, sd50   the deciding bit at hash bit 10 (59), every other bit from 10
                  up to 58 (11 up to 63) set in the ITEs that stay and clear in
                  those that move: the u64 shift"""
    d = 1 << adepth
    up = lambda i: i << 20                                          # tells the ITEs of one home slot apart
    out = []
    out.append(("none", _built(adepth, 1, [i % d | up(i) for i in range(d)]), 1))
    out.append(("all", _built(adepth, 2, [i % max(1, d // 2) | 1 << 10 | up(i) for i in range(d)]), 1))
    out.append(("alternate", _built(adepth, 3, [0 | (i & 1) << 10 | up(i) for i in range(d)]), 1))
    for which in ("head", "tail"):
        t = _built(adepth, 4, [(d - 1) | up(i) for i in range(d)])
        ch = _chain(t, d - 1)
        _mark(t, ch[0] if which == "head" else ch[-1], 1)
        out.append((which, t, 1))
    # home slot 0 holds one ITE, which moves; home slot 1 a chain whose head stays and whose second ITE moves
    t = _built(adepth, 5, [0 | up(1)] + [1 | up(2 + i) for i in range(min(3, d - 1))])
    _mark(t, 0, 1)
    ch = _chain(t, 1)
    if len(ch) > 1:
        _mark(t, ch[1], 1)
    out.append(("stale", t, 1))
    # the moving half hashes to home slot 0 of N; the rest is spread over O
    out.append(("one_home", _built(adepth, 6, [(0 | 1 << 10 | up(i)) if i % 2 else (i % d | up(i)) for i in range(d)]), 1))
    t = _built(adepth, 7, [i % d | up(i) for i in range(d)])
    if d > 2:
        t.delete(d - 2)
    _mark(t, d - 1, 1)
    out.append(("maxoff", t, 1))
    rest1 = C.M64 & ~((1 << 11) - 1)                                # bits 11 ... 63
    out.append(("sd1", _built(adepth, 8, [(i % d | 1 << 10) if i % 2 else (i % d | rest1) for i in range(d)]), 1))
    rest50 = ((1 << 59) - 1) & ~((1 << 10) - 1)                     # bits 10 ... 58
    out.append(("sd50", _built(adepth, 9, [(i % d | 1 << 59) if i % 2 else (i % d | rest50) for i in range(d)]), 50))
    return [(f"{name}@{adepth}", t.record(), sd) for name, t, sd in out]


def damaged_tables():
    """[(name, record, adepth)]: each table of kind_tables() but `valid` (and
    the two that are the valid one at no adepth), and the funnel."""
    out = [(name, rec, 2) for name, (rec, kinds, _, _) in C.kind_tables().items() if kinds]
    return out + [("funnel", C.funnel(), 10)]
