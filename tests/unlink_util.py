"""The ITB unlink's test oracle and table builders (shared by test_unlink.py and
test_gpu_unlink.py).

expect_one() restates the INDEX_UNLINK path of itb_search (mds/itb.c:1769-1797
the walk with lookup_util.ite_match, :1889-1911 the branch), ite_unlink
(:676-735) and itb_del_ite (:602-671) in Python on check_util.Table, whose
_unlink() already restates __ite_unlink (:567-592), and applies a request list
in order; header() is the struct itbh the unlinks leave, expect() the rules of
include/pom_unlink.h around them.  Nothing here reads the product's
itb_unlink.h.

Like the sweep's, the sequence cannot be pinned by a golden fixture: calling
itb_search itself needs the MDS's locks, txg and profile counters.  So this
restatement is reviewed against the cited lines, and the tests hold it to
invariants(): what is produced is clean under check() with its header facts,
and only the permitted bytes change."""
from __future__ import annotations

import struct

import numpy as np

import check_util as C
import itb_split_util as S
import lookup_util as L
from check_util import (BITMAP_OFF, EINVAL, H, IDX_CONFLICT, IDX_FREE, IDX_UNIQUE, INDEX_OFF, ITB_SIZE,  # noqa: F401
                        ITBH_ENTRIES, ITBH_ITU, ITBH_LEN, ITBH_MAX_OFFSET, ITBH_PSEUDO, ITE_OFF, ITE_SIZE, Table,
                        get_slot, set_slot)
from itb_split_util import E_DAMAGED, E_OUTPUT_OVERRUN, table_of  # noqa: F401
from lookup_util import BY_NAME, BY_UUID, ENOENT, ESPLIT, F_ACTIVE, F_SHADOW, MDU_SIZE, MD_OFF, REC_SIZE, ZERO  # noqa: F401
from readdir_util import set_ite

UNLINK = 0x00200000                                     # INDEX_UNLINK
ALLOWED = UNLINK | BY_NAME | BY_UUID | F_ACTIVE | F_SHADOW
NORMAL, LS, SDT, SYM, KV = 0x80000000, 0x40000000, 0x10000000, 0x02000000, 0x01000000
STATE_MASK, UNLINKED, SHADOW = 7, 1, 3
FLAG_OFF, MODE_OFF, NLINK_OFF = 16, 36, 38
S_IFDIR = 0o040000
NONE, SHADOWED, MARKED, DELETED, DELTA = 0, 1, 2, 3, 0x100
RESULT = struct.Struct("<iIIIiiiHH")
RESULT_FIELDS = ("err", "changed", "removed", "len", "entries", "max_offset", "pseudo_conflicts", "itu", "hits")
assert RESULT.size == 32


def result_fields(raw) -> dict:
    return dict(zip(RESULT_FIELDS, RESULT.unpack(bytes(raw))))


# ---------------------------------------------------------------------------
# ite_unlink and itb_del_ite
# ---------------------------------------------------------------------------
def ite_unlink(flag: int, mode: int, nlink: int, async_: bool):
    """mds/itb.c:676-716 on (e->flag, s.mdu.mode, s.mdu.nlink): (flag, nlink,
    what with DELTA, whether itb_del_ite is called), or None for the flags
    include/pom_unlink.h refuses (KV together with NORMAL, SYM or LS, where the
    reference would call itb_del_ite twice)."""
    if flag & KV and flag & (NORMAL | SYM | LS):
        return None
    what, delete = NONE, False
    if flag & NORMAL or flag & SYM:
        nlink = (nlink - 1) & 0xFFFF                                # e->s.mdu.nlink--, a u16
        if mode & S_IFDIR:
            nlink = (nlink - 1) & 0xFFFF
        if not nlink:
            if async_:
                flag = (flag & ~STATE_MASK) | UNLINKED
                what = MARKED
            else:
                what, delete = DELETED, True
        else:
            flag = (flag & ~STATE_MASK) | SHADOW
            what = SHADOWED
    elif flag & LS:
        nlink = 0
        what, delete = DELETED, True
    if flag & KV:
        what, delete = DELETED, True
    if flag & SDT and (flag & KV or nlink == 0):                    # goto do_delta, or the nlink == 0 test
        what |= DELTA
    return flag, nlink, what, delete


def del_ite(t: Table, offset: int, pos: int) -> int:
    """itb_del_ite(i, e, offset, pos) (mds/itb.c:602-671): offset is the slot
    to delete, pos the home slot.  -> __ite_unlink calls."""
    rec, total = t.rec, 2 * t.d
    slot = lambda o: get_slot(rec, H, o)
    before = len(t.hashes)
    if slot(pos)[2] == IDX_FREE:
        return 0
    if slot(pos)[2] == IDX_UNIQUE:
        if offset == pos:
            t._unlink(offset)
        return before - len(t.hashes)
    saved = prev = pos
    pos, offset = offset, saved
    quit_ = needswap = hit = False
    steps = 0
    while True:                                                     # do { retry:
        steps += 1
        assert steps <= 2 * total, "the loop does not end"
        entry, conflict, flag = slot(offset)
        if flag == IDX_FREE:
            break
        if pos == offset or hit:
            if offset == saved:
                needswap, prev = True, offset
            elif flag == IDX_UNIQUE:
                pe, pc, _ = slot(prev)
                set_slot(rec, H, prev, pe, pc, IDX_UNIQUE)
                t._unlink(offset)
                quit_ = True
            else:
                pe, _, pf = slot(prev)
                set_slot(rec, H, prev, pe, conflict, pf)
                t._unlink(offset)
                quit_ = True
        else:
            if needswap:
                se, sc, sf = slot(saved)
                set_slot(rec, H, offset, se, conflict, flag)
                set_slot(rec, H, saved, entry, sc, sf)
                needswap, hit = False, True
                continue                                            # goto retry
            if flag == IDX_UNIQUE:
                quit_ = True
            prev = offset
        offset = conflict
        if not (offset < total and not quit_):
            break
    assert not needswap, "a head that no slot followed: the check rules it out"
    return before - len(t.hashes)


# ---------------------------------------------------------------------------
# The request list, in order
# ---------------------------------------------------------------------------
def request_ok(q: dict, names: bytes) -> bool:
    return not (q["flag"] & ~ALLOWED or q["namelen"] > 255 or q["column"] != 0 or
                q["name_off"] + q["namelen"] > len(names))


def unlink_one(t: Table, q: dict, names: bytes, async_: bool, facts: dict):
    """One request on t as the earlier ones left it: (err, nr, depth, what,
    record).  mds/itb.c:1769-1797, then :1889-1911."""
    if not request_ok(q, names):
        return EINVAL, 0, 0, 0, ZERO
    rec = t.rec
    pos = offset = q["hash"] & (t.d - 1)
    depth = 0
    while offset < 2 * t.d:
        entry, conflict, flag = get_slot(rec, H, offset)
        if flag == IDX_FREE:
            break
        depth += 1
        assert depth <= t.d + 1, "the walk does not end"
        ite = H + ITE_OFF + ITE_SIZE * entry
        if L.ite_match(rec, ite, q, names):
            eflag, = struct.unpack_from("<I", rec, ite + FLAG_OFF)
            mode, nlink = struct.unpack_from("<HH", rec, ite + MODE_OFF)
            did = ite_unlink(eflag, mode, nlink, async_)
            if did is None:
                return EINVAL, 0, depth, 0, ZERO
            record = bytes(rec[ite + 8: ite + 16]) + bytes(rec[ite + MD_OFF: ite + MD_OFF + MDU_SIZE]) + bytes(24)
            eflag, nlink, what, delete = did
            struct.pack_into("<I", rec, ite + FLAG_OFF, eflag)
            struct.pack_into("<H", rec, ite + NLINK_OFF, nlink)
            if delete:
                facts["removed"] += del_ite(t, offset, pos)
            facts["changed"] += (what & 0xFF) != NONE
            facts["hits"] += 1
            return 0, entry, depth, what, record
        if flag == IDX_UNIQUE:
            break
        offset = conflict
    return ENOENT, 0, depth, 0, ZERO


class Unlink:
    """What one ITB's requests must leave: result (32 bytes), the payload
    after them, and per request (err, nr, depth, what, record)."""

    def __init__(self, result, payload, answers):
        self.result, self.payload, self.answers = result, payload, answers

    @property
    def fields(self):
        return result_fields(self.result)

    @property
    def produced(self):
        f = self.fields
        return f["err"] == 0 and f["changed"] > 0


def _only(err: int, hits: int = 0) -> bytes:
    return RESULT.pack(err, *([0] * 7), hits)


def expect_one(payload, adepth: int, hdr: dict, reqs, names: bytes = b"", async_: bool = False, b: int = 0,
               payload_off: int = 0, status: int = 0) -> Unlink:
    """reqs: the group's request dicts (lookup_util.as_dicts) in order."""
    payload = bytes(payload)
    code = status
    if not code:
        code, report, _, _ = C.check(payload, adepth, hdr, 0)
    if not code and payload_off % 16:
        code = EINVAL
    if not code and C.report_fields(report)["findings"] & ~(1 << C.E_MISPLACED):
        code = E_DAMAGED
    if code:
        return Unlink(_only(code), payload, [(EINVAL if q["itb"] != b else code, 0, 0, 0, ZERO) for q in reqs])
    t = table_of(payload, adepth, hdr)
    facts = dict(removed=0, changed=0, hits=0)
    answers = [(EINVAL, 0, 0, 0, ZERO) if q["itb"] != b else unlink_one(t, q, names, async_, facts) for q in reqs]
    hits = min(facts["hits"], 0xFFFF)
    if facts["changed"] == 0:
        return Unlink(_only(0, hits), payload, answers)
    i32 = lambda off: struct.unpack_from("<i", t.rec, off)[0]
    (itu,) = struct.unpack_from("<H", t.rec, ITBH_ITU)
    # (h.len follows __ite_unlink; with nothing removed it is the header's own)
    ln = i32(ITBH_LEN) if facts["removed"] else hdr["ulen"]
    result = RESULT.pack(0, facts["changed"], facts["removed"], ln, i32(ITBH_ENTRIES), i32(ITBH_MAX_OFFSET),
                         i32(ITBH_PSEUDO), itu, hits)
    return Unlink(result, bytes(t.rec[H: H + len(payload)]), answers)


def group(req: np.ndarray, nitb: int):
    """A caller's requests grouped by ITB, stably: (the order, req_first)."""
    itb = req["itb"].astype(np.int64)
    order = np.array([r for b in range(nitb) for r in np.flatnonzero(itb == b)], dtype=np.int64)
    first = np.zeros(nitb + 1, np.uint32)
    for b in range(nitb):
        first[b + 1] = first[b] + int((itb == b).sum())
    return order, first


def expect(payloads, adepths, hdrs, req: np.ndarray, req_first, names: bytes = b"", async_: bool = False,
           payload_offs=None, status=None):
    """A call as pom_itb_unlink_dev sees it (req grouped, req_first[nitb + 1]):
    ([Unlink per ITB], err[], nr[], depth[], what[], out[nreq, 136])."""
    n = len(req)
    err, nr, depth, what = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    out = np.zeros((n, REC_SIZE), np.uint8)
    dicts = L.as_dicts(req)
    pick = lambda a, b, default: default if a is None else a[b]
    per = []
    for b in range(len(payloads)):
        r0, r1 = int(req_first[b]), int(req_first[b + 1])
        u = expect_one(payloads[b], adepths[b], hdrs[b], dicts[r0:r1], names, async_, b, pick(payload_offs, b, 0),
                       pick(status, b, 0))
        per.append(u)
        for r, a in zip(range(r0, r1), u.answers):
            err[r], nr[r], depth[r], what[r] = a[:4]
            out[r] = np.frombuffer(a[4], np.uint8)
    return per, err, nr, depth, what, out


def changed_hdr(hdr: dict, f: dict) -> dict:
    return dict(hdr, entries=f["entries"], max_offset=f["max_offset"], pseudo_conflicts=f["pseudo_conflicts"],
                itu=f["itu"], ulen=f["len"])


def permitted_mask(n: int, hit_ites) -> np.ndarray:
    """The payload bytes a call may change: the bitmap, the index, bytes 16-19
    and 38-39 of the ITEs a request hit."""
    m = np.zeros(n, bool)
    m[BITMAP_OFF:ITE_OFF] = True
    for nr in hit_ites:
        at = ITE_OFF + ITE_SIZE * nr
        m[at + 16: at + 20] = True
        m[at + 38: at + 40] = True
    return m


def invariants(payload, adepth: int, hdr: dict, u: Unlink):
    """What the contract relies on, for an ITB whose requests changed
    something: only the permitted bytes differ, the counters add up, and the
    produced payload is clean under the check with its new header facts."""
    f = u.fields
    before, after = np.frombuffer(bytes(payload), np.uint8), np.frombuffer(u.payload, np.uint8)
    assert f["err"] == 0 and f["changed"] > 0 and len(after) == len(before)
    hits = [a[1] for a in u.answers if a[0] == 0]
    assert f["hits"] == len(hits) and f["changed"] <= len(hits)
    assert (after == before)[~permitted_mask(len(before), hits)].all()
    deleted = sum(1 for a in u.answers if a[0] == 0 and a[3] & 0xFF == DELETED)
    assert f["removed"] == deleted and f["entries"] == hdr["entries"] - deleted
    assert f["len"] <= hdr["ulen"] and (f["entries"] or (f["max_offset"], f["len"]) == (0, ITB_SIZE))
    e, report, _, _ = C.check(u.payload[: f["len"] - H], adepth, changed_hdr(hdr, f), 0)
    assert e == 0 and C.report_fields(report)["findings"] == 0, C.report_fields(report)


def header(old_hdr, result, z=None):
    """pom_itb_unlink_header: (the struct itbh after the unlinks, whether the
    record is stored compressed); z: the stream's size, None: none."""
    f = result_fields(result)
    h = bytearray(old_hdr[:H])
    struct.pack_into("<ii", h, ITBH_ENTRIES, f["entries"], f["max_offset"])
    struct.pack_into("<i", h, ITBH_PSEUDO, f["pseudo_conflicts"])
    struct.pack_into("<H", h, ITBH_ITU, f["itu"])
    lzo = S._stored_as(h, f["len"], z)
    return bytes(h), int(lzo)


def stored_record(oracle, old_hdr, u: Unlink) -> bytes:
    """An ITB after its unlinks as itb_lzo_compress stores it."""
    p = u.payload[: u.fields["len"] - H]
    z = oracle.compress(p)
    h, lzo = header(old_hdr, u.result, len(z))
    return h + (z if lzo else p)


# ---------------------------------------------------------------------------
# Tables.  Table.add fills an ITE with random bytes; entry() gives it the
# fields the unlink reads.
# ---------------------------------------------------------------------------
def entry(t: Table, nr: int, flag: int = NORMAL, nlink: int = 1, mode: int = 0o100644, name=None, uuid=None):
    """ITE nr: its flag, nlink, mode, name (default b"e<nr>") and uuid
    (default 1000 + nr)."""
    set_ite(t.rec, H, nr, flag=flag, name=b"e%d" % nr if name is None else name, uuid=1000 + nr if uuid is None else uuid,
            mode=mode)
    struct.pack_into("<H", t.rec, H + ITE_OFF + ITE_SIZE * nr + NLINK_OFF, nlink)
    return t


def built(adepth: int, seed: int, hashes, **fields) -> Table:
    """S._built with every ITE given entry()'s fields."""
    t = S._built(adepth, seed, hashes)
    for nr in t.hashes:
        entry(t, nr, **fields)
    return t


def by_name(t_or_rec, itb: int, nr: int, extra: int = 0, name=None) -> dict:
    """The request that finds ITE nr by its name (or `name`)."""
    rec = t_or_rec.rec if isinstance(t_or_rec, Table) else t_or_rec
    hsh, _, _, _, nm = L.ite_fields(rec, H, nr)
    return dict(itb=itb, hash=hsh, flag=BY_NAME | UNLINK | extra, name=nm if name is None else name)


def by_uuid(t_or_rec, itb: int, nr: int, extra: int = 0) -> dict:
    rec = t_or_rec.rec if isinstance(t_or_rec, Table) else t_or_rec
    hsh, uuid, _, _, _ = L.ite_fields(rec, H, nr)
    return dict(itb=itb, hash=hsh, uuid=uuid, flag=BY_UUID | extra)


def chain_of(t: Table, home: int):
    """[(slot, ITE)] of home's chain, head first."""
    out, offset = [], home
    while True:
        e, conflict, flag = get_slot(t.rec, H, offset)
        if flag == IDX_FREE:
            return out
        out.append((offset, e))
        if flag == IDX_UNIQUE:
            return out
        offset = conflict


def live_chains(payload, adepth: int) -> dict:
    """home slot -> the set of ITEs on its chain."""
    t = Table(adepth)
    t.rec[H: H + len(payload)] = payload
    return {h: {e for _, e in chain_of(t, h)} for h in range(t.d) if get_slot(t.rec, H, h)[2] != IDX_FREE}


FLAG_KINDS = (("none", 0), ("normal", NORMAL), ("sym", SYM), ("ls", LS), ("kv", KV), ("normal_ls", NORMAL | LS),
              ("kv_normal", KV | NORMAL), ("kv_sym", KV | SYM), ("kv_ls", KV | LS))
NLINKS = (0, 1, 2, 3, 65535)
MODES = (0o100644, 0o040755, 0o060660, 0o140777)


def ite_unlink_cases():
    """The exhaustive table: (flag, mode, nlink, async)."""
    for _, kind in FLAG_KINDS:
        for sdt in (0, SDT):
            for state in range(8):
                for nlink in NLINKS:
                    for mode in MODES:
                        for async_ in (False, True):
                            yield kind | sdt | state, mode, nlink, async_


def random_case(seed: int):
    """A seeded table of adepth 1 ... 4 with 1 ... 12 requests: (record,
    adepth, request dicts for ITB 0, async)."""
    rng = np.random.default_rng(seed ^ 0x0DD)
    adepth = int(rng.integers(1, 5))
    d = 1 << adepth
    t = C.random_table(seed, adepth, 2 * d + 3)
    kinds = [NORMAL, NORMAL | SDT, SYM, LS, KV, KV | SDT, 0, NORMAL | KV, NORMAL | LS]
    for nr in sorted(t.hashes):
        entry(t, nr, flag=int(rng.choice(kinds)) | int(rng.choice([0, 0, 0, 1, 3])), nlink=int(rng.integers(0, 4)),
              mode=int(rng.choice(MODES)), name=b"n%d" % int(rng.integers(0, max(2, d // 2))))
    live = sorted(t.hashes)
    items = []
    for _ in range(int(rng.integers(1, 13))):
        if not live:
            items.append(dict(itb=0, hash=int(rng.integers(0, d)), flag=BY_NAME, name=b"n0"))
            continue
        nr = int(rng.choice(live))
        extra = int(rng.choice([0, 0, F_SHADOW, F_ACTIVE]))
        items.append(by_name(t, 0, nr, extra) if rng.random() < 0.6 else by_uuid(t, 0, nr, extra))
    return t.record(), adepth, items, bool(rng.integers(0, 2))


# ---------------------------------------------------------------------------
# Directed cases: [(name, record, adepth, request dicts for ITB 0)].  A chain
# of k ITEs in home slot 0 is built by k adds of hashes with low bits 0: the
# second add goes behind the head, every later one in front of it.
# ---------------------------------------------------------------------------
UP = lambda i: i << 20                                  # tells the ITEs of one home slot apart


def chain3(adepth: int = 2, **fields) -> Table:
    t = built(adepth, 90, [0 | UP(i) for i in range(3)], **fields)
    assert [e for _, e in chain_of(t, 0)] == [2, 0, 1]
    return t


def del_ite_cases():
    """itb_del_ite at its edges, each a table of NORMAL files with nlink 1 and
    one request (a sync call deletes, an async one marks)."""
    out = []
    t = built(2, 91, [0, 1, 2])
    out.append(("unique_home", t, [by_name(t, 0, 1)]))
    t = built(1, 92, [0, 0 | UP(1)])
    out.append(("head_one_follower", t, [by_name(t, 0, chain_of(t, 0)[0][1])]))
    for which, k in (("head_two_followers", 0), ("middle", 1), ("tail", 2)):
        t = chain3()
        out.append((which, t, [by_name(t, 0, chain_of(t, 0)[k][1])]))
    t = built(3, 93, [5])
    out.append(("last_entry", t, [by_name(t, 0, 0)]))
    t = built(3, 94, [0, 1, 2, 3, 4, 5])
    out.append(("at_max_offset", t, [by_name(t, 0, 5)]))
    t = built(3, 94, [0, 1, 2, 3, 4, 5])
    out.append(("below_max_offset", t, [by_name(t, 0, 4)]))
    t = built(2, 95, [0, 0 | UP(1), 1])
    out.append(("overflow_half", t, [by_name(t, 0, chain_of(t, 0)[1][1])]))
    t = built(2, 95, [0, 0 | UP(1), 1])
    out.append(("home_half", t, [by_name(t, 0, 2)]))
    return [(name, t.record(), t.adepth, items) for name, t, items in out]


def order_cases():
    """The order within an ITB."""
    out = []
    t = built(2, 96, [3], nlink=2)
    out.append(("same_name_twice", t, [by_name(t, 0, 0)] * 2))
    t = built(2, 97, [1])
    out.append(("second_misses", t, [by_name(t, 0, 0)] * 2))
    # two entries of one name in one chain: the second request passes the first's ITE when that was only marked
    t = built(2, 98, [1, 1 | UP(1)], name=b"twin")
    out.append(("walks_past_marked", t, [by_name(t, 0, 0)] * 2))
    t = built(2, 98, [1, 1 | UP(1)], name=b"twin")
    out.append(("shadow_hits_marked", t, [by_name(t, 0, 0), by_name(t, 0, 0, F_SHADOW)]))
    t = chain3()
    head, second = chain_of(t, 0)[0][1], chain_of(t, 0)[1][1]
    out.append(("head_then_swapped", t, [by_name(t, 0, head), by_name(t, 0, second)]))
    t = built(1, 99, [1, 1 | UP(1)])
    out.append(("empties_chain", t, [by_name(t, 0, 0), by_name(t, 0, 1)]))
    t = built(1, 99, [1, 1 | UP(1)])
    out.append(("empties_chain_tail_first", t, [by_name(t, 0, 1), by_name(t, 0, 0)]))
    for name, (a, b) in (("order_ab", (0, 1)), ("order_ba", (1, 0))):
        t = chain3()
        ch = [e for _, e in chain_of(t, 0)]
        out.append((name, t, [by_name(t, 0, ch[a]), by_name(t, 0, ch[b])]))
    # a directory and its files, a hard link source, a key/value entry, an entry with no kind at all
    t = built(3, 100, [0, 1, 2, 3, 4])
    entry(t, 0, NORMAL | SDT, nlink=2, mode=0o040755)
    entry(t, 1, SYM, nlink=3)
    entry(t, 2, LS, nlink=7)
    entry(t, 3, KV | SDT, nlink=9)
    entry(t, 4, SDT, nlink=0)
    out.append(("kinds", t, [by_uuid(t, 0, nr) for nr in (0, 1, 2, 3, 4, 1, 1)]))
    return [(name, t.record(), t.adepth, items) for name, t, items in out]


def refused_cases():
    """Rule 9's flags, and every -EINVAL request rule beside two good
    requests that still apply."""
    t = built(2, 101, [0, 1, 2, 3])
    entry(t, 0, KV | NORMAL)
    entry(t, 1, KV | SYM)
    entry(t, 2, KV | LS)
    items = [by_uuid(t, 0, 0), by_uuid(t, 0, 1), by_uuid(t, 0, 2), by_name(t, 0, 3)]
    good = by_name(t, 0, 3)
    for bad in (0x10, 0x40, 0x00400000, 0x4, 0x80000000):          # LOOKUP, COLUMN, INDEX_KV and strays
        items.append(dict(good, flag=good["flag"] | bad))
    items.append(dict(good, column=1))
    return [("refused", t.record(), 2, items)]


def directed():
    return del_ite_cases() + order_cases() + refused_cases()


def call_of(cases, interleave: bool = False):
    """cases [(name, record, adepth, items)] as one call: ITB b is case b.
    -> (records, adepths, req in the caller's order, names).  interleave: the
    caller's order takes one request of each ITB in turn."""
    from pomegranate_amd import lookup
    items = []
    if interleave:
        k = 0
        while any(k < len(c[3]) for c in cases):
            items += [dict(c[3][k], itb=c[3][k]["itb"] + b) for b, c in enumerate(cases) if k < len(c[3])]
            k += 1
    else:
        for b, c in enumerate(cases):
            items += [dict(q, itb=q["itb"] + b) for q in c[3]]
    req, names = lookup.requests(items)
    return [c[1] for c in cases], [c[2] for c in cases], req, names
