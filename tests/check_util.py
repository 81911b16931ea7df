"""The ITB check's test oracle and table builders (shared by test_check.py and
test_gpu_check.py).

check() restates the rules of include/pom_check.h in Python, over sets and a
colouring of the link graph; it does not look at the product's itb_check.h.
Table builds ITBs the way the MDS does: add() restates itb_add_ite's
bookkeeping (mds/itb.c:330-493) around lookup_util.add_index, delete() restates
itb_del_ite and __ite_unlink (:567-671)."""
from __future__ import annotations

import struct
from typing import NamedTuple, Optional

import numpy as np

from gc_scan_util import BITMAP_OFF, EINVAL, E_TRUNCATED, INDEX_OFF, ITE_OFF, ITE_SIZE, lzo_record  # noqa: F401
from lookup_util import (H, IDX_CONFLICT, IDX_FREE, IDX_OVERFLOW, IDX_UNIQUE, INDEX_ENTRIES, ITBH_ADEPTH,  # noqa: F401
                         ITBH_DEPTH, ITBH_INF, ITBH_ITBID, ITBH_ITU, add_index, get_slot, set_hash, set_slot)

ITBH_ENTRIES, ITBH_MAX_OFFSET, ITBH_PSEUDO, ITBH_LEN, ITBH_ZLEN, ITBH_ALGO = 4, 8, 16, 240, 244, 248
ITB_SIZE = H + ITE_OFF                                  # sizeof(struct itb)
CK_ITBID = 1
(S_OUTSIDE, S_FLAG, S_LINK_RANGE, S_LINK_HOME, S_LINK_FREE, S_ENTRY_RANGE, S_ENTRY_DEAD, S_SHARED, S_LEAKED,
 S_ISLAND, S_LOOP, S_MISFILED, E_STRAY, E_DUP, E_ORPHAN, E_MISPLACED, H_ENTRIES, H_ITU, H_PSEUDO, H_MAXOFF, H_LEN,
 H_INF) = range(22)
REPORT = struct.Struct("<IIHHHH16H")
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# The oracle
# ---------------------------------------------------------------------------
def hdr_of(rec) -> dict:
    """The header facts pom_itb_check_batch takes from a record's struct itbh."""
    entries, max_offset = struct.unpack_from("<ii", rec, ITBH_ENTRIES)
    (pseudo,) = struct.unpack_from("<i", rec, ITBH_PSEUDO)
    ln, zlen, algo = struct.unpack_from("<IIH", rec, ITBH_LEN)
    inf, itu = struct.unpack_from("<HH", rec, ITBH_INF)
    (itbid,) = struct.unpack_from("<Q", rec, ITBH_ITBID)
    return dict(entries=entries, max_offset=max_offset, pseudo_conflicts=pseudo, ulen=zlen if algo == 1 else ln,
                inf=inf, itu=itu, depth=rec[ITBH_DEPTH], itbid=itbid)


def hdr_bytes(h: dict) -> bytes:
    """struct pom_check_hdr."""
    return struct.pack("<iiiIHHB3xQ", h["entries"], h["max_offset"], h["pseudo_conflicts"], h["ulen"], h["inf"],
                       h["itu"], h["depth"], h["itbid"])


ZERO_REPORT = REPORT.pack(*([0] * 22))


def masks_of(bits, words: int):
    out = [0] * words
    for b in bits:
        out[b // 64] |= 1 << (b % 64)
    return out


def check(payload, adepth: int, hdr: "dict | None" = None, flags: int = 0):
    """(err, the report's 48 bytes, slot_mask [32], ite_mask [16]) of one
    decoded payload."""
    nothing = (ZERO_REPORT, [0] * 32, [0] * 16)
    if adepth < 1 or adepth > 10:
        return (EINVAL,) + nothing
    n = len(payload)
    if n < ITE_OFF:
        return (E_TRUNCATED,) + nothing
    d = 1 << adepth
    bitmap = payload[BITMAP_OFF:INDEX_OFF]
    bit = lambda nr: bitmap[nr // 8] >> (nr % 8) & 1
    live = [nr for nr in range(d) if bit(nr)]
    if live and ITE_OFF + ITE_SIZE * (live[-1] + 1) > n:
        return E_TRUNCATED, REPORT.pack(0, len(live), *([0] * 20)), [0] * 32, [0] * 16
    words = struct.unpack_from("<2048I", payload, INDEX_OFF)
    slots = [(w & 0x7FFF, (w >> 15) & 0x7FFF, w >> 30) for w in words]
    used = [f != IDX_FREE for _, _, f in slots]
    hash_of = lambda nr: struct.unpack_from("<Q", payload, ITE_OFF + ITE_SIZE * nr)[0]

    kinds = [set() for _ in range(INDEX_ENTRIES)]
    succ = [None] * INDEX_ENTRIES                       # the good link's target
    indeg = [0] * INDEX_ENTRIES
    refs = [0] * 1024
    for s, (entry, conflict, flag) in enumerate(slots):
        if not used[s]:
            continue
        if s >= 2 * d:
            kinds[s].add(S_OUTSIDE)
            continue
        if flag == IDX_OVERFLOW:
            kinds[s].add(S_FLAG)
        if flag in (IDX_CONFLICT, IDX_OVERFLOW):
            if conflict >= 2 * d:
                kinds[s].add(S_LINK_RANGE)
            elif conflict < d:
                kinds[s].add(S_LINK_HOME)
            elif not used[conflict]:
                kinds[s].add(S_LINK_FREE)
            else:
                succ[s] = conflict
                indeg[conflict] += 1
        if entry >= d:
            kinds[s].add(S_ENTRY_RANGE)
        else:
            refs[entry] += 1
            if not bit(entry):
                kinds[s].add(S_ENTRY_DEAD)

    # The overflow half is a functional graph: colour it once.  tail[s] is the
    # number of slots from s to the path's end, or None when the path from s
    # runs into a cycle.
    tail, state = {}, {}
    for s0 in range(d, 2 * d):
        if not used[s0] or s0 in state:
            continue
        path, s = [], s0
        while s is not None and s not in state:
            state[s] = "open"
            path.append(s)
            s = succ[s]
        if s is None:
            after = 0
        elif state[s] == "open":                        # met this very path: a cycle
            after = None
        else:
            after = tail[s]
        for t in reversed(path):
            after = None if after is None else after + 1
            tail[t] = after
            state[t] = "done"

    # Which home slots reach a slot: at most two distinct ones are kept, enough
    # to tell whether some home other than the entry's own reaches it.
    homes = [set() for _ in range(INDEX_ENTRIES)]
    longest = 0
    for h in range(d):
        if not used[h]:
            continue
        t = succ[h]
        if t is not None and tail[t] is None:
            kinds[h].add(S_LOOP)
        else:
            longest = max(longest, 1 + (tail[t] if t is not None else 0))
        homes[h].add(h)
        work = [(t, h)] if t is not None else []
        while work:
            s, hh = work.pop()
            if hh in homes[s] or len(homes[s]) >= 2:
                continue
            homes[s].add(hh)
            if succ[s] is not None:
                work.append((succ[s], hh))
    for s in range(2 * d):
        if not homes[s]:
            continue
        entry = slots[s][0]
        if entry < d and bit(entry) and homes[s] != {hash_of(entry) & (d - 1)}:
            kinds[s].add(S_MISFILED)
    for s in range(d, 2 * d):
        if not used[s]:
            continue
        if indeg[s] >= 2:
            kinds[s].add(S_SHARED)
        if indeg[s] == 0:
            kinds[s].add(S_LEAKED)
        elif not homes[s]:
            kinds[s].add(S_ISLAND)

    ikinds = [set() for _ in range(1024)]
    for nr in range(d, 1024):
        if bit(nr):
            ikinds[nr].add(E_STRAY)
    for nr in range(d):
        if refs[nr] >= 2:
            ikinds[nr].add(E_DUP)
        if bit(nr) and refs[nr] == 0:
            ikinds[nr].add(E_ORPHAN)
        if bit(nr) and hdr is not None and flags & CK_ITBID:
            mask = M64 if hdr["depth"] >= 64 else (1 << hdr["depth"]) - 1
            if (hash_of(nr) >> 10) & mask != hdr["itbid"]:
                ikinds[nr].add(E_MISPLACED)

    count = [0] * 16
    for ks in kinds + ikinds:
        for k in ks:
            count[k] += 1
    findings = sum(1 << k for k in range(16) if count[k])
    used_home, used_over = sum(used[:d]), sum(used[d: 2 * d])
    if hdr is not None:
        if hdr["entries"] != len(live):
            findings |= 1 << H_ENTRIES
        if hdr["itu"] != used_over:
            findings |= 1 << H_ITU
        if hdr["pseudo_conflicts"] != used_over:
            findings |= 1 << H_PSEUDO
        if live and hdr["max_offset"] < live[-1]:
            findings |= 1 << H_MAXOFF
        if live and hdr["ulen"] != ITB_SIZE + ITE_SIZE * (hdr["max_offset"] + 1):
            findings |= 1 << H_LEN
        if hdr["inf"] > d:
            findings |= 1 << H_INF
    report = REPORT.pack(findings, len(live), used_home, used_over, sum(1 for hs in homes if hs), longest, *count)
    return (0, report, masks_of([s for s in range(INDEX_ENTRIES) if kinds[s]], 32),
            masks_of([nr for nr in range(1024) if ikinds[nr]], 16))


def report_fields(raw) -> dict:
    f = REPORT.unpack(bytes(raw))
    return dict(findings=f[0], live=f[1], used_home=f[2], used_over=f[3], reached=f[4], longest=f[5],
                count=list(f[6:]))


def expect(recs_or_payloads, adepths, hdrs=None, flags: int = 0, status=None):
    """The oracle over a call: (err int32 [n], reports uint8 [n, 48], slot masks
    uint64 [n, 32], ITE masks uint64 [n, 16])."""
    n = len(recs_or_payloads)
    err = np.zeros(n, np.int32)
    rep = np.zeros((n, 48), np.uint8)
    sm, im = np.zeros((n, 32), np.uint64), np.zeros((n, 16), np.uint64)
    for b, p in enumerate(recs_or_payloads):
        if status is not None and status[b]:
            err[b] = status[b]
            continue
        e, r, s, i = check(p, adepths[b], None if hdrs is None else hdrs[b], flags)
        err[b], rep[b], sm[b], im[b] = e, np.frombuffer(r, np.uint8), s, i
    return err, rep, sm, im


# ---------------------------------------------------------------------------
# Tables built the way the MDS builds them
# ---------------------------------------------------------------------------
class Table:
    """One ITB in memory, [struct itbh][payload] with room for every ITE its
    adepth allows.  hashes: nr -> hash of the live ITEs (the builder's own
    bookkeeping, beside the header's)."""

    def __init__(self, adepth: int, seed: int = 0, depth: int = 0, itbid: int = 0):
        self.adepth, self.d = adepth, 1 << adepth
        self.rec = bytearray(ITB_SIZE + ITE_SIZE * self.d)
        self.rng = np.random.default_rng(seed ^ 0xC4EC)
        self.rec[ITBH_ADEPTH], self.rec[ITBH_DEPTH] = adepth, depth
        struct.pack_into("<Q", self.rec, ITBH_ITBID, itbid)
        struct.pack_into("<I", self.rec, ITBH_LEN, ITB_SIZE)      # itb.c get_free_itb: len = sizeof(struct itb)
        self.hashes = {}

    def _i32(self, off: int, delta: int = 0, value=None) -> int:
        (v,) = struct.unpack_from("<i", self.rec, off)
        v = v + delta if value is None else value
        struct.pack_into("<i", self.rec, off, v)
        return v

    def _bit(self, nr: int, value=None) -> int:
        at = H + BITMAP_OFF + nr // 8
        old = self.rec[at] >> (nr % 8) & 1
        if value is not None:
            self.rec[at] = self.rec[at] & ~(1 << (nr % 8)) | value << (nr % 8)
        return old

    def add(self, hsh: int):
        """itb_add_ite (mds/itb.c:339-407, with __itb_add_index's tail
        :309-316): the ITE's number, or None when the ITB is full (the MDS
        splits it)."""
        if self._i32(ITBH_ENTRIES, +1) > self.d:
            self._i32(ITBH_ENTRIES, -1)
            return None
        nr = next(k for k in range(self.d) if not self._bit(k))     # find_first_zero_bit
        self._bit(nr, 1)
        ite = H + ITE_OFF + ITE_SIZE * nr
        self.rec[ite: ite + ITE_SIZE] = self.rng.integers(0, 256, ITE_SIZE, dtype=np.uint8).tobytes()
        set_hash(self.rec, nr, hsh)
        offset = hsh & (self.d - 1)
        if get_slot(self.rec, H, offset)[2] in (IDX_UNIQUE, IDX_CONFLICT):
            self._i32(ITBH_PSEUDO, +1)                              # atomic_inc(&i->h.pseudo_conflicts)
        add_index(self.rec, offset, nr)
        if self._i32(ITBH_MAX_OFFSET) <= nr:
            self._i32(ITBH_MAX_OFFSET, value=nr)
            self._i32(ITBH_LEN, value=ITB_SIZE + (nr + 1) * ITE_SIZE)
        self.hashes[nr] = hsh
        return nr

    def _unlink(self, offset: int):
        """__ite_unlink (mds/itb.c:567-592)."""
        entry, conflict, _ = get_slot(self.rec, H, offset)
        set_slot(self.rec, H, offset, entry, conflict, IDX_FREE)
        if offset >= self.d:
            self._i32(ITBH_PSEUDO, -1)
            (itu,) = struct.unpack_from("<H", self.rec, ITBH_ITU)
            struct.pack_into("<H", self.rec, ITBH_ITU, (itu - 1) & 0xFFFF)
        if self._i32(ITBH_MAX_OFFSET) == entry:
            self._i32(ITBH_MAX_OFFSET, -1)
        if self._i32(ITBH_ENTRIES, -1) == 0:
            self._i32(ITBH_MAX_OFFSET, value=0)
            self._i32(ITBH_LEN, value=ITB_SIZE)
        else:
            self._i32(ITBH_LEN, value=ITB_SIZE + (self._i32(ITBH_MAX_OFFSET) + 1) * ITE_SIZE)
        assert self._bit(entry, 0) == 1, "Test-and-Clear a zero bit?"
        del self.hashes[entry]

    def delete(self, nr: int):
        """The unlink of live ITE nr: itb_search finds it at `offset` in the
        chain of its home slot `pos`, then itb_del_ite (mds/itb.c:602-671)."""
        rec, total = self.rec, 2 * self.d
        slot = lambda o: get_slot(rec, H, o)
        pos = offset = self.hashes[nr] & (self.d - 1)
        while slot(offset)[0] != nr:                                # itb_search's walk (:1780-1797)
            assert slot(offset)[2] in (IDX_CONFLICT, IDX_OVERFLOW)
            offset = slot(offset)[1]
        if slot(pos)[2] == IDX_FREE:
            return
        if slot(pos)[2] == IDX_UNIQUE:
            if offset == pos:
                self._unlink(offset)
            return
        saved = prev = pos
        pos, offset = offset, saved
        quit_ = needswap = hit = False
        while True:                                                 # do { retry:
            entry, conflict, flag = slot(offset)
            if flag == IDX_FREE:
                break
            if pos == offset or hit:                                # the unlink target
                if offset == saved:
                    needswap, prev = True, offset
                elif flag == IDX_UNIQUE:
                    pe, pc, _ = slot(prev)
                    set_slot(rec, H, prev, pe, pc, IDX_UNIQUE)
                    self._unlink(offset)
                    quit_ = True
                else:
                    pe, _, pf = slot(prev)
                    set_slot(rec, H, prev, pe, conflict, pf)
                    self._unlink(offset)
                    quit_ = True
            else:
                if needswap:                                        # the head's entry moves behind, then that slot goes
                    se, sc, sf = slot(saved)
                    set_slot(rec, H, offset, se, conflict, flag)
                    set_slot(rec, H, saved, entry, sc, sf)
                    needswap, hit = False, True
                    continue                                        # goto retry
                if flag == IDX_UNIQUE:
                    quit_ = True
                prev = offset
            offset = conflict                                       # offset = ii->conflict
            if not (offset < total and not quit_):                  # } while (offset < total && !quit)
                break
        if needswap:
            assert slot(saved)[2] == IDX_UNIQUE
            self._unlink(saved)

    # -- what the builder knows ------------------------------------------------
    def bookkeeping(self) -> dict:
        homes = {h & (self.d - 1) for h in self.hashes.values()}
        n = len(self.hashes)
        return dict(live=n, used_home=len(homes), used_over=n - len(homes), reached=n)

    def record(self) -> bytearray:
        """The record as stored uncompressed: h.len bytes."""
        (ln,) = struct.unpack_from("<I", self.rec, ITBH_LEN)
        return bytearray(self.rec[:ln])


def payload_of(rec) -> bytes:
    (ln,) = struct.unpack_from("<I", rec, ITBH_LEN)
    return bytes(rec[H:ln])


def random_table(seed: int, adepth: int, steps: int, depth: int = 0, itbid: int = 0) -> Table:
    """`steps` random adds and deletes; hashes collide on purpose (few distinct
    home slots now and then) and carry itbid above bit 10."""
    rng = np.random.default_rng(seed)
    t = Table(adepth, seed, depth, itbid)
    narrow = max(1, t.d // 4)
    for _ in range(steps):
        if t.hashes and rng.random() < 0.4:
            t.delete(int(rng.choice(sorted(t.hashes))))
        else:
            low = int(rng.integers(0, narrow if rng.random() < 0.5 else t.d))
            t.add(low | itbid << 10 | int(rng.integers(0, 1 << 20)) << (10 + depth))
    return t


# ---------------------------------------------------------------------------
# One hand-made table per kind.  kind_tables() is the table set at adepth 2
# (d = 4: slots 0 ... 7 in use) the first tests were written on;
# kind_tables(adepth, where) puts the same defects at the low or the high end
# of every range an adepth has.
# ---------------------------------------------------------------------------
BASE_DEPTH, BASE_ITBID = 2, 1
WHERES = ("low", "high")
# the cases that need a third ITE or a third overflow slot: not at adepth 1 (2 ITEs, 4 slots)
KIND_CASES_NEED_THREE = ("entry_dead_orphan", "shared_misfiled", "leaked", "island", "leaked_island", "orphan")


class Places:
    """Where a hand-made table sits.  e: the base chain's two ITEs, then two
    spare ones; hb: the base chain's home slot, hx: a spare home slot; o: the
    base chain's overflow slot, the next one (kept free: link_free's target),
    then two spare ones.
      low   ITEs 0, 1, 2, 3; home slots 1 and 0; overflow slots d, d + 1, ...
      high  ITEs d - 2, d - 1, d - 3, d - 4; home slots d - 1 and d - 2;
            overflow slots 2d - 1, 2d - 2, ...
    At adepth 1 only e[:2] and o[:2] exist."""

    def __init__(self, adepth: int, where: str):
        assert where in WHERES and 1 <= adepth <= 10
        d = self.d = 1 << adepth
        if where == "low":
            self.e, self.hb, self.hx, self.o = [0, 1, 2, 3], 1, 0, [d, d + 1, d + 2, d + 3]
        else:
            self.e, self.hb, self.hx = [d - 2, d - 1, d - 3, d - 4], d - 1, d - 2
            self.o = [2 * d - 1, 2 * d - 2, 2 * d - 3, 2 * d - 4]
        if adepth == 1:
            self.e, self.o = self.e[:2], self.o[:2]


def base_table(adepth: int = 2, where: str = "low") -> Table:
    """ITE e0 (hash hb) in home slot hb, ITE e1 (hash hb + d) behind it in
    overflow slot o0: slot hb = (e0, o0, CONFLICT), slot o0 = (e1, -, UNIQUE)
    (Places).  Both hashes carry itbid 1 at depth 2.  Nothing else is in use.
    At adepth 2, low: ITE 0 (hash 1) in home slot 1, ITE 1 (hash 5) in overflow
    slot 4.  A low table is built by Table.add; a high one by hand, with the
    header add would leave had the MDS filled the ITEs from the top, and its
    payload holds all d ITEs."""
    t = Table(adepth, 42, BASE_DEPTH, BASE_ITBID)
    at, d = Places(adepth, where), 1 << adepth
    h0, h1 = at.hb | BASE_ITBID << 10, (at.hb + d) | BASE_ITBID << 10
    if where == "low":
        assert (t.add(h0), t.add(h1)) == (0, 1)
    else:
        for nr, hsh in ((at.e[0], h0), (at.e[1], h1)):
            t._bit(nr, 1)
            ite = H + ITE_OFF + ITE_SIZE * nr
            t.rec[ite: ite + ITE_SIZE] = t.rng.integers(0, 256, ITE_SIZE, dtype=np.uint8).tobytes()
            set_hash(t.rec, nr, hsh)
            t.hashes[nr] = hsh
        set_slot(t.rec, H, at.hb, at.e[0], at.o[0], IDX_CONFLICT)
        set_slot(t.rec, H, at.o[0], at.e[1], 0, IDX_UNIQUE)
        t._i32(ITBH_ENTRIES, value=2)
        t._i32(ITBH_PSEUDO, value=1)
        t._i32(ITBH_MAX_OFFSET, value=d - 1)
        t._i32(ITBH_LEN, value=ITB_SIZE + ITE_SIZE * d)
        struct.pack_into("<HH", t.rec, ITBH_INF, d, 1)
    assert get_slot(t.rec, H, at.hb) == (at.e[0], at.o[0], IDX_CONFLICT)
    assert get_slot(t.rec, H, at.o[0])[::2] == (at.e[1], IDX_UNIQUE)
    return t


def _live(t: Table, nr: int, hsh: int):
    """ITE nr made live by hand (no slot, no header change)."""
    t._bit(nr, 1)
    set_hash(t.rec, nr, hsh | BASE_ITBID << 10)
    # (the payload must hold the ITE: the table's room does)
    struct.pack_into("<I", t.rec, ITBH_LEN, max(struct.unpack_from("<I", t.rec, ITBH_LEN)[0],
                                                  ITB_SIZE + ITE_SIZE * (nr + 1)))


def kind_tables(adepth: int = 2, where: str = "low"):
    """name -> (record, {kind: count}, slot bits, ITE bits): what a check with
    hdr NULL must report, exactly.  Three kinds cannot stand alone:
      S_SHARED  needs two good links into one overflow slot t.  If both come
                from slots one home slot reaches, the later of them lies behind
                t on that home's only path, so the path returns to t: S_LOOP.
                If two home slots reach t, its entry hashes to at most one of
                them: S_MISFILED (or the entry is dead or out of range).
      S_LOOP    a path that comes back enters its cycle at a slot with a link
                from the path and one from the cycle: S_SHARED.
      so they are shown as the pairs shared + loop and shared + misfiled.
    S_LEAKED and S_ISLAND each can: a leaked slot that does not link, and an
    unreached cycle, where every slot has indeg 1.  The usual damage, a chain
    cut off its home slot, gives both: the head leaked, the rest an island.
    S_ENTRY_DEAD alone is a cleared bitmap bit; a slot whose entry was
    redirected to a dead ITE leaves its old ITE an orphan as well.

    The ITEs and slots are Places(adepth, where)'s, and a defect's value sits
    at the edge of its range as well: outside slots 2d and 2047, stray bits d
    and 1023, entry d (low) or 32767 (high), conflict 2d or 32767 out of range
    and 0 or d - 1 into the home half.  At adepth 10 no slot lies outside and
    no bit is stray: those two tables are the valid one.  At adepth 1 the
    KIND_CASES_NEED_THREE are absent."""
    out = {}
    at, d = Places(adepth, where), 1 << adepth
    low = where == "low"
    e, o, hb, hx = at.e + [None] * 2, at.o + [None] * 2, at.hb, at.hx
    tag = BASE_ITBID << 10

    def case(name, kinds, slots=(), ites=()):
        def deco(fn):
            if adepth == 1 and name in KIND_CASES_NEED_THREE:
                return
            t = base_table(adepth, where)
            fn(t)
            out[name] = (t.record(), kinds, tuple(slots), tuple(ites))
        return deco

    ss = lambda t, s, entry, c, f: set_slot(t.rec, H, s, entry, c, f)
    case("valid", {})(lambda t: None)
    if adepth < 10:
        case("outside", {S_OUTSIDE: 2}, (2 * d, 2047))(
            lambda t: (ss(t, 2 * d, e[0], 0, IDX_UNIQUE), ss(t, 2047, e[1], o[0], IDX_CONFLICT)))
    else:
        case("outside", {})(lambda t: None)
    case("flag", {S_FLAG: 1}, (hb,))(lambda t: ss(t, hb, e[0], o[0], IDX_OVERFLOW))
    case("link_range", {S_LINK_RANGE: 1}, (o[0],))(lambda t: ss(t, o[0], e[1], 2 * d if low else 32767, IDX_CONFLICT))
    case("link_home", {S_LINK_HOME: 1}, (o[0],))(lambda t: ss(t, o[0], e[1], 0 if low else d - 1, IDX_CONFLICT))
    case("link_free", {S_LINK_FREE: 1}, (o[0],))(lambda t: ss(t, o[0], e[1], o[1], IDX_CONFLICT))
    case("entry_range", {S_ENTRY_RANGE: 1}, (o[0],))(
        lambda t: (ss(t, o[0], d if low else 32767, 0, IDX_UNIQUE), t._bit(e[1], 0)))
    case("entry_dead", {S_ENTRY_DEAD: 1}, (o[0],))(lambda t: t._bit(e[1], 0))
    case("entry_dead_orphan", {S_ENTRY_DEAD: 1, E_ORPHAN: 1}, (o[0],), (e[1],))(
        lambda t: ss(t, o[0], e[2], 0, IDX_UNIQUE))
    case("shared_loop", {S_SHARED: 1, S_LOOP: 1}, (hb, o[0]))(lambda t: ss(t, o[0], e[1], o[0], IDX_CONFLICT))
    case("shared_misfiled", {S_SHARED: 1, S_MISFILED: 1}, (o[0],))(
        lambda t: (_live(t, e[2], hx), ss(t, hx, e[2], o[0], IDX_CONFLICT)))
    case("leaked", {S_LEAKED: 1}, (o[2],))(lambda t: (_live(t, e[2], 2), ss(t, o[2], e[2], 0, IDX_UNIQUE)))
    case("island", {S_ISLAND: 1}, (o[2],))(lambda t: (_live(t, e[2], 2), ss(t, o[2], e[2], o[2], IDX_CONFLICT)))
    case("leaked_island", {S_LEAKED: 1, S_ISLAND: 1}, (o[2], o[3]))(
        lambda t: (_live(t, e[2], 2), _live(t, e[3], 2), ss(t, o[2], e[2], o[3], IDX_CONFLICT),
                   ss(t, o[3], e[3], 0, IDX_UNIQUE)))
    # the hash moves to another home slot's low bits (hb is 1 or d - 1)
    case("misfiled_home", {S_MISFILED: 1}, (hb,))(lambda t: set_hash(t.rec, e[0], (2 if low else hb - 1) | tag))
    case("misfiled_over", {S_MISFILED: 1}, (o[0],))(lambda t: set_hash(t.rec, e[1], d | tag))
    if adepth < 10:
        case("stray", {E_STRAY: 2}, (), (d, 1023))(lambda t: (t._bit(d, 1), t._bit(1023, 1)))
    else:
        case("stray", {})(lambda t: None)
    case("dup", {E_DUP: 1}, (), (e[0],))(lambda t: (ss(t, o[0], e[0], 0, IDX_UNIQUE), t._bit(e[1], 0)))
    case("orphan", {E_ORPHAN: 1}, (), (e[2],))(lambda t: _live(t, e[2], 3))
    return out


def funnel():
    """adepth 10: every home slot h links to overflow slot 1024 + h, and the
    overflow half is one cycle of 1,024 slots.  Every ITE is live; slot s holds
    entry s % 1024, whose hash is its own number."""
    t = Table(10, 7)
    for nr in range(1024):
        _live(t, nr, nr)
        set_slot(t.rec, H, nr, nr, 1024 + nr, IDX_CONFLICT)
        set_slot(t.rec, H, 1024 + nr, nr, 1024 + (nr + 1) % 1024, IDX_CONFLICT)
    return t.record()


def fuzzed(seed: int, adepth: "int | None" = None):
    """A valid random table with 1 ... 8 flips of index words, bitmap bits, ITE
    hashes and header fields: (record, adepth)."""
    rng = np.random.default_rng(seed ^ 0xF022)
    adepth = int(rng.integers(1, 11)) if adepth is None else adepth
    d = 1 << adepth
    t = random_table(seed, adepth, int(rng.integers(1, 3 * d + 2)), depth=int(rng.integers(0, 4)),
                     itbid=int(rng.integers(0, 2)))
    rec = t.record()
    n_ites = (len(rec) - ITB_SIZE) // ITE_SIZE
    for _ in range(int(rng.integers(1, 9))):
        what = int(rng.integers(0, 6))
        if what == 0:                                   # one bit of a slot in or near the halves in use
            s = int(rng.integers(0, min(2 * d + 4, INDEX_ENTRIES)))
            rec[H + INDEX_OFF + 4 * s + int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
        elif what == 1:                                 # a whole slot, anywhere
            s = int(rng.integers(0, INDEX_ENTRIES))
            set_slot(rec, H, s, int(rng.integers(0, min(2 * d, 32768))), int(rng.integers(0, min(4 * d, 32768))),
                     int(rng.integers(0, 4)))
        elif what == 2:                                 # a bitmap bit among the ITEs the payload holds, or a stray
            nr = int(rng.integers(0, max(n_ites, 1))) if rng.random() < 0.8 and n_ites else int(rng.integers(0, 1024))
            if nr < n_ites or nr >= d:
                rec[H + BITMAP_OFF + nr // 8] ^= 1 << (nr % 8)
        elif what == 3 and n_ites:                      # a low or an itbid bit of a hash
            nr = int(rng.integers(0, n_ites))
            (hsh,) = struct.unpack_from("<Q", rec, H + ITE_OFF + ITE_SIZE * nr)
            set_hash(rec, nr, hsh ^ 1 << int(rng.integers(0, 14)))
        elif what == 4:                                 # a header counter, off by a little
            off = (ITBH_ENTRIES, ITBH_MAX_OFFSET, ITBH_PSEUDO)[int(rng.integers(0, 3))]
            (v,) = struct.unpack_from("<i", rec, off)
            struct.pack_into("<i", rec, off, v + int(rng.integers(-2, 3)))
        else:
            off = (ITBH_INF, ITBH_ITU)[int(rng.integers(0, 2))]
            (v,) = struct.unpack_from("<H", rec, off)
            struct.pack_into("<H", rec, off, (v + int(rng.integers(-1, 2)) * int(rng.choice([1, d]))) & 0xFFFF)
    return rec, adepth


# ---------------------------------------------------------------------------
# Directed tables: each aims at one piece of the kernel's machinery -- a word
# or half boundary, the once / twice bitmaps, the walk's bound -- and states in
# closed form what the check must report, so the oracle above is judged too.
# ---------------------------------------------------------------------------
class Directed(NamedTuple):
    """A table and what a check with hdr NULL must report for it: count[k] for
    every kind 0 ... 14 (a kind not named counts 0), exactly the slot-mask and
    ITE-mask bits, and `reached` and `longest` where the builder states them
    (None: not stated)."""
    name: str
    rec: bytearray
    adepth: int
    kinds: dict
    slots: tuple
    ites: tuple
    reached: Optional[int] = None
    longest: Optional[int] = None


def assert_directed(t: Directed, err, report, slot_mask=None, ite_mask=None):
    """The closed-form values of t against one result (the masks where the
    call returned them)."""
    f = report_fields(report)
    assert int(err) == 0, (t.name, int(err))
    assert f["count"][:15] == [t.kinds.get(k, 0) for k in range(15)], (t.name, f)
    assert f["findings"] & 0x7FFF == sum(1 << k for k, c in t.kinds.items() if c), (t.name, f)
    if slot_mask is not None:
        assert [int(w) for w in slot_mask] == masks_of(t.slots, 32), (t.name, "slot mask")
    if ite_mask is not None:
        assert [int(w) for w in ite_mask] == masks_of(t.ites, 16), (t.name, "ITE mask")
    if t.reached is not None:
        assert f["reached"] == t.reached, (t.name, f)
    if t.longest is not None:
        assert f["longest"] == t.longest, (t.name, f)


def _blank(adepth: int, seed: int) -> Table:
    """No ITE live, no slot in use; _live's hashes carry its itbid."""
    return Table(adepth, seed, BASE_DEPTH, BASE_ITBID)


def _comb(lo: int, hi: int):
    """P: the first and the last bit of every 64-bit word, within [lo, hi)."""
    return [x for x in range(lo, hi) if x % 64 in (0, 63)]


def slot_comb(adepth: int) -> Directed:
    """Findings at the first and last slot of every word of both halves
    (adepth 6 ... 10: d is a multiple of 64).  A home slot of P is CONFLICT
    with its own live ITE (hash: its number) and links to a free overflow slot
    outside P: S_LINK_FREE.  An overflow slot of P is UNIQUE with an entry at
    or above d and no link into it: S_ENTRY_RANGE and S_LEAKED."""
    assert 6 <= adepth <= 10
    t, d = _blank(adepth, 600 + adepth), 1 << adepth
    home, over = _comb(0, d), _comb(d, 2 * d)
    for h in home:
        _live(t, h, h)
        set_slot(t.rec, H, h, h, d + (h + 2) % d, IDX_CONFLICT)         # (h + 2) % 64 is 2 or 1
    for i, s in enumerate(over):
        set_slot(t.rec, H, s, d if i % 2 == 0 else 32767, 0, IDX_UNIQUE)
    kinds = {S_LINK_FREE: len(home), S_ENTRY_RANGE: len(over), S_LEAKED: len(over)}
    return Directed(f"slot_comb@{adepth}", t.record(), adepth, kinds, tuple(home + over), (), len(home), 1)


def ite_comb(adepth: int) -> Directed:
    """No slot in use; the bitmap is P: the bits below d are E_ORPHAN, those
    from d up E_STRAY (none at adepth 10)."""
    assert 6 <= adepth <= 10
    t, d = _blank(adepth, 610 + adepth), 1 << adepth
    for nr in _comb(0, d):
        _live(t, nr, nr)
    for nr in _comb(d, 1024):
        t._bit(nr, 1)
    kinds = {E_ORPHAN: len(_comb(0, d)), E_STRAY: len(_comb(d, 1024))}
    return Directed(f"ite_comb@{adepth}", t.record(), adepth, kinds, (), tuple(_comb(0, 1024)), 0, 0)


def alternating(adepth: int) -> Directed:
    """indeg 2 beside indeg 1, all along the overflow half: for j = 0, 1, ...
    while 3j + 2 < d, home slots 3j and 3j + 1 link to overflow slot d + 2j and
    home slot 3j + 2 to d + 2j + 1.  Home slot h holds live ITE h (hash h);
    d + 2j holds ITE 3j again and d + 2j + 1 ITE 3j + 2, both UNIQUE.  So the
    even overflow slots are S_SHARED, and S_MISFILED too (two home slots reach
    them); the odd ones are neither; ITEs 3j and 3j + 2 are E_DUP."""
    assert 2 <= adepth <= 10
    t, d = _blank(adepth, 620 + adepth), 1 << adepth
    js = [j for j in range(d) if 3 * j + 2 < d]
    for j in js:
        for h, target in ((3 * j, d + 2 * j), (3 * j + 1, d + 2 * j), (3 * j + 2, d + 2 * j + 1)):
            _live(t, h, h)
            set_slot(t.rec, H, h, h, target, IDX_CONFLICT)
        set_slot(t.rec, H, d + 2 * j, 3 * j, 0, IDX_UNIQUE)
        set_slot(t.rec, H, d + 2 * j + 1, 3 * j + 2, 0, IDX_UNIQUE)
    even = tuple(d + 2 * j for j in js)
    kinds = {S_SHARED: len(js), S_MISFILED: len(js), E_DUP: 2 * len(js)}
    dup = tuple(nr for j in js for nr in (3 * j, 3 * j + 2))
    return Directed(f"alternating@{adepth}", t.record(), adepth, kinds, even, dup, 5 * len(js), 2)


def star(adepth: int) -> Directed:
    """indeg d on one slot: every home slot h (live ITE h, hash h) links to
    overflow slot d, UNIQUE with entry 0."""
    t, d = _blank(adepth, 630 + adepth), 1 << adepth
    for h in range(d):
        _live(t, h, h)
        set_slot(t.rec, H, h, h, d, IDX_CONFLICT)
    set_slot(t.rec, H, d, 0, 0, IDX_UNIQUE)
    return Directed(f"star@{adepth}", t.record(), adepth, {S_SHARED: 1, S_MISFILED: 1, E_DUP: 1}, (d,), (0,), d + 1, 2)


def one_ite(adepth: int) -> Directed:
    """refs 2d on one ITE: every slot of both halves is UNIQUE with entry
    d - 1, the only live ITE (hash d - 1).  The overflow slots are S_LEAKED,
    the home slots other than d - 1 S_MISFILED."""
    t, d = _blank(adepth, 640 + adepth), 1 << adepth
    _live(t, d - 1, d - 1)
    for s in range(2 * d):
        set_slot(t.rec, H, s, d - 1, 0, IDX_UNIQUE)
    kinds = {E_DUP: 1, S_LEAKED: d, S_MISFILED: d - 1}
    return Directed(f"one_ite@{adepth}", t.record(), adepth, kinds,
                    tuple(s for s in range(2 * d) if s != d - 1), (d - 1,), d, 1)


CHAIN_VARIANTS = ("line", "short", "cycle", "self", "fan")


def chain(adepth: int, variant: str, permuted: bool) -> Directed:
    """The walk's bound.  A chain from home slot 0 (ITE 0) through the overflow
    slots in the order o -- ascending, or a seeded permutation that does not
    end in slot d -- where slot o[i] holds ITE o[i] - d.  Every ITE is live
    and every hash has low bits 0, so nothing on home slot 0's chain is
    misfiled; ITE 0 is in home slot 0 and in slot d: E_DUP.
      line   all d overflow slots, the last UNIQUE: a path of d + 1 slots, the
             longest a table has
      short  one slot fewer; the ITE of o[d - 1] is E_ORPHAN
      cycle  the last slot links back to o[0]: S_LOOP on home slot 0, S_SHARED on o[0]
      self   the last slot links to itself: S_LOOP, S_SHARED on o[d - 1]
      fan    the line, and every home slot h (entry h) links to o[0]: d paths
             of d + 1 slots; o[0] is S_SHARED, every slot but home slot 0
             S_MISFILED, every ITE E_DUP"""
    assert variant in CHAIN_VARIANTS
    t, d = _blank(adepth, 650 + adepth), 1 << adepth
    o = list(range(d, 2 * d))
    if permuted:
        o = [int(s) for s in np.random.default_rng(0xD1CE + adepth).permutation(o)]
        if o[-1] == d:
            o[0], o[-1] = o[-1], o[0]
    for nr in range(d):
        _live(t, nr, 0)
    set_slot(t.rec, H, 0, 0, o[0], IDX_CONFLICT)
    m = d - 1 if variant == "short" else d
    for i in range(m - 1):
        set_slot(t.rec, H, o[i], o[i] - d, o[i + 1], IDX_CONFLICT)
    back = {"cycle": o[0], "self": o[m - 1]}.get(variant)
    set_slot(t.rec, H, o[m - 1], o[m - 1] - d, back or 0, IDX_UNIQUE if back is None else IDX_CONFLICT)
    name = f"{variant}@{adepth}{'p' if permuted else 'a'}"
    if variant == "line":
        want = ({E_DUP: 1}, (), (0,), d + 1, d + 1)
    elif variant == "short":
        want = ({E_DUP: 1, E_ORPHAN: 1}, (), (0, o[d - 1] - d), d, d)
    elif variant in ("cycle", "self"):
        want = ({S_LOOP: 1, S_SHARED: 1, E_DUP: 1}, (0, back), (0,), d + 1, 0)
    else:
        for h in range(1, d):
            set_slot(t.rec, H, h, h, o[0], IDX_CONFLICT)
        want = ({S_SHARED: 1, S_MISFILED: 2 * d - 1, E_DUP: d}, tuple(range(1, 2 * d)), tuple(range(d)), 2 * d, d + 1)
    return Directed(name, t.record(), adepth, *want)


GROUPS = ("kinds", "combs", "counts", "walk")


def directed(group: str, adepths=range(1, 11)):
    """The directed tables of one group at the given adepths (where the group
    has them):
      kinds   kind_tables(adepth, where), low and high
      combs   slot_comb and ite_comb, adepth 6 ... 10
      counts  alternating (adepth 2 ... 10), star and one_ite
      walk    chain: every variant, ascending and permuted"""
    out = []
    for adepth in adepths:
        if group == "kinds":
            for where in WHERES:
                out += [Directed(f"{name}@{adepth}{where}", rec, adepth, kinds, slots, ites)
                        for name, (rec, kinds, slots, ites) in kind_tables(adepth, where).items()]
        elif group == "combs":
            out += [slot_comb(adepth), ite_comb(adepth)] if adepth >= 6 else []
        elif group == "counts":
            out += ([alternating(adepth)] if adepth >= 2 else []) + [star(adepth), one_ite(adepth)]
        else:
            assert group == "walk"
            out += [chain(adepth, v, p) for v in CHAIN_VARIANTS for p in (False, True)]
    return out
