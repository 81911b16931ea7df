"""The ITB sweep's test oracle and table builders (shared by test_itb_sweep.py
and test_gpu_itb_sweep.py).

sweep_table() restates async_unlink_ite (mds/itb.c:2690-2800) in Python on
check_util.Table, whose _unlink() already restates __ite_unlink (:567-592);
header() is the struct itbh a sweep leaves, expect() the rules of
include/pom_sweep.h around them.  Nothing here reads the product's
itb_sweep.h.

Like the split's, the loop cannot be pinned by a golden fixture: calling
async_unlink_ite itself needs the MDS's locks and profile counters.  So this
restatement is reviewed against the cited lines, and the tests hold it to what
a CPU study of it found (invariants()): a swept table is clean under check()
with its header facts, dc == removed + swaps, the ITE area and the lock region
do not change, the loop takes at most live + swaps chain steps, and max_offset
stays at or above the highest live ITE (it may stay above it)."""
from __future__ import annotations

import struct

import numpy as np

import check_util as C
import itb_split_util as S
from check_util import (BITMAP_OFF, EINVAL, H, IDX_CONFLICT, IDX_FREE, IDX_UNIQUE, ITB_SIZE, ITBH_ENTRIES,  # noqa: F401
                        ITBH_INF, ITBH_ITU, ITBH_LEN, ITBH_MAX_OFFSET, ITBH_PSEUDO, ITE_OFF, ITE_SIZE, Table, get_slot,
                        set_slot)
from itb_split_util import E_DAMAGED, E_OUTPUT_OVERRUN, ITBH_ALGO, ITBH_STATE, table_of  # noqa: F401

ITE_FLAG_OFF, STATE_MASK, UNLINKED, SHADOW = 16, 7, 1, 3
OTHER_STATES = (0, 2, 3, 5, 7)                          # never swept
NO_BUDGET = 0xFFFFFFFF
RESULT = struct.Struct("<iIIIiiiHH")
RESULT_FIELDS = ("err", "removed", "dc", "len", "entries", "max_offset", "pseudo_conflicts", "itu", "visited")
assert RESULT.size == 32


def result_fields(raw) -> dict:
    return dict(zip(RESULT_FIELDS, RESULT.unpack(bytes(raw))))


def flag_of(rec, nr: int, base: int = H) -> int:
    return struct.unpack_from("<I", rec, base + ITE_OFF + ITE_SIZE * nr + ITE_FLAG_OFF)[0]


def set_state(rec, nr: int, state: int, base: int = H):
    """The state bits of ITE nr; its other 29 flag bits stay."""
    struct.pack_into("<I", rec, base + ITE_OFF + ITE_SIZE * nr + ITE_FLAG_OFF, flag_of(rec, nr, base) & ~STATE_MASK | state)


def marked(rec, nr: int, base: int = H) -> bool:
    """(e->flag & ITE_STATE_MASK) == ITE_UNLINKED"""
    return flag_of(rec, nr, base) & STATE_MASK == UNLINKED


# ---------------------------------------------------------------------------
# The loop
# ---------------------------------------------------------------------------
def sweep_table(t: Table, budget=None) -> dict:
    """mds/itb.c:2690-2800 on t, with *dc starting at 0 and
    hmo.conf.max_async_unlink = budget (None: never reached).  -> removed, dc,
    swaps, steps (slots examined, the retry after a swap included), visited and
    the deleted ITEs in __ite_unlink order."""
    rec, d = t.rec, t.d
    slot = lambda o: get_slot(rec, H, o)
    budget = NO_BUDGET if budget is None else budget
    f = dict(removed=0, dc=0, swaps=0, steps=0, visited=d, deleted=[])

    def unlink(o):
        f["deleted"].append(slot(o)[0])
        t._unlink(o)
        f["removed"] += 1

    offset = 0
    while offset < d:
        entry, conflict, flag = slot(offset)
        if flag == IDX_FREE:                                        # a hole
            offset += 1
            continue
        if flag == IDX_UNIQUE:
            f["steps"] += 1
            if marked(rec, entry):
                unlink(offset)
                f["dc"] += 1
        else:
            saved = prev = offset
            quit_ = needswap = False
            while True:                                             # do { retry:
                f["steps"] += 1
                assert f["steps"] <= 4 * d, "the loop does not end"
                entry, conflict, flag = slot(offset)
                if flag == IDX_FREE:
                    break
                if marked(rec, entry):
                    if offset == saved:                             # the head: swap it behind, or free it last
                        needswap, prev = True, offset
                    elif flag == IDX_UNIQUE:                        # the tail
                        pe, pc, _ = slot(prev)
                        set_slot(rec, H, prev, pe, pc, IDX_UNIQUE)
                        unlink(offset)
                        quit_ = True
                    else:                                           # a middle entry
                        pe, _, pf = slot(prev)
                        set_slot(rec, H, prev, pe, conflict, pf)
                        unlink(offset)
                    f["dc"] += 1
                else:
                    if needswap:
                        se, sc, sf = slot(saved)
                        set_slot(rec, H, offset, se, conflict, flag)
                        set_slot(rec, H, saved, entry, sc, sf)
                        needswap = False
                        f["swaps"] += 1
                        continue                                    # goto retry
                    if flag == IDX_UNIQUE:
                        quit_ = True
                    prev = offset
                offset = conflict
                if not (offset < 2 * d and not quit_):              # } while (offset < (total << 1) && !quit)
                    break
            if needswap:
                assert slot(saved)[2] == IDX_UNIQUE
                unlink(saved)
            offset = saved
        offset += 1
        if f["dc"] >= budget:
            f["visited"] = offset
            break
    return f


# ---------------------------------------------------------------------------
# The rules of include/pom_sweep.h
# ---------------------------------------------------------------------------
class Sweep:
    """What one ITB's sweep must leave: result (32 bytes), the payload after
    it, and the loop's facts (None when nothing was walked)."""

    def __init__(self, result, payload, facts=None):
        self.result, self.payload, self.facts = result, payload, facts

    @property
    def fields(self):
        return result_fields(self.result)

    @property
    def produced(self):
        f = self.fields
        return f["err"] == 0 and f["removed"] > 0


def _only(err: int) -> bytes:
    return RESULT.pack(err, *([0] * 8))


def expect_one(payload, adepth: int, hdr: dict, budget=None, payload_off: int = 0, status: int = 0) -> Sweep:
    payload = bytes(payload)
    if status:
        return Sweep(_only(status), payload)
    err, report, _, _ = C.check(payload, adepth, hdr, 0)
    if err:
        return Sweep(_only(err), payload)
    if payload_off % 16:
        return Sweep(_only(EINVAL), payload)
    if C.report_fields(report)["findings"] & ~(1 << C.E_MISPLACED):
        return Sweep(_only(E_DAMAGED), payload)
    t = table_of(payload, adepth, hdr)
    f = sweep_table(t, budget)
    if f["removed"] == 0:
        return Sweep(_only(0), payload, f)
    i32 = lambda off: struct.unpack_from("<i", t.rec, off)[0]
    (itu,) = struct.unpack_from("<H", t.rec, ITBH_ITU)
    result = RESULT.pack(0, f["removed"], f["dc"], i32(ITBH_LEN), i32(ITBH_ENTRIES), i32(ITBH_MAX_OFFSET),
                         i32(ITBH_PSEUDO), itu, f["visited"])
    return Sweep(result, bytes(t.rec[H: H + len(payload)]), f)


def expect(payloads, adepths, hdrs, budgets=None, payload_offs=None, status=None):
    pick = lambda a, b, default: default if a is None else a[b]
    return [expect_one(payloads[b], adepths[b], hdrs[b], pick(budgets, b, None), pick(payload_offs, b, 0),
                       pick(status, b, 0)) for b in range(len(payloads))]


def assert_same(got, want, payloads, names=None):
    """got: [(result, the payload after, steps or None)] against expect()'s
    answers."""
    assert len(got) == len(want)
    for b, ((res, after, steps), w) in enumerate(zip(got, want)):
        what = names[b] if names else f"ITB {b}"
        assert result_fields(res) == w.fields, what
        assert after == w.payload, f"{what}: the payload"
        if not w.produced:
            assert after == bytes(payloads[b]), f"{what}: nothing produced, yet the payload changed"
        elif steps is not None:
            assert steps == w.facts["steps"], f"{what}: steps"


def swept_hdr(hdr: dict, f: dict) -> dict:
    return dict(hdr, entries=f["entries"], max_offset=f["max_offset"], pseudo_conflicts=f["pseudo_conflicts"],
                itu=f["itu"], ulen=f["len"])


def invariants(payload, adepth: int, hdr: dict, s: Sweep):
    """What the contract relies on, for a sweep that removed something."""
    f, facts = s.fields, s.facts
    before = table_of(payload, adepth, hdr)
    live = len(before.hashes)
    assert f["err"] == 0 and f["removed"] == len(facts["deleted"]) > 0
    assert f["dc"] == f["removed"] + facts["swaps"]                             # the head is counted twice
    assert s.payload[:BITMAP_OFF] == bytes(payload[:BITMAP_OFF]) and s.payload[ITE_OFF:] == bytes(payload[ITE_OFF:])
    assert len(s.payload) == len(payload)
    assert facts["steps"] <= live + facts["swaps"]
    assert all(marked(payload, nr, 0) for nr in facts["deleted"]) and len(set(facts["deleted"])) == f["removed"]
    left = sorted(set(before.hashes) - set(facts["deleted"]))
    assert f["entries"] == len(left) and f["len"] <= H + len(payload)
    assert f["max_offset"] >= (left[-1] if left else 0) and (left or (f["max_offset"], f["len"]) == (0, ITB_SIZE))
    assert 1 <= f["visited"] <= 1 << adepth
    e, report, _, _ = C.check(s.payload[: f["len"] - H], adepth, swept_hdr(hdr, f), 0)
    assert e == 0 and C.report_fields(report)["findings"] == 0, C.report_fields(report)


def header(old_hdr, result, z=None):
    """pom_itb_sweep_header: (the struct itbh after the sweep, whether the
    record is stored compressed); z: the stream's size, None: none."""
    f = result_fields(result)
    h = bytearray(old_hdr[:H])
    struct.pack_into("<ii", h, ITBH_ENTRIES, f["entries"], f["max_offset"])
    struct.pack_into("<i", h, ITBH_PSEUDO, f["pseudo_conflicts"])
    struct.pack_into("<H", h, ITBH_ITU, f["itu"])
    lzo = S._stored_as(h, f["len"], z)
    return bytes(h), int(lzo)


def stored_record(oracle, old_hdr, s: Sweep) -> bytes:
    """A swept ITB as itb_lzo_compress stores it."""
    p = s.payload[: s.fields["len"] - H]
    z = oracle.compress(p)
    h, lzo = header(old_hdr, s.result, len(z))
    return h + (z if lzo else p)


# ---------------------------------------------------------------------------
# Tables.  Table.add fills an ITE with random bytes, so the 29 flag bits beside
# the state are random; the builders set the state alone.
# ---------------------------------------------------------------------------
def mark(t: Table, fraction: float, seed: int) -> Table:
    """Every live ITE gets state ITE_UNLINKED with probability `fraction`, else
    one of the states that never sweep."""
    rng = np.random.default_rng(seed ^ 0x5EE9)
    for nr in sorted(t.hashes):
        set_state(t.rec, nr, UNLINKED if rng.random() < fraction else int(rng.choice(OTHER_STATES)))
    return t


def random_sweep_table(seed: int, adepth: int, fraction: float = 0.5) -> Table:
    d = 1 << adepth
    return mark(C.random_table(seed, adepth, 2 * d + 3), fraction, seed)


def with_states(t: Table, states: dict, rest: int = 0) -> Table:
    """ITE nr -> state; every other live ITE gets `rest`."""
    for nr in t.hashes:
        set_state(t.rec, nr, states.get(nr, rest))
    return t


PATTERNS = ("U", "L", "UL", "LU", "UU", "ULL", "LUL", "LLU", "UUL", "ULU", "LUU", "UUU", "ULUL")


def chain_table(adepth: int, where: str, pattern: str, live_state: int = 0):
    """One chain whose members are, head first, unlinked (U) or live (L).
    low: home slot 0 and the lowest ITEs, nothing else in the table; high: home
    slot d - 1 and the highest ITEs, behind d - len(pattern) live ITEs alone in
    their home slots.  None when the adepth has no room for it."""
    d, n = 1 << adepth, len(pattern)
    if n > d:
        return None
    up = lambda i: i << 20
    if where == "low":
        t = S._built(adepth, 50 + n, [0 | up(i) for i in range(n)])
        home = 0
    else:
        t = S._built(adepth, 60 + n, [i % (d - 1) | up(i) for i in range(d - n)] + [(d - 1) | up(d + i) for i in range(n)])
        home = d - 1
    members = S._chain(t, home)
    assert len(members) == n
    return with_states(t, {nr: UNLINKED if c == "U" else live_state for nr, c in zip(members, pattern)})


def directed_chains():
    """[(name, record, adepth)]: PATTERNS at adepth 1, 2 and 10, low and high,
    and every U / L chain of all four ITEs at adepth 2."""
    out = []
    for adepth in (1, 2, 10):
        for where in C.WHERES:
            for pattern in PATTERNS:
                t = chain_table(adepth, where, pattern)
                if t is not None:
                    out.append((f"{pattern}@{adepth}{where}", t.record(), adepth))
    for k in range(16):
        pattern = "".join("U" if k >> i & 1 else "L" for i in range(4))
        out.append((f"{pattern}@2all", chain_table(2, "low", pattern).record(), 2))
    return out


def spread_table(adepth: int, homes, unlinked, seed: int = 70) -> Table:
    """ITE nr alone in home slot homes[nr]; the ITEs of `unlinked` are marked."""
    assert len(set(homes)) == len(homes)
    t = S._built(adepth, seed, [h | nr << 20 for nr, h in enumerate(homes)])
    return with_states(t, {nr: UNLINKED for nr in unlinked})


def max_offset_tables():
    """[(name, record, adepth, (max_offset, len) after the sweep)] at adepth 3,
    six ITEs: the loop deletes in home-slot order, max_offset follows
    __ite_unlink's `if (mo == n) mo--`."""
    ln = lambda mo: ITB_SIZE + ITE_SIZE * (mo + 1)
    out = []
    # the highest ITE (5) sits in home slot 0 and goes first: 5 -> 4; ITE 1 then changes nothing
    out.append(("highest_first", spread_table(3, [5, 4, 3, 2, 1, 0], [5, 1]), (4, ln(4))))
    # it goes last, after ITE 4 went while max_offset was still 5: 5 -> 4, stale (ITE 3 is the highest live)
    out.append(("highest_last", spread_table(3, [0, 1, 2, 3, 4, 5], [4, 5]), (4, ln(4))))
    # it stays: nothing moves although 3 and 4 go
    out.append(("highest_stays", spread_table(3, [0, 1, 2, 3, 4, 5], [3, 4]), (5, ln(5))))
    # 5, 4, 3 go in that order: three decrements
    out.append(("descending_run", spread_table(3, [5, 4, 3, 2, 1, 0], [5, 4, 3]), (2, ln(2))))
    # one chain, 5 4 3 2 0 1 head first: the marked 4 goes before the marked head 5, which goes at 3's slot: 5 -> 4 only
    t = S._built(3, 71, [1 | i << 20 for i in range(6)])
    assert S._chain(t, 1)[0] == 5
    out.append(("chain_order", with_states(t, {5: UNLINKED, 4: UNLINKED}), (4, ln(4))))
    out.append(("emptied", spread_table(3, [0, 1, 2, 3, 4, 5], range(6)), (0, ITB_SIZE)))
    return [(name, t.record(), 3, want) for name, t, want in out]


def budget_table() -> Table:
    """adepth 4.  Home slot 0 FREE; 1: the chain UL (dc 2, removed 1); 2 FREE;
    3: U; 4: L; 5: the chain LU; 6 ... 8 FREE; 9: U; the rest FREE.  Total dc 5,
    removed 4, one swap."""
    hashes = [1, 1 | 1 << 20, 3, 4, 5, 5 | 1 << 20, 9]
    t = S._built(4, 72, hashes)
    c1, c5 = S._chain(t, 1), S._chain(t, 5)
    assert len(c1) == 2 and len(c5) == 2
    return with_states(t, {c1[0]: UNLINKED, 2: UNLINKED, c5[1]: UNLINKED, 6: UNLINKED}, rest=SHADOW)


def damaged_tables():
    return S.damaged_tables()
