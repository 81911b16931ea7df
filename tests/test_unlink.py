"""CPU: the ITB unlink (include/pom_unlink.h) without a GPU -- the rules
(pomegranate_amd/csrc/itb_unlink.h, compiled as plain C++: the reference's form
and the kernel's rounds) against the Python restatement of itb_search's unlink
branch, ite_unlink and itb_del_ite in unlink_util.py: the ite_unlink table
exhaustively, itb_del_ite at its edges, the order within an ITB, the refused
flags and requests, damaged tables, seeded random tables; then the header
builder byte for byte, the stand-alone sanitizer check and the exports."""
from __future__ import annotations

import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import check_util as C
import itb_split_util as S
import itb_sweep_util as W
import lookup_util as L
import unlink_util as U
from conftest import ROOT
from pomegranate_amd import lookup, lzo, unlink

NATIVE = os.path.join(ROOT, "tests", "native")


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_unlink.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


def test_unlink_py_mirrors_the_header():
    want = header_macros()
    del want["POM_UNLINK_H"]
    got = {"POM_UL_UNLINK": unlink.UL_UNLINK, "POM_ITE_FLAG_NORMAL": unlink.ITE_FLAG_NORMAL,
           "POM_ITE_FLAG_LS": unlink.ITE_FLAG_LS, "POM_ITE_FLAG_SDT": unlink.ITE_FLAG_SDT,
           "POM_ITE_FLAG_SYM": unlink.ITE_FLAG_SYM, "POM_ITE_NLINK_OFF": unlink.ITE_NLINK_OFF,
           "POM_UL_MODE_DIR": unlink.UL_MODE_DIR, "POM_UL_NONE": unlink.UL_NONE, "POM_UL_SHADOWED": unlink.UL_SHADOWED,
           "POM_UL_MARKED": unlink.UL_MARKED, "POM_UL_DELETED": unlink.UL_DELETED,
           "POM_UL_WHAT_MASK": unlink.UL_WHAT_MASK, "POM_UL_DELTA": unlink.UL_DELTA}
    assert want == got
    assert (U.UNLINK, U.NORMAL, U.LS, U.SDT, U.SYM, U.KV, U.NLINK_OFF, U.S_IFDIR, U.DELTA) == \
        (unlink.UL_UNLINK, unlink.ITE_FLAG_NORMAL, unlink.ITE_FLAG_LS, unlink.ITE_FLAG_SDT, unlink.ITE_FLAG_SYM,
         unlink.ITE_FLAG_KV, unlink.ITE_NLINK_OFF, unlink.UL_MODE_DIR, unlink.UL_DELTA)
    assert (U.NONE, U.SHADOWED, U.MARKED, U.DELETED) == (0, 1, 2, 3)
    assert [unlink.RESULT_DTYPE.fields[k][1] for k in U.RESULT_FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 30]
    r = unlink.Result.parse(U.RESULT.pack(*range(9)))
    assert tuple(r) == tuple(range(9)) and r._fields == U.RESULT_FIELDS
    with pytest.raises(ValueError):
        unlink.Result.parse(bytes(31))


# ---------------------------------------------------------------------------
# libitb_unlink_host.so (itb_unlink.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_lib():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_unlink_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.itb_unlink_ite_host.restype = None
    lib.itb_unlink_ite_host.argtypes = [u32, u32, u32, ctypes.c_int, vp]
    lib.itb_unlink_batch_host.restype = None
    lib.itb_unlink_batch_host.argtypes = [vp] * 6 + [u32, ctypes.c_int, vp, vp, vp, u32, ctypes.c_int] + [vp] * 6
    return lib


@pytest.fixture(scope="module")
def host_unlink(host_lib):
    def run(payloads, adepths, hdrs, req, req_first, names=b"", async_=False, status=None, off_residue=None,
            parts=False):
        """-> ([(result 32 bytes, payload after)], err, nr, depth, what, out).
        Payload b lies in an arena of 0x5A, 64 guard bytes around it, at a
        multiple of 16 plus off_residue[b]; the guards, and a result and a
        request's answers on either side of the arrays, must keep their
        fill."""
        n, nreq = len(payloads), len(req)
        res = [0] * n if off_residue is None else list(off_residue)
        offs, at = [], 64
        for b in range(n):
            offs.append(at + res[b])
            at = (at + res[b] + len(payloads[b]) + 64 + 15) // 16 * 16
        raw = np.full(at + 32, 0x5A, np.uint8)
        arena = raw[(-raw.ctypes.data) % 16:]
        for b, p in enumerate(payloads):
            arena[offs[b]: offs[b] + len(p)] = np.frombuffer(bytes(p), np.uint8)
        before = arena.copy()
        hd = np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy()
        result = np.full((n + 2, 32), 0x5A, np.uint8)
        words = np.full((4, nreq + 2), 0x5A5A5A5A, np.uint32)
        out = np.full((nreq + 2, U.REC_SIZE), 0x5A, np.uint8)
        o64 = np.array(offs, np.uint64)
        lens = np.array([len(p) for p in payloads], np.uint32)
        ads = np.array(adepths, np.uint8)
        st = None if status is None else np.array(status, np.int32)
        rq = np.ascontiguousarray(req, dtype=lookup.REQ_DTYPE)
        rf = np.ascontiguousarray(req_first, dtype=np.uint32)
        blob = np.frombuffer(bytes(names) or b"\0", np.uint8)
        w = [words[k, 1:].ctypes.data for k in range(4)]
        host_lib.itb_unlink_batch_host(arena.ctypes.data, o64.ctypes.data, lens.ctypes.data,
                                       None if st is None else st.ctypes.data, ads.ctypes.data, hd.ctypes.data, n,
                                       int(async_), rq.ctypes.data, rf.ctypes.data, blob.ctypes.data, len(names),
                                       int(parts), w[0], w[1], w[2], w[3], out[1:].ctypes.data, result[1:].ctypes.data)
        assert (result[0] == 0x5A).all() and (result[-1] == 0x5A).all()
        assert (words[:, 0] == 0x5A5A5A5A).all() and (words[:, -1] == 0x5A5A5A5A).all()
        assert (out[0] == 0x5A).all() and (out[-1] == 0x5A).all()
        keep = np.ones(len(arena), bool)
        for b in range(n):
            keep[offs[b]: offs[b] + len(payloads[b])] = False
        assert (arena[keep] == before[keep]).all(), "a guard byte changed"
        per = [(result[1 + b].tobytes(), arena[offs[b]: offs[b] + len(payloads[b])].tobytes()) for b in range(n)]
        return per, words[0, 1:-1].view(np.int32), words[1, 1:-1], words[2, 1:-1], words[3, 1:-1], out[1:-1]
    return run


def same(got, want, payloads, names=None):
    """A run's answer against U.expect()'s."""
    per, err, nr, depth, what, out = got
    wper, werr, wnr, wdepth, wwhat, wout = want
    assert err.tolist() == werr.tolist()
    assert (nr.tolist(), depth.tolist()) == (wnr.tolist(), wdepth.tolist())
    assert what.tolist() == wwhat.tolist()
    assert (out == wout).all(), "a record"
    for b, ((res, after), w) in enumerate(zip(per, wper)):
        which = names[b] if names else f"ITB {b}"
        assert U.result_fields(res) == w.fields, which
        assert after == w.payload, f"{which}: the payload"
        if not w.produced:
            assert after == bytes(payloads[b]), f"{which}: nothing produced, yet the payload changed"


def agree(host_unlink, cases, async_, interleave=False, invariants=True):
    """cases as one call, in the reference's form and in the kernel's rounds,
    against the oracle.  Returns the oracle's answers."""
    recs, adepths, req, names = U.call_of(cases, interleave)
    order, first = U.group(req, len(recs))
    req = req[order]
    payloads, hdrs = [C.payload_of(r) for r in recs], [C.hdr_of(r) for r in recs]
    want = U.expect(payloads, adepths, hdrs, req, first, names, async_)
    for parts in (False, True):
        same(host_unlink(payloads, adepths, hdrs, req, first, names, async_, parts=parts), want, payloads,
             [c[0] for c in cases])
    if invariants:
        for b, u in enumerate(want[0]):
            if u.produced:
                U.invariants(payloads[b], adepths[b], hdrs[b], u)
    return want


def test_ite_unlink_table_exhaustive(host_lib):
    """Every flag kind (none, NORMAL, SYM, LS, KV alone, NORMAL | LS, KV with
    each refused partner), with and without SDT, every state 0 ... 7, nlink 0,
    1, 2, 3 and 65535, a regular file, a directory, a block device and a
    socket, both async values."""
    out = np.zeros(3, np.uint32)
    n = refused = 0
    for flag, mode, nlink, async_ in U.ite_unlink_cases():
        host_lib.itb_unlink_ite_host(flag, mode, nlink, int(async_), out.ctypes.data)
        want = U.ite_unlink(flag, mode, nlink, async_)
        if want is None:
            assert int(out[2]) == 0xFFFFFFFE and (int(out[0]), int(out[1])) == (flag, nlink)
            refused += 1
        else:
            assert (int(out[0]), int(out[1]), int(out[2])) == want[:3], (hex(flag), oct(mode), nlink, async_)
            assert want[3] == (want[2] & 0xFF == U.DELETED)
        n += 1
    assert n == 9 * 2 * 8 * 5 * 4 * 2 and refused == 3 * 2 * 8 * 5 * 4 * 2


def test_ite_unlink_wraps_and_delta():
    """0 wraps to 65535, and a directory's 1 does; the mode test is the bit
    0040000, which a block device and a socket have too; POM_UL_DELTA in each
    of its three ways: KV | SDT, an SDT entry whose nlink reaches 0, and an SDT
    entry left with nlink 0 without being changed."""
    f = U.ite_unlink
    assert f(U.NORMAL, 0o100644, 0, False) == (U.NORMAL | U.SHADOW, 65535, U.SHADOWED, False)
    assert f(U.NORMAL, 0o040755, 1, True) == (U.NORMAL | U.SHADOW, 65535, U.SHADOWED, False)
    assert f(U.SYM | 5, 0o040755, 2, True) == (U.SYM | U.UNLINKED, 0, U.MARKED, False)
    assert f(U.NORMAL, 0o060660, 2, False)[1:] == (0, U.DELETED, True)
    assert f(U.NORMAL, 0o140777, 3, False)[1:3] == (1, U.SHADOWED)
    assert f(U.NORMAL | U.LS, 0o100644, 2, False)[1:3] == (1, U.SHADOWED)          # A, not B
    assert f(U.LS | 2, 0o100644, 9, True) == (U.LS | 2, 0, U.DELETED, True)
    assert f(U.KV | U.SDT, 0o100644, 9, True) == (U.KV | U.SDT, 9, U.DELETED | U.DELTA, True)
    assert f(U.KV, 0o100644, 0, True)[2] == U.DELETED
    assert f(U.NORMAL | U.SDT, 0o040755, 2, True)[2] == U.MARKED | U.DELTA
    assert f(U.NORMAL | U.SDT, 0o040755, 3, True)[2] == U.SHADOWED
    assert f(U.SDT, 0o040755, 0, False) == (U.SDT, 0, U.NONE | U.DELTA, False)
    assert f(U.SDT, 0o040755, 1, False)[2] == U.NONE
    assert f(U.KV | U.NORMAL, 0, 1, False) is None


@pytest.mark.parametrize("async_", [False, True])
def test_del_ite_edges(host_unlink, async_):
    """A UNIQUE home; a head with one and with two followers (the swap); a
    middle and a tail target; the ITB's last entry; the ITE at max_offset and
    the one below it; a delete in the overflow half against one in the home
    half."""
    cases = U.del_ite_cases()
    per = agree(host_unlink, cases, async_)[0]
    by = {c[0]: u for c, u in zip(cases, per)}
    hdr = {c[0]: C.hdr_of(c[1]) for c in cases}
    if async_:
        assert all(u.fields["removed"] == 0 and u.answers[0][3] == U.MARKED for u in per)
        assert all(u.payload[:C.ITE_OFF] == C.payload_of(c[1])[:C.ITE_OFF] for c, u in zip(cases, per))
        return
    assert all(u.fields["removed"] == 1 and u.answers[0][3] == U.DELETED for u in per)
    f = by["last_entry"].fields
    assert (f["entries"], f["max_offset"], f["len"]) == (0, 0, C.ITB_SIZE)
    assert by["at_max_offset"].fields["max_offset"] == 4 and by["below_max_offset"].fields["max_offset"] == 5
    f, g = by["overflow_half"].fields, by["home_half"].fields
    assert (f["itu"], f["pseudo_conflicts"]) == (hdr["overflow_half"]["itu"] - 1, hdr["overflow_half"]["pseudo_conflicts"] - 1)
    assert (g["itu"], g["pseudo_conflicts"]) == (hdr["home_half"]["itu"], hdr["home_half"]["pseudo_conflicts"])
    # the swap: the head's slot keeps the chain with the follower's ITE; the follower's slot is the one freed
    t = S.table_of(by["head_two_followers"].payload, 2, U.changed_hdr(hdr["head_two_followers"], by["head_two_followers"].fields))
    assert [e for _, e in U.chain_of(t, 0)] == [0, 1]
    follower = U.chain_of(U.chain3(), 0)[1][0]
    assert C.get_slot(t.rec, C.H, follower)[::2] == (2, C.IDX_FREE)
    t = S.table_of(by["head_one_follower"].payload, 1, U.changed_hdr(hdr["head_one_follower"], by["head_one_follower"].fields))
    assert C.get_slot(t.rec, C.H, 0)[::2] == (1, C.IDX_UNIQUE)
    t = S.table_of(by["unique_home"].payload, 2, U.changed_hdr(hdr["unique_home"], by["unique_home"].fields))
    assert C.get_slot(t.rec, C.H, 1)[::2] == (1, C.IDX_FREE)


@pytest.mark.parametrize("async_", [False, True])
def test_order_within_an_itb(host_unlink, async_):
    """Each request sees what the earlier ones of its ITB left."""
    cases = U.order_cases()
    per = agree(host_unlink, cases, async_)[0]
    by = {c[0]: u for c, u in zip(cases, per)}
    what = lambda name: [(a[0], a[3]) for a in by[name].answers]
    last = U.MARKED if async_ else U.DELETED
    assert what("same_name_twice") == [(0, U.SHADOWED), (0, last)]
    assert what("second_misses") == [(0, last), (U.ENOENT, 0)]
    assert by["second_misses"].answers[1][2] == (1 if async_ else 0)        # the marked ITE is still compared
    # past the first twin (marked, or gone) to the second
    assert [(a[0], a[1]) for a in by["walks_past_marked"].answers] == [(0, 0), (0, 1)]
    assert by["walks_past_marked"].answers[1][2] == (2 if async_ else 1)
    assert what("shadow_hits_marked") == ([(0, U.MARKED), (0, U.SHADOWED)] if async_ else [(0, U.DELETED), (U.ENOENT, 0)])
    if async_:
        after = by["shadow_hits_marked"].payload
        assert struct.unpack_from("<H", after, C.ITE_OFF + U.NLINK_OFF)[0] == 65535
        assert struct.unpack_from("<I", after, C.ITE_OFF + U.FLAG_OFF)[0] & 7 == U.SHADOW
        # the second record shows what the first request left: nlink 0
        assert struct.unpack_from("<H", by["shadow_hits_marked"].answers[1][4], 8 + U.NLINK_OFF - U.MD_OFF)[0] == 0
    assert [(a[0], a[2]) for a in by["head_then_swapped"].answers] == [(0, 1), (0, 2 if async_ else 1)]
    for name in ("empties_chain", "empties_chain_tail_first"):
        assert [a[0] for a in by[name].answers] == [0, 0]
        if not async_:
            assert by[name].fields["entries"] == 0 and not U.live_chains(by[name].payload, 1)
    if not async_:
        a, b = by["order_ab"], by["order_ba"]
        assert a.fields == b.fields and a.payload != b.payload                  # the freed slots keep different entries
        assert U.live_chains(a.payload, 2) == U.live_chains(b.payload, 2)
    k = what("kinds")
    assert k[0] == (0, last | U.DELTA) and k[1] == (0, U.SHADOWED) and k[2] == (0, U.DELETED)
    assert k[3] == (0, U.DELETED | U.DELTA) and k[4] == (0, U.NONE | U.DELTA) and k[5:] == [(0, U.SHADOWED), (0, last)]
    assert by["kinds"].fields["changed"] == 6 and by["kinds"].fields["hits"] == 7


def test_interleaved_callers_order(host_unlink):
    """The caller's interleaving of several ITBs' requests, grouped stably,
    gives each ITB its own requests in the caller's order."""
    cases = U.order_cases()
    plain = agree(host_unlink, cases, False)
    mixed = agree(host_unlink, cases, False, interleave=True)
    assert [u.result for u in plain[0]] == [u.result for u in mixed[0]]
    assert [u.payload for u in plain[0]] == [u.payload for u in mixed[0]]


@pytest.mark.parametrize("async_", [False, True])
def test_refused_flags_and_requests(host_unlink, async_):
    """KV with NORMAL, SYM or LS: -EINVAL and nothing changed; a request with
    POM_LK_LOOKUP, POM_LK_COLUMN, INDEX_KV or a stray bit, with column 1, or
    with another group's ITB number: -EINVAL; the good request among them still
    applies.  Then namelen 256 and a name that leaves the blob."""
    cases = U.refused_cases()
    per, err = agree(host_unlink, cases, async_)[:2]
    assert err.tolist() == [C.EINVAL] * 3 + [0] + [C.EINVAL] * 6
    rec = cases[0][1]
    for nr in range(3):
        at = C.ITE_OFF + C.ITE_SIZE * nr
        assert per[0].payload[at: at + C.ITE_SIZE] == C.payload_of(rec)[at: at + C.ITE_SIZE]
    payload, hdr = C.payload_of(rec), C.hdr_of(rec)
    good = U.by_name(rec, 0, 3)
    req, names = lookup.requests([good, good])
    req = np.concatenate([req, req, req[:1]])
    req["namelen"][1] = 256
    req["name_off"][2], req["namelen"][2] = len(names) - 1, 2
    req["name_off"][3], req["namelen"][3] = len(names), 0
    req["itb"][4] = 1                                                   # in group 0, yet not ITB 0's
    first = np.array([0, 5], np.uint32)
    want = U.expect([payload], [2], [hdr], req, first, names, async_)
    assert want[1].tolist() == [0, C.EINVAL, C.EINVAL, U.ENOENT, C.EINVAL]
    for parts in (False, True):
        same(host_unlink([payload], [2], [hdr], req, first, names, async_, parts=parts), want, [payload])


def test_damaged_tables_are_never_walked(host_unlink):
    """Every table of itb_sweep_util.damaged_tables(): each request gets
    POM_SPLIT_E_DAMAGED with a zero record and no byte changes; a decoder's
    code, a misaligned payload and a bad adepth go the same way."""
    tables = W.damaged_tables()
    cases = []
    for name, rec, adepth in tables:
        items = [dict(itb=0, hash=h, uuid=1, flag=U.BY_UUID) for h in (0, 1, (1 << adepth) - 1)]
        cases.append((name, rec, adepth, items))
    per, err = agree(host_unlink, cases, False, invariants=False)[:2]
    assert all(u.fields == dict.fromkeys(U.RESULT_FIELDS, 0) | {"err": U.E_DAMAGED} for u in per)
    assert err.tolist() == [U.E_DAMAGED] * (3 * len(tables))
    t = U.built(2, 7, [0, 1])
    payload, hdr = C.payload_of(t.record()), C.hdr_of(t.record())
    req, names = lookup.requests([U.by_name(t, b, 0) for b in range(4)])
    first = np.arange(5, dtype=np.uint32)
    args = ([payload] * 4, [2, 2, 0, 2], [hdr] * 4, req, first, names)
    want = U.expect(*args, False, [64, 72, 64, 64], [0, 0, 0, -6])
    assert want[1].tolist() == [0, C.EINVAL, C.EINVAL, -6]
    for parts in (False, True):
        same(host_unlink(*args, False, [0, 0, 0, -6], [0, 8, 0, 0], parts=parts), want, [payload] * 4)


def test_random_tables(host_unlink):
    """200 seeded tables of adepth 1 ... 4 built by random adds and deletes,
    every kind of entry, 1 ... 12 requests each: itb_unlink.h equals the
    restatement in every byte, and every invariant holds."""
    produced = 0
    for lo in range(0, 200, 50):
        by_async = {False: [], True: []}
        for seed in range(lo, lo + 50):
            rec, adepth, items, async_ = U.random_case(7000 + seed)
            by_async[async_].append((f"seed {seed}", rec, adepth, items))
        for async_, cases in by_async.items():
            per = agree(host_unlink, cases, async_)[0]
            produced += sum(u.produced for u in per)
    assert produced > 100


# ---------------------------------------------------------------------------
# The header builder
# ---------------------------------------------------------------------------
def changed_example(async_: bool):
    cases = [c for c in U.order_cases() if c[0] == "kinds"]
    recs, adepths, req, names = U.call_of(cases)
    rec = bytearray(recs[0])
    u = U.expect_one(C.payload_of(rec), adepths[0], C.hdr_of(rec), L.as_dicts(req), names, async_)
    assert u.produced
    rec[:C.H] = np.random.default_rng(3).integers(0, 256, C.H, dtype=np.uint8).tobytes()      # pointers, locks, txg
    return rec, u


@pytest.mark.parametrize("async_", [False, True])
def test_header_byte_for_byte(async_):
    """pom_itb_unlink_header against the oracle's header(): of the 264 bytes
    only the named fields differ from the old header; `state` stays.  It is
    valid with removed == 0."""
    rec, u = changed_example(async_)
    f = u.fields
    for state in (0, 1, 4):
        rec[S.ITBH_STATE] = state
        h, lzo_ = unlink.unlink_header(rec[:C.H], u.result)
        assert (h, lzo_) == U.header(rec[:C.H], u.result) and lzo_ == 0 and h[S.ITBH_STATE] == state
        span = lambda off, size: set(range(off, off + size))
        fields = span(C.ITBH_ENTRIES, 8) | span(C.ITBH_PSEUDO, 4) | span(C.ITBH_ITU, 2) | span(C.ITBH_LEN, 8) | \
            span(S.ITBH_ALGO, 2)
        assert {i for i in range(C.H) if h[i] != rec[i]} <= fields
        got = C.hdr_of(h)
        assert (got["entries"], got["max_offset"], got["pseudo_conflicts"], got["itu"], got["ulen"]) == \
            (f["entries"], f["max_offset"], f["pseudo_conflicts"], f["itu"], f["len"])
    only_marked = U.RESULT.pack(0, 1, 0, C.ITB_SIZE + C.ITE_SIZE, 1, 0, 0, 0, 1)
    assert unlink.unlink_header(rec[:C.H], only_marked) == U.header(rec[:C.H], only_marked)
    for res in (U._only(U.E_DAMAGED), U._only(0, 3), U.RESULT.pack(0, 1, 1, 263, 0, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            unlink.unlink_header(rec[:C.H], res)


def test_not_smaller_rule_at_its_tie():
    """itb_lzo_compress keeps a stream only when it is smaller than the
    payload: a stream one byte longer, as long, one and two bytes shorter.  The
    rule is the split's own function."""
    import record_util as R
    rec, u = changed_example(False)
    f = u.fields
    for diff in R.TIE_DIFFS:
        z = f["len"] - C.H + diff
        h, lzo_ = unlink.unlink_header(rec[:C.H], u.result, z)
        assert (h, lzo_) == U.header(rec[:C.H], u.result, z), diff
        assert lzo_ == int(diff < 0), diff
        ln, zlen, algo = struct.unpack_from("<IIH", h, C.ITBH_LEN)
        assert (ln, zlen, algo) == ((C.H + z, f["len"], 1) if diff < 0 else (f["len"], 0, 0)), diff
    text = open(os.path.join(ROOT, "pomegranate_amd", "csrc", "unlink.c")).read()
    assert "pom_itb_stored_as(" in text and "POM_COMPR_LZO" not in text


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_unlink_batch_refuses():
    """LZO_E_ERROR, with every output as the caller left it."""
    t = U.built(2, 7, [0, 1])
    rec = bytes(t.record())
    req, names = lookup.requests([U.by_name(t, 0, 0)])
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        unlink.unlink_batch([rec], req, names)
    buf = np.frombuffer(rec, dtype=np.uint8)
    blob = np.frombuffer(names, np.uint8)
    ptrs, lens = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(buf.size)
    out = np.full(len(rec), 7, np.uint8)
    optr, caps, ol = (ctypes.c_void_p * 1)(out.ctypes.data), (ctypes.c_size_t * 1)(len(rec)), (ctypes.c_size_t * 1)(7)
    result, rec_out = np.full(32, 7, np.uint8), np.full(136, 7, np.uint8)
    words = np.full((4, 1), 7, np.int32)
    ierr, ok = np.full(1, 7, np.int32), np.full(1, 7, np.int32)
    rc = unlink._lib().pom_itb_unlink_batch(ptrs, lens, 1, 0, 0, req.ctypes.data, 1, blob.ctypes.data, len(names),
                                            rec_out.ctypes.data, *(words[k].ctypes.data for k in range(4)), optr, caps,
                                            ol, result.ctypes.data, ierr.ctypes.data, ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    assert (out == 7).all() and (result == 7).all() and (rec_out == 7).all() and (words == 7).all()
    assert (ierr[0], ok[0], ol[0]) == (7, 7, 7)


# ---------------------------------------------------------------------------
# The stand-alone program, the exports
# ---------------------------------------------------------------------------
def test_standalone_check_passes():
    """itb_unlink_check: both forms of itb_unlink.h over seeded tables and
    flipped ones, every payload a heap block of exactly its length, built with
    AddressSanitizer and UBSan where they link."""
    r = subprocess.run([os.path.join(NATIVE, "itb_unlink_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_unlink_check: ok" in r.stdout


def test_exports_are_declared():
    names = {"pom_itb_unlink_dev", "pom_itb_unlink_scratch", "pom_itb_unlink_header", "pom_itb_unlink_batch"}
    assert names <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert all(hasattr(lib, name) for name in names)
    text = open(os.path.join(ROOT, "include", "pom_unlink.h")).read()
    assert all(re.search(rf"\b{name}\(", text) for name in names)
    # the launchers and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_itb_unlink", "lzo_mi355x_launch_itb_unlink_lens", "pom_itb_unlink_chunked"} & \
        set(lzo.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", lzo.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines()}
    assert unlink.unlink_scratch_bytes(0) == 0 and unlink.unlink_scratch_bytes(5) >= 5 * 52
    # the device entry refuses a NULL hdr and misaligned arrays before it queues anything
    dev = unlink._lib().pom_itb_unlink_dev
    nul = [None] * 8
    assert dev(None, None, None, None, None, None, 0, 0, None, None, 0, None, 0, *nul) == C.EINVAL
    assert dev(8, None, None, None, None, 8, 0, 0, None, None, 0, None, 0, *nul) == C.EINVAL
    assert dev(16, None, None, None, None, 8, 0, 0, 4, None, 0, None, 0, *nul) == C.EINVAL
    assert dev(16, None, None, None, None, 8, 0, 0, 8, None, 0, None, 0, None, None, None, None, 4, None, None,
               None) == C.EINVAL
