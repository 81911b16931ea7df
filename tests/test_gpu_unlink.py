"""GPU: the ITB unlink (include/pom_unlink.h) against the Python restatement of
itb_search's unlink branch, ite_unlink and itb_del_ite in unlink_util.py --
pom_itb_unlink_dev on guarded arenas filled with a constant, then
pom_itb_unlink_batch.  Everything is compared with the oracle: the requests'
words and records, the results, the payloads, and every byte that must not
change (the whole arena is compared with the one the oracle expects, so a
payload outside its bitmap, its index and the six bytes of a hit ITE, the
guards around every payload and the guards around every result array)."""
from __future__ import annotations

import ctypes
import os
import re
import struct

import numpy as np
import pytest

import check_util as C
import itb_split_util as S
import itb_sweep_util as W
import lookup_util as L
import unlink_util as U
from conftest import ROOT
from gpu_util import guarded_batch
from pomegranate_amd import check, itb, itbsweep, lookup, lzo, unlink

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL_SRC, FILL = 0xEE, 0x5A
H = itb.ITBH_SIZE
PAD = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def unlink_dev_once(dev, payloads, adepths, hdrs, req, req_first, names, async_, want, status=None, shifts=None):
    """One call over a guarded batch: payload b at residue shifts[b] mod 16
    (default 0), the blob at an odd address.  The answer, against `want`
    (U.expect's): words, records, results, and the whole arena."""
    n, nreq = len(payloads), len(req)
    shifts = [0] * n if shifts is None else list(shifts)
    src = guarded_batch(torch, [bytes(p) for p in payloads], dev, shifts, fill=FILL_SRC)
    before = src.arena.cpu().numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    adepth = t(np.asarray(adepths, dtype=np.uint8))
    hd = t(np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy())
    st = None if status is None else t(np.asarray(status, dtype=np.int32))
    rq = t(np.frombuffer(np.ascontiguousarray(req, dtype=lookup.REQ_DTYPE).tobytes() or bytes(32), np.uint8).copy())
    rf = t(np.asarray(req_first, dtype=np.uint32).view(np.int32))
    blob = t(np.frombuffer(b"\xEE" + bytes(names) + b"\xEE", np.uint8).copy())[1:]
    res = torch.full((PAD + 32 * n + PAD,), FILL, dtype=torch.uint8, device=dev)
    words = [torch.full((PAD + 4 * nreq + PAD,), FILL, dtype=torch.uint8, device=dev) for _ in range(4)]
    out = torch.full((PAD + 136 * nreq + PAD,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(unlink.unlink_scratch_bytes(n), 256), dtype=torch.uint8, device=dev)
    w = [x[PAD: PAD + 4 * nreq] for x in words]
    unlink.unlink_dev(src, adepth, hd, async_, rq, rf, nreq, blob, len(names), w[0], w[1], w[2], w[3],
                      out[PAD: PAD + 136 * nreq], res[PAD: PAD + 32 * n], scratch, status=st)
    torch.cuda.synchronize()
    per, werr, wnr, wdepth, wwhat, wout = want
    host = [x.cpu().numpy() for x in words]
    for x in host + [res.cpu().numpy(), out.cpu().numpy()]:
        assert (x[:PAD] == FILL).all() and (x[len(x) - PAD:] == FILL).all(), "a result array's guards"
    word = lambda k, dt: host[k][PAD: PAD + 4 * nreq].view(dt)
    assert word(0, np.int32).tolist() == werr.tolist()
    assert (word(1, np.uint32).tolist(), word(2, np.uint32).tolist()) == (wnr.tolist(), wdepth.tolist())
    assert word(3, np.uint32).tolist() == wwhat.tolist()
    assert (out.cpu().numpy()[PAD: PAD + 136 * nreq].reshape(nreq, 136) == wout).all(), "a record"
    results = res.cpu().numpy()[PAD: PAD + 32 * n]
    expected = before.copy()
    for b, u in enumerate(per):
        assert U.result_fields(results[32 * b: 32 * b + 32].tobytes()) == u.fields, f"ITB {b}"
        o = int(src.host_off[b])
        expected[o: o + len(payloads[b])] = np.frombuffer(u.payload, np.uint8)
        if not u.produced:
            assert u.payload == bytes(payloads[b])
    after = src.arena.cpu().numpy()
    diff = np.flatnonzero(after != expected)
    assert diff.size == 0, f"the arena differs from the oracle's, first at {int(diff[0]) if diff.size else -1}"


def call(cases, async_, interleave=False, status=None, shifts=None):
    """cases as one grouped call and the oracle's answer to it."""
    recs, adepths, req, names = U.call_of(cases, interleave)
    order, first = U.group(req, len(recs))
    req = req[order]
    payloads, hdrs = [C.payload_of(r) for r in recs], [C.hdr_of(r) for r in recs]
    want = U.expect(payloads, adepths, hdrs, req, first, names, async_, shifts, status)
    return (payloads, adepths, hdrs, req, first, names, async_, want), want


@pytest.mark.parametrize("async_", [False, True])
def test_dev_directed_tables(dev, async_):
    """itb_del_ite's edges, the order cases and the refused flags and
    requests, each table an ITB of one launch; then with the caller's requests
    interleaved over the ITBs, so that an ITB's order is not the call's."""
    cases = U.directed()
    for interleave in (False, True):
        args, want = call(cases, async_, interleave)
        unlink_dev_once(dev, *args)
    by = {c[0]: u for c, u in zip(cases, want[0])}
    assert by["same_name_twice"].answers[1][3] == (U.MARKED if async_ else U.DELETED)
    assert by["kinds"].fields["hits"] == 7 and by["refused"].fields["changed"] == 1
    for b, u in enumerate(want[0]):
        if u.produced:
            U.invariants(args[0][b], args[1][b], args[2][b], u)


def long_chain_table():
    """adepth 10: 65 ITEs in home slot 0's chain, so that the walk's round of
    64 members is crossed, and a few more elsewhere."""
    t = U.built(10, 110, [0 | U.UP(i) for i in range(65)] + [5, 6, 7 | U.UP(1)])
    assert len(U.chain_of(t, 0)) == 65
    return t


@pytest.mark.parametrize("async_", [False, True])
def test_dev_chain_of_65(dev, async_):
    """A miss behind 65 compares, the 64th and the 65th member, a miss, the head, then
    members again: depth 65, 64, 65, 65, 1 where the ITEs are only marked, and
    65, 64, 64, 63, 1 where each delete shortens the chain."""
    t = long_chain_table()
    ch = [e for _, e in U.chain_of(t, 0)]
    miss = dict(U.by_name(t, 0, ch[64]), name=b"nobody")
    items = [miss, U.by_name(t, 0, ch[63]), U.by_name(t, 0, ch[64]), miss, U.by_name(t, 0, ch[0]), U.by_uuid(t, 0, ch[64]),
             U.by_name(t, 0, ch[62]), miss, U.by_name(t, 0, ch[1], U.F_SHADOW)]
    args, want = call([("chain65", t.record(), 10, items)], async_)
    assert want[3][:5].tolist() == ([65, 64, 65, 65, 1] if async_ else [65, 64, 64, 63, 1])
    assert want[1][5] == U.ENOENT and want[3][7] == (65 if async_ else 61)
    unlink_dev_once(dev, *args)


def test_dev_names_at_odd_offsets(dev):
    """Names of 0, 1, 7, 8, 9 and 255 bytes, each at an odd offset of a blob
    that itself lies at an odd address; each with a twin whose last byte
    differs (a miss)."""
    lens = (0, 1, 7, 8, 9, 255)
    t = U.built(3, 111, [nr for nr in range(len(lens))], nlink=2)
    rng = np.random.default_rng(111)
    blob, rows = bytearray(b"\xEE"), []
    for nr, ln in enumerate(lens):
        name = rng.integers(1, 256, ln, dtype=np.uint8).tobytes()
        U.entry(t, nr, nlink=2, name=name)
        for twin in (name, name[:-1] + bytes([name[-1] ^ 1]) if ln else None):
            if twin is None:
                continue
            if len(blob) % 2 == 0:
                blob.append(0xEE)
            rows.append((nr, 0, 0, U.BY_NAME | U.UNLINK, len(blob), ln, 0))
            blob += twin
    req = np.array(rows, dtype=lookup.REQ_DTYPE)
    assert all(int(o) % 2 == 1 for o in req["name_off"])
    payload, hdr = C.payload_of(t.record()), C.hdr_of(t.record())
    first = np.array([0, len(req)], np.uint32)
    want = U.expect([payload], [3], [hdr], req, first, bytes(blob), False)
    assert want[1].tolist() == [0, 0, U.ENOENT, 0, U.ENOENT, 0, U.ENOENT, 0, U.ENOENT, 0, U.ENOENT]
    unlink_dev_once(dev, [payload], [3], [hdr], req, first, bytes(blob), False, want)


@pytest.mark.parametrize("async_", [False, True])
def test_dev_mixed_call(dev, async_):
    """A refused ITB, an ITB with no requests, an ITB whose requests all miss, a
    decoder's code, a payload at residue 8 and a bad adepth between ITBs that
    change: one launch."""
    good = U.order_cases()[-1]
    t = U.built(2, 112, [0, 1, 2])
    rec = t.record()
    misses = [dict(U.by_name(t, 0, nr), name=b"absent") for nr in range(3)]
    drec = C.kind_tables()["dup"][0]
    probe = [dict(itb=0, hash=h, uuid=1, flag=U.BY_UUID) for h in (0, 1)]
    cases = [good, ("damaged", drec, 2, probe), ("no_requests", rec, 2, []), ("all_miss", rec, 2, misses),
             ("status", rec, 2, [U.by_name(t, 0, 0)]), ("residue", rec, 2, [U.by_name(t, 0, 1)]),
             ("adepth", rec, 0, [U.by_name(t, 0, 2)]), good]
    status, shifts = [0, 0, 0, 0, -6, 0, 0, 0], [0, 0, 0, 0, 0, 8, 0, 0]
    args, want = call(cases, async_, True, status, shifts)
    per = want[0]
    assert [u.fields["err"] for u in per] == [0, U.E_DAMAGED, 0, 0, -6, C.EINVAL, C.EINVAL, 0]
    assert per[3].fields == dict.fromkeys(U.RESULT_FIELDS, 0) and per[2].fields == per[3].fields
    assert per[0].produced and per[7].produced and not any(u.produced for u in per[1:7])
    unlink_dev_once(dev, *args, status=status, shifts=shifts)


GRID_MAX = 4096                 # itb_unlink.hip kUnlinkGridMax: above it a workgroup takes ITB b, b + 4096, ...


def test_dev_many_itbs_reuse_the_workgroup(dev):
    """4097 ITBs of adepth 1 with one request each, of five kinds in turn, so
    that one workgroup applies two ITBs in the LDS it never clears as a whole,
    and every kind follows an unlike one somewhere in the grid."""
    with open(os.path.join(ROOT, "pomegranate_amd", "csrc", "itb_unlink.hip")) as f:
        assert re.search(r"kUnlinkGridMax = (\d+);", f.read()).group(1) == str(GRID_MAX)
    n = GRID_MAX + 1
    t = U.built(1, 113, [0, 0 | U.UP(1)])
    ch = [e for _, e in U.chain_of(t, 0)]
    dup = C.kind_tables(1)["dup"][0]
    kinds = [("head", t.record(), 1, [U.by_name(t, 0, ch[0])]), ("tail", t.record(), 1, [U.by_name(t, 0, ch[1])]),
             ("miss", t.record(), 1, [dict(U.by_name(t, 0, 0), name=b"x")]),
             ("damaged", dup, 1, [dict(itb=0, hash=0, uuid=1, flag=U.BY_UUID)]),
             ("shadowed", U.built(1, 114, [1], nlink=3).record(), 1, [dict(itb=0, hash=1, uuid=1000, flag=U.BY_UUID)])]
    which = np.array([4 if b == GRID_MAX else b % 5 for b in range(n)])     # workgroup 0: "head", then "shadowed"
    one = call(kinds, False)[1]                                     # the oracle once a kind: an ITB has one request
    recs, adepths, req, names = U.call_of([kinds[k] for k in which])
    assert req["itb"].tolist() == list(range(n))
    payloads, hdrs = [C.payload_of(r) for r in recs], [C.hdr_of(r) for r in recs]
    want = ([one[0][k] for k in which],) + tuple(a[which] for a in one[1:])
    assert [u.fields["err"] for u in want[0][:5]] == [0, 0, 0, U.E_DAMAGED, 0]
    assert want[0][0].fields["removed"] == 1 and want[0][GRID_MAX].fields["changed"] == 1
    unlink_dev_once(dev, payloads, adepths, hdrs, req, np.arange(n + 1, dtype=np.uint32), names, False, want)


@pytest.mark.parametrize("async_", [False, True])
def test_dev_adepth_10_with_64_requests(dev, async_):
    """One random table of adepth 10 and 64 requests, by name and by uuid, some
    twice, some with ITE_SHADOW."""
    t = C.random_table(115, 10, 1500)
    rng = np.random.default_rng(115)
    kinds = [U.NORMAL, U.NORMAL | U.SDT, U.SYM, U.LS, U.KV, 0]
    for nr in sorted(t.hashes):
        U.entry(t, nr, flag=int(rng.choice(kinds)), nlink=int(rng.integers(0, 4)), mode=int(rng.choice(U.MODES)))
    live = sorted(t.hashes)
    picks = [int(x) for x in rng.choice(live, 48)]
    picks += picks[:16]
    items = [U.by_name(t, 0, nr, U.F_SHADOW if k % 7 == 3 else 0) if k % 2 else U.by_uuid(t, 0, nr)
             for k, nr in enumerate(picks)]
    args, want = call([("wide", t.record(), 10, items)], async_)
    assert want[0][0].fields["changed"] >= 30 and (want[1] == U.ENOENT).any()
    unlink_dev_once(dev, *args)
    U.invariants(args[0][0], 10, args[2][0], want[0][0])


def test_dev_refuses_what_it_cannot_run(dev):
    """hdr is required, the arena is 16-byte aligned, req and out 8-byte
    aligned, the scratch has its size: refused before anything is queued."""
    t = U.built(2, 116, [0, 1])
    payload, hdr = C.payload_of(t.record()), C.hdr_of(t.record())
    req, names = lookup.requests([U.by_name(t, 0, 0)])
    src = guarded_batch(torch, [payload], dev, [0], fill=FILL_SRC)
    before = src.arena.cpu().numpy()
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    adepth = torch.tensor([2], dtype=torch.uint8, device=dev)
    hd = tt(np.frombuffer(C.hdr_bytes(hdr), np.uint8).copy())
    rq = tt(np.frombuffer(bytes(8) + req.tobytes(), np.uint8).copy())
    rf = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    blob = tt(np.frombuffer(names, np.uint8).copy())
    res = torch.full((32,), FILL, dtype=torch.uint8, device=dev)
    w = [torch.full((4,), FILL, dtype=torch.uint8, device=dev) for _ in range(4)]
    out = torch.full((8 + 136,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(unlink.unlink_scratch_bytes(1), dtype=torch.uint8, device=dev)
    run = lambda s, h, r, o, sc: unlink.unlink_dev(s, adepth, h, False, r, rf, 1, blob, len(names), *w, o, res, sc)
    skewed = lzo.DeviceBatch(src.arena[8:], src.off, src.length)
    for bad in ((skewed, hd, rq[8:], out[8:], scratch), (src, hd, rq[4:36], out[8:], scratch),
                (src, hd, rq[8:], out[4:140], scratch), (src, hd, rq[8:], out[8:], scratch[:16]),
                (src, hd[:8], rq[8:], out[8:], scratch)):
        with pytest.raises(ValueError):
            run(*bad)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == FILL).all() and (src.arena.cpu().numpy() == before).all()
    run(src, hd, rq[8:], out[8:], scratch)
    torch.cuda.synchronize()
    r = unlink.Result.parse(res.cpu().numpy().tobytes())
    assert (r.err, r.changed, r.removed, r.hits) == (0, 1, 1, 1)


# ---------------------------------------------------------------------------
# pom_itb_unlink_batch against the oracle
# ---------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _needs_gpu(dev):
    """The host batches pick the device themselves; without one they skip too."""


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


def itbid_matches(st, q) -> bool:
    depth = st[S.ITBH_DEPTH]
    (itbid,) = struct.unpack_from("<Q", st, S.ITBH_ITBID)
    return (q["hash"] >> 10) & (C.M64 if depth >= 64 else (1 << depth) - 1) == itbid


def expect_batch(oracle, stored, recs, req, names, async_, itbid_check=False, codes=None, out_cap=None):
    """The oracle over stored records whose uncompressed records are `recs`
    (None: a record the header checks refuse); codes: {b: the decoder's code}.
    -> (err, nr, depth, what, rec_out [nreq, 136], itb_err [n], results [n]
    bytes, the records after)"""
    n, nreq = len(stored), len(req)
    err, nr, depth, what = [C.EINVAL] * nreq, [0] * nreq, [0] * nreq, [0] * nreq
    rec_out = np.zeros((nreq, 136), np.uint8)
    itb_err = [0 if r is not None else C.EINVAL for r in recs]
    res, outs = [bytes(32)] * n, [b""] * n
    dicts = L.as_dicts(req)
    groups = {}
    for r, q in enumerate(dicts):
        b = q["itb"]
        if b >= n or recs[b] is None:
            continue
        if itbid_check and not itbid_matches(stored[b], q):
            err[r] = U.ESPLIT
            continue
        groups.setdefault(b, []).append(r)
    for b, rs in groups.items():
        st = stored[b]
        u = U.expect_one(C.payload_of(recs[b]), st[S.ITBH_ADEPTH], C.hdr_of(st), [dicts[r] for r in rs], names, async_, b,
                         0, codes.get(b, 0) if codes else 0)
        for r, a in zip(rs, u.answers):
            err[r], nr[r], depth[r], what[r] = a[:4]
            rec_out[r] = np.frombuffer(a[4], np.uint8)
            if a[0] == U.ENOENT and st[S.ITBH_FLAG] == S.ITB_JUST_SPLIT:
                err[r] = U.ESPLIT
        itb_err[b], res[b] = u.fields["err"], u.result
        if u.produced:
            o = U.stored_record(oracle, st[:H], u)
            if out_cap is not None and len(o) > out_cap[b]:
                itb_err[b] = U.E_OUTPUT_OVERRUN
            else:
                outs[b] = o
    return err, nr, depth, what, rec_out, itb_err, res, outs


def same_batch(got, want, tag=""):
    err, nr, depth, what, rec_out, itb_err, res, outs = want
    assert got.err.tolist() == err, tag
    assert (got.nr.tolist(), got.depth.tolist(), got.what.tolist()) == (nr, depth, what), tag
    assert (got.rec == rec_out).all(), f"{tag}a record"
    assert got.itb_err.tolist() == itb_err, tag
    for b in range(len(itb_err)):
        assert got.result[b].tobytes() == res[b], f"{tag}ITB {b}: {got.result[b]} != {U.result_fields(res[b])}"
        assert got.out[b] == outs[b], f"{tag}ITB {b}: the record"


def store(oracle, rec, lzo_form):
    return bytes(C.lzo_record(oracle, rec)) if lzo_form else bytes(rec)


def table_requests(t, b, rng, count):
    """count requests for live ITEs of t, by name and by uuid, some twice."""
    live = sorted(t.hashes)
    picks = [int(x) for x in rng.choice(live, count)]
    return [U.by_name(t, b, nr) if k % 3 else U.by_uuid(t, b, nr) for k, nr in enumerate(picks)]


def mixed_tables():
    """Tables at adepth 1 ... 3, 6 and 10 with every kind of entry, a table
    that does not compress, a table no request reaches, a damaged one."""
    rng = np.random.default_rng(117)
    kinds = [U.NORMAL, U.NORMAL | U.SDT, U.SYM, U.LS, U.KV, 0]
    tables = []
    for k, adepth in enumerate((1, 2, 3, 3, 6, 10, 2)):
        t = C.random_table(9300 + k, adepth, 2 * (1 << adepth) + 3)
        if not t.hashes:
            t.add(1)
        for nr in sorted(t.hashes):
            U.entry(t, nr, flag=int(rng.choice(kinds)), nlink=int(rng.integers(1, 3)), mode=int(rng.choice(U.MODES)))
        tables.append(t)
    # nothing of it compresses: 1000 random ITEs at adepth 10 (entry() sets only a few bytes of each) and a random
    # lock region
    dense = S._built(10, 77, [i | i << 20 for i in range(1000)])
    for nr in range(1000):
        W.set_state(dense.rec, nr, 0)                                   # (none is ITE_UNLINKED before the call)
    for nr in range(0, 1000, 97):
        U.entry(dense, nr, name=b"dense%d" % nr)
    dense.rec[H: H + C.BITMAP_OFF] = rng.integers(0, 256, C.BITMAP_OFF, dtype=np.uint8).tobytes()
    # and random stale bits in the index (a FREE slot's entry and conflict, a UNIQUE slot's conflict: never examined)
    for slot in range(C.INDEX_ENTRIES):
        e, _, flag = C.get_slot(dense.rec, H, slot)
        if flag in (C.IDX_FREE, C.IDX_UNIQUE):
            C.set_slot(dense.rec, H, slot, e if flag else int(rng.integers(0, 32768)), int(rng.integers(0, 32768)), flag)
    return tables, dense


@pytest.fixture(scope="module")
def mixed(oracle):
    """-> (stored, uncompressed records or None, req, names, {b: decoder code})"""
    tables, dense = mixed_tables()
    rng = np.random.default_rng(118)
    recs = [t.record() for t in tables] + [dense.record(), C.kind_tables()["dup"][0]]
    items = []
    for b, t in enumerate(tables[:-1]):                                 # (the last table: no request reaches it)
        items += table_requests(t, b, rng, min(6, 2 * len(t.hashes)))
    nd, ndup = len(tables), len(tables) + 1
    items += [U.by_name(dense, nd, nr) for nr in (0, 97, 970)]
    items += [dict(itb=ndup, hash=1, uuid=1, flag=U.BY_UUID)]
    stored = [store(oracle, r, b % 3 != 1) for b, r in enumerate(recs)]
    # records the header checks refuse, a stream cut short, an ITB that has just split
    bad_adepth, short = bytearray(recs[0]), bytearray(recs[1][:200])
    bad_adepth[3] = 11
    src = C.lzo_record(oracle, recs[4])
    ln, zlen, _ = itb.header_fields(src)
    cut = bytearray(src[: ln - 9])
    struct.pack_into("<I", cut, itb.LEN_OFF, ln - 9)
    rc, _ = oracle.decompress_safe(bytes(cut[H:]), zlen - H)
    assert rc != 0
    split = bytearray(recs[2])
    split[S.ITBH_FLAG] = S.ITB_JUST_SPLIT
    base = len(stored)
    stored += [bytes(bad_adepth), bytes(short), bytes(cut), store(oracle, split, True)]
    recs += [None, None, recs[4], split]
    t2 = tables[2]
    items += [U.by_name(tables[0], base, 0), U.by_name(tables[1], base + 1, 0), U.by_name(tables[4], base + 2, 0),
              U.by_name(t2, base + 3, sorted(t2.hashes)[0]), dict(U.by_name(t2, base + 3, sorted(t2.hashes)[0]), name=b"gone"),
              dict(itb=base + 9, hash=0, flag=U.BY_NAME, name=b"x")]
    order = rng.permutation(len(items))                                 # the caller's order interleaves the ITBs
    req, names = lookup.requests([items[i] for i in order])
    return stored, recs, req, names, {base + 2: rc}


@pytest.mark.parametrize("async_", [False, True])
def test_batch_mixed(oracle, mixed, async_):
    """Every answer and every output equals the oracle's, the output the
    record itb_lzo_compress would store, byte for byte, in caller order; an ITB
    no request reaches or changes has out_len 0; the outputs pass
    pom_itb_check_batch with no finding; a lookup of every unlinked name on
    the output misses by default and hits with ITE_SHADOW where it was marked
    or shadowed."""
    stored, recs, req, names, codes = mixed
    want = expect_batch(oracle, stored, recs, req, names, async_, False, codes)
    got = unlink.unlink_batch(stored, req, names, async_)
    same_batch(got, want)
    err, itb_err, outs = want[0], want[5], want[7]
    n = len(stored)
    produced = [b for b in range(n) if outs[b]]
    assert len(produced) >= 7 and err.count(0) >= 20 and U.ESPLIT in err and C.EINVAL in err and codes[n - 2] in err
    assert itb_err[n - 4: n - 1] == [C.EINVAL, C.EINVAL, codes[n - 2]] and U.E_DAMAGED in itb_err
    assert got.out[6] == b"" and got.result[6].tobytes() == bytes(32) and got.itb_err[6] == 0    # no request reaches it
    algos = {struct.unpack_from("<H", outs[b], itb.ALGO_OFF)[0] for b in produced}
    assert algos == {0, 1}                                              # a payload that does not compress, too
    assert got.len_ok.tolist() == [int(recs[b] is not None and b != n - 2 and b != 6) for b in range(n)]
    again = check.check_batch([got.out[b] for b in produced], 0)
    assert not again.err.any() and not again.report["findings"].any() and again.len_ok.all()
    # every request that hit, looked up on the output
    hit = [r for r in range(len(req)) if err[r] == 0 and outs[int(req["itb"][r])]]
    q = req[hit].copy()
    q["flag"] &= ~np.uint32(U.UNLINK)
    index = {b: k for k, b in enumerate(produced)}
    q["itb"] = [index[int(b)] for b in q["itb"]]
    found = lookup.lookup_batch([got.out[b] for b in produced], q, names)
    q["flag"] |= np.uint32(U.F_SHADOW)
    shadow = lookup.lookup_batch([got.out[b] for b in produced], q, names)
    final = {}
    for r in hit:                                                       # what the ITE's last unlink left
        final[(int(req["itb"][r]), want[1][r])] = want[3][r] & 0xFF
    missed = (U.ENOENT, U.ESPLIT)                                       # (-ESPLIT: the record that has just split)
    for k, r in enumerate(hit):
        last = final[(int(req["itb"][r]), want[1][r])]
        if last in (U.DELETED, U.MARKED):
            assert found.err[k] in missed
        else:
            assert found.err[k] == 0 and found.nr[k] == want[1][r]
        if last in (U.MARKED, U.SHADOWED):
            assert shadow.err[k] == 0 and shadow.nr[k] == want[1][r]
        elif last == U.DELETED:
            assert shadow.err[k] in missed
    assert {U.DELETED, U.SHADOWED} <= set(final.values()) and (not async_ or U.MARKED in final.values())
    assert len(unlink.unlink_batch([], req[:0]).itb_err) == 0


def test_batch_itbid_check(oracle, mixed):
    """itbid_check: a request whose hash does not belong to the ITB is -ESPLIT
    on the host and never reaches the GPU."""
    stored, recs, req, names, codes = mixed
    stored = list(stored)
    deep = bytearray(recs[3])
    deep[S.ITBH_DEPTH] = 2
    struct.pack_into("<Q", deep, S.ITBH_ITBID, 1)
    stored[3] = store(oracle, deep, True)
    want = expect_batch(oracle, stored, recs[:3] + [deep] + recs[4:], req, names, False, True, codes)
    assert want[0].count(U.ESPLIT) >= 3
    same_batch(unlink.unlink_batch(stored, req, names, False, itbid_check=True), want)


def test_round_trip_with_the_sweep(oracle, mixed):
    """Unlink with async_unlink, then pom_itb_sweep_batch on the output,
    against a synchronous unlink of the same list.  The two are not byte equal:
    the sweep walks home slots in order and swaps a marked head behind the
    first live member, itb_del_ite deletes in request order, so freed slots
    keep different entries and live members may sit in different slots of
    their chain, and max_offset may stay above the highest live ITE in
    different ways.  They agree in what a reader sees: entries, the bitmap, and
    for every home slot the set of ITEs on its chain.  (Requests with
    ITE_SHADOW, which can hit a marked ITE again, are left out, and so are ITEs
    an earlier request of the list has marked and a later one meets again.)"""
    stored, recs, req, names, codes = mixed
    sync = unlink.unlink_batch(stored, req, names, False)
    asyn = unlink.unlink_batch(stored, req, names, True)
    marked = [b for b in range(len(stored)) if asyn.out[b] and
              any(w & 0xFF == U.MARKED for w, q in zip(asyn.what, req["itb"]) if q == b)]
    assert len(marked) >= 4
    swept = itbsweep.sweep_batch([asyn.out[b] for b in marked])
    compared = 0
    for k, b in enumerate(marked):
        ws = [int(w) & 0xFF for w, e, q in zip(sync.what, sync.err, req["itb"]) if q == b and e == 0]
        wa = [int(w) & 0xFF for w, e, q in zip(asyn.what, asyn.err, req["itb"]) if q == b and e == 0]
        if len(ws) != len(wa) or any((x == U.DELETED) != (y in (U.DELETED, U.MARKED)) for x, y in zip(ws, wa)):
            continue                                                    # a marked ITE was met again: the lists diverge
        assert swept.err[k] == 0 and swept.out[k]
        pa = payload_after(oracle, sync.out[b])
        pb = payload_after(oracle, swept.out[k])
        adepth = stored[b][S.ITBH_ADEPTH]
        assert C.hdr_of(sync.out[b])["entries"] == C.hdr_of(swept.out[k])["entries"]
        assert pa[C.BITMAP_OFF: C.INDEX_OFF] == pb[C.BITMAP_OFF: C.INDEX_OFF]
        assert U.live_chains(pa, adepth) == U.live_chains(pb, adepth)
        compared += 1
    assert compared >= 3


def payload_after(oracle, rec) -> bytes:
    """The uncompressed payload of a stored record, padded to every ITE its
    adepth allows."""
    ln, zlen, algo = itb.header_fields(rec)
    if algo == 1:
        rc, p = oracle.decompress_safe(bytes(rec[H:ln]), zlen - H)
        assert rc == 0
    else:
        p = bytes(rec[H:ln])
    return p + bytes(C.ITE_OFF + C.ITE_SIZE * 1024 - len(p))


@pytest.fixture(scope="module")
def chunky(oracle):
    """48 adepth-8 tables of about 60 KB with 8 requests each, every fourth
    stored uncompressed: several chunks under chunk_mb=1."""
    rng = np.random.default_rng(119)
    recs, items = [], []
    for b in range(48):
        t = C.random_table(4100 + b, 8, 400)
        for nr in sorted(t.hashes):
            U.entry(t, nr, flag=(U.NORMAL, U.NORMAL | U.SDT, U.LS)[nr % 3], nlink=1 + nr % 2)
        recs.append(t.record())
        items.append(table_requests(t, b, rng, 8))
    flat = [items[b][k] for k in range(8) for b in range(48)]           # interleaved over the ITBs
    req, names = lookup.requests(flat)
    stored = [store(oracle, r, b % 4 != 1) for b, r in enumerate(recs)]
    return stored, req, names, expect_batch(oracle, stored, recs, req, names, False)


def test_batch_spans_chunks(chunky, debug_env, monkeypatch):
    """chunk_mb=1: several chunks, on every visible GPU and on one; results in
    caller order."""
    stored, req, names, want = chunky
    debug_env("chunk_mb=1")
    same_batch(unlink.unlink_batch(stored, req, names), want, "all GPUs: ")
    monkeypatch.setenv("POM_LZO_DEVICES", "0")
    same_batch(unlink.unlink_batch(stored, req, names), want, "one GPU: ")
    assert sum(1 for o in want[7] if o) >= 40


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the call returns LZO_E_ERROR; a lost ITB reads LZO_E_ERROR
    with a zeroed result, a zero length and an untouched buffer, its requests
    LZO_E_ERROR with a zero record; the rest are right, and both kinds occur; a
    clean rerun is right."""
    stored, req, names, want = chunky
    n, nreq = len(stored), len(req)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    caps = [max(itb.header_fields(r)[0], itb.header_fields(r)[1]) for r in stored]
    outs = [np.full(c, 7, np.uint8) for c in caps]
    arr = lambda items: (ctypes.c_void_p * n)(*[b.ctypes.data for b in items])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    ccap = (ctypes.c_size_t * n)(*caps)
    ol = (ctypes.c_size_t * n)(*([7] * n))
    result = np.full(n, 7, dtype=np.uint8).repeat(32).view(unlink.RESULT_DTYPE)
    ierr, ok = np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    words = np.full((4, nreq), 7, np.int32)
    rec_out = np.full((nreq, 136), 7, np.uint8)
    blob = np.frombuffer(names, np.uint8)
    rq = np.ascontiguousarray(req)
    debug_env("chunk_mb=1,fail_chunk=1")
    rc = unlink._lib().pom_itb_unlink_batch(arr(bufs), lens, n, 0, 0, rq.ctypes.data, nreq, blob.ctypes.data, len(names),
                                            rec_out.ctypes.data, *(words[k].ctypes.data for k in range(4)), arr(outs),
                                            ccap, ol, result.ctypes.data, ierr.ctypes.data, ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    lost = ierr == lzo.LZO_E_ERROR
    assert 0 < lost.sum() < n
    for b in range(n):
        if lost[b]:
            assert result[b].tobytes() == bytes(32) and (ol[b], ok[b]) == (0, 0) and (outs[b] == 7).all()
        else:
            assert ierr[b] == want[5][b] and result[b].tobytes() == want[6][b] and ok[b] == 1
            assert outs[b][: ol[b]].tobytes() == want[7][b] and (outs[b][ol[b]:] == 7).all()
    for r in range(nreq):
        if lost[int(req["itb"][r])]:
            assert words[0, r] == lzo.LZO_E_ERROR and not rec_out[r].any() and not words[1:, r].any()
        else:
            assert (words[0, r], words[1, r], words[2, r], words[3, r]) == (want[0][r], want[1][r], want[2][r], want[3][r])
            assert (rec_out[r] == want[4][r]).all()
    debug_env("chunk_mb=1")
    same_batch(unlink.unlink_batch(stored, req, names), want)


def test_batch_out_cap_exact_and_one_short(oracle, mixed):
    """A capacity equal to the record's length suffices; one byte less is
    LZO_E_OUTPUT_OVERRUN with the buffer not written, and the requests'
    answers stand."""
    stored, recs, req, names, codes = mixed
    full = expect_batch(oracle, stored, recs, req, names, False, False, codes)
    exact = [max(len(full[7][b]), 1) for b in range(len(stored))]
    same_batch(unlink.unlink_batch(stored, req, names, out_cap=exact), full, "exact: ")
    short = [c - 1 if full[7][b] and b % 2 == 0 else c for b, c in enumerate(exact)]
    want = expect_batch(oracle, stored, recs, req, names, False, False, codes, out_cap=short)
    assert want[5].count(U.E_OUTPUT_OVERRUN) >= 3 and want[0] == full[0]
    same_batch(unlink.unlink_batch(stored, req, names, out_cap=short), want, "one short: ")
