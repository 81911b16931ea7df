"""GPU: the ITB split (include/pom_split.h) against the Python restatement of
the reference's loop in itb_split_util.py -- pom_itb_split_dev on guarded
arenas filled with a constant.  Everything is compared with the oracle:
result, both payloads, and every byte that must not change (O outside its
bitmap and index, the new payload's room past new_len - 264, the guards
around every payload, every room and the results)."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import check_util as C
import itb_split_util as S
from conftest import ROOT
from gpu_util import guarded_batch
from pomegranate_amd import itbsplit, lzo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL_SRC, FILL = 0xEE, 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def split_dev_once(dev, payloads, adepths, hdrs, sds=None, new_caps=None, status=None, shifts=None):
    """One call over guarded batches: payload b and its new payload's room at
    residue shifts[b] mod 16 (default 0).  -> [(result, the payload after, the
    whole room after, None)], after checking every guard."""
    n = len(payloads)
    caps = [len(p) for p in payloads] if new_caps is None else [int(c) for c in new_caps]
    shifts = [0] * n if shifts is None else list(shifts)
    src = guarded_batch(torch, [bytes(p) for p in payloads], dev, shifts, fill=FILL_SRC)
    dst = guarded_batch(torch, caps, dev, shifts, fill=FILL)
    before = src.arena.cpu().numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    adepth = t(np.asarray(adepths, dtype=np.uint8))
    hd = t(np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy())
    sd = None if sds is None else t(np.asarray(sds, dtype=np.uint8))
    st = None if status is None else t(np.asarray(status, dtype=np.int32))
    res = torch.full((4096 + 48 * n + 4096,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(itbsplit.split_scratch_bytes(n), 256), dtype=torch.uint8, device=dev)
    itbsplit.split_dev(src, adepth, hd, dst, res[4096: 4096 + 48 * n], scratch, split_depth=sd, status=st)
    torch.cuda.synchronize()
    after, room, results = src.arena.cpu().numpy(), dst.arena.cpu().numpy(), res.cpu().numpy()
    assert (results[:4096] == FILL).all() and (results[4096 + 48 * n:] == FILL).all(), "the results' guards"
    keep, rkeep = after != before, room != FILL
    out = []
    for b in range(n):
        o, k = int(src.host_off[b]), int(dst.host_off[b])
        keep[o: o + len(payloads[b])] = False
        rkeep[k: k + caps[b]] = False
        out.append((results[4096 + 48 * b: 4096 + 48 * (b + 1)].tobytes(), after[o: o + len(payloads[b])].tobytes(),
                    room[k: k + caps[b]].tobytes(), None))
    assert not keep.any(), f"a byte outside the payloads changed, first at {int(np.flatnonzero(keep)[0])}"
    assert not rkeep.any(), f"a byte outside the new payloads' rooms changed, first at {int(np.flatnonzero(rkeep)[0])}"
    return out


def of_records(recs):
    return [C.payload_of(r) for r in recs], [C.hdr_of(r) for r in recs]


def test_dev_random_tables(dev):
    """Random tables at adepth 1, 3, 6 and 10 with depths 0 ... 2, split at
    depth + 1, in one call; then with split_depth NULL, which is the same."""
    recs, adepths, sds = [], [], []
    for adepth, count in ((1, 6), (3, 6), (6, 6), (10, 3)):
        for k in range(count):
            recs.append(S.random_split_table(8000 + 31 * adepth + k, adepth, k % 3).record())
            adepths.append(adepth)
            sds.append(k % 3 + 1)
    payloads, hdrs = of_records(recs)
    want = S.expect(payloads, adepths, hdrs, sds)
    assert sum(w.new_payload is not None for w in want) >= 12 and all(w.fields["err"] == 0 for w in want)
    S.assert_same(split_dev_once(dev, payloads, adepths, hdrs, sds), want, payloads)
    S.assert_same(split_dev_once(dev, payloads, adepths, hdrs, None), want, payloads)
    for b, w in enumerate(want):
        if w.new_payload is not None:
            S.invariants(payloads[b], adepths[b], hdrs[b], sds[b], w)


def test_dev_directed_tables(dev):
    """itb_split_util.directed at adepth 1, 2, 3 and 10 in one call: nothing
    moves, everything moves, one chain with alternating move bits, only the
    head, only the tail, the stale need_rescan, one home slot in N, the
    max_offset-- quirk, sd 1 and 50 with every other bit against them."""
    tables = [(name, rec, sd, adepth) for adepth in (1, 2, 3, 10) for name, rec, sd in S.directed(adepth)]
    names = [t[0] for t in tables]
    payloads, hdrs = of_records([t[1] for t in tables])
    adepths, sds = [t[3] for t in tables], [t[2] for t in tables]
    want = S.expect(payloads, adepths, hdrs, sds)
    S.assert_same(split_dev_once(dev, payloads, adepths, hdrs, sds), want, payloads, names)
    by = dict(zip(names, want))
    assert by["all@10"].fields["old_len"] == C.ITB_SIZE and by["all@10"].fields["moved"] == 1024
    assert by["none@3"].new_payload is None and by["alternate@10"].fields["moved"] == 512
    assert by["maxoff@3"].fields["old_max_offset"] == 6 and by["sd50@10"].fields["moved"] == 512
    assert by["one_home@10"].fields["new_inf"] == 511


def test_dev_error_rules(dev):
    """Decoder codes in status, adepth 0 and 11, n = 11903, a live ITE cut
    short, sd 0 and 51, offsets at residues 1 and 8, new_cap one byte short and
    exact; every damaged table (each of kind_tables() but `valid`, and the
    funnel): POM_SPLIT_E_DAMAGED.  With an error no byte of a payload or of a
    room changes."""
    t = S.random_split_table(9, 3, 0)
    rec = t.record()
    payload, hdr = C.payload_of(rec), C.hdr_of(rec)
    moved = sum(S.moves(h, 1) for h in t.hashes.values())
    assert 0 < moved < len(t.hashes)
    cut = payload[: C.ITE_OFF + C.ITE_SIZE * (max(t.hashes) + 1) - 1]
    need = C.ITE_OFF + 512 * moved
    #        payload, adepth, hdr, sd, status, residue, new_cap, err
    cases = [(payload, 3, hdr, 1, 0, 0, None, 0),
             (payload, 3, hdr, 1, -6, 0, None, -6),
             (payload, 3, hdr, 0, -4, 8, None, -4),
             (payload, 0, hdr, 0, 0, 1, None, C.EINVAL),
             (payload, 11, hdr, 1, 0, 0, None, C.EINVAL),
             (payload[: C.ITE_OFF - 1], 3, hdr, 51, 0, 8, None, C.E_TRUNCATED),
             (cut, 3, hdr, 1, 0, 0, None, C.E_TRUNCATED),
             (payload, 3, hdr, 0, 0, 0, None, C.EINVAL),
             (payload, 3, hdr, 51, 0, 0, None, C.EINVAL),
             (payload, 3, hdr, 1, 0, 1, None, C.EINVAL),
             (payload, 3, hdr, 1, 0, 8, None, C.EINVAL),
             (payload, 3, dict(hdr, entries=hdr["entries"] + 1), 1, 0, 0, None, S.E_DAMAGED),
             (payload, 3, hdr, 1, 0, 0, need - 1, S.E_OUTPUT_OVERRUN),
             (payload, 3, hdr, 1, 0, 0, need, 0)]
    for name, drec, adepth in S.damaged_tables():
        cases.append((C.payload_of(drec), adepth, C.hdr_of(drec), 1, 0, 0, None, S.E_DAMAGED))
    cases.append((C.payload_of(S.damaged_tables()[0][1]), 2, C.hdr_of(S.damaged_tables()[0][1]), 1, 0, 0, 0,
                  S.E_DAMAGED))                                          # damage is found before the capacity
    payloads, adepths, hdrs, sds, status, res, caps, errs = (list(x) for x in zip(*cases))
    caps = [len(p) if c is None else c for p, c in zip(payloads, caps)]
    # (guarded_batch puts block b at residue res[b]: the offsets the oracle sees)
    want = S.expect(payloads, adepths, hdrs, sds, res, res, caps, status)
    assert [w.fields["err"] for w in want] == errs
    assert want[12].fields["moved"] == moved and all(w.fields["moved"] == 0 for w in want[1:12])
    got = split_dev_once(dev, payloads, adepths, hdrs, sds, caps, status, res)
    S.assert_same(got, want, payloads)
    assert got[0][1] != payload and got[13][0] == got[0][0]


GRID_MAX = 4096                 # itb_split.hip kSplitGridMax: above it a workgroup takes ITB b, b + 4096, ...


def test_dev_many_itbs_reuse_the_workgroup(dev):
    """2 * 4096 + 37 ITBs of 8 kinds, each ITB with its own copy of its kind's
    payload (the split writes in place), so that every workgroup splits two or
    three ITBs in the LDS it never clears as a whole: a full overflow half
    before a table with one chain, an error's early end before and after a
    split, nothing moved before everything moved.  Every ordered pair of the 8
    kinds, equal pairs included, meets in one workgroup."""
    n = 2 * GRID_MAX + 37
    with open(os.path.join(ROOT, "pomegranate_amd", "csrc", "itb_split.hip")) as f:
        assert re.search(r"kSplitGridMax = (\d+);", f.read()).group(1) == str(GRID_MAX)
    t3 = S.random_split_table(9, 3, 0)
    p3 = C.payload_of(t3.record())
    dup = C.kind_tables()["dup"][0]
    # adepth 10 with few ITEs: 2048 slots and 1024 bits of LDS in play, 16 KB of payload
    collide = S._built(10, 31, [(5 + 512 * (i % 2)) | (i // 2 % 2) << 10 | i << 20 for i in range(8)]).record()
    stay = S._built(10, 32, [i * 100 | i << 20 for i in range(8)]).record()
    #            record, adepth, sd, status
    kinds = [(collide, 10, 1, 0),
             (stay, 10, 1, 0),
             (S.directed(1)[1][1], 1, 1, 0),                            # all@1
             (t3.record(), 3, 1, 0),
             (dup, 2, 1, 0),
             (t3.record(), 3, 1, -6),
             (None, 3, 1, 0),                                           # a live ITE cut short
             (S.directed(5)[2][1], 5, 1, 0)]                            # alternate@5
    assert S.directed(1)[1][0] == "all@1" and S.directed(5)[2][0] == "alternate@5"
    payloads8 = [p3[: C.ITE_OFF + C.ITE_SIZE * (max(t3.hashes) + 1) - 1] if k[0] is None else C.payload_of(k[0])
                 for k in kinds]
    hdr8 = [C.hdr_of(t3.record() if k[0] is None else k[0]) for k in kinds]
    one = S.expect(payloads8, [k[1] for k in kinds], hdr8, [k[2] for k in kinds], status=[k[3] for k in kinds])
    assert [w.fields["err"] for w in one] == [0, 0, 0, 0, S.E_DAMAGED, -6, C.E_TRUNCATED, 0]
    assert [w.fields["moved"] for w in one] == [4, 0, 2, one[3].fields["moved"], 0, 0, 0, 16] and one[3].fields["moved"]

    def kind(b):
        return b % 8 if b < GRID_MAX else (b - GRID_MAX) // 8 % 8 if b < 2 * GRID_MAX else (b + 3) % 8
    which = [kind(b) for b in range(n)]
    # workgroup g takes ITBs g, g + 4096 (and g + 8192): every ordered pair of kinds follows one another
    assert {(kind(g), kind(g + GRID_MAX)) for g in range(GRID_MAX)} == {(i, j) for i in range(8) for j in range(8)}
    payloads = [payloads8[k] for k in which]
    got = split_dev_once(dev, payloads, [kinds[k][1] for k in which], [hdr8[k] for k in which],
                         [kinds[k][2] for k in which], status=[kinds[k][3] for k in which])
    S.assert_same(got, [one[k] for k in which], payloads)


def test_dev_refuses_what_it_cannot_run(dev):
    """hdr is required, both arenas are 16-byte aligned, the scratch has its
    size: refused before anything is queued."""
    rec = S.directed(2)[1][1]
    payloads, hdrs = of_records([rec])
    src = guarded_batch(torch, [bytes(payloads[0])], dev, [0], fill=FILL_SRC)
    dst = guarded_batch(torch, [len(payloads[0])], dev, [0], fill=FILL)
    adepth = torch.tensor([2], dtype=torch.uint8, device=dev)
    hd = torch.from_numpy(np.frombuffer(C.hdr_bytes(hdrs[0]), dtype=np.uint8).copy()).to(dev)
    res = torch.full((48,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(itbsplit.split_scratch_bytes(1), dtype=torch.uint8, device=dev)
    skewed = lzo.DeviceBatch(dst.arena[8:], dst.off, dst.length)
    with pytest.raises(ValueError):
        itbsplit.split_dev(src, adepth, hd, skewed, res, scratch)
    with pytest.raises(ValueError):
        itbsplit.split_dev(src, adepth, hd, dst, res, scratch[:16])
    with pytest.raises(ValueError):
        itbsplit.split_dev(src, adepth, hd[:8], dst, res, scratch)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == FILL).all() and (dst.arena.cpu().numpy() == FILL).all()
    itbsplit.split_dev(src, adepth, hd, dst, res, scratch)
    torch.cuda.synchronize()
    assert itbsplit.Result.parse(res.cpu().numpy().tobytes()).moved == 4


# ---------------------------------------------------------------------------
# pom_itb_split_batch against the oracle
# ---------------------------------------------------------------------------
import ctypes  # noqa: E402
import struct  # noqa: E402

from pomegranate_amd import check, itb  # noqa: E402

H = itb.ITBH_SIZE


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


def expect_batch(oracle, stored, recs, sds=None, codes=None, out_cap=None):
    """The oracle over stored records whose uncompressed records are `recs`
    (None: a record the header checks refuse); codes: {b: the decoder's code}.
    -> (err [n], results [n] bytes, old records, new records)"""
    n = len(stored)
    err, res, olds, news = [C.EINVAL] * n, [bytes(48)] * n, [b""] * n, [b""] * n
    for b, (st, rec) in enumerate(zip(stored, recs)):
        if rec is None:
            continue
        if codes and b in codes:
            err[b], res[b] = codes[b], S._only(codes[b])
            continue
        hdr = C.hdr_of(st)
        sd = hdr["depth"] + 1 if sds is None else sds[b]
        w = S.expect_one(C.payload_of(rec), st[S.ITBH_ADEPTH], hdr, sd)
        err[b], res[b] = w.fields["err"], w.result
        if w.new_payload is not None:
            o, nw = S.stored_records(oracle, st[:H], sd, w)
            if out_cap is not None and max(len(o), len(nw)) > out_cap[b]:
                err[b] = S.E_OUTPUT_OVERRUN
            else:
                olds[b], news[b] = o, nw
    return err, res, olds, news


def same_batch(got, want, what=""):
    err, res, olds, news = want
    assert got.err.tolist() == err, what
    for b in range(len(err)):
        assert got.result[b].tobytes() == res[b], f"{what}ITB {b}: {got.result[b]} != {S.result_fields(res[b])}"
        assert got.old[b] == olds[b], f"{what}ITB {b}: the old record"
        assert got.new[b] == news[b], f"{what}ITB {b}: the new record"


def store(oracle, rec, lzo_form):
    return bytes(C.lzo_record(oracle, rec)) if lzo_form else bytes(rec)


@pytest.fixture(scope="module")
def mixed(oracle):
    """Random tables at adepth 1, 3, 6 and 10, some directed ones, a table whose
    old half does not compress,
    a damaged table, LZO and stored alternately; records the header checks
    refuse and a stream cut short.  -> (stored, uncompressed records or None,
    {b: decoder code})"""
    recs = []
    for adepth, count in ((1, 3), (3, 4), (6, 3), (10, 2)):
        recs += [S.random_split_table(9000 + 31 * adepth + k, adepth, k % 3).record() for k in range(count)]
    recs += [rec for name, rec, sd in S.directed(3) if sd == 1] + [S.directed(10)[2][1]]
    # nothing of it compresses: 1000 ITEs at adepth 10 of which one moves, a random lock region, and random
    # stale bits in the index (a FREE slot's entry and conflict, a UNIQUE slot's conflict: never examined)
    dense = S._built(10, 77, [i | (i == 5) << 10 | i << 20 for i in range(1000)])
    rng = np.random.default_rng(5)
    dense.rec[H: H + C.BITMAP_OFF] = rng.integers(0, 256, C.BITMAP_OFF, dtype=np.uint8).tobytes()
    for slot in range(C.INDEX_ENTRIES):
        entry, _, flag = C.get_slot(dense.rec, H, slot)
        if flag in (C.IDX_FREE, C.IDX_UNIQUE):
            C.set_slot(dense.rec, H, slot, entry if flag else int(rng.integers(0, 32768)),
                       int(rng.integers(0, 32768)), flag)
    recs.append(dense.record())
    recs.append(C.kind_tables()["dup"][0])
    stored = [store(oracle, r, b % 3 != 1) for b, r in enumerate(recs)]
    bad_adepth, bad_algo, short = bytearray(recs[0]), bytearray(recs[1]), bytearray(recs[2][:200])
    bad_adepth[3] = 11
    struct.pack_into("<H", bad_algo, itb.ALGO_OFF, 7)
    src = C.lzo_record(oracle, recs[4])
    ln, zlen, _ = itb.header_fields(src)
    cut = bytearray(src[: ln - 9])
    struct.pack_into("<I", cut, itb.LEN_OFF, ln - 9)
    rc, _ = oracle.decompress_safe(bytes(cut[H:]), zlen - H)
    assert rc != 0
    extra = [(bytes(bad_adepth), None), (bytes(bad_algo), None), (bytes(short), None), (bytes(cut), recs[4])]
    stored = stored[:5] + [e[0] for e in extra] + stored[5:]
    recs = recs[:5] + [e[1] for e in extra] + recs[5:]
    return stored, recs, {8: rc}


def test_batch_mixed(oracle, mixed):
    """Both outputs equal the records itb_lzo_compress would store, byte for
    byte, in caller order; feeding both outputs to pom_itb_check_batch with
    POM_CK_ITBID gives no finding, kind 15 included."""
    stored, recs, codes = mixed
    want = expect_batch(oracle, stored, recs, None, codes)
    got = itbsplit.split_batch(stored)
    same_batch(got, want)
    produced = [b for b in range(len(stored)) if want[2][b]]
    assert len(produced) >= 12 and want[0][5:9] == [C.EINVAL] * 3 + [codes[8]] and want[0][-1] == S.E_DAMAGED
    algos = {(struct.unpack_from("<H", want[2][b], itb.ALGO_OFF)[0], struct.unpack_from("<H", want[3][b], itb.ALGO_OFF)[0])
             for b in produced}
    assert (0, 1) in algos and (1, 1) in algos                          # an old half that did not compress, too
    assert got.len_ok.tolist() == [int(r is not None and b != 8) for b, r in enumerate(recs)]
    halves = [got.old[b] for b in produced] + [got.new[b] for b in produced]
    again = check.check_batch(halves, check.CK_ITBID)
    assert not again.err.any() and not again.report["findings"].any() and again.len_ok.all()
    assert len(itbsplit.split_batch([]).err) == 0


@pytest.fixture(scope="module")
def chunky(oracle):
    """48 adepth-8 tables of about 60 KB, every fourth stored uncompressed:
    several chunks under chunk_mb=1."""
    recs = [S.random_split_table(4000 + b, 8, b % 2).record() for b in range(48)]
    stored = [store(oracle, r, b % 4 != 1) for b, r in enumerate(recs)]
    return stored, expect_batch(oracle, stored, recs)


def test_batch_spans_chunks(chunky, debug_env, monkeypatch):
    """chunk_mb=1: several chunks, on every visible GPU and on one; results in
    caller order."""
    stored, want = chunky
    debug_env("chunk_mb=1")
    same_batch(itbsplit.split_batch(stored), want, "all GPUs: ")
    monkeypatch.setenv("POM_LZO_DEVICES", "0")
    same_batch(itbsplit.split_batch(stored), want, "one GPU: ")
    assert sum(1 for o in want[2] if o) >= 40


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the call returns LZO_E_ERROR; a lost ITB reads LZO_E_ERROR
    with a zeroed result, zero lengths and untouched buffers, the rest are
    right, and both kinds occur; a clean rerun is right."""
    stored, want = chunky
    n = len(stored)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    caps = [max(itb.header_fields(r)[0], itb.header_fields(r)[1]) for r in stored]
    olds = [np.full(c, 7, np.uint8) for c in caps]
    news = [np.full(c, 7, np.uint8) for c in caps]
    arr = lambda items: (ctypes.c_void_p * n)(*[b.ctypes.data for b in items])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    ccap = (ctypes.c_size_t * n)(*caps)
    ol, nl = (ctypes.c_size_t * n)(*([7] * n)), (ctypes.c_size_t * n)(*([7] * n))
    result = np.full(n, 7, dtype=np.uint8).repeat(48).view(itbsplit.RESULT_DTYPE)
    err, ok = np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    debug_env("chunk_mb=1,fail_chunk=1")
    rc = itbsplit._lib().pom_itb_split_batch(arr(bufs), lens, n, None, arr(olds), arr(news), ccap, ol, nl,
                                             result.ctypes.data, err.ctypes.data, ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    lost = err == lzo.LZO_E_ERROR
    assert 0 < lost.sum() < n
    for b in range(n):
        if lost[b]:
            assert result[b].tobytes() == bytes(48) and (ol[b], nl[b], ok[b]) == (0, 0, 0)
            assert (olds[b] == 7).all() and (news[b] == 7).all()
        else:
            assert err[b] == want[0][b] and result[b].tobytes() == want[1][b] and ok[b] == 1
            assert olds[b][: ol[b]].tobytes() == want[2][b] and news[b][: nl[b]].tobytes() == want[3][b]
            assert (olds[b][ol[b]:] == 7).all() and (news[b][nl[b]:] == 7).all()
    debug_env("chunk_mb=1")
    same_batch(itbsplit.split_batch(stored), want)


def test_batch_out_cap_exact_and_one_short(oracle, mixed):
    """A capacity equal to the longer of the two records suffices; one byte
    less is LZO_E_OUTPUT_OVERRUN with neither buffer written."""
    stored, recs, codes = mixed
    full = expect_batch(oracle, stored, recs, None, codes)
    exact = [max(len(full[2][b]), len(full[3][b]), 1) for b in range(len(stored))]
    same_batch(itbsplit.split_batch(stored, out_cap=exact), full, "exact: ")
    short = [c - 1 if full[2][b] and b % 2 == 0 else c for b, c in enumerate(exact)]
    want = expect_batch(oracle, stored, recs, None, codes, out_cap=short)
    assert want[0].count(S.E_OUTPUT_OVERRUN) >= 5
    same_batch(itbsplit.split_batch(stored, out_cap=short), want, "one short: ")
