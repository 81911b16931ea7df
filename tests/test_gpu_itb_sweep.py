"""GPU: the ITB sweep (include/pom_sweep.h) against the Python restatement of
the reference's loop in itb_sweep_util.py -- pom_itb_sweep_dev on guarded
arenas filled with a constant, then pom_itb_sweep_batch.  Everything is
compared with the oracle: the result, the payload, and every byte that must
not change (a payload outside its bitmap and index, the guards around every
payload and the results)."""
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
from conftest import ROOT
from gpu_util import guarded_batch
from pomegranate_amd import check, itb, itbsweep, lzo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL_SRC, FILL = 0xEE, 0x5A
H = itb.ITBH_SIZE


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def sweep_dev_once(dev, payloads, adepths, hdrs, budgets=None, status=None, shifts=None):
    """One call over a guarded batch: payload b at residue shifts[b] mod 16
    (default 0).  -> [(result, the payload after, None)], after checking every
    guard."""
    n = len(payloads)
    shifts = [0] * n if shifts is None else list(shifts)
    src = guarded_batch(torch, [bytes(p) for p in payloads], dev, shifts, fill=FILL_SRC)
    before = src.arena.cpu().numpy()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    adepth = t(np.asarray(adepths, dtype=np.uint8))
    hd = t(np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy())
    bud = None if budgets is None else t(np.asarray([W.NO_BUDGET if x is None else x for x in budgets],
                                                    dtype=np.uint32).view(np.int32))
    st = None if status is None else t(np.asarray(status, dtype=np.int32))
    res = torch.full((4096 + 32 * n + 4096,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(itbsweep.sweep_scratch_bytes(n), 256), dtype=torch.uint8, device=dev)
    itbsweep.sweep_dev(src, adepth, hd, res[4096: 4096 + 32 * n], scratch, budget=bud, status=st)
    torch.cuda.synchronize()
    after, results = src.arena.cpu().numpy(), res.cpu().numpy()
    assert (results[:4096] == FILL).all() and (results[4096 + 32 * n:] == FILL).all(), "the results' guards"
    keep = after != before
    out = []
    for b in range(n):
        o = int(src.host_off[b])
        keep[o + C.BITMAP_OFF: o + min(C.ITE_OFF, len(payloads[b]))] = False
        out.append((results[4096 + 32 * b: 4096 + 32 * (b + 1)].tobytes(), after[o: o + len(payloads[b])].tobytes(), None))
    assert not keep.any(), \
        f"a byte outside the payloads' bitmaps and index tables changed, first at {int(np.flatnonzero(keep)[0])}"
    return out


def of_records(recs):
    return [C.payload_of(r) for r in recs], [C.hdr_of(r) for r in recs]


def test_dev_directed_tables(dev):
    """The directed chains, the max_offset tables and the budget table at each
    of its budgets, in one launch with a budget per ITB; the chains again with
    budget NULL."""
    chains, mo = W.directed_chains(), W.max_offset_tables()
    brec = W.budget_table().record()
    budgets = [0, 1, 2, 3, 4, 5, 6, None]
    recs = [c[1] for c in chains] + [m[1] for m in mo] + [brec] * len(budgets)
    adepths = [c[2] for c in chains] + [m[2] for m in mo] + [4] * len(budgets)
    names = [c[0] for c in chains] + [m[0] for m in mo] + [f"budget {x}" for x in budgets]
    buds = [None] * (len(chains) + len(mo)) + budgets
    payloads, hdrs = of_records(recs)
    want = W.expect(payloads, adepths, hdrs, buds)
    W.assert_same(sweep_dev_once(dev, payloads, adepths, hdrs, buds), want, payloads, names)
    by = dict(zip(names, want))
    assert by["ULUL@10high"].fields["dc"] == 3 and by["UUUU@2all"].fields["len"] == C.ITB_SIZE
    assert by["highest_last"].fields["max_offset"] == 4 and by["budget 3"].fields["visited"] == 4
    k = len(chains)
    W.assert_same(sweep_dev_once(dev, payloads[:k], adepths[:k], hdrs[:k], None), want[:k], payloads[:k], names[:k])


@pytest.fixture(scope="module")
def random_tables():
    """About 200 random tables over all ten adepths, marked at fractions 0,
    0.1, 0.5, 0.9 and 1; every third one has a budget."""
    fractions = (0.0, 0.1, 0.5, 0.9, 1.0)
    recs, adepths, budgets = [], [], []
    rng = np.random.default_rng(77)
    for adepth, count in ((1, 20), (2, 25), (3, 30), (4, 30), (5, 30), (6, 25), (7, 15), (8, 10), (9, 10), (10, 5)):
        for k in range(count):
            recs.append(W.random_sweep_table(8000 + 31 * adepth + k, adepth, fractions[k % 5]).record())
            adepths.append(adepth)
            budgets.append(int(rng.integers(0, 1 << adepth)) if k % 3 == 2 else None)
    payloads, hdrs = of_records(recs)
    return payloads, adepths, hdrs, budgets, W.expect(payloads, adepths, hdrs, budgets)


def test_dev_random_tables(dev, random_tables):
    payloads, adepths, hdrs, budgets, want = random_tables
    assert len(payloads) == 200 and sum(w.produced for w in want) >= 120 and all(w.fields["err"] == 0 for w in want)
    assert sum(w.fields["visited"] < 1 << a for w, a in zip(want, adepths) if w.produced) >= 15
    W.assert_same(sweep_dev_once(dev, payloads, adepths, hdrs, budgets), want, payloads)
    for b, w in enumerate(want):
        if w.produced:
            W.invariants(payloads[b], adepths[b], hdrs[b], w)


def test_dev_error_rules(dev):
    """Decoder codes in status, adepth 0 and 11, n = 11903, a live ITE cut
    short, offsets at residues 1 and 8, every damaged table (each of
    kind_tables() but `valid`, and the funnel) with every ITE marked, a table
    with nothing marked, between tables that sweep: one launch, mixed."""
    t = W.random_sweep_table(9, 3, 0.5)
    rec = t.record()
    payload, hdr = C.payload_of(rec), C.hdr_of(rec)
    cut = payload[: C.ITE_OFF + C.ITE_SIZE * (max(t.hashes) + 1) - 1]
    clean = C.payload_of(W.random_sweep_table(9, 3, 0.0).record())
    #        payload, adepth, hdr, status, residue, err
    cases = [(payload, 3, hdr, 0, 0, 0),
             (payload, 3, hdr, -6, 0, -6),
             (payload, 0, hdr, -4, 8, -4),
             (payload, 0, hdr, 0, 1, C.EINVAL),
             (payload, 11, hdr, 0, 0, C.EINVAL),
             (payload[: C.ITE_OFF - 1], 3, hdr, 0, 8, C.E_TRUNCATED),
             (cut, 3, hdr, 0, 0, C.E_TRUNCATED),
             (payload, 3, hdr, 0, 1, C.EINVAL),
             (payload, 3, hdr, 0, 8, C.EINVAL),
             (payload, 3, dict(hdr, entries=hdr["entries"] + 1), 0, 0, W.E_DAMAGED),
             (clean, 3, hdr, 0, 0, 0)]
    for name, drec, adepth in W.damaged_tables():
        drec = bytearray(drec)
        for nr in range(min(1 << adepth, (len(drec) - C.ITB_SIZE) // C.ITE_SIZE)):
            W.set_state(drec, nr, W.UNLINKED)
        cases.append((C.payload_of(drec), adepth, C.hdr_of(drec), 0, 0, W.E_DAMAGED))
    cases.append((payload, 3, hdr, 0, 0, 0))
    payloads, adepths, hdrs, status, res, errs = (list(x) for x in zip(*cases))
    # (guarded_batch puts block b at residue res[b]: the offsets the oracle sees)
    want = W.expect(payloads, adepths, hdrs, None, res, status)
    assert [w.fields["err"] for w in want] == errs
    assert want[0].produced and want[-1].produced and not any(w.produced for w in want[1:-1])
    got = sweep_dev_once(dev, payloads, adepths, hdrs, None, status, res)
    W.assert_same(got, want, payloads)
    assert got[0][1] != payload and got[-1][0] == got[0][0]


GRID_MAX = 4096                 # itb_sweep.hip kSweepGridMax: above it a workgroup takes ITB b, b + 4096, ...


def test_dev_many_itbs_reuse_the_workgroup(dev):
    """4096 + 130 ITBs at adepth 1 (and a few wider kinds among them), each
    with its own copy of its kind's payload, so that 130 workgroups sweep two
    ITBs in the LDS they never clear as a whole: a swept table before an
    error's early end, before nothing marked, before another sweep."""
    n = GRID_MAX + 130
    with open(os.path.join(ROOT, "pomegranate_amd", "csrc", "itb_sweep.hip")) as f:
        assert re.search(r"kSweepGridMax = (\d+);", f.read()).group(1) == str(GRID_MAX)
    t3 = W.random_sweep_table(9, 3, 0.5)
    #            record, adepth, budget, status
    kinds = [(W.chain_table(1, "low", "UL").record(), 1, None, 0),
             (W.chain_table(1, "high", "UU").record(), 1, None, 0),
             (W.chain_table(1, "low", "L").record(), 1, None, 0),
             (W.chain_table(1, "low", "LU").record(), 1, 0, 0),
             (C.kind_tables(1)["dup"][0], 1, None, 0),
             (W.chain_table(1, "low", "U").record(), 1, None, -6),
             (t3.record(), 3, None, 0),
             (W.chain_table(10, "low", "ULUL").record(), 10, None, 0)]
    payloads8, hdr8 = of_records([k[0] for k in kinds])
    one = W.expect(payloads8, [k[1] for k in kinds], hdr8, [k[2] for k in kinds], status=[k[3] for k in kinds])
    assert [w.fields["err"] for w in one] == [0, 0, 0, 0, W.E_DAMAGED, -6, 0, 0]
    assert [w.fields["removed"] for w in one] == [1, 2, 0, 1, 0, 0, one[6].fields["removed"], 2] and one[6].produced

    def kind(b):
        return b % 8 if b < GRID_MAX else (b - GRID_MAX) // 8 % 8 if b < GRID_MAX + 64 else (b + 3) % 8
    which = [kind(b) for b in range(n)]
    # workgroup g takes ITBs g and g + 4096: every ordered pair of kinds follows one another
    assert {(kind(g), kind(g + GRID_MAX)) for g in range(64)} == {(i, j) for i in range(8) for j in range(8)}
    payloads = [payloads8[k] for k in which]
    got = sweep_dev_once(dev, payloads, [kinds[k][1] for k in which], [hdr8[k] for k in which],
                         [kinds[k][2] for k in which], status=[kinds[k][3] for k in which])
    W.assert_same(got, [one[k] for k in which], payloads)


def test_dev_refuses_what_it_cannot_run(dev):
    """hdr is required, the arena is 16-byte aligned, the scratch has its
    size: refused before anything is queued."""
    rec = W.chain_table(2, "low", "ULUL").record()
    payloads, hdrs = of_records([rec])
    src = guarded_batch(torch, [bytes(payloads[0])], dev, [0], fill=FILL_SRC)
    before = src.arena.cpu().numpy()
    adepth = torch.tensor([2], dtype=torch.uint8, device=dev)
    hd = torch.from_numpy(np.frombuffer(C.hdr_bytes(hdrs[0]), dtype=np.uint8).copy()).to(dev)
    res = torch.full((32,), FILL, dtype=torch.uint8, device=dev)
    scratch = torch.empty(itbsweep.sweep_scratch_bytes(1), dtype=torch.uint8, device=dev)
    skewed = lzo.DeviceBatch(src.arena[8:], src.off, src.length)
    with pytest.raises(ValueError):
        itbsweep.sweep_dev(skewed, adepth, hd, res, scratch)
    with pytest.raises(ValueError):
        itbsweep.sweep_dev(src, adepth, hd, res, scratch[:16])
    with pytest.raises(ValueError):
        itbsweep.sweep_dev(src, adepth, hd[:8], res, scratch)
    torch.cuda.synchronize()
    assert (res.cpu().numpy() == FILL).all() and (src.arena.cpu().numpy() == before).all()
    itbsweep.sweep_dev(src, adepth, hd, res, scratch)
    torch.cuda.synchronize()
    r = itbsweep.Result.parse(res.cpu().numpy().tobytes())
    assert (r.removed, r.dc, r.visited) == (2, 3, 4)


# ---------------------------------------------------------------------------
# pom_itb_sweep_batch against the oracle
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


def expect_batch(oracle, stored, recs, budgets=None, codes=None, out_cap=None):
    """The oracle over stored records whose uncompressed records are `recs`
    (None: a record the header checks refuse); codes: {b: the decoder's code}.
    -> (err [n], results [n] bytes, swept records)"""
    n = len(stored)
    err, res, outs = [C.EINVAL] * n, [bytes(32)] * n, [b""] * n
    for b, (st, rec) in enumerate(zip(stored, recs)):
        if rec is None:
            continue
        if codes and b in codes:
            err[b], res[b] = codes[b], W._only(codes[b])
            continue
        w = W.expect_one(C.payload_of(rec), st[S.ITBH_ADEPTH], C.hdr_of(st), None if budgets is None else budgets[b])
        err[b], res[b] = w.fields["err"], w.result
        if w.produced:
            o = W.stored_record(oracle, st[:H], w)
            if out_cap is not None and len(o) > out_cap[b]:
                err[b] = W.E_OUTPUT_OVERRUN
            else:
                outs[b] = o
    return err, res, outs


def same_batch(got, want, what=""):
    err, res, outs = want
    assert got.err.tolist() == err, what
    for b in range(len(err)):
        assert got.result[b].tobytes() == res[b], f"{what}ITB {b}: {got.result[b]} != {W.result_fields(res[b])}"
        assert got.out[b] == outs[b], f"{what}ITB {b}: the record"


def store(oracle, rec, lzo_form):
    return bytes(C.lzo_record(oracle, rec)) if lzo_form else bytes(rec)


@pytest.fixture(scope="module")
def mixed(oracle):
    """Random tables at adepth 1, 3, 6 and 10 at every mark fraction, the
    max_offset tables (one swept empty), a table whose swept payload does not
    compress, a damaged table, LZO and stored alternately; records the header
    checks refuse and a stream cut short.  -> (stored, uncompressed records or
    None, {b: decoder code})"""
    fractions = (0.5, 0.0, 1.0, 0.1, 0.9)
    recs = []
    for adepth, count in ((1, 3), (3, 5), (6, 5), (10, 2)):
        recs += [W.random_sweep_table(9000 + 31 * adepth + k, adepth, fractions[k % 5]).record() for k in range(count)]
    recs += [m[1] for m in W.max_offset_tables()]
    # nothing of it compresses: 1000 ITEs at adepth 10 of which one is marked, a random lock region, and random
    # stale bits in the index (a FREE slot's entry and conflict, a UNIQUE slot's conflict: never examined)
    dense = W.with_states(S._built(10, 77, [i | i << 20 for i in range(1000)]), {5: W.UNLINKED})
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
    """Every output equals the record itb_lzo_compress would store, byte for
    byte, in caller order; removed == 0 leaves out_len 0; feeding the outputs
    to pom_itb_check_batch gives no finding; sweeping them again removes
    nothing."""
    stored, recs, codes = mixed
    want = expect_batch(oracle, stored, recs, None, codes)
    got = itbsweep.sweep_batch(stored)
    same_batch(got, want)
    produced = [b for b in range(len(stored)) if want[2][b]]
    assert len(produced) >= 12 and want[0][5:9] == [C.EINVAL] * 3 + [codes[8]] and want[0][-1] == W.E_DAMAGED
    unmarked = [b for b in range(len(stored)) if want[0][b] == 0 and not want[2][b]]
    assert len(unmarked) >= 3 and all(want[1][b] == bytes(32) for b in unmarked)
    algos = {struct.unpack_from("<H", want[2][b], itb.ALGO_OFF)[0] for b in produced}
    assert algos == {0, 1}                                              # a swept payload that did not compress, too
    ulens = [f[1] if f[2] == 1 else f[0] for f in (itb.header_fields(want[2][b]) for b in produced)]
    assert C.ITB_SIZE in ulens                                          # a record swept empty
    assert got.len_ok.tolist() == [int(r is not None and b != 8) for b, r in enumerate(recs)]
    outs = [got.out[b] for b in produced]
    again = check.check_batch(outs, 0)
    assert not again.err.any() and not again.report["findings"].any() and again.len_ok.all()
    twice = itbsweep.sweep_batch(outs)
    assert not twice.err.any() and not twice.result["removed"].any() and twice.out == [b""] * len(outs)
    assert len(itbsweep.sweep_batch([]).err) == 0


def test_batch_budget(oracle, mixed):
    """A budget per record reaches the kernel in caller order."""
    stored, recs, codes = mixed
    budgets = [(0, 1, 3, W.NO_BUDGET)[b % 4] for b in range(len(stored))]
    want = expect_batch(oracle, stored, recs, [None if x == W.NO_BUDGET else x for x in budgets], codes)
    assert want != expect_batch(oracle, stored, recs, None, codes)
    same_batch(itbsweep.sweep_batch(stored, budget=budgets), want)


@pytest.fixture(scope="module")
def chunky(oracle):
    """48 adepth-8 tables of about 60 KB, every fourth stored uncompressed:
    several chunks under chunk_mb=1."""
    recs = [W.random_sweep_table(4000 + b, 8, (0.5, 0.1, 1.0)[b % 3]).record() for b in range(48)]
    stored = [store(oracle, r, b % 4 != 1) for b, r in enumerate(recs)]
    return stored, expect_batch(oracle, stored, recs)


def test_batch_spans_chunks(chunky, debug_env, monkeypatch):
    """chunk_mb=1: several chunks, on every visible GPU and on one; results in
    caller order."""
    stored, want = chunky
    debug_env("chunk_mb=1")
    same_batch(itbsweep.sweep_batch(stored), want, "all GPUs: ")
    monkeypatch.setenv("POM_LZO_DEVICES", "0")
    same_batch(itbsweep.sweep_batch(stored), want, "one GPU: ")
    assert sum(1 for o in want[2] if o) >= 40


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the call returns LZO_E_ERROR; a lost ITB reads LZO_E_ERROR
    with a zeroed result, a zero length and an untouched buffer, the rest are
    right, and both kinds occur; a clean rerun is right."""
    stored, want = chunky
    n = len(stored)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    caps = [max(itb.header_fields(r)[0], itb.header_fields(r)[1]) for r in stored]
    outs = [np.full(c, 7, np.uint8) for c in caps]
    arr = lambda items: (ctypes.c_void_p * n)(*[b.ctypes.data for b in items])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    ccap = (ctypes.c_size_t * n)(*caps)
    ol = (ctypes.c_size_t * n)(*([7] * n))
    result = np.full(n, 7, dtype=np.uint8).repeat(32).view(itbsweep.RESULT_DTYPE)
    err, ok = np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    debug_env("chunk_mb=1,fail_chunk=1")
    rc = itbsweep._lib().pom_itb_sweep_batch(arr(bufs), lens, n, None, arr(outs), ccap, ol, result.ctypes.data,
                                             err.ctypes.data, ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    lost = err == lzo.LZO_E_ERROR
    assert 0 < lost.sum() < n
    for b in range(n):
        if lost[b]:
            assert result[b].tobytes() == bytes(32) and (ol[b], ok[b]) == (0, 0) and (outs[b] == 7).all()
        else:
            assert err[b] == want[0][b] and result[b].tobytes() == want[1][b] and ok[b] == 1
            assert outs[b][: ol[b]].tobytes() == want[2][b] and (outs[b][ol[b]:] == 7).all()
    debug_env("chunk_mb=1")
    same_batch(itbsweep.sweep_batch(stored), want)


def test_batch_out_cap_exact_and_one_short(oracle, mixed):
    """A capacity equal to the record's length suffices; one byte less is
    LZO_E_OUTPUT_OVERRUN with the buffer not written."""
    stored, recs, codes = mixed
    full = expect_batch(oracle, stored, recs, None, codes)
    exact = [max(len(full[2][b]), 1) for b in range(len(stored))]
    same_batch(itbsweep.sweep_batch(stored, out_cap=exact), full, "exact: ")
    short = [c - 1 if full[2][b] and b % 2 == 0 else c for b, c in enumerate(exact)]
    want = expect_batch(oracle, stored, recs, None, codes, out_cap=short)
    assert want[0].count(W.E_OUTPUT_OVERRUN) >= 5
    same_batch(itbsweep.sweep_batch(stored, out_cap=short), want, "one short: ")
