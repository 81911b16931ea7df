"""GPU: the ITB check (include/pom_check.h) against the Python restatement of
its rules in check_util.py -- pom_itb_check_dev on one guarded arena,
pom_itb_check_batch through the host chunk pipeline.  err, all 48 bytes of
every report and both masks are compared; the directed tables
(check_util.directed) also carry closed-form answers."""
from __future__ import annotations

import ctypes
import os
import re
import struct

import numpy as np
import pytest

import check_util as C
from conftest import ROOT
from gpu_util import guarded_batch
from pomegranate_amd import check, itb, lzo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H = itb.ITBH_SIZE
FILL = 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


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


@pytest.fixture(scope="module")
def tables():
    """The CPU test's families in small, once: valid tables at adepth 1, 3 and
    10, a hand-made table per kind, the funnel and 64 fuzzed tables, with the
    oracle's answers for (hdr, POM_CK_ITBID), (hdr, no flag) and (no hdr).
    -> (records, adepths, hdrs, {key: want})"""
    recs, adepths = [], []
    for adepth, steps in ((1, 30), (3, 60), (10, 700)):
        recs.append(C.random_table(50 + adepth, adepth, steps, depth=2, itbid=3).record())
        adepths.append(adepth)
    for rec, _, _, _ in C.kind_tables().values():
        recs.append(rec)
        adepths.append(2)
    recs.append(C.funnel())
    adepths.append(10)
    for seed in range(64):
        rec, adepth = C.fuzzed(1000 + seed)
        recs.append(rec)
        adepths.append(adepth)
    payloads = [C.payload_of(r) for r in recs]
    hdrs = [C.hdr_of(r) for r in recs]
    want = {("hdr", C.CK_ITBID): C.expect(payloads, adepths, hdrs, C.CK_ITBID),
            ("hdr", 0): C.expect(payloads, adepths, hdrs, 0),
            (None, C.CK_ITBID): C.expect(payloads, adepths, None, C.CK_ITBID)}
    return recs, adepths, hdrs, want


def same(got, want):
    for g, w, name in zip(got, want, ("err", "report", "slot_mask", "ite_mask")):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        if len(bad):
            b = int(bad[0])
            detail = f"{C.report_fields(g[b])} != {C.report_fields(w[b])}" if name == "report" else f"{g[b]} != {w[b]}"
            raise AssertionError(f"{name}: ITB {b}: {detail}")


# ---------------------------------------------------------------------------
# pom_itb_check_dev on one guarded arena
# ---------------------------------------------------------------------------
class Outputs:
    """err, the reports and the masks carved out of ONE arena of FILL bytes
    with guard bytes around each, so a stray store shows; a mask the call does
    not get keeps its FILL."""

    def __init__(self, dev, n):
        self.n = n
        self.sizes = [("err", 4 * n), ("report", 48 * n), ("slot_mask", 256 * n), ("ite_mask", 128 * n)]
        self.at, pos = {}, 4096
        for name, nbytes in self.sizes:
            self.at[name] = (pos, nbytes)
            pos = (pos + nbytes + 4096 + 255) // 256 * 256
        self.arena = torch.full((pos,), FILL, dtype=torch.uint8, device=dev)
        assert self.arena.data_ptr() % 256 == 0

    def view(self, name, dtype=torch.uint8):
        o, nbytes = self.at[name]
        return self.arena[o: o + nbytes].view(dtype)

    def results(self, masks):
        """(err, reports, slot masks, ITE masks) on the host, after checking
        that nothing outside the outputs the call was given changed."""
        host = self.arena.cpu().numpy()
        changed = host != FILL
        for name, nbytes in self.sizes:
            if masks or not name.endswith("mask"):
                o = self.at[name][0]
                changed[o: o + nbytes] = False
        bad = np.flatnonzero(changed)
        assert len(bad) == 0, f"{len(bad)} bytes changed outside the outputs, first at arena byte {int(bad[0])}"
        cut = lambda name: host[self.at[name][0]: self.at[name][0] + self.at[name][1]]
        return (cut("err").view(np.int32), cut("report").reshape(self.n, 48),
                cut("slot_mask").view(np.uint64).reshape(self.n, 32) if masks else None,
                cut("ite_mask").view(np.uint64).reshape(self.n, 16) if masks else None)


def check_dev_once(dev, payloads, adepths, hdrs, flags, shift=0, masks=True, status=None, src=None):
    """src: the caller's own batch of the payloads (its offsets may repeat) in
    place of one guarded batch of them at residues from `shift`."""
    n = len(payloads)
    if src is None:
        src = guarded_batch(torch, [bytes(p) for p in payloads], dev, [(shift + 3 * b) % 16 if shift else 0
                                                                       for b in range(n)], fill=0xEE)
    adepth = torch.tensor(adepths, dtype=torch.uint8, device=dev)
    st = None if status is None else torch.tensor(status, dtype=torch.int32, device=dev)
    hd = None
    if hdrs is not None:
        hd = torch.from_numpy(np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy()).to(dev)
    out = Outputs(dev, n)
    check.check_dev(src, adepth, out.view("report"), out.view("err", torch.int32), hdr=hd, flags=flags,
                    slot_mask=out.view("slot_mask", torch.int64) if masks else None,
                    ite_mask=out.view("ite_mask", torch.int64) if masks else None, status=st)
    torch.cuda.synchronize()
    return out.results(masks)


@pytest.mark.parametrize("shift", [0, 1, 7])
def test_dev_families(dev, tables, shift):
    """Valid tables, a table per kind, the funnel and the fuzzed tables in one
    call, the payloads at residues of their own (shift 0: all aligned), with
    the header facts and POM_CK_ITBID, masks asked for: nothing outside
    report, masks and err changes, and all of it equals the oracle."""
    recs, adepths, hdrs, want = tables
    payloads = [C.payload_of(r) for r in recs]
    same(check_dev_once(dev, payloads, adepths, hdrs, C.CK_ITBID, shift), want[("hdr", C.CK_ITBID)])
    w = want[("hdr", C.CK_ITBID)]
    assert not w[1][:3, :4].any()                                       # the valid tables report nothing
    funnel = C.report_fields(w[1][3 + len(C.kind_tables())])
    assert funnel["count"][C.S_LOOP] == 1024 and funnel["longest"] == 0


def test_dev_without_masks_header_or_flag(dev, tables):
    """Masks NULL (their place in the arena keeps its fill), hdr NULL (kinds
    15 ... 21 are not evaluated), POM_CK_ITBID off."""
    recs, adepths, hdrs, want = tables
    payloads = [C.payload_of(r) for r in recs]
    same(check_dev_once(dev, payloads, adepths, hdrs, C.CK_ITBID, 7, masks=False), want[("hdr", C.CK_ITBID)])
    same(check_dev_once(dev, payloads, adepths, None, C.CK_ITBID, 1), want[(None, C.CK_ITBID)])
    same(check_dev_once(dev, payloads, adepths, hdrs, 0, 0), want[("hdr", 0)])
    bare = want[(None, C.CK_ITBID)][1][:, :4].copy().view("<u4").ravel()
    full = want[("hdr", C.CK_ITBID)][1][:, :4].copy().view("<u4").ravel()
    assert not (bare >> 15).any() and (full >> 16).any() and (full >> 15 & 1).any()


def test_dev_status_and_error_rules(dev):
    """A status array with decoder codes, adepth 0 and 11, n = 11903 and a live
    ITE cut one byte short (live is kept), the cut byte's place holding guard
    fill; the whole tables beside them are checked as ever."""
    t = C.random_table(9, 3, 40)
    rec = t.record()
    payload, hdr = C.payload_of(rec), C.hdr_of(rec)
    top = max(t.hashes)
    cut = payload[: C.ITE_OFF + C.ITE_SIZE * (top + 1) - 1]
    payloads = [payload, payload, payload, payload, payload[: C.ITE_OFF - 1], cut, cut, payload[: C.ITE_OFF - 1],
                payload[: C.ITE_OFF + C.ITE_SIZE * (top + 1)]]
    adepths = [3, 3, 0, 11, 3, 3, 0, 11, 3]
    status = [0, -6, 0, 0, 0, 0, -4, 0, 0]
    want = C.expect(payloads, adepths, [hdr] * 9, 0, status)
    assert want[0].tolist() == [0, -6, C.EINVAL, C.EINVAL, C.E_TRUNCATED, C.E_TRUNCATED, -4, C.EINVAL, 0]
    for shift in (0, 1, 7):
        same(check_dev_once(dev, payloads, adepths, [hdr] * 9, 0, shift, status=status), want)
    same(check_dev_once(dev, payloads, adepths, None, 0, 5, masks=False, status=status),
         C.expect(payloads, adepths, None, 0, status))


def test_dev_refuses_other_flags(dev, tables):
    recs, adepths, hdrs, _ = tables
    with pytest.raises(ValueError):
        check_dev_once(dev, [C.payload_of(recs[0])], adepths[:1], hdrs[:1], 2)
    with pytest.raises(ValueError):
        check_dev_once(dev, [C.payload_of(recs[0])], adepths[:1], hdrs[:1], C.CK_ITBID | 0x80000000)


# ---------------------------------------------------------------------------
# Directed tables: the kernel's words, halves, once / twice bitmaps, walk bound
# and its reuse of one workgroup's LDS
# ---------------------------------------------------------------------------
_directed_cache = {}


def directed_tables(group):
    """(tables, payloads, hdrs, the oracle's answer with hdr and POM_CK_ITBID),
    built once per group."""
    if group not in _directed_cache:
        tables = C.directed(group)
        payloads = [C.payload_of(t.rec) for t in tables]
        hdrs = [C.hdr_of(t.rec) for t in tables]
        want = C.expect(payloads, [t.adepth for t in tables], hdrs, C.CK_ITBID)
        for b, t in enumerate(tables):                                  # the oracle is judged too
            C.assert_directed(t, want[0][b], want[1][b], want[2][b], want[3][b])
        _directed_cache[group] = (tables, payloads, hdrs, want)
    return _directed_cache[group]


@pytest.mark.parametrize("group", C.GROUPS)
def test_dev_directed(dev, group):
    """One call per group and shift (0: every payload aligned; 5: residues of
    their own), with masks, the header facts and POM_CK_ITBID: the kernel
    equals the oracle in err, report and masks, and both state the closed-form
    values the builders give.
      kinds   a table per kind at adepth 1 ... 10, its slots, ITEs and values
              at the low and the high end of their ranges: every ballot word
              and span mask from word 0 to the last, d and 2d mid-word and on
              word edges
      combs   bit 0 and bit 63 of every word
      counts  indeg 1 beside indeg 2, indeg d on one bit, refs 2d on one bit
      walk    paths of d + 1 slots (legal) and their loops, 1,024 lanes on
              1,025 slots each in the adepth-10 fan"""
    tables, payloads, hdrs, want = directed_tables(group)
    adepths = [t.adepth for t in tables]
    for shift in (0, 5):
        got = check_dev_once(dev, payloads, adepths, hdrs, C.CK_ITBID, shift)
        same(got, want)
        for b, t in enumerate(tables):
            C.assert_directed(t, got[0][b], got[1][b], got[2][b], got[3][b])


GRID_MAX = 4096                 # itb_check.hip kCheckGridMax: above it a workgroup takes ITB b, b + 4096, ...


def test_dev_many_itbs_reuse_the_workgroup(dev):
    """2 * 4096 + 37 ITBs over 8 distinct payloads (payload_off repeats), so
    that every workgroup checks two or three ITBs in the LDS it never clears
    as a whole: a full table before an empty one, an error's early `continue`
    before and after a checked table, 1,024 stale hash words before a table of
    two ITEs.  Every ordered pair of the 8 kinds, equal pairs included, meets
    in one workgroup.  All results are compared (the outputs' guards with them);
    the second call has no header facts and no masks."""
    n = 2 * GRID_MAX + 37
    with open(os.path.join(ROOT, "pomegranate_amd", "csrc", "itb_check.hip")) as f:
        assert re.search(r"kCheckGridMax = (\d+);", f.read()).group(1) == str(GRID_MAX)
    t = C.random_table(9, 3, 40)
    cut = C.payload_of(t.record())[: C.ITE_OFF + C.ITE_SIZE * (max(t.hashes) + 1) - 1]
    empty = C.Table(10).record()
    tables = C.kind_tables()
    fan = C.chain(6, "fan", True)
    #            record or payload, adepth, status
    kinds = [(C.funnel(), 10, 0),
             (empty, 10, 0),
             (C.random_table(51, 1, 30, depth=2, itbid=3).record(), 1, 0),
             (tables["leaked_island"][0], 2, 0),
             (cut, 3, 0),
             (tables["valid"][0], 0, 0),
             (tables["dup"][0], 2, -6),
             (fan.rec, 6, 0)]
    payloads = [k[0] if isinstance(k[0], bytes) else C.payload_of(k[0]) for k in kinds]
    assert len(payloads[1]) == C.ITE_OFF and len(set(payloads)) == 8
    hdr8 = [C.hdr_of(t.record()) if isinstance(k[0], bytes) else C.hdr_of(k[0]) for k in kinds]

    def kind(b):
        return b % 8 if b < GRID_MAX else (b - GRID_MAX) // 8 % 8 if b < 2 * GRID_MAX else (b + 3) % 8
    which = np.array([kind(b) for b in range(n)])
    # workgroup g takes ITBs g, g + 4096 (and g + 8192): every ordered pair of kinds follows one another
    assert {(kind(g), kind(g + GRID_MAX)) for g in range(GRID_MAX)} == {(i, j) for i in range(8) for j in range(8)}

    adepths = [kinds[k][1] for k in which]
    status = [kinds[k][2] for k in which]
    hdrs = [hdr8[k] for k in which]
    held = guarded_batch(torch, payloads, dev, [(5 * i + 1) % 16 for i in range(8)], fill=0xEE)
    pick = torch.from_numpy(which).to(dev)
    src = lzo.DeviceBatch(held.arena, held.off[pick].contiguous(), held.length[pick].contiguous())
    many = [payloads[k] for k in which]
    for with_hdr, masks in ((True, True), (False, False)):
        one = C.expect(payloads, [k[1] for k in kinds], hdr8 if with_hdr else None, C.CK_ITBID, [k[2] for k in kinds])
        want = tuple(w[which] for w in one)                             # the oracle ran once per distinct payload
        got = check_dev_once(dev, many, adepths, hdrs if with_hdr else None, C.CK_ITBID, masks=masks, status=status,
                             src=src)
        same(got, want)
    assert one[0].tolist() == [0, 0, 0, 0, C.E_TRUNCATED, C.EINVAL, -6, 0]
    f = [C.report_fields(r) for r in one[1]]
    assert f[0]["count"][C.S_LOOP] == 1024 and f[1]["live"] == f[1]["used_home"] == 0 and not one[1][1].any()
    assert f[4]["live"] == len(t.hashes) and f[3]["count"][C.S_ISLAND] == 1
    C.assert_directed(fan, got[0][7], got[1][7])


# ---------------------------------------------------------------------------
# pom_itb_check_batch against the oracle
# ---------------------------------------------------------------------------
def expect_batch(stored, payloads, flags, codes=None):
    """The oracle over stored records whose decoded payloads are `payloads`
    (None: a record the header checks refuse); codes: {b: the decoder's code}."""
    n = len(stored)
    err = np.full(n, C.EINVAL, np.int32)
    rep = np.zeros((n, 48), np.uint8)
    sm, im = np.zeros((n, 32), np.uint64), np.zeros((n, 16), np.uint64)
    for b, (rec, p) in enumerate(zip(stored, payloads)):
        if p is None:
            continue
        if codes and b in codes:
            err[b] = codes[b]
            continue
        e, r, s, i = C.check(p, rec[C.ITBH_ADEPTH], C.hdr_of(rec), flags)
        err[b], rep[b], sm[b], im[b] = e, np.frombuffer(r, np.uint8), s, i
    return err, rep, sm, im


def as_tuple(res):
    return res.err, res.report.view(np.uint8).reshape(len(res.err), 48), res.slot_mask, res.ite_mask


def test_batch_mixed(oracle, tables):
    """The dev test's tables as records, LZO and stored alternately, with an
    h.entries == 0 record (checked like any other: its bitmap and index must
    be empty too, and one of the two is not), records the header checks refuse
    and an LZO stream cut short; with and without masks; results in caller
    order."""
    recs, adepths, _, _ = tables
    stored = [r if b % 3 == 1 else C.lzo_record(oracle, r) for b, r in enumerate(recs)]
    payloads = [C.payload_of(r) for r in recs]
    empty = C.Table(4).record()
    assert C.hdr_of(empty)["entries"] == 0 and len(empty) == C.ITB_SIZE
    stale = bytearray(empty)
    C.set_slot(stale, H, 3, 0, 0, C.IDX_UNIQUE)                          # entries 0, yet a slot in use
    bad_adepth, bad_algo, short = bytearray(recs[0]), bytearray(recs[1]), bytearray(recs[2][:200])
    bad_adepth[3] = 11
    struct.pack_into("<H", bad_algo, itb.ALGO_OFF, 7)
    ln, zlen, _ = itb.header_fields(stored[2])
    cut = bytearray(stored[2][: ln - 9])
    struct.pack_into("<I", cut, itb.LEN_OFF, ln - 9)
    rc, _ = oracle.decompress_safe(bytes(cut[H:]), zlen - H)
    assert rc != 0
    extra = [(C.lzo_record(oracle, empty), C.payload_of(empty)), (empty, C.payload_of(empty)),
             (C.lzo_record(oracle, stale), C.payload_of(stale)), (bad_adepth, None), (bad_algo, None), (short, None),
             (cut, b"")]
    stored = stored[:5] + [e[0] for e in extra] + stored[5:]
    payloads = payloads[:5] + [e[1] for e in extra] + payloads[5:]
    want = expect_batch(stored, payloads, C.CK_ITBID, {5 + 6: rc})
    res = check.check_batch(stored, C.CK_ITBID, masks=True)
    same(as_tuple(res), want)
    assert want[0][5:12].tolist() == [0, 0, 0, C.EINVAL, C.EINVAL, C.EINVAL, rc]
    assert not want[1][5:7].any()
    stale_f = C.report_fields(want[1][7])
    assert stale_f["live"] == 0 and stale_f["count"][C.S_ENTRY_DEAD] == 1 and stale_f["used_home"] == 1
    lzo_ok = [int(p is not None and (r[itb.ALGO_OFF] == 0 or b != 11)) for b, (r, p) in enumerate(zip(stored, payloads))]
    assert res.len_ok.tolist() == lzo_ok
    plain = check.check_batch(stored, 0)
    assert plain.slot_mask is None and plain.ite_mask is None
    same(as_tuple(plain), expect_batch(stored, payloads, 0, {11: rc}))
    with pytest.raises(ValueError):
        check.check_batch(stored[:2], 4)
    assert len(check.check_batch([], 0).err) == 0


@pytest.fixture(scope="module")
def chunky(oracle):
    """60 adepth-8 tables of about 60 KB, every fourth stored uncompressed,
    every fifth with a few flips: several chunks under chunk_mb=1.
    (stored, want)"""
    stored, payloads = [], []
    for b in range(60):
        if b % 5 == 2:
            rec, _ = C.fuzzed(3000 + b, adepth=8)
        else:
            rec = C.random_table(2000 + b, 8, 140 + 3 * (b % 9), depth=1, itbid=b % 2).record()
        payloads.append(C.payload_of(rec))
        stored.append(rec if b % 4 == 1 else C.lzo_record(oracle, rec))
    return stored, expect_batch(stored, payloads, C.CK_ITBID)


def test_batch_spans_chunks(chunky, debug_env, monkeypatch):
    """chunk_mb=1: 60 records take several chunks, on one GPU and on every
    visible one; the chunks reorder the blocks (smallest first, LZO before
    stored) and the results still come in caller order."""
    stored, want = chunky
    debug_env("chunk_mb=1")
    same(as_tuple(check.check_batch(stored, C.CK_ITBID, masks=True)), want)
    monkeypatch.setenv("POM_LZO_DEVICES", "0")
    same(as_tuple(check.check_batch(stored, C.CK_ITBID, masks=True)), want)
    assert (want[1][:, :4].copy().view("<u4").ravel() != 0).sum() >= 8


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the device's second chunk delivery fails as a failed GPU
    stream would.  The call returns LZO_E_ERROR; an ITB either reads
    LZO_E_ERROR with a zeroed report and zeroed masks or has the unfailed
    run's result, and both kinds occur; the same call succeeds in full
    afterwards (the slots are reusable)."""
    stored, want = chunky
    n = len(stored)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    rep = np.full((n, 48), 7, dtype=np.uint8)
    sm, im = np.full((n, 32), 7, dtype=np.uint64), np.full((n, 16), 7, dtype=np.uint64)
    err, len_ok = np.full(n, 7, dtype=np.int32), np.full(n, 7, dtype=np.int32)
    debug_env("chunk_mb=1,fail_chunk=1")
    rc = check._lib().pom_itb_check_batch(ptrs, lens, n, C.CK_ITBID, rep.ctypes.data, sm.ctypes.data, im.ctypes.data,
                                          err.ctypes.data, len_ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    lost = err == lzo.LZO_E_ERROR
    assert 0 < lost.sum() < n and not rep[lost].any() and not sm[lost].any() and not im[lost].any()
    assert not len_ok[lost].any() and (len_ok[~lost] == 1).all()
    kept = ~lost
    same((err[kept], rep[kept], sm[kept], im[kept]), tuple(w[kept] for w in want))
    debug_env("chunk_mb=1")
    same(as_tuple(check.check_batch(stored, C.CK_ITBID, masks=True)), want)


def test_batch_directed(oracle):
    """The count and walk tables at adepth 1, 6 and 10 as records, LZO and
    stored alternately, through the decode and the chunk pipeline: results in
    caller order, equal to the oracle's and to the closed forms."""
    tables = C.directed("counts", (1, 6, 10)) + C.directed("walk", (1, 6, 10))
    assert len(tables) == 8 + 30
    stored = [t.rec if b % 2 else C.lzo_record(oracle, t.rec) for b, t in enumerate(tables)]
    want = expect_batch(stored, [C.payload_of(t.rec) for t in tables], C.CK_ITBID)
    res = check.check_batch(stored, C.CK_ITBID, masks=True)
    same(as_tuple(res), want)
    assert res.len_ok.tolist() == [1] * len(tables)
    got = as_tuple(res)
    for b, t in enumerate(tables):
        C.assert_directed(t, got[0][b], got[1][b], got[2][b], got[3][b])
