"""GPU: the garbage-collector scan (include/pom_gc.h) against the Python
restatement of mdsl/gc.c:968-993 in gc_scan_util.py -- pom_gc_scan_dev on
guarded arenas, pom_gc_scan_batch through the host chunk pipeline, and its
agreement with the walk over what pom_itb_lzo_decompress_batch decodes."""
from __future__ import annotations

import struct

import numpy as np
import pytest

from gc_scan_util import (EINVAL, E_NOSPACE, E_TRUNCATED, ITE_OFF, ITE_SIZE, expect_batch, lzo_record,
                          make_record, walk)
from gpu_util import guarded_batch
from pomegranate_amd import gc, itb, lzo

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


def payload_of(rec) -> bytes:
    return bytes(rec[H: itb.header_fields(rec)[0]])


# ---------------------------------------------------------------------------
# pom_gc_scan_dev on guarded arenas
# ---------------------------------------------------------------------------
DIRECTED = [("empty", []), ("full", list(range(1024))), ("bit0", [0]), ("bit63", [63]), ("bit64", [64]),
            ("bit1023", [1023]), ("even", list(range(0, 1024, 2))), ("odd", list(range(1, 1024, 2)))]


@pytest.fixture(scope="module")
def dev_cases():
    """16 payloads, one per residue mod 16: the directed bitmaps at adepth 10,
    then adepths 1 ... 6 with bits above the limit, then two payloads that end
    before a live ITE does -- one holds 7 ITEs with bit 7 live, the whole ITE
    just past it; one is cut one byte short of its live ITE's end -- with the
    missing ITE bytes as their neighbours.  (payload, continuation, adepth) each."""
    cases = []
    for i, (_, bits) in enumerate(DIRECTED):
        n_ites = (max(bits) + 1) if bits else 1
        cases.append((payload_of(make_record(100 + i, n_ites, 10, bits)), b"", 10))
    for adepth in range(1, 7):
        bits = [0, 1, 2, 5, 17, 40, 63, 64, 65, 100, 127]
        cases.append((payload_of(make_record(200 + adepth, 128, adepth, bits)), b"", adepth))
    whole = payload_of(make_record(300, 8, 10, [1, 7]))
    cases.append((whole[:-ITE_SIZE], whole[-ITE_SIZE:], 10))
    cases.append((whole[:-1], whole[-1:] + bytes(make_record(301, 1, 10, [0])[H + ITE_OFF:]), 10))
    assert len(cases) == 16
    return cases


class Outputs:
    """live, nranges, err, first and ranges carved out of ONE arena of FILL
    bytes with guard bytes around each, so a stray store shows."""

    def __init__(self, dev, n, room):
        self.n, self.room = n, room
        sizes = [("live", 4 * n), ("nranges", 4 * n), ("err", 4 * n), ("first", 8 * (n + 1)), ("ranges", 16 * room)]
        self.at, pos = {}, 4096
        for name, nbytes in sizes:
            self.at[name] = (pos, nbytes)
            pos = (pos + nbytes + 4096 + 255) // 256 * 256
        self.arena = torch.full((pos,), FILL, dtype=torch.uint8, device=dev)

    def view(self, name, dtype):
        o, nbytes = self.at[name]
        return self.arena[o: o + nbytes].view(dtype)

    def check_untouched(self, written_ranges):
        host = self.arena.cpu().numpy()
        changed = host != FILL
        for name, nbytes in (("live", 4 * self.n), ("nranges", 4 * self.n), ("err", 4 * self.n),
                             ("first", 8 * (self.n + 1)), ("ranges", 16 * written_ranges)):
            o = self.at[name][0]
            changed[o: o + nbytes] = False
        bad = np.flatnonzero(changed)
        assert len(bad) == 0, f"{len(bad)} bytes changed outside the outputs, first at arena byte {int(bad[0])}"


def scan_dev_once(dev, cases, shifts, column, status, cap_of_total, src=None):
    payloads = [c[0] for c in cases]
    if src is None:
        src = guarded_batch(torch, payloads, dev, shifts, fill=0xEE, neighbours="continuation",
                            continuation=[c[1] for c in cases])
    n = len(cases)
    adepth = torch.tensor([c[2] for c in cases], dtype=torch.uint8, device=dev)
    st = None if status is None else torch.tensor(status, dtype=torch.int32, device=dev)
    want_err, want_live, want_first, want_ranges = expect_batch(
        [None if status is not None and status[b] else payloads[b] for b in range(n)],
        [c[2] for c in cases], column)
    total = int(want_first[n])
    cap = cap_of_total(total)
    out = Outputs(dev, n, total + 8)
    gc.scan_dev(src, adepth, column, out.view("live", torch.int32), out.view("nranges", torch.int32),
                out.view("first", torch.int64), out.view("ranges", torch.int64).view(-1, 2),
                out.view("err", torch.int32), status=st, ranges_cap=cap)
    torch.cuda.synchronize()
    out.check_untouched(min(total, cap))
    live = out.view("live", torch.int32).cpu().numpy().view(np.uint32)
    nranges = out.view("nranges", torch.int32).cpu().numpy().view(np.uint32)
    err = out.view("err", torch.int32).cpu().numpy()
    first = out.view("first", torch.int64).cpu().numpy().view(np.uint64)
    ranges = out.view("ranges", torch.int64).cpu().numpy().view(np.uint64).reshape(-1, 2)
    for b in range(n):
        e = status[b] if want_err[b] is None else want_err[b]
        assert (int(err[b]), int(live[b])) == (e, want_live[b]), b
    assert (first == want_first).all()
    assert (nranges == np.diff(want_first)).all()
    assert (ranges[: min(total, cap)] == want_ranges[: min(total, cap)]).all()
    return err, total


@pytest.mark.parametrize("rot", [0, 5, 11])
def test_dev_every_residue_directed_bitmaps(dev, dev_cases, rot):
    """Each of the 16 payloads at a residue of its own (three rotations put the
    large and the cut payloads at different residues); every column over the
    rotations."""
    shifts = [(b + rot) % 16 for b in range(16)]
    for column in (rot % 6, (rot + 3) % 6):
        err, total = scan_dev_once(dev, dev_cases, shifts, column, None, lambda t: t)
        assert total > 1000
        # the cut payloads: the rest of the live ITE lies right behind them and is not read
        assert (err[14:] == E_TRUNCATED).all() and (err[:14] == 0).all()


def test_dev_status_passes_through(dev, dev_cases):
    status = [0] * 16
    status[1], status[9] = -6, lzo.LZO_E_INPUT_OVERRUN
    err, _ = scan_dev_once(dev, dev_cases, list(range(16)), 2, status, lambda t: t)
    assert (err[1], err[9]) == (-6, lzo.LZO_E_INPUT_OVERRUN)


@pytest.mark.parametrize("cap", ["zero", "total-1", "total"])
def test_dev_ranges_cap(dev, dev_cases, cap):
    """Nothing is written at or past ranges_cap; first[] is complete anyway."""
    pick = {"zero": lambda t: 0, "total-1": lambda t: t - 1, "total": lambda t: t}[cap]
    scan_dev_once(dev, dev_cases, [(3 * b + 1) % 16 for b in range(16)], 4, None, pick)


def test_dev_bad_adepth_and_many_blocks(dev):
    """adepth 0 and 11 are -EINVAL; 10,000 blocks take several tiles of the
    prefix kernel and more waves than the capped grid has (2,048 workgroups of
    4), so the grid stride runs.  The blocks share 50 payloads: payload_off
    may repeat."""
    n = 10000
    recs = [make_record(400 + i, 1 + i % 3, 1 + i % 2, [0, 1][: 1 + i % 2]) for i in range(50)]
    held = guarded_batch(torch, [payload_of(r) for r in recs], dev, [i % 16 for i in range(50)], fill=0xEE)
    pick = torch.arange(n, device=dev) % 50
    src = lzo.DeviceBatch(held.arena, held.off[pick].contiguous(), held.length[pick].contiguous())
    cases = [(payload_of(recs[i % 50]), b"", 0 if i == 7 else 11 if i == 9300 else 1 + i % 2) for i in range(n)]
    err, total = scan_dev_once(dev, cases, None, 1, None, lambda t: t, src=src)
    assert err[7] == EINVAL and err[9300] == EINVAL and total > 5000


# ---------------------------------------------------------------------------
# pom_gc_scan_batch against the oracle
# ---------------------------------------------------------------------------
def check_batch(records, payloads, adepths, column, want_err=None, **kw):
    """payloads[b]: what the walk sees (None: the ITB yields nothing and its
    err is want_err[b])."""
    res = gc.scan_batch(records, column, **kw)
    errs, lives, first, ranges = expect_batch(payloads, adepths, column)
    n = len(records)
    for b in range(n):
        e = want_err[b] if errs[b] is None else errs[b]
        assert (int(res.err[b]), int(res.live[b])) == (e, lives[b]), b
    assert (res.first == first).all()
    cap = kw.get("ranges_cap")
    fit = int(first[n]) if cap is None else min(int(first[n]), cap)
    assert res.rc == (E_NOSPACE if fit < int(first[n]) else 0)
    assert res.ranges.shape[0] == fit and (res.ranges == ranges[:fit]).all()
    return res


def test_batch_one(oracle):
    rec = make_record(500, 105, 7, range(0, 105))
    res = check_batch([lzo_record(oracle, rec)], [payload_of(rec)], [7], 0)
    assert (int(res.len_ok[0]), int(res.entries_ok[0])) == (1, 1) and res.first[1] > 50


def test_batch_three_mixed(oracle):
    recs = [make_record(510 + i, n, ad, bits) for i, (n, ad, bits) in
            enumerate([(4, 2, [0, 3]), (70, 10, [0, 64, 69]), (9, 4, [1, 2, 8])])]
    stored = [recs[0], lzo_record(oracle, recs[1]), recs[2]]
    for column in range(6):
        res = check_batch(stored, [payload_of(r) for r in recs], [2, 10, 4], column)
        assert res.len_ok.tolist() == [1, 1, 1] and res.entries_ok.tolist() == [1, 1, 1]


@pytest.fixture(scope="module")
def many(oracle):
    """700 LZO ITBs of 1 ... 4 ITEs: more than two per CU, so the chunk's decode
    takes the op-set decoder."""
    recs = [make_record(600 + i, 1 + i % 4, 2, range(1 + i % 4)) for i in range(700)]
    return recs, [lzo_record(oracle, r) for r in recs]


def test_batch_700_small(many):
    recs, stored = many
    res = check_batch(stored, [payload_of(r) for r in recs], [2] * 700, 3)
    assert res.len_ok.all() and res.entries_ok.all() and res.first[700] > 700


def test_batch_2500_tiny(oracle):
    """Several tiles of the prefix kernel in one chunk; every fifth record
    stored uncompressed (walked where it is staged, behind the LZO blocks)."""
    base = [make_record(700 + i, 1, 1, [0]) for i in range(25)]
    zbase = [lzo_record(oracle, r) for r in base]
    stored = [base[i % 25] if i % 5 == 0 else zbase[i % 25] for i in range(2500)]
    check_batch(stored, [payload_of(base[i % 25]) for i in range(2500)], [1] * 2500, 5)


def test_batch_full_itb(oracle):
    rec = make_record(800, 1024, 10, range(1024))
    res = check_batch([lzo_record(oracle, rec)], [payload_of(rec)], [10], 1)
    assert int(res.live[0]) == 1024 and res.first[1] > 600


def test_batch_damaged_stream_between_neighbours(oracle):
    recs = [make_record(810 + i, 6, 3, range(6)) for i in range(5)]
    stored = [lzo_record(oracle, r) for r in recs]
    # cut the middle record's stream short: the decoder's own code comes back
    ln, zlen, _ = itb.header_fields(stored[2])
    cut = bytearray(stored[2][: ln - 9])
    struct.pack_into("<I", cut, itb.LEN_OFF, ln - 9)
    stored[2] = cut
    rc, _ = oracle.decompress_safe(bytes(cut[H:]), zlen - H)
    assert rc != 0
    payloads = [payload_of(r) for r in recs]
    payloads[2] = None
    res = check_batch(stored, payloads, [3] * 5, 0, want_err={2: rc})
    assert res.first[2] == res.first[3] and res.len_ok.tolist() == [1, 1, 0, 1, 1]


def test_batch_len_and_entries_flags(oracle):
    recs = [make_record(820, 5, 3, range(5)), make_record(821, 5, 3, range(5), entries=4),
            make_record(822, 5, 3, range(5)), make_record(823, 3, 3, [0, 2], entries=3)]
    stored = [lzo_record(oracle, recs[0], zlen_delta=1), lzo_record(oracle, recs[1]), recs[2], recs[3]]
    res = check_batch(stored, [payload_of(r) for r in recs], [3] * 4, 2)
    assert res.len_ok.tolist() == [0, 1, 1, 1]            # zlen one too large: logged, still walked
    assert res.entries_ok.tolist() == [1, 0, 1, 0]


def test_batch_bad_headers(oracle):
    good = make_record(830, 3, 2, [0, 1, 2])
    z = lzo_record(oracle, good)

    def patched(rec, fmt, off, value):
        r = bytearray(rec)
        struct.pack_into(fmt, r, off, value)
        return r
    stored = [good,
              patched(good, "<I", itb.LEN_OFF, 263),                      # h.len < 264
              patched(good, "<I", itb.LEN_OFF, len(good) + 1),            # h.len > rec_len
              patched(good, "<H", itb.ALGO_OFF, 2),                       # neither NONE nor LZO
              patched(z, "<I", itb.ZLEN_OFF, 264),                        # zlen - 264 == 0
              patched(z, "<I", itb.ZLEN_OFF, 264 + itb.PAYLOAD_MAX + 1),  # above the largest ITB
              patched(good, "<B", 3, 0), patched(z, "<B", 3, 11),         # adepth
              good[:200],                                                 # no whole header
              z]
    payloads = [payload_of(good)] + [None] * 8 + [payload_of(good)]
    res = check_batch(stored, payloads, [2] * 10, 0, want_err={b: EINVAL for b in range(1, 9)})
    assert res.entries_ok.tolist() == [1] + [0] * 8 + [1]


def test_batch_truncated_record_stored_uncompressed():
    """A COMPR_NONE record whose payload ends inside a live ITE."""
    rec = make_record(840, 4, 2, [0, 3])
    short = bytearray(rec[:-1])
    struct.pack_into("<I", short, itb.LEN_OFF, len(short))
    res = check_batch([rec, short, rec], [payload_of(rec), payload_of(short), payload_of(rec)], [2] * 3, 0)
    assert res.err.tolist() == [0, E_TRUNCATED, 0]


def test_batch_nospace_then_retry(many):
    recs, stored = many
    payloads = [payload_of(r) for r in recs[:40]]
    res = check_batch(stored[:40], payloads, [2] * 40, 0, ranges_cap=10)
    assert res.rc == E_NOSPACE
    check_batch(stored[:40], payloads, [2] * 40, 0, ranges_cap=int(res.first[40]))
    check_batch(stored[:40], payloads, [2] * 40, 0, ranges_cap=0)


@pytest.fixture(scope="module")
def chunky(oracle):
    """60 records of about 50 KB, every fourth stored uncompressed: several
    chunks under chunk_mb=1."""
    recs = [make_record(900 + i, 20 + 7 * (i % 9), 8, range(0, 20 + 7 * (i % 9), 1 + i % 3)) for i in range(60)]
    return recs, [r if i % 4 == 1 else lzo_record(oracle, r) for i, r in enumerate(recs)]


def test_batch_spans_chunks(chunky, debug_env):
    """chunk_mb=1: about 50 KB a record, so 60 records take several chunks;
    the chunks reorder the blocks (smallest first, LZO before stored) and the
    ranges still come out in ITB order."""
    recs, stored = chunky
    debug_env("chunk_mb=1")
    check_batch(stored, [payload_of(r) for r in recs], [8] * 60, 1)


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the device's second chunk delivery fails as a failed GPU
    stream would.  The call returns LZO_E_ERROR, every record that went to the
    GPU reads LZO_E_ERROR with nothing live, a bad header keeps -EINVAL, and
    the same call succeeds in full afterwards (the slots are reusable)."""
    import ctypes
    recs, stored = chunky[0], list(chunky[1])
    stored.insert(30, recs[0][:200])                            # no whole header
    payloads = [payload_of(r) for r in recs]
    payloads.insert(30, None)
    n = len(stored)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    ranges = np.zeros((1024 * n, 2), dtype=np.uint64)
    first = np.zeros(n + 1, dtype=np.uint64)
    live = np.full(n, 7, dtype=np.uint32)
    err, len_ok, entries_ok = (np.full(n, 7, dtype=np.int32) for _ in range(3))
    debug_env("chunk_mb=1,fail_chunk=1")
    rc = gc._lib().pom_gc_scan_batch(ptrs, lens, n, 1, ranges.ctypes.data, 1024 * n, first.ctypes.data,
                                    live.ctypes.data, err.ctypes.data, len_ok.ctypes.data, entries_ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    assert err.tolist() == [EINVAL if b == 30 else lzo.LZO_E_ERROR for b in range(n)]
    assert not live.any()
    debug_env("chunk_mb=1")
    check_batch(stored, payloads, [8] * n, 1, want_err={30: EINVAL})


def test_batch_agrees_with_decompress_batch(oracle):
    """64 ITBs: the ranges equal the reference loop run over what
    pom_itb_lzo_decompress_batch decodes."""
    recs = [make_record(1000 + i, 1 + 3 * i, 8, range(0, 1 + 3 * i, 1 + i % 2)) for i in range(64)]
    stored = [lzo_record(oracle, r) for r in recs]
    res = gc.scan_batch(stored, 2)
    bufs = [bytearray(s) + bytearray(itb.ITB_FULL - len(s)) for s in stored]
    err, ok = itb.decompress_batch(bufs)
    assert not any(err) and all(ok)
    rows, first = [], [0]
    for b in bufs:
        ln = itb.header_fields(b)[0]
        e, live, rg = walk(bytes(b[H:ln]), b[3], 2)
        assert e == 0
        rows.extend(rg)
        first.append(len(rows))
    assert res.rc == 0 and (res.err == 0).all()
    assert res.first.tolist() == first and res.ranges.tolist() == [list(r) for r in rows]
