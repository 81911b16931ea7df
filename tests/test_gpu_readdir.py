"""GPU: the directory listing (include/pom_readdir.h) against the Python
restatement of mds/itb.c:2536-2589 in readdir_util.py -- pom_readdir_dev on
guarded arenas, pom_readdir_batch through the host chunk pipeline.  Every
comparison is byte-exact."""
from __future__ import annotations

import struct

import numpy as np
import pytest

import gc_scan_util
from gpu_util import guarded_batch
from pomegranate_amd import itb, lzo, readdir
from readdir_util import (EINVAL, E_NAME, E_NOSPACE, E_TRUNCATED, ITE_FLAG_KV, ITE_FLAG_NORMAL, ITE_OFF, ITE_SIZE,
                          expect_batch, listing, lzo_record, make_record)

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
# pom_readdir_dev on guarded arenas
# ---------------------------------------------------------------------------
DIRECTED = [("empty", []), ("full", list(range(1024))), ("bit0", [0]), ("bit63", [63]), ("bit64", [64]),
            ("bit1023", [1023]), ("even", list(range(0, 1024, 2))), ("odd", list(range(1, 1024, 2)))]
NAME_LENS = [0, 1, 15, 16, 17, 255, 256]


@pytest.fixture(scope="module")
def dev_cases():
    """(payload, continuation, adepth) each, with the oracle's listing cached
    by expect():
      0 ... 7    the directed bitmaps at adepth 10
      8 ... 11   adepth 1, 6, 7, 10 with bits above the limit
      12 ... 18  every ITE with one of the name lengths 0 ... 256
      19         every name length side by side, twice over
      20, 21     namelen 257 on an emitted ITE (POM_RD_E_NAME); on skipped ITEs (no error)
      22         every non-active state and the KV flag
      23, 24     payloads that end before a live ITE does -- one holds 7 ITEs
                 with bit 7 live, the whole ITE just past it; one is cut one byte
                 short of its live ITE's end -- with the missing ITE bytes as
                 their neighbours
      25         a payload that ends exactly with its last live ITE."""
    cases = []
    for i, (_, bits) in enumerate(DIRECTED):
        n_ites = (max(bits) + 1) if bits else 1
        cases.append((payload_of(make_record(100 + i, n_ites, 10, bits)), b"", 10))
    for adepth in (1, 6, 7, 10):
        bits = [0, 1, 2, 5, 17, 40, 63, 64, 65, 100, 127, 128, 199]
        cases.append((payload_of(make_record(200 + adepth, 200, adepth, bits)), b"", adepth))
    for n in NAME_LENS:
        cases.append((payload_of(make_record(300 + n, 70, 7, range(70), namelens={nr: n for nr in range(70)})), b"", 7))
    mixed = {nr: NAME_LENS[nr % 7] for nr in range(14)}
    cases.append((payload_of(make_record(320, 14, 4, range(14), namelens=mixed)), b"", 4))
    cases.append((payload_of(make_record(321, 8, 3, range(8), namelens={5: 257})), b"", 3))
    cases.append((payload_of(make_record(322, 8, 3, range(8), namelens={2: 257, 5: 1 << 20},
                                         flags={2: ITE_FLAG_NORMAL | 1, 5: ITE_FLAG_KV})), b"", 3))
    flags = {nr: ITE_FLAG_NORMAL | nr for nr in range(8)}
    flags[8] = ITE_FLAG_NORMAL | ITE_FLAG_KV
    cases.append((payload_of(make_record(323, 10, 4, range(10), flags=flags)), b"", 4))
    whole = payload_of(make_record(330, 8, 10, [1, 7]))
    cases.append((whole[:-ITE_SIZE], whole[-ITE_SIZE:], 10))
    cases.append((whole[:-1], whole[-1:] + bytes(make_record(331, 1, 10, [0])[H + ITE_OFF:]), 10))
    cases.append((whole, b"", 10))
    assert len(cases) == 26
    return cases


_listing_cache = {}


def expect(cases, status=None):
    """expect_batch with one listing() per distinct payload."""
    errs, lives, dnums, first, data = [], [], [], [0], bytearray()
    for b, (p, _, ad) in enumerate(cases):
        if status is not None and status[b]:
            res = (None, 0, 0, b"")
        else:
            key = (id(p), ad)
            if key not in _listing_cache:
                _listing_cache[key] = (p, listing(p, ad))           # (p kept alive: its id stays its own)
            res = _listing_cache[key][1]
        errs.append(res[0])
        lives.append(res[1])
        dnums.append(res[2])
        data += res[3]
        first.append(len(data))
    return errs, lives, dnums, np.array(first, dtype=np.uint64), bytes(data)


class Outputs:
    """live, dnum, bytes, err, first and out carved out of ONE arena of FILL
    bytes with guard bytes around each, so a stray store shows; out starts at
    residue `oshift` mod 16."""

    def __init__(self, dev, n, room, oshift):
        self.n = n
        sizes = [("live", 4 * n), ("dnum", 4 * n), ("bytes", 4 * n), ("err", 4 * n), ("first", 8 * (n + 1)),
                 ("out", room)]
        self.at, pos = {}, 4096
        for name, nbytes in sizes:
            if name == "out":
                pos += oshift
            self.at[name] = (pos, nbytes)
            pos = (pos + nbytes + 4096 + 255) // 256 * 256
        self.arena = torch.full((pos,), FILL, dtype=torch.uint8, device=dev)
        assert self.arena.data_ptr() % 256 == 0 and self.at["out"][0] % 16 == oshift

    def view(self, name, dtype=torch.uint8):
        o, nbytes = self.at[name]
        return self.arena[o: o + nbytes].view(dtype)

    def check_untouched(self, written_bytes):
        host = self.arena.cpu().numpy()
        changed = host != FILL
        for name, nbytes in (("live", 4 * self.n), ("dnum", 4 * self.n), ("bytes", 4 * self.n), ("err", 4 * self.n),
                             ("first", 8 * (self.n + 1)), ("out", written_bytes)):
            o = self.at[name][0]
            changed[o: o + nbytes] = False
        bad = np.flatnonzero(changed)
        assert len(bad) == 0, f"{len(bad)} bytes changed outside the outputs, first at arena byte {int(bad[0])}"


def scan_dev_once(dev, cases, shifts, status=None, cap_of_total=lambda t: t, oshift=0, src=None):
    payloads = [c[0] for c in cases]
    if src is None:
        src = guarded_batch(torch, payloads, dev, shifts, fill=0xEE, neighbours="continuation",
                            continuation=[c[1] for c in cases])
    n = len(cases)
    adepth = torch.tensor([c[2] for c in cases], dtype=torch.uint8, device=dev)
    st = None if status is None else torch.tensor(status, dtype=torch.int32, device=dev)
    want_err, want_live, want_dnum, want_first, want = expect(cases, status)
    total = int(want_first[n])
    cap = cap_of_total(total)
    out = Outputs(dev, n, total + 64, oshift)
    readdir.scan_dev(src, adepth, out.view("live", torch.int32), out.view("dnum", torch.int32),
                     out.view("bytes", torch.int32), out.view("first", torch.int64), out.view("out"),
                     out.view("err", torch.int32), status=st, out_cap=cap)
    torch.cuda.synchronize()
    out.check_untouched(min(total, cap))            # the poisoned tail behind the cap stays poisoned
    live = out.view("live", torch.int32).cpu().numpy().view(np.uint32)
    dnum = out.view("dnum", torch.int32).cpu().numpy().view(np.uint32)
    nbytes = out.view("bytes", torch.int32).cpu().numpy().view(np.uint32)
    err = out.view("err", torch.int32).cpu().numpy()
    first = out.view("first", torch.int64).cpu().numpy().view(np.uint64)
    got = out.view("out").cpu().numpy()[: min(total, cap)].tobytes()
    want_e = np.array([status[b] if want_err[b] is None else want_err[b] for b in range(n)], dtype=np.int32)
    assert (err == want_e).all(), np.flatnonzero(err != want_e)[:8]
    assert (live == np.array(want_live, dtype=np.uint32)).all()
    assert (dnum == np.array(want_dnum, dtype=np.uint32)).all()
    assert (first == want_first).all()
    assert (nbytes == np.diff(want_first)).all()
    assert got == want[: min(total, cap)]
    return err, first


@pytest.mark.parametrize("rot", [0, 5, 11])
def test_dev_directed_cases(dev, dev_cases, rot):
    """Every directed case, each payload at a residue of its own (three
    rotations), the output at a residue that moves too."""
    shifts = [(b + rot) % 16 for b in range(len(dev_cases))]
    err, first = scan_dev_once(dev, dev_cases, shifts, oshift=(3 * rot + 1) % 16)
    assert err[20] == E_NAME and err[21] == 0
    # the cut payloads: the rest of the live ITE lies right behind them and is not read
    assert (err[23:25] == E_TRUNCATED).all() and err[25] == 0
    assert (np.delete(err, [20, 23, 24]) == 0).all()
    assert first[-1] > 50000


def test_dev_every_payload_residue_by_every_output_residue(dev, dev_cases):
    """16 payloads (name lengths 0 ... 256 mixed, states, the cut ones) at the
    residues 0 ... 15, rotated against the output's 16 residues: every pair."""
    pick = [dev_cases[i] for i in (19, 22, 12, 13, 14, 15, 16, 17, 18, 8, 9, 23, 24, 25, 21, 2)]
    assert len({((b + 5 * o) % 16, o) for o in range(16) for b in range(16)}) == 256
    for oshift in range(16):
        scan_dev_once(dev, pick, [(b + 5 * oshift) % 16 for b in range(16)], oshift=oshift)


def test_dev_maximum_itb(dev):
    """One ITB with all 1,024 entries live and 256-byte names: 278,528 bytes,
    read off first[]."""
    rec = make_record(400, 1024, 10, range(1024), namelens={nr: 256 for nr in range(1024)},
                      flags={nr: 0 for nr in range(1024)})
    for shift, oshift in ((0, 0), (3, 9)):
        _, first = scan_dev_once(dev, [(payload_of(rec), b"", 10)], [shift], oshift=oshift)
        assert first.tolist() == [0, 278528]


def test_dev_empty_itbs_between(dev, dev_cases):
    """ITBs that emit nothing -- an empty bitmap, every entry skipped, an
    error -- between ITBs that do."""
    none = payload_of(make_record(410, 6, 3, range(6), flags={nr: ITE_FLAG_NORMAL | 2 for nr in range(6)}))
    empty, some, bad, cut = dev_cases[0], dev_cases[19], dev_cases[20], dev_cases[23]
    order = [empty, some, (none, b"", 3), some, bad, cut, some, empty, empty, some, (none, b"", 3)]
    err, first = scan_dev_once(dev, order, [(3 * b) % 16 for b in range(len(order))], oshift=5)
    per = np.diff(first)
    assert (per[[0, 2, 4, 5, 7, 8, 10]] == 0).all() and (per[[1, 3, 6, 9]] > 0).all()


def test_dev_status_passes_through(dev, dev_cases):
    status = [0] * len(dev_cases)
    status[1], status[9], status[20] = -6, lzo.LZO_E_INPUT_OVERRUN, -5
    err, first = scan_dev_once(dev, dev_cases, [b % 16 for b in range(len(dev_cases))], status=status, oshift=2)
    assert (err[1], err[9], err[20]) == (-6, lzo.LZO_E_INPUT_OVERRUN, -5)
    assert first[1] == first[2] and first[9] == first[10]


@pytest.mark.parametrize("cap", ["0", "1", "15", "16", "17", "total-1", "total"])
def test_dev_out_cap(dev, dev_cases, cap):
    """Nothing is written at or past out_cap -- the cap cuts a header (1, 15),
    sits at its end (16) or cuts a name (17, and wherever total - 1 falls) --
    and first[] is complete anyway."""
    pick = {"total-1": lambda t: t - 1, "total": lambda t: t}.get(cap, lambda t: int(cap))
    cases = [dev_cases[i] for i in (19, 2, 12, 15, 22, 9)]
    for oshift in (0, 7):
        scan_dev_once(dev, cases, [(3 * b + 1) % 16 for b in range(len(cases))], cap_of_total=pick, oshift=oshift)


def test_dev_out_cap_inside_a_later_itb(dev, dev_cases):
    """Caps that fall inside the second and the last ITB's records."""
    cases = [dev_cases[i] for i in (19, 16, 9, 13)]
    _, first = scan_dev_once(dev, cases, [0, 5, 9, 14], oshift=3)
    for cap in (int(first[1]) + 1, int(first[1]) + 16, int(first[2]) - 1, int(first[3]), int(first[3]) + 9):
        scan_dev_once(dev, cases, [0, 5, 9, 14], cap_of_total=lambda t, c=cap: c, oshift=3)


def test_dev_many_blocks_repeated_payloads(dev):
    """8,200 ITBs over 8 distinct payloads: several tiles of the prefix kernel
    and more waves than the capped grid has (2,048 workgroups of 4), so the
    grid stride runs; payload_off repeats.  adepth 0 and 11 are -EINVAL."""
    n = 8200
    recs = [make_record(420 + i, 2 + i, 1 + i % 3, range(2 + i)) for i in range(8)]
    payloads = [payload_of(r) for r in recs]
    held = guarded_batch(torch, payloads, dev, [(2 * i + 1) % 16 for i in range(8)], fill=0xEE)
    pick = torch.arange(n, device=dev) % 8
    src = lzo.DeviceBatch(held.arena, held.off[pick].contiguous(), held.length[pick].contiguous())
    cases = [(payloads[i % 8], b"", 0 if i == 7 else 11 if i == 8191 else 1 + i % 3) for i in range(n)]
    err, first = scan_dev_once(dev, cases, None, oshift=11, src=src)
    assert err[7] == EINVAL and err[8191] == EINVAL and first[n] > 200000


# ---------------------------------------------------------------------------
# pom_readdir_batch against the oracle
# ---------------------------------------------------------------------------
def check_batch(records, payloads, adepths, want_err=None, **kw):
    """payloads[b]: what the walk sees (None: the ITB yields nothing and its
    err is want_err[b])."""
    res = readdir.scan_batch(records, **kw)
    errs, lives, dnums, first, data = expect_batch(payloads, adepths)
    n = len(records)
    for b in range(n):
        e = want_err[b] if errs[b] is None else errs[b]
        assert (int(res.err[b]), int(res.live[b]), int(res.dnum[b])) == (e, lives[b], dnums[b]), b
    assert (res.first == first).all()
    cap = kw.get("out_cap")
    fit = int(first[n]) if cap is None else min(int(first[n]), cap)
    assert res.rc == (E_NOSPACE if fit < int(first[n]) else 0)
    assert res.out.tobytes() == data[:fit]
    return res


def test_batch_mixed_lzo_none_and_no_entries(oracle):
    """COMPR_LZO, COMPR_NONE and h.entries == 0 records side by side; a record
    with no entries is not walked, whatever its bitmap says."""
    recs = [make_record(510 + i, n, ad, bits) for i, (n, ad, bits) in
            enumerate([(4, 2, [0, 3]), (70, 10, [0, 64, 69]), (9, 4, [1, 2, 8]), (5, 3, [0, 1]), (6, 3, range(6))])]
    idle = make_record(520, 3, 2, [0, 1, 2], entries=0)
    stored = [recs[0], lzo_record(oracle, recs[1]), idle, recs[2], lzo_record(oracle, idle), lzo_record(oracle, recs[3]),
              recs[4]]
    payloads = [payload_of(recs[0]), payload_of(recs[1]), None, payload_of(recs[2]), None, payload_of(recs[3]),
                payload_of(recs[4])]
    res = check_batch(stored, payloads, [2, 10, 2, 4, 2, 3, 3], want_err={2: 0, 4: 0})
    assert res.len_ok.tolist() == [1, 1, 0, 1, 0, 1, 1] and res.entries_ok.tolist() == [1] * 7
    assert res.first[2] == res.first[3] and res.first[4] == res.first[5]
    # the reference's reply, rebuilt as the header says
    for b, rec in ((1, recs[1]), (6, recs[4])):
        entries = struct.unpack_from("<i", rec, 4)[0]
        nbytes = int(res.first[b + 1] - res.first[b])
        assert 16 * entries + (nbytes - 16 * int(res.dnum[b])) == nbytes          # every live entry active
        assert entries - (int(res.live[b]) - int(res.dnum[b])) == int(res.dnum[b])


def test_batch_skipped_entries_and_reply_lengths(oracle):
    """Entries that are live and not listed: hmr->len and hmr->dnum as the
    header rebuilds them equal what mds/itb.c:2540-2587 computes."""
    flags = {1: ITE_FLAG_NORMAL | 1, 4: ITE_FLAG_KV}
    rec = make_record(530, 6, 3, range(6), flags=flags)
    res = check_batch([lzo_record(oracle, rec)], [payload_of(rec)], [3])
    nbytes = int(res.first[1])
    names = sum(len(r[2]) for r in readdir.parse(res.out))
    assert (int(res.live[0]), int(res.dnum[0])) == (6, 4)
    assert 16 * 6 + (nbytes - 16 * 4) == 16 * 6 + names              # hmr->len
    assert 6 - (6 - 4) == 4                                          # hmr->dnum


@pytest.fixture(scope="module")
def many(oracle):
    """700 LZO ITBs of 1 ... 4 ITEs: more than two per CU, so the chunk's decode
    takes the op-set decoder."""
    recs = [make_record(600 + i, 1 + i % 4, 2, range(1 + i % 4)) for i in range(700)]
    return recs, [lzo_record(oracle, r) for r in recs]


def test_batch_700_small(many):
    recs, stored = many
    res = check_batch(stored, [payload_of(r) for r in recs], [2] * 700)
    assert res.len_ok.all() and res.entries_ok.all() and res.first[700] > 700 * 16


def test_batch_full_itb(oracle):
    rec = make_record(800, 1024, 10, range(1024))
    res = check_batch([lzo_record(oracle, rec)], [payload_of(rec)], [10])
    assert (int(res.live[0]), int(res.dnum[0])) == (1024, 1024)


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
    res = check_batch(stored, payloads, [3] * 5, want_err={2: rc})
    assert res.first[2] == res.first[3] and res.len_ok.tolist() == [1, 1, 0, 1, 1]


def test_batch_wrong_zlen(oracle):
    """zlen one too large: the decode is short of it (len_ok 0) and the ITB is
    listed from what was produced; one too small: the decoder's overrun code."""
    recs = [make_record(820 + i, 5, 3, range(5)) for i in range(3)]
    small = lzo_record(oracle, recs[1], zlen_delta=-1)
    rc, _ = oracle.decompress_safe(bytes(small[H:]), itb.header_fields(small)[1] - H)
    assert rc == lzo.LZO_E_OUTPUT_OVERRUN
    stored = [lzo_record(oracle, recs[0], zlen_delta=1), small, lzo_record(oracle, recs[2])]
    res = check_batch(stored, [payload_of(recs[0]), None, payload_of(recs[2])], [3] * 3, want_err={1: rc})
    assert res.len_ok.tolist() == [0, 0, 1] and res.entries_ok.tolist() == [1, 0, 1]


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
              patched(good, "<i", 4, -1), patched(z, "<i", 4, -(1 << 31)),    # h.entries < 0
              patched(good, "<i", 4, 2),                                  # h.entries != live: listed, flagged
              z]
    payloads = [payload_of(good)] + [None] * 10 + [payload_of(good)] * 2
    res = check_batch(stored, payloads, [2] * 13, want_err={b: EINVAL for b in range(1, 11)})
    assert res.entries_ok.tolist() == [1] + [0] * 11 + [1]


def test_batch_name_too_long_and_truncated(oracle):
    """POM_RD_E_NAME and POM_GC_E_TRUNCATED between ITBs that list."""
    ok = make_record(840, 4, 2, [0, 3])
    long_name = make_record(841, 4, 2, [0, 3], namelens={3: 300})
    short = bytearray(ok[:-1])
    struct.pack_into("<I", short, itb.LEN_OFF, len(short))
    stored = [ok, lzo_record(oracle, long_name), short, lzo_record(oracle, ok)]
    res = check_batch(stored, [payload_of(ok), payload_of(long_name), payload_of(short), payload_of(ok)], [2] * 4)
    assert res.err.tolist() == [0, E_NAME, E_TRUNCATED, 0]


def test_batch_nospace_then_retry(many):
    recs, stored = many
    payloads = [payload_of(r) for r in recs[:40]]
    res = check_batch(stored[:40], payloads, [2] * 40, out_cap=100)
    assert res.rc == E_NOSPACE
    assert check_batch(stored[:40], payloads, [2] * 40, out_cap=int(res.first[40])).rc == 0
    check_batch(stored[:40], payloads, [2] * 40, out_cap=int(res.first[40]) - 1)
    check_batch(stored[:40], payloads, [2] * 40, out_cap=0)


@pytest.fixture(scope="module")
def chunky(oracle):
    """60 records of about 50 KB, every fourth stored uncompressed: several
    chunks under chunk_mb=1."""
    recs = [make_record(900 + i, 20 + 7 * (i % 9), 8, range(0, 20 + 7 * (i % 9), 1 + i % 3)) for i in range(60)]
    return recs, [r if i % 4 == 1 else lzo_record(oracle, r) for i, r in enumerate(recs)]


def test_batch_spans_chunks(chunky, debug_env):
    """chunk_mb=1: about 50 KB a record, so 60 records take several chunks;
    the chunks reorder the blocks (smallest first, LZO before stored) and the
    records still come out in ITB order."""
    recs, stored = chunky
    debug_env("chunk_mb=1")
    check_batch(stored, [payload_of(r) for r in recs], [8] * 60)


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the device's second chunk delivery fails as a failed GPU
    stream would.  The call returns LZO_E_ERROR, every record that went to the
    GPU reads LZO_E_ERROR with live == dnum == 0, a bad header keeps -EINVAL
    and a record with no entries its 0, and the same call succeeds in full
    afterwards (the slots are reusable)."""
    import ctypes
    recs, stored = chunky[0], list(chunky[1])
    stored.insert(30, recs[0][:200])                            # no whole header
    stored.insert(45, make_record(990, 3, 2, [0, 1, 2], entries=0))
    payloads = [payload_of(r) for r in recs]
    payloads.insert(30, None)
    payloads.insert(45, None)
    n = len(stored)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    out = np.zeros(1 << 20, dtype=np.uint8)
    first = np.zeros(n + 1, dtype=np.uint64)
    live, dnum = (np.full(n, 7, dtype=np.uint32) for _ in range(2))
    err, len_ok, entries_ok = (np.full(n, 7, dtype=np.int32) for _ in range(3))
    debug_env("chunk_mb=1,fail_chunk=1")
    rc = readdir._lib().pom_readdir_batch(ptrs, lens, n, out.ctypes.data, out.size, first.ctypes.data,
                                          live.ctypes.data, dnum.ctypes.data, err.ctypes.data, len_ok.ctypes.data,
                                          entries_ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    assert err.tolist() == [EINVAL if b == 30 else 0 if b == 45 else lzo.LZO_E_ERROR for b in range(n)]
    assert not live.any() and not dnum.any()
    debug_env("chunk_mb=1")
    check_batch(stored, payloads, [8] * n, want_err={30: EINVAL, 45: 0})


def test_batch_synth_names(oracle):
    """The bench's own synthetic ITBs (synth.c: names "file-%08x.jpg" of the
    ITE's hash, mode 0100644): the parsed listing names every ITE."""
    recs = [gc_scan_util.make_record(1000 + i, 3 + 5 * i, 8, range(3 + 5 * i)) for i in range(12)]
    stored = [lzo_record(oracle, r) if i % 3 else r for i, r in enumerate(recs)]
    res = check_batch(stored, [payload_of(r) for r in recs], [8] * 12)
    assert res.rc == 0 and (res.err == 0).all() and res.entries_ok.all()
    for b, rec in enumerate(recs):
        got = readdir.parse(res.out[int(res.first[b]): int(res.first[b + 1])])
        want = []
        for nr in range(3 + 5 * b):
            hsh, uuid = struct.unpack_from("<QQ", rec, H + ITE_OFF + ITE_SIZE * nr)
            want.append((uuid, 0o100644, b"file-%08x.jpg" % (hsh >> 32)))
        assert got == want and all(len(w[2]) == 17 for w in want)
