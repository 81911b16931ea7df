"""GPU: the key/value table listing (include/pom_kvlist.h) against the Python
restatement of mds/itb.c:2478-2534 in kvlist_util.py -- pom_kvlist_dev on
guarded arenas, pom_kvlist_batch through the host chunk pipeline.  Every
comparison is byte-exact."""
from __future__ import annotations

import struct

import numpy as np
import pytest

import kvlist_util as U
from gpu_util import guarded_batch
from kvlist_util import (EINVAL, E_KEY, E_NAME, E_NOSPACE, E_TRUNCATED, ITE_OFF, ITE_SIZE, KV_NORMAL, KV_STR, OP_GREP,
                         OP_GREP_CNT, OP_SCAN, OP_SCAN_CNT, expect_batch, listing, lzo_record, make_record, payload_of)
from pomegranate_amd import itb, kvlist, lzo

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


# ---------------------------------------------------------------------------
# pom_kvlist_dev on guarded arenas
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scan_cases():
    return U.scan_cases()


def by_name(cases, *names):
    return [next(c for c in cases if c[0] == n) for n in names]


_listing_cache = {}


def expect(cases, op, needle, status=None):
    """expect_batch with one listing() per distinct (payload, op, needle)."""
    errs, lives, dnums, kbs, masks, first, data = [], [], [], [], [], [0], bytearray()
    for b, (_, p, _, ad) in enumerate(cases):
        if status is not None and status[b]:
            res = (None, 0, 0, 0, [0] * 16, b"")
        else:
            key = (id(p), ad, op if op >= OP_GREP else 0, bytes(needle) if op >= OP_GREP else b"")
            if key not in _listing_cache:
                _listing_cache[key] = (p, listing(p, ad, op, needle))       # (p kept alive: its id stays its own)
            res = _listing_cache[key][1]
        errs.append(res[0])
        lives.append(res[1])
        dnums.append(res[2])
        kbs.append(res[3])
        masks.append(res[4])
        data += res[5]
        first.append(len(data))
    return errs, lives, dnums, kbs, np.array(masks, dtype=np.uint64).reshape(-1, 16), \
        np.array(first, dtype=np.uint64), bytes(data)


class Outputs:
    """live, dnum, bytes, keybytes, err, mask, first and out carved out of ONE
    arena of FILL bytes with guard bytes around each, so a stray store shows;
    out starts at residue `oshift` mod 16."""

    def __init__(self, dev, n, room, oshift, with_mask=True):
        self.n = n
        self.sizes = [("live", 4 * n), ("dnum", 4 * n), ("bytes", 4 * n), ("keybytes", 4 * n), ("err", 4 * n),
                      ("mask", 128 * n if with_mask else 0), ("first", 8 * (n + 1)), ("out", room)]
        self.at, pos = {}, 4096
        for name, nbytes in self.sizes:
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
        for name, nbytes in self.sizes:
            o = self.at[name][0]
            changed[o: o + (written_bytes if name == "out" else nbytes)] = False
        bad = np.flatnonzero(changed)
        assert len(bad) == 0, f"{len(bad)} bytes changed outside the outputs, first at arena byte {int(bad[0])}"


def scan_dev_once(dev, cases, shifts, op=OP_SCAN, needle=b"", status=None, cap_of_total=lambda t: t, oshift=0,
                  nshift=0, src=None, with_mask=True):
    if src is None:
        src = guarded_batch(torch, [c[1] for c in cases], dev, shifts, fill=0xEE, neighbours="continuation",
                            continuation=[c[2] for c in cases])
    n = len(cases)
    adepth = torch.tensor([c[3] for c in cases], dtype=torch.uint8, device=dev)
    st = None if status is None else torch.tensor(status, dtype=torch.int32, device=dev)
    # the needle in a guarded arena of its own, at residue nshift, 0xEE around it (no zero byte behind it)
    held = guarded_batch(torch, [bytes(needle)], dev, [nshift], fill=0xEE)
    nd = held.arena[int(held.host_off[0]): int(held.host_off[0]) + len(needle)] if len(needle) else None
    want_err, want_live, want_dnum, want_kb, want_mask, want_first, want = expect(cases, op, needle, status)
    total = int(want_first[n])
    cap = cap_of_total(total)
    out = Outputs(dev, n, total + 64, oshift, with_mask)
    kvlist.scan_dev(src, adepth, op, nd, out.view("live", torch.int32), out.view("dnum", torch.int32),
                    out.view("bytes", torch.int32), out.view("keybytes", torch.int32),
                    out.view("mask", torch.int64) if with_mask else None, out.view("first", torch.int64),
                    out.view("out"), out.view("err", torch.int32), status=st, out_cap=cap, needle_len=len(needle))
    torch.cuda.synchronize()
    out.check_untouched(min(total, cap))            # the poisoned tail behind the cap stays poisoned
    u32 = lambda name: out.view(name, torch.int32).cpu().numpy().view(np.uint32)
    err = out.view("err", torch.int32).cpu().numpy()
    first = out.view("first", torch.int64).cpu().numpy().view(np.uint64)
    got = out.view("out").cpu().numpy()[: min(total, cap)].tobytes()
    want_e = np.array([status[b] if want_err[b] is None else want_err[b] for b in range(n)], dtype=np.int32)
    assert (err == want_e).all(), np.flatnonzero(err != want_e)[:8]
    assert (u32("live") == np.array(want_live, dtype=np.uint32)).all()
    assert (u32("dnum") == np.array(want_dnum, dtype=np.uint32)).all(), np.flatnonzero(u32("dnum") != want_dnum)[:8]
    assert (u32("keybytes") == np.array(want_kb, dtype=np.uint32)).all()
    assert (first == want_first).all()
    assert (u32("bytes") == np.diff(want_first)).all()
    mask = None
    if with_mask:
        mask = out.view("mask", torch.int64).cpu().numpy().view(np.uint64).reshape(n, 16)
        assert (mask == want_mask).all(), np.flatnonzero((mask != want_mask).any(axis=1))[:8]
    assert got == want[: min(total, cap)]
    return err, first, mask


@pytest.mark.parametrize("op,needle,rot", [(OP_SCAN, b"", 0), (OP_SCAN_CNT, b"aB", 5), (OP_GREP, b"aB", 11),
                                           (OP_GREP_CNT, b"zz", 14), (OP_GREP, b"", 7)])
def test_dev_scan_cases(dev, scan_cases, op, needle, rot):
    """Bitmaps, adepths, kinds, states, keys, lengths, errors and truncation
    under every op, each payload at a residue of its own."""
    shifts = [(b + rot) % 16 for b in range(len(scan_cases))]
    err, first, _ = scan_dev_once(dev, scan_cases, shifts, op, needle, oshift=(3 * rot + 1) % 16, nshift=rot % 8)
    e = {c[0]: int(err[b]) for b, c in enumerate(scan_cases)}
    assert e["klen 321"] == e[f"klen {1 << 20}"] == e["both errors 0"] == e["both errors 1"] == E_KEY
    assert e["namelen 257"] == E_NAME
    # the cut payloads: the rest of the live ITE lies right behind them and is not read
    assert e["cut ite"] == e["cut byte"] == e["no bitmap"] == E_TRUNCATED
    assert sum(1 for v in e.values() if v) == 8 and e["exact end"] == e["lengths not examined"] == e["states"] == 0
    assert first[-1] > 1000


def test_dev_normal_keys(dev, scan_cases):
    case = by_name(scan_cases, "normal keys")
    _, first, _ = scan_dev_once(dev, case, [9], oshift=2)
    assert int(first[1]) == 4 * 79 + sum(len(str(k - (1 << 64) if k >= 1 << 63 else k)) for k in U.NORMAL_KEYS)


@pytest.mark.parametrize("i", range(len(U.NEEDLES)), ids=lambda i: f"needle{len(U.NEEDLES[i])}-{U.NEEDLES[i][:3].hex()}")
def test_dev_grep_needles(dev, scan_cases, i):
    """Every match position rule 7 names, for every needle of the family, the
    needle at the residues 0 ... 7; the verdicts are the ones the builder meant."""
    needle = U.NEEDLES[i]
    case, want = U.grep_cases(needle)
    cases = [case] + by_name(scan_cases, "kinds", "str klens", "klen 321")
    for op in (OP_GREP, OP_GREP_CNT):
        _, _, mask = scan_dev_once(dev, cases, [(3 * i + b) % 16 for b in range(4)], op, needle, oshift=(5 * i + op) % 16,
                                   nshift=(i + op) % 8)
        assert {nr: bool(int(mask[0, 0]) >> nr & 1) for nr in want} == want


def test_dev_grep_haystacks(dev):
    case = U.haystack_case()
    emitted = {}
    for k, needle in enumerate(U.HAYSTACK_NEEDLES):
        emitted[needle] = int(scan_dev_once(dev, [case], [k % 16], OP_GREP, needle, oshift=k, nshift=k % 8)[2][0, 0])
    assert emitted[b"aab"] == 0b00000011                    # "aaab" restarts; "aaa\0b" ends before the b
    assert emitted[b"\x7f\x80"] == 0b00001000 and emitted[b"\xff"] == 0b01011000
    assert emitted[b"\x80\x01"] == 0 and emitted[b"\xff\x01"] == 0b01000000


def test_dev_grep_adversarial_full_itb(dev, debug_env):
    """320 x 'a' against 159 x 'a' + 'b' on every entry of one full ITB, with
    both forms of the search."""
    case, needle = U.adversarial_case()
    for key in ("", "keys_search=1"):
        if key:
            debug_env(key)
        _, first, _ = scan_dev_once(dev, [case], [4], OP_GREP, needle, nshift=3)
        assert first.tolist() == [0, 0]
    _, first, _ = scan_dev_once(dev, [case], [4], OP_GREP, b"a" * 160, nshift=1)
    assert first[1] == sum(4 + len(str(k)) for k in range(1024))


def test_dev_every_payload_residue_by_every_output_residue(dev, scan_cases):
    """16 payloads at the residues 0 ... 15, rotated against the output's 16
    residues: every pair; the needle moves through its 8."""
    pick = by_name(scan_cases, "kinds", "states", "normal keys", "str klens", "name lens", "adepth1", "adepth6",
                   "adepth7", "cut ite", "cut byte", "exact end", "bit63", "lengths not examined", "klen 321",
                   "namelen 257") + [U.grep_cases(b"ab")[0]]
    assert len(pick) == 16 and len({((b + 5 * o) % 16, o) for o in range(16) for b in range(16)}) == 256
    for oshift in range(16):
        scan_dev_once(dev, pick, [(b + 5 * oshift) % 16 for b in range(16)], OP_GREP if oshift % 2 else OP_SCAN, b"ab",
                      oshift=oshift, nshift=oshift % 8)


@pytest.mark.parametrize("copy", ["", "keys_copy=1"])
def test_dev_maximum_itb(dev, debug_env, copy):
    """One ITB with all 1,024 entries STR and klen 320: 331,776 bytes, read
    off first[]; with both copy plans."""
    if copy:
        debug_env(copy)
    rec = make_record(470, 1024, 10, range(1024), ites={nr: dict(flags=KV_STR, klen=320) for nr in range(1024)})
    for shift, oshift in ((0, 0), (3, 9)):
        _, first, _ = scan_dev_once(dev, [("max", payload_of(rec), b"", 10)], [shift], oshift=oshift)
        assert first.tolist() == [0, 331776]


def test_dev_per_lane_copy_matches(dev, scan_cases, debug_env):
    debug_env("keys_copy=1")
    cases = by_name(scan_cases, "kinds", "normal keys", "str klens", "name lens", "adepth10")
    scan_dev_once(dev, cases, [1, 6, 11, 0, 13], oshift=7)
    scan_dev_once(dev, cases, [1, 6, 11, 0, 13], cap_of_total=lambda t: t - 3, oshift=2)


def test_dev_empty_itbs_between(dev, scan_cases):
    """ITBs that emit nothing -- an empty bitmap, every entry filtered, an
    error -- between ITBs that do."""
    none = ("none", payload_of(make_record(480, 6, 3, range(6), ites={nr: dict(flags=KV_NORMAL, value=b"q\0")
                                                                      for nr in range(6)})), b"", 3)
    empty, bad, cut = by_name(scan_cases, "empty", "klen 321", "cut ite")
    some = U.grep_cases(b"ab")[0]
    order = [empty, some, none, some, bad, cut, some, empty, empty, some, none]
    _, first, _ = scan_dev_once(dev, order, [(3 * b) % 16 for b in range(len(order))], OP_GREP, b"ab", oshift=5)
    per = np.diff(first)
    assert (per[[0, 2, 4, 5, 7, 8, 10]] == 0).all() and (per[[1, 3, 6, 9]] > 0).all()


def test_dev_status_passes_through(dev, scan_cases):
    status = [0] * len(scan_cases)
    status[1], status[9], status[17] = -6, lzo.LZO_E_INPUT_OVERRUN, -5
    err, first, _ = scan_dev_once(dev, scan_cases, [b % 16 for b in range(len(scan_cases))], status=status, oshift=2)
    assert (err[1], err[9], err[17]) == (-6, lzo.LZO_E_INPUT_OVERRUN, -5)
    assert first[1] == first[2] and first[9] == first[10]


@pytest.mark.parametrize("cap", ["0", "1", "3", "4", "5", "9", "14", "total-1", "total"])
def test_dev_out_cap(dev, scan_cases, cap):
    """Nothing is written at or past out_cap -- the cap cuts a length word (1,
    3), sits at its end (4), cuts the next length word (5), sits between two
    records (9) or cuts a key (14: the third record's key is bytes 13 ... 15;
    and wherever total - 1 falls) -- and first[] is complete anyway."""
    pick = {"total-1": lambda t: t - 1, "total": lambda t: t}.get(cap, lambda t: int(cap))
    cases = by_name(scan_cases, "str klens", "bit64", "normal keys", "name lens", "kinds", "adepth6")
    for oshift in (0, 7):
        scan_dev_once(dev, cases, [(3 * b + 1) % 16 for b in range(len(cases))], cap_of_total=pick, oshift=oshift)


def test_dev_out_cap_inside_a_later_itb(dev, scan_cases):
    """Caps that fall inside the second and the last ITB's records."""
    cases = by_name(scan_cases, "kinds", "str klens", "adepth6", "normal keys")
    _, first, _ = scan_dev_once(dev, cases, [0, 5, 9, 14], oshift=3)
    for cap in (int(first[1]) + 1, int(first[1]) + 4, int(first[2]) - 1, int(first[3]), int(first[3]) + 9):
        scan_dev_once(dev, cases, [0, 5, 9, 14], cap_of_total=lambda t, c=cap: c, oshift=3)


def test_dev_without_a_mask(dev, scan_cases):
    """mask == NULL: the call keeps the masks in memory of its own; the same
    records come out."""
    cases = by_name(scan_cases, "kinds", "odd", "klen 321", "adepth7") + [U.grep_cases(b"abcdefgh")[0]]
    for op in (OP_SCAN, OP_GREP):
        scan_dev_once(dev, cases, [2, 7, 8, 15, 4], op, b"abcdefgh", oshift=6, with_mask=False)


def test_dev_rejects_bad_op_and_needle_length(dev, scan_cases):
    with pytest.raises(RuntimeError):
        scan_dev_once(dev, by_name(scan_cases, "kinds"), [0], op=4)
    src = guarded_batch(torch, [scan_cases[0][1]], dev, [0], fill=0xEE)
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=dev)
    with pytest.raises(RuntimeError):
        kvlist.scan_dev(src, z(1, torch.uint8), OP_GREP, z(256, torch.uint8), z(1), z(1), z(1), z(1), None,
                        z(2, torch.int64), None, z(1), needle_len=256)


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
    cases = [("", payloads[i % 8], b"", 0 if i == 7 else 11 if i == 8191 else 1 + i % 3) for i in range(n)]
    err, first, _ = scan_dev_once(dev, cases, None, OP_GREP, b"Ab", oshift=11, nshift=5, src=src)
    assert err[7] == EINVAL and err[8191] == EINVAL and first[n] > 20000


# ---------------------------------------------------------------------------
# pom_kvlist_batch against the oracle
# ---------------------------------------------------------------------------
def check_batch(records, payloads, adepths, op=OP_SCAN, needle=b"", want_err=None, **kw):
    """payloads[b]: what the walk sees (None: the ITB yields nothing and its
    err is want_err[b])."""
    res = kvlist.scan_batch(records, op, needle, **kw)
    errs, lives, dnums, kbs, masks, first, data = expect_batch(payloads, adepths, op, needle)
    n = len(records)
    for b in range(n):
        e = want_err[b] if errs[b] is None else errs[b]
        assert (int(res.err[b]), int(res.live[b]), int(res.dnum[b]), int(res.keybytes[b])) == \
            (e, lives[b], dnums[b], kbs[b]), b
    assert (res.first == first).all()
    if res.mask is not None:
        assert (res.mask == masks).all()
    if kw.get("count_only"):
        assert res.rc == 0 and res.out.size == 0
        return res
    cap = kw.get("out_cap")
    fit = int(first[n]) if cap is None else min(int(first[n]), cap)
    assert res.rc == (E_NOSPACE if fit < int(first[n]) else 0)
    assert res.out.tobytes() == data[:fit]
    return res


@pytest.mark.parametrize("op,needle", [(OP_SCAN, b""), (OP_SCAN_CNT, b"x"), (OP_GREP, b"aB"), (OP_GREP_CNT, b"Ab")])
def test_batch_mixed_lzo_none_and_no_entries(oracle, op, needle):
    """COMPR_LZO, COMPR_NONE and h.entries == 0 records side by side under all
    four ops; a record with no entries is not walked, whatever its bitmap
    says.  hmr->len and hmr->dnum rebuilt from the counts as the header says."""
    recs = [make_record(510 + i, n, ad, bits) for i, (n, ad, bits) in
            enumerate([(4, 2, [0, 3]), (70, 10, [0, 64, 69]), (9, 4, [1, 2, 8]), (5, 3, [0, 1]), (6, 3, range(6))])]
    idle = make_record(520, 3, 2, [0, 1, 2], entries=0)
    stored = [recs[0], lzo_record(oracle, recs[1]), idle, recs[2], lzo_record(oracle, idle), lzo_record(oracle, recs[3]),
              recs[4]]
    payloads = [payload_of(recs[0]), payload_of(recs[1]), None, payload_of(recs[2]), None, payload_of(recs[3]),
                payload_of(recs[4])]
    res = check_batch(stored, payloads, [2, 10, 2, 4, 2, 3, 3], op, needle, want_err={2: 0, 4: 0})
    assert res.len_ok.tolist() == [1, 1, 0, 1, 0, 1, 1] and res.entries_ok.tolist() == [1] * 7
    assert res.first[2] == res.first[3] and res.first[4] == res.first[5]
    for b, rec in ((1, recs[1]), (6, recs[4])):
        entries = struct.unpack_from("<i", rec, 4)[0]
        # mds/itb.c:2478-2494 over the payload itself: 4 a live entry and its key's length
        scan = listing(payload_of(rec), rec[3], OP_SCAN)
        assert entries == int(res.live[b]) == scan[2]
        assert 4 * entries + int(res.keybytes[b]) == len(scan[5])           # hmr->len
        assert int(res.first[b + 1] - res.first[b]) <= 4 * entries + int(res.keybytes[b])
        assert int(res.dnum[b]) <= entries                                  # hmr->dnum = h.entries


@pytest.fixture(scope="module")
def many(oracle):
    """700 LZO ITBs of 1 ... 4 ITEs: more than two per CU, so the chunk's decode
    takes the op-set decoder."""
    recs = [make_record(600 + i, 1 + i % 4, 2, range(1 + i % 4)) for i in range(700)]
    return recs, [lzo_record(oracle, r) for r in recs]


def test_batch_700_small(many):
    recs, stored = many
    payloads = [payload_of(r) for r in recs]
    res = check_batch(stored, payloads, [2] * 700)
    assert res.len_ok.all() and res.entries_ok.all() and res.first[700] > 700 * 4
    check_batch(stored, payloads, [2] * 700, OP_GREP, b"a")


def test_batch_count_only_and_masks(many):
    """out == NULL: 0, every count and first[] complete, no record; mask ==
    NULL against mask given: the same records."""
    recs, stored = many
    payloads = [payload_of(r) for r in recs[:90]]
    for op, needle in ((OP_SCAN_CNT, b""), (OP_GREP_CNT, b"B")):
        full = check_batch(stored[:90], payloads, [2] * 90, op, needle)
        cnt = check_batch(stored[:90], payloads, [2] * 90, op, needle, count_only=True)
        bare = check_batch(stored[:90], payloads, [2] * 90, op, needle, want_mask=False)
        assert bare.mask is None and bare.out.tobytes() == full.out.tobytes() and cnt.first[90] == full.first[90] > 0
        check_batch(stored[:90], payloads, [2] * 90, op, needle, count_only=True, want_mask=False)


def test_batch_full_itb(oracle):
    rec = make_record(800, 1024, 10, range(1024))
    res = check_batch([lzo_record(oracle, rec)], [payload_of(rec)], [10], OP_GREP, b"bA")
    assert int(res.live[0]) == 1024 and 0 < int(res.dnum[0]) < 1024


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
    assert not res.mask[2].any()


def test_batch_wrong_zlen(oracle):
    """zlen one too large: the decode is short of it (len_ok 0) and the ITB is
    listed from what was produced; one too small: the decoder's overrun code."""
    recs = [make_record(820 + i, 5, 3, range(5)) for i in range(3)]
    small = lzo_record(oracle, recs[1], zlen_delta=-1)
    rc, _ = oracle.decompress_safe(bytes(small[H:]), itb.header_fields(small)[1] - H)
    assert rc == lzo.LZO_E_OUTPUT_OVERRUN
    stored = [lzo_record(oracle, recs[0], zlen_delta=1), small, lzo_record(oracle, recs[2])]
    res = check_batch(stored, [payload_of(recs[0]), None, payload_of(recs[2])], [3] * 3, OP_GREP, b"a", want_err={1: rc})
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


def test_batch_key_errors_and_truncated(oracle):
    """POM_KV_E_KEY, POM_RD_E_NAME and POM_GC_E_TRUNCATED between ITBs that list."""
    ok = make_record(840, 4, 2, [0, 3])
    long_key = make_record(841, 4, 2, [0, 3], ites={3: dict(flags=KV_STR, klen=321)})
    long_name = make_record(842, 4, 2, [0, 3], ites={0: dict(flags=0, namelen=300)})
    short = bytearray(ok[:-1])
    struct.pack_into("<I", short, itb.LEN_OFF, len(short))
    stored = [ok, lzo_record(oracle, long_key), short, long_name, lzo_record(oracle, ok)]
    res = check_batch(stored, [payload_of(r) for r in (ok, long_key, short, long_name, ok)], [2] * 5, OP_GREP, b"")
    assert res.err.tolist() == [0, E_KEY, E_TRUNCATED, E_NAME, 0]


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
    records, the masks and the needle still arrive where they belong."""
    recs, stored = chunky
    debug_env("chunk_mb=1")
    payloads = [payload_of(r) for r in recs]
    check_batch(stored, payloads, [8] * 60)
    res = check_batch(stored, payloads, [8] * 60, OP_GREP, b"BB")
    assert 0 < int(res.dnum.sum()) < int(res.live.sum())
    check_batch(stored, payloads, [8] * 60, OP_GREP_CNT, b"BB", count_only=True)


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
    keybytes = np.full(n, 7, dtype=np.uint32)
    mask = np.zeros((n, 16), dtype=np.uint64)
    rc = kvlist._lib().pom_kvlist_batch(ptrs, lens, n, OP_SCAN, None, 0, out.ctypes.data, out.size,
                                        first.ctypes.data, live.ctypes.data, dnum.ctypes.data, keybytes.ctypes.data,
                                        mask.ctypes.data, err.ctypes.data, len_ok.ctypes.data, entries_ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    assert err.tolist() == [EINVAL if b == 30 else 0 if b == 45 else lzo.LZO_E_ERROR for b in range(n)]
    assert not live.any() and not dnum.any()
    debug_env("chunk_mb=1")
    check_batch(stored, payloads, [8] * n, want_err={30: EINVAL, 45: 0})
