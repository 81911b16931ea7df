"""The record codecs at their edges, on the GPU: the boundary family of
tests/record_util.py through pom_itb_lzo_compress_batch,
pom_xnet_itb_wb_batch, pom_itb_lzo_compress_append_batch,
pom_itb_lzo_decompress_batch, pom_itb_read_lzo_decompress_batch,
pom_xnet_itb_recv_batch, pom_col_zip_batch and pom_col_unzip_batch, each
compared byte for byte and code for code with the restatements there (the
oracle is the reference, nothing has a tolerance).  Every buffer is a guarded
window with its exact capacity handed to the C ABI; every test runs in
batches of 1, 8, 9 (the latency decoder and the LDS encoder up to 8 blocks,
the throughput paths above) and 300 records (the family cycled)."""
from __future__ import annotations

import errno
import os

import pytest

import record_util as ru
from pomegranate_amd import column, itb, lzo, xnet

pytestmark = pytest.mark.gpu
H = ru.H


@pytest.fixture(scope="module")
def fam(oracle):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return ru.family(oracle)


# ---- compress -------------------------------------------------------------------
def _compress_cases(oracle, fam):
    """(name, record, tmp_cap): every record of the family at every capacity."""
    return [(f"{name}@{cap}", rec, cap) for name, rec in fam.records() for cap in ru.tmp_caps(oracle, rec)]


def _check_compress(oracle, batch, ins, tmps, which, err):
    """What every compress entry point leaves behind; returns the expected
    (err, record bytes as sent or stored) per case."""
    sent = []
    for i, (name, rec, cap) in enumerate(batch):
        ew, eerr, ebytes = ru.expected_compress(oracle, rec, cap)
        assert (which[i], err[i]) == (ew, eerr), name
        assert ins.get(i) == rec, f"{name}: in[b] changed"
        if ebytes is not None:
            oi = tmps if ew else ins
            assert oi.get(i, 0, len(ebytes)) == ebytes, f"{name}: oi[b]"
        if cap < H:
            assert tmps.untouched(i), f"{name}: tmp[b] written below the header size"
        elif not ew and cap < H + lzo.worst_compress(max(len(rec), H) - H):
            assert tmps.untouched(i, H), f"{name}: tmp[b] written past the header of a kept record"
        ln = itb.header_fields(rec)[0]
        sent.append((eerr, ebytes if ebytes is not None else rec[:ln]))
    return sent


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_compress_at_every_tie_and_capacity(oracle, fam, bs):
    for batch in ru.batches(_compress_cases(oracle, fam), bs):
        ins = ru.guarded_with([rec for _, rec, _ in batch])
        caps = [cap for _, _, cap in batch]
        tmps = ru.Guarded(caps)
        which, err = ru.call_compress(ins, tmps, caps)
        _check_compress(oracle, batch, ins, tmps, which, err)


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_writeback_frames_carry_the_expected_records(oracle, fam, bs):
    """pom_xnet_itb_wb_batch: one REQ per record with the record the restatement
    expects (the original on -EINVAL, as txg_wb_itb sends it), at a wire of
    exactly the bytes needed; one byte less is -ENOSPC with wire_len at the
    last whole frame."""
    for batch in ru.batches(_compress_cases(oracle, fam), bs):
        caps = [cap for _, _, cap in batch]
        dests = [(0x200 + i % 3, 40 + i) for i in range(len(batch))]
        want = [ru.expected_compress(oracle, rec, cap) for _, rec, cap in batch]
        data = [w[2] if w[2] is not None else rec[:itb.header_fields(rec)[0]]
                for w, (_, rec, _) in zip(want, batch)]
        need = sum(xnet.TX_SIZE + len(d) for d in data)
        first = None
        for room in (need, need - 1):
            ins = ru.guarded_with([rec for _, rec, _ in batch])
            tmps = ru.Guarded(caps)
            wire = ru.Guarded([room])
            rc, wl, err = ru.call_wb(ins, tmps, caps, dests, 0x11, 77, 2, wire)
            assert err == [w[1] for w in want]
            assert all(ins.get(i) == rec for i, (_, rec, _) in enumerate(batch))
            if room == need:
                assert (rc, wl) == (0, need)
                at = 0
                for i, d in enumerate(data):
                    t = xnet.Tx.from_buffer_copy(wire.get(0, at, at + xnet.TX_SIZE))
                    assert (t.type, t.flag, t.cmd, t.arg0, t.arg1, t.reserved) == (
                        xnet.MSG_REQ, 0, xnet.MDS2MDSL_WBTXG, xnet.WBTXG_ITB, 77, dests[i][1]), batch[i][0]
                    assert (t.ssite_id, t.dsite_id, t.magic, t.len) == (0x11, dests[i][0], 2, len(d)), batch[i][0]
                    at += xnet.TX_SIZE
                    assert wire.get(0, at, at + len(d)) == d, batch[i][0]
                    at += len(d)
                first = wire.get(0)
            else:
                whole = need - xnet.TX_SIZE - len(data[-1])
                assert (rc, wl) == (-errno.ENOSPC, whole)
                assert wire.get(0, 0, whole) == first[:whole]


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_compress_append_holds_the_expected_records(oracle, fam, bs, tmp_path):
    """pom_itb_lzo_compress_append_batch: the same records, each in the file at
    locations[b]; a record with h.len below the header is not written."""
    path = str(tmp_path / "rules.itb")
    af = itb.AppendFile(path, win=1 << 16)          # small windows: the batches cross several
    stored = []
    for batch in ru.batches(_compress_cases(oracle, fam), bs):
        ins = ru.guarded_with([rec for _, rec, _ in batch])
        caps = [cap for _, _, cap in batch]
        tmps = ru.Guarded(caps)
        which, err, locs = ru.call_compress_append(ins, tmps, caps, af)
        sent = _check_compress(oracle, batch, ins, tmps, which, err)
        for (name, _, _), (eerr, data), loc in zip(batch, sent, locs):
            if eerr == -errno.EINVAL:
                assert loc == ru.NO_LOCATION, name
            else:
                stored.append((name, loc, data))
    af.close()
    assert os.path.getsize(path) == sum(len(d) for _, _, d in stored)
    with open(path, "rb") as f:
        image = f.read()
    spans = sorted((loc, loc + len(d)) for _, loc, d in stored)
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    for name, loc, d in stored:
        assert image[loc:loc + len(d)] == d, name


# ---- decompress -------------------------------------------------------------------
def _decode_cases(fam):
    """(stream, cap) at every capacity of the family, every case that is not a
    clean decode standing between two that are."""
    cases = [(s, cap) for s in fam.streams for cap in ru.decode_caps(s.out_len)]
    clean = [c for c in cases if not c[0].damaged and c[1] >= H + c[0].out_len]
    other = [c for c in cases if not (not c[0].damaged and c[1] >= H + c[0].out_len)]
    return ru.interleave(clean, other)


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_decompress_in_place_back_to_back(oracle, fam, bs):
    """The records back to back in one arena: a record's output capacity ends
    where the next header begins, and the neighbours of a damaged or too
    large record still decode bit for bit."""
    for batch in ru.batches(_decode_cases(fam), bs):
        caps = [cap for _, cap in batch]
        arena = ru.guarded_with([s.rec for s, _ in batch], [max(len(s.rec), cap) for s, cap in batch], packed=True)
        err, ok = ru.call_decompress(arena, caps)
        for i, (s, cap) in enumerate(batch):
            eerr, eok, _, out = ru.expected_decompress(oracle, s.rec, cap)
            what = f"{s.name}@{cap}"
            assert (err[i], ok[i]) == (eerr, eok), what
            assert arena.get(i, 0, H) == ru.decoded_header(s.rec, len(out)), f"{what}: header"
            assert arena.get(i, H, H + len(out)) == out, f"{what}: payload"
            if len(s.rec) > cap:                    # the stream's bytes past the capacity stay
                assert arena.get(i, cap) == s.rec[cap:], f"{what}: written past cap"


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_read_decompress_from_a_file(oracle, fam, bs, tmp_path):
    """pom_itb_read_lzo_decompress_batch on the same records, stored back to
    back in a file (plus uncompressed ones): err, derr, len_ok, len and the
    record in the buffer."""
    raw = [(ru.Stream("raw_" + name, rec, None, 0, False), len(rec) + dc)
           for name, rec in fam.records()[:-1][::5] for dc in (-1, 0)]
    cases = _decode_cases(fam) + raw
    path = str(tmp_path / "stored.itb")
    image = bytearray()
    at = {}
    for s, _ in cases:
        if s.name not in at:
            at[s.name] = len(image)
            image += s.rec
    with open(path, "wb") as f:
        f.write(image)
    fd = os.open(path, os.O_RDONLY)
    try:
        for batch in ru.batches(cases, bs):
            bufs = ru.Guarded([cap for _, cap in batch], packed=True)
            lens, err, derr, ok = ru.call_read_decompress(fd, [at[s.name] for s, _ in batch], bufs)
            for i, (s, cap) in enumerate(batch):
                eerr, ederr, eok, elen, ebytes = ru.expected_read(oracle, s.rec, cap)
                what = f"{s.name}@{cap}"
                assert (err[i], derr[i], ok[i], lens[i]) == (eerr, ederr, eok, elen), what
                if ebytes is not None:
                    assert bufs.get(i, 0, len(ebytes)) == ebytes, what
    finally:
        os.close(fd)


# ---- xnet receive -------------------------------------------------------------------
def _frames(fam):
    by = {s.name: s.rec for s in fam.streams}
    small = dict(fam.small)
    F = ru.WireFrame
    return [F("lzo_itb", by["ok_itb"]), F("raw_random40", small["random40"]),
            F("dropped", by["ok_itb"], dropped=True), F("raw_itb", fam.itb_rec),
            F("tx.len=h.len-1", by["ok_itb"][:-1]), F("trail1", by["trail1"]),
            F("tx.len=h.len+1", by["ok_itb"] + b"\x00"), F("lzo_tie1000-2", by["ok_tie1000-2"]),
            F("tx.len=100", fam.short_rec[:100]), F("lookbehind", by["lookbehind"]),
            F("tx.len=263", by["ok_itb"][:263]), F("lzo_zeros40", by["ok_zeros40"]),
            F("cut3", by["cut3"]), F("raw_tie300+0", fam.ties[(300, 0)]), F("zlen+1", by["zlen+1"]),
            F("empty", by["empty"]), F("lzo_tie12416-1", by["ok_tie12416-1"]),
            F("dropped_raw", small["zeros1"], dropped=True), F("raw_zeros0", small["zeros0"])]


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_xnet_receive_mixed_frames(oracle, fam, bs):
    """LZO, uncompressed, dropped, tx.len != h.len, tx.len < 264 and tx.len >
    itb_cap frames in one batch, their data wherever the 72-byte headers put
    it, at the ITB capacities around the one-ITE ITB's size: at one byte less
    the LZO records that decode to it are -EFAULT, the uncompressed one -EIO."""
    for itb_cap in ru.decode_caps(itb.PAYLOAD_MIN):
        for batch in ru.batches(_frames(fam), bs):
            wire, offs = ru.build_wire(batch)
            bufs = ru.Guarded([itb_cap] * len(batch))
            err = ru.call_recv(wire, batch, offs, bufs, itb_cap)
            for i, f in enumerate(batch):
                eerr, ebytes = ru.expected_recv(oracle, f, itb_cap)
                what = f"{f.name}@{itb_cap}"
                assert err[i] == eerr, what
                if ebytes is not None:
                    assert bufs.get(i, 0, len(ebytes)) == ebytes, what
    # the claims of the docstring, from the restatement
    lzo_itb = _frames(fam)[0]
    assert ru.expected_recv(oracle, lzo_itb, H + itb.PAYLOAD_MIN - 1)[0] == -errno.EFAULT
    assert ru.expected_recv(oracle, ru.WireFrame("raw", fam.itb_rec), H + itb.PAYLOAD_MIN - 1)[0] == -errno.EIO


# ---- column -------------------------------------------------------------------------
def _column_cases(oracle, fam):
    """(name, column, zip_cap)."""
    zc = len(ru.ocompress(oracle, fam.col_comp))
    cases = []
    for d, c in sorted(fam.col_ties.items()):
        z = len(ru.ocompress(oracle, c))
        cases += [(f"tie{d:+d}@bound", c, column.zip_bound(len(c))), (f"tie{d:+d}@fit", c, 8 + z),
                  (f"tie{d:+d}@fit-1", c, 8 + z - 1)]
    cases += [("comp@bound", fam.col_comp, column.zip_bound(len(fam.col_comp))),
              ("comp@fit", fam.col_comp, 8 + zc), ("comp@fit-1", fam.col_comp, 8 + zc - 1),
              ("comp@8", fam.col_comp, 8), ("comp@0", fam.col_comp, 0)]
    for name, rec in fam.small:
        cases.append((f"{name}@bound", rec[H:], column.zip_bound(len(rec) - H)))
    return cases


@pytest.mark.parametrize("bs", ru.BATCH_SIZES)
def test_column_zip_ties_and_capacity(oracle, fam, bs):
    """len(zc) + 8 >= len(c) means raw; a column that compresses is written at
    zip_cap = 8 + len(zc) and goes raw, with nothing written, one byte below;
    the compressed ones unzip to the original in a buffer of exactly its size."""
    for batch in ru.batches(_column_cases(oracle, fam), bs):
        cols = ru.guarded_with([c for _, c, _ in batch])
        zips = ru.Guarded([cap for _, _, cap in batch])
        zl, comp = ru.call_col_zip(cols, zips)
        back = []
        for i, (name, c, cap) in enumerate(batch):
            ecomp, ebytes = ru.expected_col_zip(oracle, c, cap)
            assert (comp[i], zl[i]) == (ecomp, len(ebytes)), name
            assert cols.get(i) == c, f"{name}: column changed"
            if ecomp:
                assert zips.get(i, 0, zl[i]) == ebytes, name
                back.append((name, c, ebytes))
            elif cap < column.zip_bound(len(c)):
                assert zips.untouched(i), f"{name}: raw, yet zip[b] written"
        if back:
            zz = ru.guarded_with([z for _, _, z in back])
            outs = ru.Guarded([len(c) for _, c, _ in back])
            ol, err = ru.call_col_unzip(zz, outs)
            for i, (name, c, _) in enumerate(back):
                assert (ol[i], err[i]) == (len(c), 0) and outs.get(i) == c, name
    by = {name: (c, cap) for name, c, cap in _column_cases(oracle, fam)}
    assert ru.expected_col_zip(oracle, *by["comp@fit"])[0] == 1
    assert ru.expected_col_zip(oracle, *by["comp@fit-1"])[0] == 0
    assert [ru.expected_col_zip(oracle, *by[f"tie{d:+d}@bound"])[0] for d in (1, 0, -1)] == [0, 0, 1]
