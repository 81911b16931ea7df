"""The record codecs' boundary family and its tools, without a GPU: the family
(tests/record_util.py) holds what it claims, the oracle gives every damaged
stream the code the family names, the restatements flip where the rules say,
the guarded buffers notice a stray byte, and the stand-alone checker of
pomegranate_amd/csrc/itb_rules.h passes under the sanitizers."""
from __future__ import annotations

import errno
import os
import struct
import subprocess

import pytest

import record_util as ru
from conftest import ROOT
from pomegranate_amd import itb, lzo

H = ru.H
NATIVE = os.path.join(ROOT, "tests", "native")
CHECK = os.path.join(NATIVE, "itb_rules_check")


@pytest.fixture(scope="module")
def fam(oracle):
    return ru.family(oracle)


def _diff(oracle, rec):
    ln = itb.header_fields(rec)[0]
    return len(oracle.compress(bytes(rec[H:ln]))) - (ln - H)


def test_small_payloads(oracle, fam):
    """Payload sizes 0, 1, 13, 14, 15 and 40, random and zero bytes: the
    encoder's n <= 13 branch and the first sizes that parse."""
    sizes = sorted(itb.header_fields(r)[0] - H for _, r in fam.small)
    assert sizes == sorted(list(ru.SMALL_SIZES) * 2)
    for name, rec in fam.small:
        ln, zlen, algo = itb.header_fields(rec)
        assert len(rec) == ln and zlen == 0 and algo == itb.COMPR_NONE, name
    # 40 zero bytes are the one member that compresses; all else is kept
    kept = {name: _diff(oracle, rec) >= 0 for name, rec in fam.small}
    assert [n for n, k in kept.items() if not k] == ["zeros40"]


def test_ties_are_all_there(oracle, fam):
    """Every difference at every size, measured with the oracle itself, and
    nothing else in the family."""
    assert set(fam.ties) == {(n, d) for n in ru.TIE_SIZES for d in ru.TIE_DIFFS}
    for (n, d), rec in fam.ties.items():
        assert itb.header_fields(rec) == (H + n, 0, itb.COMPR_NONE) and len(rec) == H + n
        assert _diff(oracle, rec) == d, (n, d)
    assert set(fam.col_ties) == set(ru.COL_TIE_DIFFS)
    for d, c in fam.col_ties.items():
        assert len(c) == ru.COL_TIE_SIZE and len(oracle.compress(c)) + 8 - len(c) == d
    assert len(oracle.compress(fam.col_comp)) + 8 < len(fam.col_comp)


def test_real_itb_and_short_record(oracle, fam):
    ln, zlen, algo = itb.header_fields(fam.itb_rec)
    assert ln == H + itb.PAYLOAD_MIN == len(fam.itb_rec) and algo == itb.COMPR_NONE     # one ITE
    assert _diff(oracle, fam.itb_rec) < 0
    assert itb.header_fields(fam.short_rec)[0] < H
    names = [n for n, _ in fam.records()]
    assert len(names) == len(set(names)) == 2 * len(ru.SMALL_SIZES) + len(fam.ties) + 2


# the oracle's code for every damaged stream, with room to spare: the ones the
# family names, and the oracle's own for the cuts and the empty stream
STREAM_CODES = {
    "cut1": lzo.LZO_E_INPUT_OVERRUN,            # the end marker's last byte is gone
    "cut3": lzo.LZO_E_EOF_NOT_FOUND,            # the stream ends where the marker began
    "cut5": lzo.LZO_E_EOF_NOT_FOUND,
    "trail1": lzo.LZO_E_INPUT_NOT_CONSUMED,
    "trail4": lzo.LZO_E_INPUT_NOT_CONSUMED,
    "lookbehind": lzo.LZO_E_LOOKBEHIND_OVERRUN,
    "zlen+1": lzo.LZO_E_OK,
    "zlen-1": lzo.LZO_E_OK,
    "empty": lzo.LZO_E_EOF_NOT_FOUND,
}


def test_streams_are_what_they_claim(oracle, fam):
    by_name = {s.name: s for s in fam.streams}
    assert len(by_name) == len(fam.streams)
    good = [s for s in fam.streams if not s.damaged]
    assert {s.name for s in fam.streams if s.damaged} == set(STREAM_CODES)
    assert len(good) == 2 + 2 * len(ru.TIE_SIZES)
    for s in good:
        ln, zlen, algo = itb.header_fields(s.rec)
        assert len(s.rec) == ln and algo == itb.COMPR_LZO and zlen == H + s.out_len, s.name
        assert s.code == 0
        err, ok, hdr, out = ru.expected_decompress(oracle, s.rec, H + s.out_len)
        assert (err, ok, hdr) == (0, 1, (zlen, zlen, itb.COMPR_NONE)), s.name
    for name, code in STREAM_CODES.items():
        s = by_name[name]
        ln = itb.header_fields(s.rec)[0]
        rc, out = oracle.decompress_safe(s.rec[H:max(ln, H)], ru.AMPLE)
        assert rc == code == s.code and len(out) == s.out_len, name
        assert len(s.rec) == max(ln, H)
    base = by_name["ok_itb"]
    whole = oracle.decompress_safe(base.rec[H:], ru.AMPLE)[1]
    assert whole == fam.itb_rec[H:]
    bl, bz, _ = itb.header_fields(base.rec)
    for k in (1, 3, 5):
        s = by_name[f"cut{k}"]
        assert itb.header_fields(s.rec)[0] == bl - k and s.rec[H:] == base.rec[H:bl - k]
    for k in (1, 4):                                # the whole output, then bytes left over
        s = by_name[f"trail{k}"]
        assert itb.header_fields(s.rec)[0] == bl + k and s.rec[H:bl] == base.rec[H:]
        assert oracle.decompress_safe(s.rec[H:], ru.AMPLE)[1] == whole
    lb = by_name["lookbehind"]                      # one match patched, nothing else
    changed = [i for i in range(len(base.rec)) if lb.rec[i] != base.rec[i]]
    assert len(lb.rec) == len(base.rec) and 1 <= len(changed) <= 2 and changed[-1] - changed[0] <= 1
    assert 0 < lb.out_len < len(whole)
    for name, dz in (("zlen+1", 1), ("zlen-1", -1)):
        s = by_name[name]
        assert itb.header_fields(s.rec) == (bl, bz + dz, itb.COMPR_LZO) and s.rec[H:] == base.rec[H:]
        assert ru.expected_decompress(oracle, s.rec, H + s.out_len)[:2] == (0, 0)
    assert itb.header_fields(by_name["empty"].rec)[::2] == (H, itb.COMPR_LZO)


def test_compress_restatement_flips_at_the_capacity(oracle, fam):
    """Kept below 264 + stream, compressed from there on; kept at every
    capacity when the stream is not smaller than the payload."""
    for name, rec in fam.records():
        ln = itb.header_fields(rec)[0]
        caps = ru.tmp_caps(oracle, rec)
        assert len(caps) == 8 and caps[:3] == [0, 263, 264] and caps[-1] == itb.ITB_FULL
        if ln < H:
            assert all(ru.expected_compress(oracle, rec, c) == (0, -errno.EINVAL, None) for c in caps)
            continue
        d = _diff(oracle, rec)
        dlen = ln - H + d
        for c in caps + [H + dlen + 1]:
            which, err, out = ru.expected_compress(oracle, rec, c)
            assert err == 0 and which == int(d < 0 and c >= H + dlen), (name, c)
            if which:
                assert itb.header_fields(out) == (H + dlen, ln, itb.COMPR_LZO) and len(out) == H + dlen
                assert out[H:] == oracle.compress(rec[H:]) and out[:itb.LEN_OFF] == rec[:itb.LEN_OFF]
            else:
                assert out == rec


def test_decode_restatement_at_the_capacity(oracle, fam):
    s = next(s for s in fam.streams if s.name == "ok_itb")
    assert ru.decode_caps(s.out_len) == [H, H + s.out_len - 1, H + s.out_len, H + s.out_len + 1]
    assert ru.decode_caps(0) == [H, H + 1]
    for cap in ru.decode_caps(s.out_len):
        err, ok, (ln, _, algo), out = ru.expected_decompress(oracle, s.rec, cap)
        fits = cap >= H + s.out_len
        assert err == (0 if fits else lzo.LZO_E_OUTPUT_OVERRUN) and ok == int(fits)
        assert ln == H + len(out) <= cap and algo == itb.COMPR_NONE
        assert out == fam.itb_rec[H:H + len(out)]
        rerr, derr, rok, rlen, rbytes = ru.expected_read(oracle, s.rec, cap)
        if cap < len(s.rec):
            assert (rerr, derr, rok, rlen, rbytes) == (-errno.EINVAL, 0, 0, 0, None)
        else:
            assert (rerr, derr, rok, rlen) == (0, err, ok, ln) and rbytes[H:] == out
    assert ru.expected_read(oracle, fam.itb_rec, len(fam.itb_rec)) == (0, 0, 1, len(fam.itb_rec), fam.itb_rec)


def test_recv_restatement(oracle, fam):
    s = next(s for s in fam.streams if s.name == "ok_itb")
    cap = H + s.out_len
    f = ru.WireFrame("lzo", s.rec)
    assert ru.expected_recv(oracle, f, cap) == (0, ru.decoded_header(s.rec, s.out_len) + fam.itb_rec[H:])
    assert ru.expected_recv(oracle, f, cap - 1)[0] == -errno.EFAULT
    assert ru.expected_recv(oracle, f, len(s.rec) - 1) == (-errno.EIO, None)
    assert ru.expected_recv(oracle, ru.WireFrame("d", s.rec, dropped=True), cap) == (-errno.EBADMSG, None)
    assert ru.expected_recv(oracle, ru.WireFrame("cutframe", s.rec[:-1]), cap) == (-errno.EIO, None)
    assert ru.expected_recv(oracle, ru.WireFrame("short", s.rec[:100]), cap) == (-errno.EIO, None)
    assert ru.expected_recv(oracle, ru.WireFrame("raw", fam.itb_rec), cap) == (0, fam.itb_rec)


def test_column_restatement(oracle, fam):
    for d, c in fam.col_ties.items():               # len(zc) + 8 >= len(c) means raw
        comp, z = ru.expected_col_zip(oracle, c, 1 << 20)
        assert comp == int(d < 0) and (z[:8] == struct.pack("<Q", len(c)) if comp else z == b"")
    zc = oracle.compress(fam.col_comp)
    assert ru.expected_col_zip(oracle, fam.col_comp, 8 + len(zc))[0] == 1
    assert ru.expected_col_zip(oracle, fam.col_comp, 8 + len(zc) - 1) == (0, b"")


def test_guards_notice_a_stray_byte():
    for packed in (False, True):
        g = ru.Guarded([5, 0, 300], packed=packed)
        g.check()
        assert all(g.untouched(i) for i in range(3))
        assert g.off[1] - (g.off[0] + 5) == (0 if packed else ru.GUARD)
        g.put(0, b"abcde")
        g.put(2, b"x", at=299)
        g.check()
        assert g.get(0) == b"abcde" and not g.untouched(2) and g.untouched(2, 0, 299)
        for at in (g.off[0] - 1, g.off[2] + 300, 0, len(g.buf) - 1):
            keep = g.buf[at]
            g.buf[at] = 0
            with pytest.raises(AssertionError):
                g.check()
            g.buf[at] = keep
        g.check()
    assert ru.batches(range(20), 8) == [list(range(8)), list(range(8, 16)), [16, 17, 18, 19]]
    assert [len(b) for b in ru.batches(range(20), 300)] == [300]
    mixed = ru.interleave(["g0", "g1", "g2"], ["b0", "b1"])
    assert mixed == ["g0", "b0", "g1", "b1", "g2"]


def test_receive_without_decoder_through_guarded_buffers(oracle, fam):
    """The frames that need no decoder, through the real library and the
    guarded windows (no GPU work: nothing is LZO), at an ITB capacity of
    exactly the largest record and one byte less."""
    F = ru.WireFrame
    small = dict(fam.small)
    frames = [F("raw_random40", small["random40"]), F("dropped", fam.itb_rec, dropped=True),
              F("raw_itb", fam.itb_rec), F("tx.len=h.len-1", fam.itb_rec[:-1]),
              F("tx.len=h.len+1", small["zeros15"] + b"\x00"), F("tx.len=100", fam.short_rec[:100]),
              F("tx.len=263", fam.itb_rec[:263]), F("raw_zeros0", small["zeros0"])]
    for itb_cap in (len(fam.itb_rec), len(fam.itb_rec) - 1, H):
        wire, offs = ru.build_wire(frames)
        assert any(o % 8 for o in offs)             # the data is not aligned
        bufs = ru.Guarded([itb_cap] * len(frames))
        err = ru.call_recv(wire, frames, offs, bufs, itb_cap)
        want = [ru.expected_recv(oracle, f, itb_cap) for f in frames]
        assert err == [w[0] for w in want]
        for i, (e, data) in enumerate(want):
            if data is not None:
                assert bufs.get(i, 0, len(data)) == data
            else:
                assert bufs.untouched(i)
    assert [w[0] for w in want] == [-errno.EIO, -errno.EBADMSG] + [-errno.EIO] * 5 + [0]


def test_rules_checker_exits_0():
    """tests/native/itb_rules_check: both finish functions of itb_rules.h over
    the family's sizes, ties and capacities, every buffer a heap block of
    exactly its capacity, under ASan and UBSan where they link (a stand-alone
    program)."""
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", NATIVE, "-f", "itb_rules.mk"], check=True)
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_rules_check: ok" in r.stdout
