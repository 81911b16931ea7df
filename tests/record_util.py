"""The record codecs' rules restated, guarded buffers, and the boundary family
(tests/test_record_rules.py checks the family, tests/test_gpu_record_rules.py
runs it through the library).

The restatements are plain Python over the oracle (tests/conftest.py), after
the reference:
  expected_compress    itb_lzo_compress    mds/itb.c:2904-2945, plus the
                       capacity rule of include/pom_itb.h (a record whose
                       header + stream do not fit tmp_cap is kept, as
                       column_codec.c keeps a column raw)
  expected_decompress  itb_lzo_decompress  mds/itb.c:2949-2980, mdsl/gc.c:755-786
  expected_read        the header-then-payload read, mdsl/storage.c:2507-2640,
                       then expected_decompress (include/pom_itb.h)
  expected_recv        the MDS load path   mds/itb.c:140-168 (include/pom_xnet.h)
  expected_col_zip     hvfs_fwrite SCD_LZO api/api.c:6509-6541

Every buffer the library gets is a window of a larger bytearray with 64 bytes
of 0xC3 on each side (Guarded); the call_* helpers pass explicit capacities to
the C ABI and check the guards after every call.
"""
from __future__ import annotations

import ctypes
import errno
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import lzo_directed as ld
from pomegranate_amd import column, itb, xnet

H = itb.ITBH_SIZE
GUARD = 64
GUARD_BYTE = 0xC3
FILL_BYTE = 0x5A                    # what a window holds before the test writes to it
NO_LOCATION = (1 << 64) - 1

SMALL_SIZES = (0, 1, 13, 14, 15, 40)
TIE_SIZES = (300, 1000, 12416)
TIE_DIFFS = (1, 0, -1, -2)          # len(oracle stream) - len(payload)
COL_TIE_DIFFS = (1, 0, -1)          # len(zc) + 8 - len(c)
COL_TIE_SIZE = 1000
BATCH_SIZES = (1, 8, 9, 300)

_vp = ctypes.c_void_p
_sz = ctypes.c_size_t


# ---- the oracle, remembered ---------------------------------------------------
_zcache: Dict[bytes, bytes] = {}


def ocompress(oracle, payload: bytes) -> bytes:
    z = _zcache.get(payload)
    if z is None:
        z = _zcache[payload] = oracle.compress(payload)
    return z


# ---- restatements ---------------------------------------------------------------
def expected_compress(oracle, rec, tmp_cap: int) -> Tuple[int, int, Optional[bytes]]:
    """itb_lzo_compress into a tmp of tmp_cap bytes: (which: 0 = in kept, 1 = tmp;
    err; the bytes of oi up to its h.len, None with -EINVAL)."""
    ln = itb.header_fields(rec)[0]
    if ln < H:
        return 0, -errno.EINVAL, None
    payload = bytes(rec[H:ln])
    z = ocompress(oracle, payload)
    if len(z) >= len(payload):                      # mds/itb.c:2931: impossible to compress
        return 0, 0, bytes(rec[:ln])
    if H + len(z) > tmp_cap:                        # include/pom_itb.h: no room, kept
        return 0, 0, bytes(rec[:ln])
    hdr = bytearray(rec[:H])
    struct.pack_into("<II", hdr, itb.LEN_OFF, H + len(z), ln)       # :2937-2939
    struct.pack_into("<H", hdr, itb.ALGO_OFF, itb.COMPR_LZO)        # :2940
    return 1, 0, bytes(hdr) + z


def decoded_header(rec, produced: int) -> bytes:
    """The header as itb_lzo_decompress leaves it (mds/itb.c:2975-2978)."""
    hdr = bytearray(rec[:H])
    struct.pack_into("<I", hdr, itb.LEN_OFF, H + produced)
    struct.pack_into("<H", hdr, itb.ALGO_OFF, itb.COMPR_NONE)
    return bytes(hdr)


def expected_decompress(oracle, rec, cap: int):
    """itb_lzo_decompress in a buffer of cap bytes: (err, len_ok, (len, zlen,
    algo), payload bytes produced)."""
    ln, zlen, _ = itb.header_fields(rec)
    payload = bytes(rec[H:max(ln, H)])
    rc, out = oracle.decompress_safe(payload, cap - H)
    return rc, int(rc == 0 and H + len(out) == zlen), (H + len(out), zlen, itb.COMPR_NONE), out


def expected_read(oracle, rec, cap: int):
    """pom_itb_read_lzo_decompress_batch on the stored record: (err, derr, len_ok,
    len, the record's bytes up to len or None)."""
    ln, _, algo = itb.header_fields(rec)
    if ln < H or ln > cap:
        return -errno.EINVAL, 0, 0, 0, None
    if algo != itb.COMPR_LZO:
        return 0, 0, 1, ln, bytes(rec[:ln])
    rc, ok, (nl, _, _), out = expected_decompress(oracle, rec, cap)
    return 0, rc, ok, nl, decoded_header(rec, len(out)) + out


@dataclass
class WireFrame:
    """One message as it stands on the wire: tx.len data bytes."""
    name: str
    data: bytes
    dropped: bool = False

    @property
    def tx_len(self) -> int:
        return len(self.data)


def expected_recv(oracle, frame: WireFrame, itb_cap: int) -> Tuple[int, Optional[bytes]]:
    """pom_xnet_itb_recv_batch for one frame: (err, the bytes the ITB buffer
    starts with, None where include/pom_xnet.h says nothing of the buffer)."""
    n = frame.tx_len
    if frame.dropped:
        return -errno.EBADMSG, None
    if n < H or n > itb_cap:
        return -errno.EIO, None
    ln, _, algo = itb.header_fields(frame.data)
    if ln != n:                                     # the load path's ASSERT
        return -errno.EIO, None
    if algo != itb.COMPR_LZO:
        return 0, bytes(frame.data)
    rc, out = oracle.decompress_safe(frame.data[H:], itb_cap - H)
    return (0 if rc == 0 else -errno.EFAULT), decoded_header(frame.data, len(out)) + out


def expected_col_zip(oracle, c: bytes, zip_cap: int) -> Tuple[int, bytes]:
    """hvfs_fwrite SCD_LZO: raw when len(zc) + 8 >= len(c) (api/api.c:6525-6538),
    or when it does not fit zip_cap (include/pom_column.h)."""
    zc = ocompress(oracle, c)
    if len(zc) + 8 >= len(c) or len(zc) + 8 > zip_cap:
        return 0, b""
    return 1, struct.pack("<Q", len(c)) + zc


# ---- guarded buffers -------------------------------------------------------------
class Guarded:
    """Windows of the given sizes in one bytearray: GUARD bytes of 0xC3 before
    the first, after the last and, unless packed, between neighbours.  A window
    starts out as FILL_BYTE."""

    def __init__(self, sizes: Sequence[int], packed: bool = False):
        self.size = [int(s) for s in sizes]
        self.off = []
        at = GUARD
        for s in self.size:
            self.off.append(at)
            at += s + (0 if packed else GUARD)
        if packed or not self.size:
            at += GUARD
        self.buf = bytearray([GUARD_BYTE]) * at
        self._guards = []
        prev = 0
        for o, s in zip(self.off, self.size):
            if o > prev:
                self._guards.append((prev, o))
            self.buf[o:o + s] = bytes([FILL_BYTE]) * s
            prev = o + s
        self._guards.append((prev, at))
        self._c = (ctypes.c_char * at).from_buffer(self.buf)
        self.base = ctypes.addressof(self._c)

    def __len__(self):
        return len(self.size)

    def addr(self, i: int) -> int:
        return self.base + self.off[i]

    def ptrs(self):
        return (_vp * max(len(self.size), 1))(*[self.addr(i) for i in range(len(self.size))])

    def caps(self):
        return (_sz * max(len(self.size), 1))(*self.size)

    def put(self, i: int, data, at: int = 0) -> None:
        assert at + len(data) <= self.size[i]
        o = self.off[i] + at
        self.buf[o:o + len(data)] = data

    def get(self, i: int, lo: int = 0, hi: Optional[int] = None) -> bytes:
        hi = self.size[i] if hi is None else hi
        assert 0 <= lo <= hi <= self.size[i], (lo, hi, self.size[i])
        return bytes(self.buf[self.off[i] + lo: self.off[i] + hi])

    def untouched(self, i: int, lo: int = 0, hi: Optional[int] = None) -> bool:
        b = self.get(i, lo, hi)
        return b == bytes([FILL_BYTE]) * len(b)

    def index_of(self, address: int) -> int:
        return self.off.index(address - self.base)

    def check(self) -> None:
        for lo, hi in self._guards:
            assert self.buf[lo:hi] == bytes([GUARD_BYTE]) * (hi - lo), f"guard [{lo}, {hi}) written"


def guarded_with(blobs: Sequence[bytes], sizes: Optional[Sequence[int]] = None, packed: bool = False) -> Guarded:
    g = Guarded([len(b) for b in blobs] if sizes is None else sizes, packed)
    for i, b in enumerate(blobs):
        g.put(i, b)
    return g


def _check(*gs: Guarded) -> None:
    for g in gs:
        g.check()


# ---- the C ABI with explicit capacities -------------------------------------------
def call_compress(ins: Guarded, tmps: Guarded, tmp_caps: Sequence[int]):
    """pom_itb_lzo_compress_batch -> (which[b], err[b])."""
    lib = itb._lib()
    n = len(ins)
    pin = ins.ptrs()
    ptmp = tmps.ptrs()
    caps = (_sz * n)(*tmp_caps)
    oi = (_vp * n)()
    err = (ctypes.c_int * n)()
    rc = lib.pom_itb_lzo_compress_batch(pin, ptmp, caps, oi, err, n)
    _check(ins, tmps)
    assert rc == 0, f"pom_itb_lzo_compress_batch: {rc}"
    return [_which(oi[b], pin[b], ptmp[b]) for b in range(n)], list(err)


def _which(oi, pin, ptmp) -> int:
    assert oi in (pin, ptmp), "oi[b] is neither in[b] nor tmp[b]"
    return 0 if oi == pin else 1


def call_compress_append(ins: Guarded, tmps: Guarded, tmp_caps: Sequence[int], af: "itb.AppendFile"):
    """pom_itb_lzo_compress_append_batch -> (which[b], err[b], location[b])."""
    lib = itb._lib()
    n = len(ins)
    pin = ins.ptrs()
    ptmp = tmps.ptrs()
    caps = (_sz * n)(*tmp_caps)
    oi = (_vp * n)()
    err = (ctypes.c_int * n)()
    locs = (ctypes.c_uint64 * n)()
    rc = lib.pom_itb_lzo_compress_append_batch(pin, ptmp, caps, oi, err, n, ctypes.byref(af.ab), locs)
    _check(ins, tmps)
    assert rc == 0, f"pom_itb_lzo_compress_append_batch: {rc}"
    return [_which(oi[b], pin[b], ptmp[b]) for b in range(n)], list(err), list(locs)


def call_wb(ins: Guarded, tmps: Guarded, tmp_caps: Sequence[int], dests, site_id: int, txg: int, magic: int,
            wire: Guarded):
    """pom_xnet_itb_wb_batch into window 0 of wire -> (rc, wire_len, err[b])."""
    lib = xnet._lib()
    n = len(ins)
    caps = (_sz * n)(*tmp_caps)
    wb = (xnet.Wb * n)(*[xnet.Wb(d, v) for d, v in dests])
    wl = _sz(0)
    err = (ctypes.c_int * n)()
    rc = lib.pom_xnet_itb_wb_batch(ins.ptrs(), tmps.ptrs(), caps, wb, n, site_id, txg, magic, wire.addr(0),
                                   wire.size[0], ctypes.byref(wl), err)
    _check(ins, tmps, wire)
    return rc, wl.value, list(err)


def call_decompress(arena: Guarded, caps: Sequence[int]):
    """pom_itb_lzo_decompress_batch in place -> (err[b], len_ok[b])."""
    lib = itb._lib()
    n = len(arena)
    cp = (_sz * n)(*caps)
    err = (ctypes.c_int * n)()
    ok = (ctypes.c_int * n)()
    rc = lib.pom_itb_lzo_decompress_batch(arena.ptrs(), cp, err, ok, n)
    _check(arena)
    assert rc == 0, f"pom_itb_lzo_decompress_batch: {rc}"
    return list(err), list(ok)


def call_read_decompress(fd: int, locations: Sequence[int], bufs: Guarded):
    """pom_itb_read_lzo_decompress_batch (cap[b] = the window's size)
    -> (len[b], err[b], derr[b], len_ok[b])."""
    lib = itb._lib()
    n = len(bufs)
    loc = (ctypes.c_uint64 * n)(*locations)
    lens = (_sz * n)()
    err = (ctypes.c_int * n)()
    derr = (ctypes.c_int * n)()
    ok = (ctypes.c_int * n)()
    rc = lib.pom_itb_read_lzo_decompress_batch(fd, loc, n, bufs.ptrs(), bufs.caps(), lens, err, derr, ok)
    _check(bufs)
    assert rc == 0, f"pom_itb_read_lzo_decompress_batch: {rc}"
    return list(lens), list(err), list(derr), list(ok)


def build_wire(frames: Sequence[WireFrame], magic: int = 0) -> Tuple[Guarded, List[int]]:
    """The frames back to back in one guarded window, each a 72-byte header and
    its data at whatever alignment that gives; and every frame's data offset."""
    blob = bytearray()
    offs = []
    for i, f in enumerate(frames):
        tx = xnet.Tx(vm=(magic & 15) << 4, type=xnet.MSG_RPY, flag=xnet.NEED_DATA_FREE, cmd=xnet.RPY_DATA_ITB,
                     reqno=i, len=f.tx_len)
        blob += bytes(tx)
        offs.append(len(blob))
        blob += f.data
    return guarded_with([bytes(blob)]), offs


def call_recv(wire: Guarded, frames: Sequence[WireFrame], offs: Sequence[int], bufs: Guarded, itb_cap: int):
    """pom_xnet_itb_recv_batch -> err[b]."""
    lib = xnet._lib()
    n = len(frames)
    fr = (xnet._Frame * n)()
    for i, f in enumerate(frames):
        fr[i].tx = xnet.Tx.from_buffer_copy(wire.get(0, offs[i] - xnet.TX_SIZE, offs[i]))
        fr[i].data = wire.addr(0) + offs[i]
        fr[i].dropped = int(f.dropped)
    err = (ctypes.c_int * n)()
    before = bytes(wire.buf)
    rc = lib.pom_xnet_itb_recv_batch(fr, n, bufs.ptrs(), itb_cap, err)
    _check(wire, bufs)
    assert bytes(wire.buf) == before, "the wire was written"
    assert rc == 0, f"pom_xnet_itb_recv_batch: {rc}"
    return list(err)


def call_col_zip(cols: Guarded, zips: Guarded):
    """pom_col_zip_batch (zip_cap[b] = the window's size) -> (zip_len[b], compressed[b])."""
    lib = column._lib()
    n = len(cols)
    zl = (_sz * n)()
    comp = (ctypes.c_int * n)()
    rc = lib.pom_col_zip_batch(cols.ptrs(), cols.caps(), n, zips.ptrs(), zips.caps(), zl, comp)
    _check(cols, zips)
    assert rc == 0, f"pom_col_zip_batch: {rc}"
    return list(zl), list(comp)


def call_col_unzip(zips: Guarded, outs: Guarded):
    """pom_col_unzip_batch (out_cap[b] = the window's size) -> (out_len[b], err[b])."""
    lib = column._lib()
    n = len(zips)
    ol = (_sz * n)()
    err = (ctypes.c_int * n)()
    rc = lib.pom_col_unzip_batch(zips.ptrs(), zips.caps(), n, outs.ptrs(), outs.caps(), ol, err)
    _check(zips, outs)
    assert rc == 0, f"pom_col_unzip_batch: {rc}"
    return list(ol), list(err)


# ---- the family ---------------------------------------------------------------------
def make_header(rng, ln: int, zlen: int = 0, algo: int = itb.COMPR_NONE) -> bytearray:
    hdr = bytearray(rng.integers(0, 256, H, dtype=np.uint8).tobytes())
    struct.pack_into("<II", hdr, itb.LEN_OFF, ln, zlen)
    struct.pack_into("<H", hdr, itb.ALGO_OFF, algo)
    return hdr


def make_rec(rng, payload: bytes) -> bytes:
    """A 264-byte header (random fields, len = 264 + payload, zlen 0,
    COMPR_NONE) over a hand-made payload."""
    return bytes(make_header(rng, H + len(payload))) + bytes(payload)


def tie_search(oracle, n: int, wanted: Sequence[int], seed: int) -> Dict[int, bytes]:
    """n-byte payloads whose oracle stream is len + d bytes, for each d wanted:
    random bytes, then one word every 16 bytes overwritten with the bytes 40
    back, 5 bytes at a time (each moves the difference by about 2; 4- and
    6-byte copies reach the other parity), until every d has been met."""
    rng = np.random.default_rng(seed)
    cur = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    found: Dict[int, bytes] = {}

    def look(p: bytes) -> int:
        d = len(ocompress(oracle, p)) - n
        if d in wanted and d not in found:
            found[d] = bytes(p)
        return d

    d = look(bytes(cur))
    at = 48
    while len(found) < len(wanted) and at + 6 <= n and d >= min(wanted) - 2:
        for k in (4, 6, 5):                         # 5 last: it is the one that stays
            trial = bytearray(cur)
            trial[at:at + k] = trial[at - 40:at - 40 + k]
            d = look(bytes(trial))
        cur = trial
        at += 16
    return found


@dataclass
class Stream:
    """A stored record handed to the decoders."""
    name: str
    rec: bytes                  # max(h.len, 264) bytes
    code: Optional[int]         # the oracle's code with room to spare
    out_len: int                # bytes the oracle produces with room to spare
    damaged: bool


@dataclass
class Family:
    small: List[Tuple[str, bytes]]
    ties: Dict[Tuple[int, int], bytes]
    itb_rec: bytes
    short_rec: bytes            # h.len < 264
    col_ties: Dict[int, bytes]
    col_comp: bytes
    streams: List[Stream]

    def records(self) -> List[Tuple[str, bytes]]:
        """Every record the compress tests take, the short one last."""
        out = list(self.small)
        out += [(f"tie{n}{d:+d}", r) for (n, d), r in sorted(self.ties.items())]
        out += [("itb", self.itb_rec), ("short", self.short_rec)]
        return out


_family: Optional[Family] = None
AMPLE = 1 << 16                 # output room no stream of the family needs


def compressed_form(oracle, rec: bytes) -> bytes:
    which, err, out = expected_compress(oracle, rec, itb.ITB_FULL)
    assert which == 1 and err == 0
    return out


def patch_first_match(z: bytes) -> bytes:
    """The stream with one match distance made to reach one byte before the
    output start (the rest as it was)."""
    z = bytearray(z)
    p = o = 0                                       # stream and output offsets

    def ext(base: int) -> int:
        nonlocal p
        x = 0
        while z[p] == 0:
            x += 255
            p += 1
        p += 1
        return base + x + z[p - 1]

    state = "A"
    if z[0] > 17:
        k = z[0] - 17
        p, o = 1 + k, k
        state = "C" if k < 4 else "B"
    while True:
        t = z[p]
        p += 1
        if t < 16 and state == "A":                 # a literal run
            k = t + 3 if t else ext(18)
            p += k
            o += k
            state = "B"
            continue
        if t < 16:                                  # M1
            n, t_lo = (3 if state == "B" else 2), t & 3
            p += 1
        elif t >= 64:                               # M2: 3 distance bits here, 8 in the next byte
            d = o + 1
            if d <= 2048:
                z[p - 1] = (t & 0xE3) | (((d - 1) & 7) << 2)
                z[p] = (d - 1) >> 3
                return bytes(z)
            n, t_lo = (t >> 5) + 1, t & 3
            p += 1
        elif t >= 32:                               # M3: 14 distance bits over the trailing-literal count
            n = (t & 31) + 2 if t & 31 else ext(ld.M3_BASE)
            d = o + 1
            if d <= 0x4000:
                v = ((d - 1) << 2) | (z[p] & 3)
                z[p], z[p + 1] = v & 255, v >> 8
                return bytes(z)
            t_lo = z[p] & 3
            p += 2
        else:                                       # M4
            n = (t & 7) + 2 if t & 7 else ext(ld.M4_BASE)
            v = z[p] | z[p + 1] << 8
            assert v >> 2 or t & 8, "the end marker before any match to patch"
            t_lo = v & 3
            p += 2
        o += n
        p += t_lo
        o += t_lo
        state = "C" if t_lo else "A"


def _stream(oracle, name: str, rec: bytes, damaged: bool) -> Stream:
    ln = itb.header_fields(rec)[0]
    rc, out = oracle.decompress_safe(bytes(rec[H:max(ln, H)]), AMPLE)
    return Stream(name, bytes(rec), rc, len(out), damaged)


def family(oracle) -> Family:
    """The boundary family, built once with fixed seeds."""
    global _family
    if _family is not None:
        return _family
    rng = np.random.default_rng(20240917)
    small = []
    for n in SMALL_SIZES:
        small.append((f"random{n}", make_rec(rng, rng.integers(0, 256, n, dtype=np.uint8).tobytes())))
        small.append((f"zeros{n}", make_rec(rng, bytes(n))))
    ties = {}
    for n in TIE_SIZES:
        got = tie_search(oracle, n, TIE_DIFFS, seed=n)
        for d in TIE_DIFFS:
            if d in got:
                ties[(n, d)] = make_rec(rng, got[d])
    real = itb.make_record(4242, 1)                              # a real one-ITE ITB
    itb_rec = bytes(real[: itb.header_fields(real)[0]])
    short_rec = bytes(make_header(rng, 100))
    col = tie_search(oracle, COL_TIE_SIZE, [d - 8 for d in COL_TIE_DIFFS], seed=77)
    col_ties = {d: col[d - 8] for d in COL_TIE_DIFFS if d - 8 in col}
    col_comp = bytes(real[H:H + 5000])

    # streams: correctly compressed records, then the variants of one of them
    streams = []
    good = [("itb", itb_rec), ("zeros40", dict(small)["zeros40"])]
    good += [(f"tie{n}{d:+d}", ties[(n, d)]) for n in TIE_SIZES for d in (-1, -2) if (n, d) in ties]
    for name, rec in good:
        streams.append(_stream(oracle, "ok_" + name, compressed_form(oracle, rec), False))
    base = compressed_form(oracle, itb_rec)
    bl, bz, _ = itb.header_fields(base)

    def variant(name, rec, ln=None, zlen=None):
        h = bytearray(rec[:H])
        if ln is not None:
            struct.pack_into("<I", h, itb.LEN_OFF, ln)
        if zlen is not None:
            struct.pack_into("<I", h, itb.ZLEN_OFF, zlen)
        new = bytes(h) + bytes(rec[H:])
        ln = itb.header_fields(new)[0]
        streams.append(_stream(oracle, name, new[:max(ln, H)], True))

    for k in (1, 3, 5):
        variant(f"cut{k}", base, ln=bl - k)
    for k in (1, 4):
        variant(f"trail{k}", base + bytes([0x5A] * k), ln=bl + k)
    variant("lookbehind", base[:H] + patch_first_match(base[H:]))
    variant("zlen+1", base, zlen=bz + 1)
    variant("zlen-1", base, zlen=bz - 1)
    variant("empty", bytes(make_header(rng, H, zlen=H + 40, algo=itb.COMPR_LZO)))
    _family = Family(small, ties, itb_rec, short_rec, col_ties, col_comp, streams)
    return _family


def tmp_caps(oracle, rec: bytes) -> List[int]:
    """The tmp capacities of the family for one record: around the header,
    around header + stream, around the record itself, and a whole ITB."""
    ln = itb.header_fields(rec)[0]
    dlen = len(ocompress(oracle, bytes(rec[H:max(ln, H)])))
    return [0, 263, 264, H + dlen - 1, H + dlen, max(ln, 1) - 1, ln, itb.ITB_FULL]


def decode_caps(out_len: int) -> List[int]:
    """The buffer capacities of the family for a record that decodes to out_len."""
    return sorted({c for c in (H, H + out_len - 1, H + out_len, H + out_len + 1) if c >= H})


def batches(cases: Sequence, size: int) -> List[List]:
    """The cases in batches of `size`; the 300-record batch cycles them."""
    cases = list(cases)
    if size >= 300:
        return [[cases[i % len(cases)] for i in range(size)]]
    return [cases[i:i + size] for i in range(0, len(cases), size)]


def interleave(good: Sequence, bad: Sequence) -> List:
    """good, bad, good, bad, ..., good: every damaged case between two good ones."""
    out = []
    for i, b in enumerate(bad):
        out += [good[i % len(good)], b]
    out.append(good[len(bad) % len(good)])
    seen = {id(x) for x in out}
    return out + [g for g in good if id(g) not in seen]
