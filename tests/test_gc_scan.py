"""CPU: the garbage-collector scan (include/pom_gc.h) without a GPU -- the
header's layout constants against the reference's structs, the shared walk
(pomegranate_amd/csrc/itb_scan.h, compiled as plain C++) against the Python
restatement of mdsl/gc.c:968-993 in gc_scan_util.py, the stand-alone checker,
the exports, and the refusal without a GPU."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gc_scan_util import EINVAL, E_TRUNCATED, ITE_OFF, ITE_SIZE, set_itb, walk
from pomegranate_amd import gc, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"
FULL = ITE_OFF + ITE_SIZE * 1024


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_gc.h")).read()
    return {m.group(1): int(m.group(2)) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?\d+)u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof / sizeof over the reference's own headers (LP64, its build
    flags), against every layout macro of pom_gc.h."""
    (tmp_path / "attr").mkdir()
    (tmp_path / "attr" / "xattr.h").write_text("/* stub: the probe needs no xattr call */\n")
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include "hvfs.h"
#include "xtable.h"
#include "ite.h"
#include "mds_api.h"
#include <stddef.h>
#include <stdio.h>
#define P(name, v) printf("%s %ld\n", name, (long)(v))
int main(void)
{
    const long lock = (long)offsetof(struct itb, lock);
    P("POM_ITBH_SIZE", sizeof(struct itbh));
    P("POM_ITBH_ADEPTH_OFF", offsetof(struct itbh, adepth));
    P("POM_ITBH_ENTRIES_OFF", offsetof(struct itbh, entries));
    P("POM_ITBH_LEN_OFF", offsetof(struct itbh, len));
    P("POM_ITBH_ZLEN_OFF", offsetof(struct itbh, zlen));
    P("POM_ITBH_ALGO_OFF", offsetof(struct itbh, compress_algo));
    P("lock", lock);
    P("POM_ITB_BITMAP_OFF", (long)offsetof(struct itb, bitmap) - lock);
    P("POM_ITB_BITMAP_BYTES", sizeof(((struct itb *)0)->bitmap));
    P("POM_ITB_INDEX_OFF", (long)offsetof(struct itb, index) - lock);
    P("POM_ITB_ITE_OFF", (long)offsetof(struct itb, ite) - lock);
    P("POM_ITB_ADEPTH_MAX", ITB_DEPTH);
    P("POM_ITE_SIZE", sizeof(struct ite));
    P("POM_ITE_COLUMN_OFF", offsetof(struct ite, column));
    P("POM_ITE_COLUMNS", sizeof(((struct ite *)0)->column) / sizeof(struct column));
    P("POM_COLUMN_SIZE", sizeof(struct column));
    P("POM_COLUMN_ITBID_OFF", offsetof(struct column, stored_itbid));
    P("POM_COLUMN_LEN_OFF", offsetof(struct column, len));
    P("POM_COLUMN_OFFSET_OFF", offsetof(struct column, offset));
    P("adepth_size", sizeof(((struct itbh *)0)->adepth));
    P("len_size", sizeof(((struct column *)0)->len));
    return 0;
}
''')
    exe = tmp_path / "probe"
    inc = [f"-I{os.path.join(REFERENCE, d)}" for d in ("include", "lib", "mds", "xnet", "mdsl", "r2")]
    subprocess.run(["gcc", "-w", "-D__CORES__=8", "-DDISABLE_PYTHON=1", f"-I{tmp_path}", *inc,
                    str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert got.pop("lock") == got["POM_ITBH_SIZE"]          # the payload starts right behind the header
    assert got.pop("adepth_size") == 1 and got.pop("len_size") == 8
    want = header_macros()
    # the header-record macros live in pom_itb.h; the scan's own in pom_gc.h
    itb_h = open(os.path.join(ROOT, "include", "pom_itb.h")).read()
    for name in ("POM_ITBH_SIZE", "POM_ITBH_LEN_OFF", "POM_ITBH_ZLEN_OFF", "POM_ITBH_ALGO_OFF"):
        assert int(re.search(rf"#define {name} (\d+)u", itb_h).group(1)) == got.pop(name), name
    layout = {k: v for k, v in want.items() if not k.startswith("POM_GC_")}      # (codes, include guard)
    assert layout == got
    assert (want["POM_GC_E_TRUNCATED"], want["POM_GC_E_NOSPACE"]) == (-4097, -4098)
    # gc.py mirrors them
    assert (gc.ADEPTH_OFF, gc.ENTRIES_OFF, gc.BITMAP_OFF, gc.BITMAP_BYTES, gc.INDEX_OFF, gc.ITE_OFF,
            gc.ITE_SIZE, gc.ITE_COLUMN_OFF, gc.ITE_COLUMNS, gc.COLUMN_SIZE, gc.COLUMN_LEN_OFF,
            gc.COLUMN_OFFSET_OFF) == tuple(want[k] for k in (
                "POM_ITBH_ADEPTH_OFF", "POM_ITBH_ENTRIES_OFF", "POM_ITB_BITMAP_OFF", "POM_ITB_BITMAP_BYTES",
                "POM_ITB_INDEX_OFF", "POM_ITB_ITE_OFF", "POM_ITE_SIZE", "POM_ITE_COLUMN_OFF",
                "POM_ITE_COLUMNS", "POM_COLUMN_SIZE", "POM_COLUMN_LEN_OFF", "POM_COLUMN_OFFSET_OFF"))


# ---------------------------------------------------------------------------
# libitb_scan_host.so (itb_scan.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_scan():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_scan_host.so"))
    lib.itb_scan_host.restype = ctypes.c_int
    lib.itb_scan_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32),
                                  ctypes.POINTER(ctypes.c_uint32)]

    def run(payload: bytes, adepth: int, column: int, shift: int = 0, cap: int = 1024):
        # the payload at residue `shift` mod 16, in a buffer of its own
        room = np.zeros(len(payload) + 32, dtype=np.uint8)
        at = (-room.ctypes.data) % 16 + shift
        room[at: at + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
        out = np.full((cap + 1, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        live, nr = ctypes.c_uint32(99), ctypes.c_uint32(99)
        err = lib.itb_scan_host(room.ctypes.data + at, len(payload), adepth, column, out.ctypes.data, cap,
                                ctypes.byref(live), ctypes.byref(nr))
        assert (out[min(nr.value, cap):] == 0xA5A5A5A5A5A5A5A5).all()    # nothing past the count or the cap
        return err, live.value, nr.value, [tuple(int(x) for x in row) for row in out[: min(nr.value, cap)]]
    return run


def image(seed: int, bits, columns=None, n_bytes: int = FULL) -> bytes:
    buf = bytearray(np.random.default_rng(seed).integers(0, 256, FULL, dtype=np.uint8).tobytes())
    set_itb(buf, 0, bits, columns, seed)
    return bytes(buf[:n_bytes])


def agree(host_scan, payload, adepth, column, shift=0):
    err, live, ranges = walk(payload, adepth, column)
    got = host_scan(payload, adepth, column, shift)
    # live of an ITB that errs before the walk (EINVAL, bitmap cut) is 0 on both sides
    assert got == (err, live, len(ranges), ranges), (len(payload), adepth, column, shift)
    return err, live, ranges


def test_adepth_limits_the_walk(host_scan):
    """adepth 1 ... 10 with bits set above 1 << adepth; 0 and 11 are -EINVAL."""
    full = image(1, range(1024))
    sparse = image(2, [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513, 1023])
    for adepth in range(1, 11):
        err, live, ranges = agree(host_scan, full, adepth, adepth % 6, shift=adepth)
        assert (err, live) == (0, 1 << adepth) and 0 < len(ranges) <= live
        err, live, _ = agree(host_scan, sparse, adepth, 0)
        assert (err, live) == (0, sum(1 for b in [0, 1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 513, 1023]
                                      if b < (1 << adepth)))
    for adepth in (0, 11, 12, 64, 255):
        assert agree(host_scan, full, adepth, 0)[0] == EINVAL


@pytest.mark.parametrize("bits", [[], list(range(1024)), [0], [63], [64], [1023], list(range(0, 1024, 2)),
                                  list(range(1, 1024, 2))],
                         ids=["empty", "full", "bit0", "bit63", "bit64", "bit1023", "even", "odd"])
def test_directed_bitmaps_every_column_and_residue(host_scan, bits):
    payload = image(3, bits)
    for column in range(6):
        err, live, _ = agree(host_scan, payload, 10, column, shift=(5 * column + len(bits)) % 16)
        assert (err, live) == (0, len(bits))
    for shift in range(16):
        agree(host_scan, payload, 10, 2, shift)


def test_len_zero_and_offset_wrap(host_scan):
    cols = {0: [(0, 7)] * 6,                              # len == 0: no range
            1: [(1, (1 << 64) - 1)] * 6,                  # offset 2^64 - 1: high wraps to 1
            2: [((1 << 64) - 1, 5)] * 6,                  # len 2^64 - 1: high = offset
            3: [(0, 0), (1, 0), (0, 1), (2, 2), (0, 3), (3, 3)]}
    payload = image(4, [0, 1, 2, 3], cols)
    err, live, ranges = agree(host_scan, payload, 10, 0)
    assert (err, live) == (0, 4)
    assert ranges == [((1 << 64) - 1, 1), (5, 5)]
    assert agree(host_scan, payload, 2, 1)[2] == [((1 << 64) - 1, 1), (5, 5), (0, 2)]
    assert agree(host_scan, payload, 2, 3)[2] == [((1 << 64) - 1, 1), (5, 5), (2, 5)]


def test_cut_payloads(host_scan):
    """3711 (bitmap incomplete), 3712 (bitmap only), 11904 (no ITE), and one
    byte short of a live ITE's end: all or nothing per ITB."""
    bits = [0, 3, 200]
    payload = image(5, bits)
    end = ITE_OFF + ITE_SIZE * 201
    for n, want_err, want_live in ((0, E_TRUNCATED, 0), (3711, E_TRUNCATED, 0), (3712, E_TRUNCATED, 3),
                                   (11904, E_TRUNCATED, 3), (ITE_OFF + ITE_SIZE * 4, E_TRUNCATED, 3),
                                   (end - 1, E_TRUNCATED, 3), (end, 0, 3), (end + 1, 0, 3)):
        for shift in (0, 1, 8, 15):
            err, live, ranges = agree(host_scan, payload[:n], 10, 1, shift)
            assert (err, live) == (want_err, want_live), n
            assert err == 0 or ranges == []
    # the cut ITE is above the limit: it is not live, the ITB is whole
    assert agree(host_scan, payload[:ITE_OFF + ITE_SIZE * 4], 7, 1)[:2] == (0, 2)
    # an empty bitmap needs no ITE at all
    assert agree(host_scan, image(6, [])[:3712], 10, 0) == (0, 0, [])


def test_random_itbs(host_scan):
    rng = np.random.default_rng(0x6C5CA)
    for t in range(200):
        density = rng.random() ** 2
        bits = np.flatnonzero(rng.random(1024) < density).tolist()
        n_ites = int(rng.integers(0, 1025))
        n = ITE_OFF + ITE_SIZE * n_ites - (int(rng.integers(0, 600)) if t % 5 == 0 else 0)
        payload = image(1000 + t, bits, n_bytes=n)
        agree(host_scan, payload, int(rng.integers(1, 11)), int(rng.integers(0, 6)), int(rng.integers(0, 16)))


def test_cap_bounds_the_ranges_written(host_scan):
    payload = image(7, range(64))
    _, _, ranges = walk(payload, 10, 0)
    for cap in (0, 1, len(ranges) - 1, len(ranges)):
        err, live, nr, got = host_scan(payload, 10, 0, cap=cap)
        assert (err, live, nr) == (0, 64, len(ranges)) and got == ranges[:cap]


def test_itb_scan_check_passes():
    """The stand-alone checker (itb_scan.h against its own naive walk; built
    with AddressSanitizer and UBSan where they link) exits 0."""
    r = subprocess.run([os.path.join(NATIVE, "itb_scan_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_scan_check: ok" in r.stdout


def test_exports_are_declared():
    assert {"pom_gc_scan_dev", "pom_gc_scan_batch"} <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert hasattr(lib, "pom_gc_scan_dev") and hasattr(lib, "pom_gc_scan_batch")
    text = open(os.path.join(ROOT, "include", "pom_gc.h")).read()
    assert re.search(r"\bint pom_gc_scan_dev\(", text) and re.search(r"\bint pom_gc_scan_batch\(", text)
    assert "lzo_mi355x_launch_gc_scan" not in lzo.EXPORTS      # the launcher is internal


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_scan_batch_refuses():
    from gc_scan_util import make_record
    rec = make_record(1, 2, 1, [0, 1])
    res = None
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        res = gc.scan_batch([rec], 0)
    assert res is None
    # and the C call itself, with no record at all
    first = (ctypes.c_size_t * 1)()
    assert gc._lib().pom_gc_scan_batch(None, None, 0, 0, None, 0, first, None, None, None, None) == lzo.LZO_E_ERROR
