"""CPU: the directory listing (include/pom_readdir.h) without a GPU -- the
header's layout constants against the reference's structs, the shared walk
and the wave's copy plan (pomegranate_amd/csrc/itb_dents.h, compiled as plain
C++) against the Python restatement of mds/itb.c:2536-2589 in readdir_util.py,
the stand-alone checker, the exports, and the refusal without a GPU."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from readdir_util import (EINVAL, E_NAME, E_TRUNCATED, ITE_FLAG_KV, ITE_FLAG_NORMAL, ITE_OFF, ITE_SIZE, fill_ites,
                          listing, make_record, set_ite)
from gc_scan_util import set_itb
from pomegranate_amd import lzo, readdir

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"
FULL = ITE_OFF + ITE_SIZE * 1024
POISON = 0xA5


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_readdir.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof / sizeof over the reference's own headers (LP64, its build
    flags), against every layout macro of pom_readdir.h."""
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
    P("POM_ITE_UUID_OFF", offsetof(struct ite, uuid));
    P("POM_ITE_FLAG_OFF", offsetof(struct ite, flag));
    P("POM_ITE_NAMELEN_OFF", offsetof(struct ite, namelen));
    P("POM_ITE_MODE_OFF", offsetof(struct ite, s.mdu.mode));
    P("POM_ITE_NAME_OFF", offsetof(struct ite, s.name));
    P("POM_ITE_NAME_MAX", sizeof(((struct ite *)0)->s.name));
    P("POM_ITE_STATE_MASK", ITE_STATE_MASK);
    P("POM_ITE_FLAG_KV", ITE_FLAG_KV);
    P("POM_DENT_HDR", sizeof(struct dentry_info));
    P("POM_DENT_MODE_OFF", offsetof(struct dentry_info, mode));
    P("POM_DENT_NAMELEN_OFF", offsetof(struct dentry_info, namelen));
    P("active", ITE_ACTIVE);
    P("uuid_size", sizeof(((struct ite *)0)->uuid));
    P("flag_size", sizeof(((struct ite *)0)->flag));
    P("namelen_size", sizeof(((struct ite *)0)->namelen));
    P("mode_size", sizeof(((struct ite *)0)->s.mdu.mode));
    P("dent_uuid_off", offsetof(struct dentry_info, uuid));
    P("dent_mode_size", sizeof(((struct dentry_info *)0)->mode));
    P("dent_namelen_size", sizeof(((struct dentry_info *)0)->namelen));
    P("dent_name_off", offsetof(struct dentry_info, name));
    return 0;
}
''')
    exe = tmp_path / "probe"
    inc = [f"-I{os.path.join(REFERENCE, d)}" for d in ("include", "lib", "mds", "xnet", "mdsl", "r2")]
    subprocess.run(["gcc", "-w", "-D__CORES__=8", "-DDISABLE_PYTHON=1", f"-I{tmp_path}", *inc,
                    str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert got.pop("active") == 0
    assert (got.pop("uuid_size"), got.pop("flag_size"), got.pop("namelen_size"), got.pop("mode_size")) == (8, 4, 4, 2)
    assert (got.pop("dent_uuid_off"), got.pop("dent_mode_size"), got.pop("dent_namelen_size"),
            got.pop("dent_name_off")) == (0, 2, 2, 16)
    want = header_macros()
    assert (want.pop("POM_RD_E_NAME"), want.pop("POM_READDIR_H")) == (-4099, 1)      # (the code, the include guard)
    assert want == got
    # readdir.py mirrors them
    assert (readdir.ITE_UUID_OFF, readdir.ITE_FLAG_OFF, readdir.ITE_NAMELEN_OFF, readdir.ITE_MODE_OFF,
            readdir.ITE_NAME_OFF, readdir.ITE_NAME_MAX, readdir.ITE_STATE_MASK, readdir.ITE_FLAG_KV,
            readdir.DENT_HDR, readdir.DENT_MODE_OFF, readdir.DENT_NAMELEN_OFF) == tuple(got[k] for k in (
                "POM_ITE_UUID_OFF", "POM_ITE_FLAG_OFF", "POM_ITE_NAMELEN_OFF", "POM_ITE_MODE_OFF",
                "POM_ITE_NAME_OFF", "POM_ITE_NAME_MAX", "POM_ITE_STATE_MASK", "POM_ITE_FLAG_KV",
                "POM_DENT_HDR", "POM_DENT_MODE_OFF", "POM_DENT_NAMELEN_OFF"))
    assert readdir.E_NAME == -4099


# ---------------------------------------------------------------------------
# libitb_dents_host.so (itb_dents.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_dents():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_dents_host.so"))
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.itb_dents_host.restype = ctypes.c_int
    lib.itb_dents_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                   ctypes.c_uint64, u32p, u32p, u32p]
    lib.itb_dents_wave_host.restype = ctypes.c_int
    lib.itb_dents_wave_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                        ctypes.c_uint64, ctypes.c_uint64, u32p, u32p, u32p]

    def run(payload: bytes, adepth: int, shift: int = 0, oshift: int = 0, cap: "int | None" = None,
            wave: bool = False, at: int = 0):
        """-> (err, live, dnum, bytes, what was written).  The payload sits at
        residue `shift` mod 16 and the output at `oshift`, each in a buffer of
        its own; the output is poisoned around [at, cap)."""
        room = np.zeros(len(payload) + 32, dtype=np.uint8)
        pa = (-room.ctypes.data) % 16 + shift
        room[pa: pa + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
        if cap is None:
            cap = at + 272 * 1024
        out = np.full(cap + 64, POISON, dtype=np.uint8)
        oa = (-out.ctypes.data) % 16 + oshift
        live, dnum, nbytes = ctypes.c_uint32(99), ctypes.c_uint32(99), ctypes.c_uint32(99)
        refs = (ctypes.byref(live), ctypes.byref(dnum), ctypes.byref(nbytes))
        if wave:
            err = lib.itb_dents_wave_host(room.ctypes.data + pa, len(payload), adepth, out.ctypes.data + oa, at,
                                          cap, *refs)
        else:
            assert at == 0
            err = lib.itb_dents_host(room.ctypes.data + pa, len(payload), adepth, out.ctypes.data + oa, cap, *refs)
        end = min(at + nbytes.value, cap) if err == 0 else at
        # nothing before the ITB's first byte, nothing past its last or the cap
        assert (out[:oa + at] == POISON).all() and (out[oa + max(end, at):] == POISON).all()
        return err, live.value, dnum.value, nbytes.value, out[oa + at: oa + max(end, at)].tobytes()
    return run


def image(seed: int, bits, namelens=None, flags=None, n_bytes: int = FULL) -> bytes:
    buf = bytearray(np.random.default_rng(seed).integers(0, 256, FULL, dtype=np.uint8).tobytes())
    set_itb(buf, 0, bits, None, seed)
    fill_ites(buf, 0, seed, 1024, namelens, flags)
    return bytes(buf[:n_bytes])


def agree(host_dents, payload, adepth, shift=0, oshift=0):
    """Both the bit-by-bit walk and the wave's plan, whole; the wave's also at
    an output offset.  Returns the oracle's answer."""
    err, live, dnum, data = listing(payload, adepth)
    want = (err, live, dnum, len(data), data)
    assert host_dents(payload, adepth, shift, oshift) == want, (len(payload), adepth, shift, oshift)
    assert host_dents(payload, adepth, shift, oshift, wave=True) == want, (len(payload), adepth, shift, oshift)
    assert host_dents(payload, adepth, shift, oshift, wave=True, at=1000 + 7 * shift) == want
    return err, live, dnum, data


def test_adepth_limits_the_walk(host_dents):
    """adepth 1, 6, 7, 10 (and the rest) with bits set above 1 << adepth; 0 and
    11 are -EINVAL."""
    full = image(1, range(1024))
    for adepth in range(1, 11):
        err, live, dnum, data = agree(host_dents, full, adepth, shift=adepth, oshift=16 - adepth)
        assert (err, live, dnum) == (0, 1 << adepth, 1 << adepth)
        assert [r[2] for r in readdir.parse(data)] == [r[2] for r in readdir.parse(listing(full, 10)[3])][:live]
    for adepth in (0, 11, 12, 64, 255):
        assert agree(host_dents, full, adepth)[0] == EINVAL


@pytest.mark.parametrize("bits", [[], [0], [63], [64], [1023], list(range(1024)), list(range(0, 1024, 2)),
                                  list(range(1, 1024, 2))],
                         ids=["empty", "bit0", "bit63", "bit64", "bit1023", "full", "even", "odd"])
def test_directed_bitmaps_every_payload_residue(host_dents, bits):
    payload = image(3, bits)
    for shift in range(16):
        err, live, dnum, _ = agree(host_dents, payload, 10, shift, (7 * shift + len(bits)) % 16)
        assert (err, live, dnum) == (0, len(bits), len(bits))


def test_every_output_residue(host_dents):
    payload = image(4, range(0, 200, 3))
    for oshift in range(16):
        agree(host_dents, payload, 10, 0, oshift)
        agree(host_dents, payload, 10, 5, oshift)


@pytest.mark.parametrize("namelen", [0, 1, 15, 16, 17, 255, 256])
def test_name_lengths(host_dents, namelen):
    """The length alone, between neighbours of other lengths, and on every ITE."""
    for bits, lens in (([9], {9: namelen}), ([8, 9, 10], {8: 3, 9: namelen, 10: 40}),
                       (list(range(70)), {nr: namelen for nr in range(70)})):
        payload = image(5 + namelen, bits, lens)
        err, live, dnum, data = agree(host_dents, payload, 10, namelen % 16, (namelen + 3) % 16)
        assert (err, dnum) == (0, len(bits))
        assert len(readdir.parse(data)[bits.index(9)][2]) == namelen


def test_name_too_long(host_dents):
    """257 on an emitted ITE: POM_RD_E_NAME and nothing written; on a skipped
    ITE it is not examined."""
    for namelen in (257, 65536 + 12, (1 << 32) - 1):
        bad = image(6, [3, 4, 5], {4: namelen})
        assert agree(host_dents, bad, 10, 1, 2) == (E_NAME, 3, 0, b"")
        for flag in (ITE_FLAG_NORMAL | 1, ITE_FLAG_NORMAL | ITE_FLAG_KV):
            skipped = image(6, [3, 4, 5], {4: namelen}, {4: flag})
            err, live, dnum, _ = agree(host_dents, skipped, 10, 1, 2)
            assert (err, live, dnum) == (0, 3, 2)


def test_states_and_kv_are_skipped(host_dents):
    flags = {nr: ITE_FLAG_NORMAL | nr for nr in range(8)}            # states 0 ... 7 on ITEs 0 ... 7
    flags[8] = ITE_FLAG_KV
    flags[9] = ITE_FLAG_NORMAL | ITE_FLAG_KV | 0x00800000
    flags[10] = 0                                                    # active, no other flag
    flags[11] = 0xFEFFFFF8                                           # active, every flag but KV
    payload = image(7, range(12), flags=flags)
    err, live, dnum, data = agree(host_dents, payload, 10, 3, 9)
    assert (err, live, dnum) == (0, 12, 3)
    uuids = [np.frombuffer(payload, dtype="<u8", count=1, offset=ITE_OFF + ITE_SIZE * nr + 8)[0] for nr in (0, 10, 11)]
    assert [r[0] for r in readdir.parse(data)] == uuids


def test_cut_payloads(host_dents):
    """3711 (bitmap incomplete), 3712 (bitmap only), 11904 (no ITE), inside a
    live ITE, one byte short of its end, and exactly at it: all or nothing."""
    bits = [0, 3, 200]
    payload = image(8, bits)
    end = ITE_OFF + ITE_SIZE * 201
    for n, want_err, want_live in ((0, E_TRUNCATED, 0), (3600, E_TRUNCATED, 0), (3711, E_TRUNCATED, 0),
                                   (3712, E_TRUNCATED, 3), (11904, E_TRUNCATED, 3),
                                   (ITE_OFF + ITE_SIZE * 4, E_TRUNCATED, 3), (end - 300, E_TRUNCATED, 3),
                                   (end - 1, E_TRUNCATED, 3), (end, 0, 3), (end + 1, 0, 3)):
        for shift in (0, 1, 8, 15):
            err, live, dnum, data = agree(host_dents, payload[:n], 10, shift, shift ^ 5)
            assert (err, live) == (want_err, want_live), n
            assert err == 0 or (dnum, data) == (0, b"")
    # the cut ITE is above the limit: it is not live, the ITB is whole
    assert agree(host_dents, payload[:ITE_OFF + ITE_SIZE * 4], 7)[:3] == (0, 2, 2)
    # an empty bitmap needs no ITE at all
    assert agree(host_dents, image(9, [])[:3712], 10) == (0, 0, 0, b"")


def test_caps_cut_records(host_dents):
    """Caps inside a header, inside a name and at a record boundary; the
    poisoned bytes behind the cap stay (checked in the fixture)."""
    payload = image(10, range(0, 140, 2), {0: 20, 2: 0, 4: 33})
    _, _, dnum, data = listing(payload, 10)
    total = len(data)
    caps = [0, 1, 15, 16, 17, 35, 36, 36 + 16, 36 + 16 + 5, 36 + 16 + 16 + 33, total - 1, total, total // 2]
    for cap in caps:
        for wave in (False, True):
            for oshift in (0, 1, 15):
                got = host_dents(payload, 10, 4, oshift, cap=cap, wave=wave)
                assert got == (0, 70, dnum, total, data[:cap]), (cap, wave, oshift)


def test_random_itbs(host_dents):
    rng = np.random.default_rng(0xD1E57)
    for t in range(60):
        density = rng.random() ** 2
        bits = np.flatnonzero(rng.random(1024) < density).tolist()
        n_ites = int(rng.integers(0, 1025))
        n = ITE_OFF + ITE_SIZE * n_ites - (int(rng.integers(0, 600)) if t % 5 == 0 else 0)
        lens = {int(nr): int(rng.choice([0, 1, 15, 16, 17, 255, 256, 100])) for nr in rng.integers(0, 1024, 200)}
        flags = {int(nr): int(rng.integers(0, 1 << 32)) for nr in rng.integers(0, 1024, 300)}
        if t % 7 == 0:
            lens[int(rng.integers(0, 1024))] = 300
        payload = image(2000 + t, bits, lens, flags, n_bytes=max(n, 0))
        agree(host_dents, payload, int(rng.integers(1, 11)), int(rng.integers(0, 16)), int(rng.integers(0, 16)))


def test_maximum_listing(host_dents):
    """1,024 active entries with 256-byte names: 278,528 bytes."""
    payload = image(11, range(1024), {nr: 256 for nr in range(1024)}, {nr: 0 for nr in range(1024)})
    err, live, dnum, data = agree(host_dents, payload, 10, 8, 7)
    assert (err, live, dnum, len(data)) == (0, 1024, 1024, 278528)


def test_itb_dents_check_passes():
    """The stand-alone checker (itb_dents.h against its own naive walk; built
    with AddressSanitizer and UBSan where they link) exits 0."""
    r = subprocess.run([os.path.join(NATIVE, "itb_dents_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_dents_check: ok" in r.stdout


def test_parse_round_trip_and_cut():
    payload = image(12, [1, 2, 3], {1: 0, 2: 5, 3: 256})
    data = listing(payload, 10)[3]
    recs = readdir.parse(data)
    assert [len(r[2]) for r in recs] == [0, 5, 256]
    assert recs[1][2] == payload[ITE_OFF + ITE_SIZE * 2 + 104: ITE_OFF + ITE_SIZE * 2 + 109]
    for cut in (len(data) - 1, 16 + 8, 16 + 16 + 5 + 3):
        with pytest.raises(ValueError):
            readdir.parse(data[:cut])


def test_exports_are_declared():
    assert {"pom_readdir_dev", "pom_readdir_batch"} <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert hasattr(lib, "pom_readdir_dev") and hasattr(lib, "pom_readdir_batch")
    text = open(os.path.join(ROOT, "include", "pom_readdir.h")).read()
    assert re.search(r"\bint pom_readdir_dev\(", text) and re.search(r"\bint pom_readdir_batch\(", text)
    assert '#include "pom_gc.h"' in text
    # the launcher and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_readdir", "pom_readdir_chunked", "pom_itb_walk_header"} & set(lzo.EXPORTS)


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_scan_batch_refuses():
    rec = make_record(1, 2, 1, [0, 1])
    res = None
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        res = readdir.scan_batch([rec])
    assert res is None
    # and the C call itself, with no record at all
    first = (ctypes.c_size_t * 1)()
    assert readdir._lib().pom_readdir_batch(None, None, 0, None, 0, first, None, None, None, None, None) == \
        lzo.LZO_E_ERROR
