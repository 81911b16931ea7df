"""CPU: the key/value table listing (include/pom_kvlist.h) without a GPU -- the
header's layout constants against the reference's structs, the shared walk
and the wave's copy plan (pomegranate_amd/csrc/itb_keys.h, compiled as plain
C++) against the Python restatement of mds/itb.c:2478-2534 in kvlist_util.py,
the stand-alone checker, and the refusals without a GPU."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kvlist_util as U
from conftest import ROOT
from pomegranate_amd import kvlist, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"
POISON = 0xA5


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_kvlist.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof / sizeof over the reference's own headers (LP64, its build
    flags), against every POM_KV_* macro of pom_kvlist.h."""
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
#include <string.h>
#define P(name, v) printf("%s %ld\n", name, (long)(v))
int main(void)
{
    char kbuf[128];
    P("POM_KV_FLAGS_OFF", offsetof(struct ite, v.flags));
    P("POM_KV_LEN_OFF", offsetof(struct ite, v.len));
    P("POM_KV_KEY_OFF", offsetof(struct ite, v.key));
    P("POM_KV_KLEN_OFF", offsetof(struct ite, v.klen));
    P("POM_KV_VALUE_OFF", offsetof(struct ite, v.value));
    P("POM_KV_VALUE_MAX", sizeof(((struct ite *)0)->v.value));
    P("POM_KV_SIZE", sizeof(struct kv));
    P("POM_KV_HEADER_LEN", KV_HEADER_LEN);
    P("POM_KV_NORMAL", HVFS_KV_NORMAL);
    P("POM_KV_STR", HVFS_KV_STR);
    P("POM_KV_OP_SCAN", KV_OP_SCAN);
    P("POM_KV_OP_SCAN_CNT", KV_OP_SCAN_CNT);
    P("POM_KV_OP_GREP", KV_OP_GREP);
    P("POM_KV_OP_GREP_CNT", KV_OP_GREP_CNT);
    P("POM_KV_NEEDLE_MAX", (1 << 8 * sizeof(((struct hvfs_index *)0)->namelen)) - 1);
    snprintf(kbuf, 127, "%ld", (long)0x8000000000000000UL);
    P("POM_KV_TEXT_MAX", strlen(kbuf));
    P("mdu_flags_off", offsetof(struct ite, s.mdu.flags));
    P("name_off", offsetof(struct ite, s.name));
    P("column_off", offsetof(struct ite, column));
    P("hi_op_size", sizeof(((struct hvfs_index *)0)->op));
    P("key_size", sizeof(((struct ite *)0)->v.key));
    return 0;
}
''')
    exe = tmp_path / "probe"
    inc = [f"-I{os.path.join(REFERENCE, d)}" for d in ("include", "lib", "mds", "xnet", "mdsl", "r2")]
    subprocess.run(["gcc", "-w", "-D__CORES__=8", "-DDISABLE_PYTHON=1", f"-I{tmp_path}", *inc,
                    str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert (got.pop("mdu_flags_off"), got.pop("name_off"), got.pop("column_off")) == (24, 104, 368)
    assert (got.pop("hi_op_size"), got.pop("key_size")) == (2, 8)
    want = header_macros()
    # the three codes (the new one, and the two it shares), the mask's size, the include guard
    assert (want.pop("POM_KV_E_KEY"), want.pop("POM_KV_MASK_WORDS"), want.pop("POM_KVLIST_H")) == (-4101, 16, 1)
    assert want == got
    assert (kvlist.E_KEY, kvlist.E_NAME, kvlist.E_TRUNCATED) == (-4101, -4099, -4097)
    assert (U.E_KEY, U.E_NAME, U.E_TRUNCATED) == (-4101, -4099, -4097)
    assert (got["POM_KV_FLAGS_OFF"], got["POM_KV_LEN_OFF"], got["POM_KV_KEY_OFF"], got["POM_KV_KLEN_OFF"],
            got["POM_KV_VALUE_OFF"], got["POM_KV_SIZE"], got["POM_KV_HEADER_LEN"], got["POM_KV_TEXT_MAX"]) == \
        (24, 28, 32, 40, 44, 344, 20, 20)
    # the test oracle's and the binding's own constants are the reference's too
    assert (U.KV_NORMAL, U.KV_STR, U.VALUE_OFF, U.VALUE_MAX, U.OP_GREP, U.OP_GREP_CNT) == tuple(
        got[k] for k in ("POM_KV_NORMAL", "POM_KV_STR", "POM_KV_VALUE_OFF", "POM_KV_VALUE_MAX", "POM_KV_OP_GREP",
                         "POM_KV_OP_GREP_CNT"))
    assert (kvlist.KV_NORMAL, kvlist.KV_STR, kvlist.KV_VALUE_OFF, kvlist.KV_VALUE_MAX, kvlist.NEEDLE_MAX) == tuple(
        got[k] for k in ("POM_KV_NORMAL", "POM_KV_STR", "POM_KV_VALUE_OFF", "POM_KV_VALUE_MAX", "POM_KV_NEEDLE_MAX"))


def test_codes_without_the_reference():
    want = header_macros()
    assert (want["POM_KV_E_KEY"], want["POM_KV_NORMAL"], want["POM_KV_STR"]) == (-4101, 0x8000, 0x4000)
    text = open(os.path.join(ROOT, "include", "pom_readdir.h")).read() + open(os.path.join(ROOT, "include", "pom_gc.h")).read()
    assert "#define POM_RD_E_NAME (-4099)" in text and re.search(r"#define POM_GC_E_TRUNCATED \(?-4097\)?", text)


def test_key_text_is_the_c_librarys():
    assert U.key_text(0) == b"0" and U.key_text(-1) == b"-1"
    assert U.key_text(U.INT64_MIN) == b"-9223372036854775808" and len(U.key_text(U.INT64_MIN)) == 20
    assert U.key_text(U.INT64_MAX) == b"9223372036854775807"


# ---------------------------------------------------------------------------
# itb_keys.h on the CPU against the oracle
# ---------------------------------------------------------------------------
_vp, _u32, _u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope="module")
def host():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_keys_host.so"))
    lib.itb_keys_host.restype = ctypes.c_int
    lib.itb_keys_host.argtypes = [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _u64] + [_vp] * 5 + [ctypes.c_int]
    lib.itb_keys_wave_host.restype = ctypes.c_int
    lib.itb_keys_wave_host.argtypes = [_vp, _u32, _u32, _u32, _vp, _u32, _vp, _u64, _u64] + [_vp] * 5 + [ctypes.c_int]
    return lib


def run_host(lib, payload, adepth, op, needle, cap, wave, linear, shift=0, oshift=0):
    """One call over a payload at residue `shift` into an output at residue
    `oshift` with `cap` bytes of room and poison behind."""
    src = np.zeros(len(payload) + 32, dtype=np.uint8)
    base = (-src.ctypes.data) % 16 + shift
    src[base: base + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    nd = np.frombuffer(bytes(needle) + b"\xEE", dtype=np.uint8).copy()
    out = np.full(cap + 64, POISON, dtype=np.uint8)
    obase = (-out.ctypes.data) % 16 + oshift
    cnt = np.full(4, 77, dtype=np.uint32)
    mask = np.full(16, 0x77, dtype=np.uint64)
    args = [src.ctypes.data + base, len(payload), adepth, op, nd.ctypes.data, len(needle), out.ctypes.data + obase]
    args += [0, cap] if wave else [cap]
    args += [cnt[i:].ctypes.data for i in range(4)] + [mask.ctypes.data, linear]
    err = (lib.itb_keys_wave_host if wave else lib.itb_keys_host)(*args)
    assert (out[:obase] == POISON).all() and (out[obase + cap:] == POISON).all(), "a store outside the output"
    return err, cnt.tolist(), mask.tolist(), out[obase: obase + cap].tobytes()


def check_host(lib, case, op, needle, forms=((0, 1), (1, 1), (0, 0), (1, 0)), caps=None, shift=0, oshift=0):
    _, payload, _, adepth = case
    e, live, dnum, kb, mask, rec = U.listing(payload, adepth, op, needle)
    total = len(rec)
    for cap in (caps or [total]):
        cap = min(cap, total)
        for wave, linear in forms:
            err, cnt, got_mask, got = run_host(lib, payload, adepth, op, needle, cap, wave, linear, shift, oshift)
            assert (err, cnt) == (e, [live, dnum, total, kb]), (case[0], op, wave, linear, cap)
            assert got_mask == mask, (case[0], op, wave, linear)
            assert got == rec[:cap], (case[0], op, wave, linear, cap)
    return e, dnum, mask


@pytest.fixture(scope="module")
def scan_cases():
    return U.scan_cases()


def test_scan_cases_against_the_oracle(host, scan_cases):
    errs = {}
    for i, case in enumerate(scan_cases):
        for op, needle in ((U.OP_SCAN, b""), (U.OP_GREP, b"aB"), (U.OP_GREP_CNT, b"zz"), (U.OP_SCAN_CNT, b"aB")):
            forms = ((0, 1), (1, 1), (0, 0), (1, 0)) if len(case[1]) < 200000 else ((i % 2, 1),)
            errs[case[0], op] = check_host(host, case, op, needle, forms=forms, shift=i % 16, oshift=(5 * i) % 16)[0]
    for op in range(4):
        assert errs["klen 321", op] == errs[f"klen {1 << 20}", op] == U.E_KEY
        assert errs["namelen 257", op] == U.E_NAME
        assert errs["both errors 0", op] == errs["both errors 1", op] == U.E_KEY
        assert errs["cut ite", op] == errs["cut byte", op] == errs["no bitmap", op] == U.E_TRUNCATED
        assert errs["exact end", op] == errs["lengths not examined", op] == errs["states", op] == 0


def test_normal_keys_are_the_decimal_text(host, scan_cases):
    case = next(c for c in scan_cases if c[0] == "normal keys")
    _, _, _, _, _, rec = U.listing(case[1], case[3])
    keys = kvlist.parse(rec)
    assert keys == [str(k - (1 << 64) if k >= 1 << 63 else k).encode() for k in U.NORMAL_KEYS]
    assert {len(k) for k in keys} == set(range(1, 21))


@pytest.mark.parametrize("needle", U.NEEDLES, ids=lambda n: f"needle{len(n)}-{n[:3].hex()}")
def test_grep_cases_against_the_oracle(host, needle):
    """Every match position the header's rule 7 names, for every needle of
    the family; the oracle's verdicts are the ones the builder meant."""
    case, want = U.grep_cases(needle)
    for op in (U.OP_GREP, U.OP_GREP_CNT):
        e, dnum, mask = check_host(host, case, op, needle, caps=[10 ** 9, 0, 1, 3, 4, 5, 11], shift=len(needle) % 16,
                                   oshift=3)
        assert e == 0 and {nr: bool(mask[0] >> nr & 1) for nr in want} == want
    e, dnum, _ = check_host(host, case, U.OP_SCAN, needle)
    assert e == 0 and dnum == len(want)


def test_haystacks_against_the_oracle(host):
    case = U.haystack_case()
    emitted = {}
    for needle in U.HAYSTACK_NEEDLES:
        emitted[needle] = check_host(host, case, U.OP_GREP, needle, shift=5, oshift=9)[2][0]
    assert emitted[b"aab"] == 0b00000011                    # "aaab" restarts; "aaa\0b" ends before the b
    assert emitted[b"\x7f\x80"] == 0b00001000               # the STR entry's key part holds the other one
    assert emitted[b"\xff"] == 0b01011000
    assert emitted[b"\x80\x01"] == 0 and emitted[b"\xff\x01"] == 0b01000000


def test_adversarial_value_finishes(host):
    case, needle = U.adversarial_case()
    e, dnum, _ = check_host(host, case, U.OP_GREP, needle, forms=((1, 1), (0, 0)))
    assert (e, dnum) == (0, 0)
    e, dnum, _ = check_host(host, case, U.OP_GREP, b"a" * 160, forms=((1, 1),))
    assert (e, dnum) == (0, 1024)


def test_every_residue_and_cap(host):
    case, _ = U.grep_cases(b"ab")
    total = len(U.listing(case[1], case[3], U.OP_GREP, b"ab")[5])
    for shift in range(16):
        check_host(host, case, U.OP_GREP, b"ab", forms=((1, 1),), caps=[total, total - 1, total // 2],
                   shift=shift, oshift=(7 * shift + 3) % 16)


def test_checker_passes():
    """itb_keys_check: itb_keys_one and the wave plan against a naive walk,
    over exact-size heap blocks (under ASan/UBSan where their runtimes link)."""
    res = subprocess.run([os.path.join(NATIVE, "itb_keys_check")], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "itb_keys_check: ok" in res.stdout


# ---------------------------------------------------------------------------
# The product library without a GPU
# ---------------------------------------------------------------------------
def _batch(op, needle_len, n=1):
    lib = lzo.load()
    kvlist._lib()
    rec = bytes(U.make_record(1, 2, 1, [0, 1]))
    buf = np.frombuffer(rec, dtype=np.uint8)
    ptrs = (ctypes.c_void_p * 1)(buf.ctypes.data)
    lens = (ctypes.c_size_t * 1)(buf.size)
    out = np.zeros(4096, dtype=np.uint8)
    first = np.zeros(2, dtype=np.uint64)
    u = [np.zeros(1, dtype=np.uint32) for _ in range(3)]
    err = np.zeros(1, dtype=np.int32)
    needle = np.zeros(300, dtype=np.uint8)
    return lib.pom_kvlist_batch(ptrs, lens, n, op, needle.ctypes.data, needle_len, out.ctypes.data, out.size,
                                first.ctypes.data, u[0].ctypes.data, u[1].ctypes.data, u[2].ctypes.data, None,
                                err.ctypes.data, None, None)


def test_batch_rejects_bad_op_and_needle_length():
    assert _batch(4, 0) == U.EINVAL and _batch(0xFFFFFFFF, 0) == U.EINVAL
    assert _batch(2, 256) == U.EINVAL and _batch(0, 256) == U.EINVAL
    with pytest.raises(ValueError):
        kvlist.scan_batch([], op=4)
    with pytest.raises(ValueError):
        kvlist.scan_batch([], op=2, needle=b"x" * 256)


def test_batch_refuses_without_a_gpu():
    if lzo.load().lzo_mi355x_device_count() > 0:
        pytest.skip("a GPU is present")
    assert _batch(0, 0) == lzo.LZO_E_ERROR and _batch(3, 255) == lzo.LZO_E_ERROR
    with pytest.raises(RuntimeError):
        kvlist.scan_batch([bytes(U.make_record(1, 2, 1, [0, 1]))])


def test_exports():
    assert "pom_kvlist_dev" in lzo.EXPORTS and "pom_kvlist_batch" in lzo.EXPORTS


def test_parse():
    assert kvlist.parse(b"\x01\0\0\0a\0\0\0\0\x02\0\0\0bc") == [b"a", b"", b"bc"]
    with pytest.raises(ValueError):
        kvlist.parse(b"\x02\0\0\0a")
    with pytest.raises(ValueError):
        kvlist.parse(b"\x02\0")
