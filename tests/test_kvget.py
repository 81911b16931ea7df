"""CPU: the key/value point get (include/pom_kvget.h) without a GPU -- the
header's layout constants against the reference's structs, the shared rules
and the wave's granule plan (pomegranate_amd/csrc/itb_kvget.h, compiled as
plain C++) against the Python restatement of mds/itb.c:1095-1116, :1769-1814
and mds/cbht.c:929-977 in kvget_util.py, the stand-alone checker, the exports,
and the refusal without a GPU."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import kvget_util as U
from conftest import ROOT
from pomegranate_amd import kvget, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"
POISON = 0xA5


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_kvget.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof / sizeof and the flag values of the reference's own headers
    (LP64, its build flags) against every macro of pom_kvget.h."""
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
    P("POM_KG_LOOKUP", INDEX_LOOKUP);
    P("POM_KG_COLUMN", INDEX_COLUMN);
    P("POM_KG_KV", INDEX_KV);
    P("POM_KG_MAX_COLUMN", HVFS_KV_MAX_COLUMN);
    P("POM_KG_KVFLAG_MASK", HVFS_KV_NORMAL | HVFS_KV_STR | HVFS_KV_MAX_COLUMN);
    P("POM_KG_LEASE_OFF", offsetof(struct ite, s.mdu.dtime));
    P("POM_KG_REC_MAX", KV_HEADER_LEN + sizeof(((struct kv *)0)->value) + sizeof(struct column));
    P("kv_off", offsetof(struct ite, v));
    P("kv_flags", offsetof(struct ite, v.flags));
    P("kv_len", offsetof(struct ite, v.len));
    P("kv_key", offsetof(struct ite, v.key));
    P("kv_klen", offsetof(struct ite, v.klen));
    P("kv_value", offsetof(struct ite, v.value));
    P("kv_value_size", sizeof(((struct kv *)0)->value));
    P("kv_size", sizeof(struct kv));
    P("kv_header_len", KV_HEADER_LEN);
    P("column_off", offsetof(struct ite, column));
    P("column_size", sizeof(struct column));
    P("columns", sizeof(((struct ite *)0)->column) / sizeof(struct column));
    P("kv_normal", HVFS_KV_NORMAL);
    P("kv_str", HVFS_KV_STR);
    P("dtime_in_value", offsetof(struct ite, s.mdu.dtime) - offsetof(struct ite, v.value));
    P("dtime_size", sizeof(((struct mdu *)0)->dtime));
    P("hi_kvflag_size", sizeof(((struct hvfs_index *)0)->kvflag));
    P("hi_hash_size", sizeof(((struct hvfs_index *)0)->hash));
    P("hi_uuid_size", sizeof(((struct hvfs_index *)0)->uuid));
    P("einval", -EINVAL);
    P("enoent", -ENOENT);
    P("md_reply_with_kv", MD_REPLY_WITH_KV);
    return 0;
}
''')
    exe = tmp_path / "probe"
    inc = [f"-I{os.path.join(REFERENCE, d)}" for d in ("include", "lib", "mds", "xnet", "mdsl", "r2")]
    subprocess.run(["gcc", "-w", "-D__CORES__=8", "-DDISABLE_PYTHON=1", f"-I{tmp_path}", *inc,
                    str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    want = header_macros()
    assert (want.pop("POM_KG_E_VALUE"), want.pop("POM_KVGET_H")) == (-4102, 1)       # (the code, the include guard)
    assert want == {k: v for k, v in got.items() if k.startswith("POM_")}
    # the test oracle's own constants are the reference's too
    assert (U.KV_OFF, U.KV_OFF, U.KV_OFF + 4, 32, 40, U.VALUE_OFF, U.VALUE_MAX, 344, U.KV_HEADER_LEN) == tuple(
        got[k] for k in ("kv_off", "kv_flags", "kv_len", "kv_key", "kv_klen", "kv_value", "kv_value_size", "kv_size",
                         "kv_header_len"))
    assert (U.COLUMN_OFF, 24, 6, U.KV_NORMAL, U.KV_STR) == tuple(
        got[k] for k in ("column_off", "column_size", "columns", "kv_normal", "kv_str"))
    assert (U.F_LOOKUP, U.F_COLUMN, U.F_KV, U.MAX_COLUMN, U.KVFLAG_MASK, U.LEASE_OFF, U.REC_MAX) == tuple(
        got[k] for k in ("POM_KG_LOOKUP", "POM_KG_COLUMN", "POM_KG_KV", "POM_KG_MAX_COLUMN", "POM_KG_KVFLAG_MASK",
                         "POM_KG_LEASE_OFF", "POM_KG_REC_MAX"))
    # the lease word is v.value[36 ... 43]; the request's fields hold what the reference carries
    assert (got["dtime_in_value"], got["dtime_size"]) == (36, 8)
    # (hi->kvflag is a u16: the request's u32 holds it with room to spare)
    assert (got["hi_kvflag_size"], got["hi_hash_size"], got["hi_uuid_size"]) == (2, 8, 8)
    assert (got["einval"], got["enoent"], got["md_reply_with_kv"]) == (U.EINVAL, U.ENOENT, 0x0200)


def test_kvget_py_mirrors_the_header():
    want = header_macros()
    del want["POM_KVGET_H"]
    for macro, value in want.items():
        assert getattr(kvget, macro[4:]) == value, macro
    assert kvget.REQ_DTYPE.itemsize == 32 and kvget.REQ_DTYPE.alignment <= 8
    assert [kvget.REQ_DTYPE.fields[k][1] for k in ("key", "itb", "flag", "kvflag", "skey_off", "sklen", "reserved")] \
        == [0, 8, 12, 16, 20, 24, 28]
    assert (kvget.E_TRUNCATED, kvget.E_NOSPACE, kvget.E_LOOP, kvget.EINVAL, kvget.ENOENT, kvget.ESPLIT) == \
        (U.E_TRUNCATED, U.E_NOSPACE, U.E_LOOP, U.EINVAL, U.ENOENT, U.ESPLIT)
    assert (kvget.KV_NORMAL, kvget.KV_STR, kvget.KV_HEADER_LEN, kvget.KV_VALUE_MAX) == (0x8000, 0x4000, 20, 320)


# ---------------------------------------------------------------------------
# libitb_kvget_host.so (itb_kvget.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_get():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_kvget_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.itb_kvget_batch_host.restype = ctypes.c_int
    lib.itb_kvget_batch_host.argtypes = [vp] * 5 + [u32, vp, u32, vp, u32] + [vp] * 7 + [ctypes.c_uint64, ctypes.c_int]

    def run(payloads, adepths, req, keys, pshift=0, kshift=0, oshift=0, per_lane=0, status=None, out_cap=None):
        """-> (err, nr, depth, len, lease, first, out bytes below the cap).
        Payload b sits at residue (pshift + b) mod 16, the blob at kshift, the
        output at oshift, each in a buffer of its own; every output is
        poisoned around what is its own."""
        n, nreq = len(payloads), len(req)
        off, pos = [], 0
        for b, p in enumerate(payloads):
            pos = (pos + 15) // 16 * 16 + (pshift + b) % 16
            off.append(pos)
            pos += len(p)
        room = np.zeros(pos + 32, dtype=np.uint8)
        base = (-room.ctypes.data) % 16
        for o, p in zip(off, payloads):
            room[base + o: base + o + len(p)] = np.frombuffer(p, dtype=np.uint8)
        blob = np.zeros(len(keys) + 32, dtype=np.uint8)
        ka = (-blob.ctypes.data) % 16 + kshift
        blob[ka: ka + len(keys)] = np.frombuffer(keys, dtype=np.uint8)
        cap = U.REC_MAX * nreq if out_cap is None else out_cap
        out = np.full(cap + 64, POISON, dtype=np.uint8)
        oa = (-out.ctypes.data) % 16 + oshift
        res = np.full((4, nreq + 2), 0x5A5A5A5A, dtype=np.uint32)
        res64 = np.full((2, nreq + 3), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        req = np.ascontiguousarray(req)
        offs = np.array(off, dtype=np.uint64)
        lens = np.array([len(p) for p in payloads], dtype=np.uint32)
        ads = np.array(adepths, dtype=np.uint8)
        st = None if status is None else np.array(status, dtype=np.int32)
        assert lib.itb_kvget_batch_host(room.ctypes.data + base, offs.ctypes.data, lens.ctypes.data,
                                        None if st is None else st.ctypes.data, ads.ctypes.data, n,
                                        req.ctypes.data, nreq, blob.ctypes.data + ka, len(keys),
                                        res[0, 1:].ctypes.data, res[1, 1:].ctypes.data, res[2, 1:].ctypes.data,
                                        res[3, 1:].ctypes.data, res64[0, 1:].ctypes.data, res64[1, 1:].ctypes.data,
                                        out.ctypes.data + oa, cap, per_lane) == 0
        assert (res[:, 0] == 0x5A5A5A5A).all() and (res[:, -1] == 0x5A5A5A5A).all()
        assert res64[0, 0] == res64[1, 0] == res64[0, nreq + 1] == res64[1, nreq + 2] == 0x5A5A5A5A5A5A5A5A
        first = res64[1, 1: nreq + 2]
        used = min(int(first[nreq]), cap)
        assert (out[:oa] == POISON).all() and (out[oa + used:] == POISON).all()
        return (res[0, 1:-1].view(np.int32), res[1, 1:-1], res[2, 1:-1], res[3, 1:-1], res64[0, 1: nreq + 1], first,
                out[oa: oa + used].tobytes())
    return run


@pytest.fixture(scope="module")
def families():
    """Every case family once, with the oracle's answer worked out."""
    fams = {}
    for name, fam in U.FAMILIES.items():
        recs, adepths, req, keys = fam()
        fams[name] = (recs, adepths, req, keys, U.Want([U.payload_of(r) for r in recs], adepths, req, keys))
    return fams


def agree(host_get, recs, adepths, req, keys, want=None, status=None):
    """The batch as the kernels cut it -- the granule copy and the byte copy,
    aligned and unaligned outputs, shifted payloads and blob."""
    payloads = [U.payload_of(r) for r in recs]
    want = U.Want(payloads, adepths, req, keys, status) if want is None else want
    U.same(host_get(payloads, adepths, req, keys, status=status), want)
    U.same(host_get(payloads, adepths, req, keys, 3, 5, 0, 1, status=status), want)
    U.same(host_get(payloads, adepths, req, keys, 8, 1, 9, status=status), want)
    U.same(host_get(payloads, adepths, req, keys, 7, 3, 1, 1, status=status), want)
    return want


def test_values_and_columns(host_get, families):
    """v.len 0 ... 321 without a column, with columns 0 ... 5 and with column 6."""
    recs, adepths, req, keys, want = families["values"]
    agree(host_get, recs, adepths, req, keys, want)
    rec = recs[0]
    for nr, vlen in enumerate(U.VLENS):
        rows = range(8 * nr, 8 * nr + 8)
        ite = U.H + U.ITE_OFF + U.ITE_SIZE * nr
        if vlen > 320:
            assert [int(want.err[r]) for r in rows] == [U.E_VALUE] * 7 + [U.EINVAL]
            assert not want.len[list(rows)].any() and not want.lease[list(rows)].any()
            continue
        assert [int(want.err[r]) for r in rows] == [0] * 7 + [U.EINVAL]
        assert [int(want.len[r]) for r in rows] == [20 + vlen] + [44 + vlen] * 6 + [0]
        assert want.recs[8 * nr] == bytes(rec[ite + 24: ite + 44 + vlen])
        for c in range(6):
            assert want.recs[8 * nr + 1 + c] == bytes(rec[ite + 24: ite + 44 + vlen]) + \
                bytes(rec[ite + 368 + 24 * c: ite + 392 + 24 * c])
        assert int(want.lease[8 * nr]) == int.from_bytes(rec[ite + 80: ite + 88], "little")
        # the record holds the lease word only from v.len 44 on
        if vlen >= 44:
            assert want.recs[8 * nr][56:64] == bytes(rec[ite + 80: ite + 88])
        flags, ln, key, klen, value, column = kvget.parse(want.recs[8 * nr + 3], column=True)
        assert (ln, key, value) == (vlen, int(req[8 * nr]["key"]), bytes(rec[ite + 44: ite + 44 + vlen]))
        assert column == tuple(int.from_bytes(rec[ite + 416 + 8 * i: ite + 424 + 8 * i], "little") for i in range(3))
    assert want.err[-2:].tolist() == [0, 0] and want.len[-2:].tolist() == [32, 56]


def test_string_keys_at_every_residue(host_get, families):
    recs, adepths, req, keys, want = families["strkeys"]
    payloads = [U.payload_of(recs[0])]
    for shift in range(8):
        U.same(host_get(payloads, adepths, req, keys, shift, shift, shift), want)
        U.same(host_get(payloads, adepths, req, keys, (3 * shift) % 16, 7 - shift, shift + 8, 1), want)
    r = 0
    for nr, k in enumerate(U.SKLENS):
        n = 8 + (4 if 0 < k <= 320 else 0)
        e = want.err[r: r + n].tolist()
        if k > 320:
            assert e == [U.ENOENT] * 8 and (want.depth[r: r + n] >= 1).all()
        else:
            assert e[:8] == [0] * 8 and (want.nr[r: r + 8] == nr).all() and e[8:] == [U.ENOENT] * (n - 8)
        r += n
    tail = want.err[r:].tolist()
    assert tail[0] == 0 and tail[1:12] == [U.EINVAL] * 11 and tail[12:20] == [U.EINVAL] * 8
    assert tail[20:] == [0, U.EINVAL, 0, U.EINVAL, U.EINVAL, 0, U.ENOENT, U.ENOENT]


def test_matching_corners_and_chains(host_get, families):
    recs, adepths, req, keys, want = families["corners"]
    agree(host_get, recs, adepths, req, keys, want)
    e, nr = want.err.tolist(), want.nr.tolist()
    assert (e[0], nr[0], e[1], nr[1]) == (0, 0, 0, 0)               # NORMAL and STR gets of a STR entry
    assert (e[2], nr[2], e[3], e[4], nr[4]) == (0, 1, U.ENOENT, 0, 1)       # STR gets of a NORMAL entry
    # one v.key, klen 3, 5, 3: add_index leaves the chain as 4, 2, 3
    assert (e[5:9], nr[5:9]) == ([0, 0, 0, U.ENOENT], [4, 4, 3, 0])
    assert e[9:13] == [U.EINVAL, U.EINVAL, U.E_VALUE, U.E_VALUE]
    assert want.depth[13: 21].tolist() == [7, 8, 6, 5, 4, 3, 2, 1] and e[21] == U.ENOENT and want.depth[21] == 8
    assert want.depth.max() == 1024 and e[-1] == U.ENOENT and (want.err[22:-1] == 0).all()


def test_handmade_tables(host_get, families):
    recs, adepths, req, keys, want = families["handmade"]
    agree(host_get, recs, adepths, req, keys, want)
    e, d = want.err.tolist(), want.depth.tolist()
    assert (e[0], d[0], e[1], d[1]) == (0, 1, U.ENOENT, 1)
    assert (e[2:5], d[2:5], want.nr[3], want.len[3]) == ([0, 0, U.ENOENT], [1, 2, 2], 3, 20 + 12 + 24)
    assert (e[5:7], d[5:7]) == ([0, U.ENOENT], [1, 1])
    assert (e[7], d[7], e[8], d[8]) == (0, 1, U.E_LOOP, 2048)                        # the self-loop
    assert e[9:13] == [0, 0, U.E_LOOP, U.E_LOOP] and d[9:13] == [1, 2, 2048, 2048]  # the 2-cycle
    assert e[13:16] == [U.E_TRUNCATED] * 3 and d[13:16] == [1, 1, 1]
    # one byte short: ITE 7 is cut for the requests that reach it, ITE 6 before it is whole
    assert e[16 + 9] == 0 and e[16 + 10] == U.E_TRUNCATED and d[16 + 10] == 2
    assert e[16 + 11] == U.E_TRUNCATED and e[16 + 13: 32] == [U.E_TRUNCATED] * 3
    bad = want.err != 0
    assert not want.len[bad].any() and not want.nr[bad].any() and not want.lease[bad].any()


def test_mixed_batch_and_request_counts(host_get, families):
    """The mixed family, shuffled; then 1, 2, 63, 64, 65, 129 and 257 requests
    with out at residues 0, 8 and 1, in both copy forms: identical bytes."""
    recs, adepths, req, keys, want = families["mixed"]
    assert len(req) > 500 and (want.err == 0).sum() > 200 and (want.err == U.ENOENT).sum() > 200
    assert want.depth.max() >= 3 and set(want.err.tolist()) == {0, U.ENOENT}
    order = np.random.default_rng(5).permutation(len(req))
    agree(host_get, recs, adepths, req[order], keys, want.pick(order))
    payloads = [U.payload_of(r) for r in recs]
    for nreq in (1, 2, 63, 64, 65, 129, 257):
        pick = np.arange(nreq) * 3 % len(req)
        sub = want.pick(pick)
        assert (sub.err != 0).any() or nreq < 3
        outs = [host_get(payloads, adepths, req[pick], keys, 0, 0, oshift, per_lane)
                for oshift in (0, 8, 1) for per_lane in (0, 1)]
        for got in outs:
            U.same(got, sub)
        assert all(got[6] == outs[0][6] for got in outs)


def test_out_cap_cuts(host_get, families):
    """out_cap inside a header, inside a value, inside a column, at a record's
    end and at 0: first[] and the per-request arrays are complete, and only
    out[0, out_cap) is written (the runner checks the poison behind it)."""
    recs, adepths, req, keys, want = families["values"]
    payloads = [U.payload_of(r) for r in recs]
    r = 8 * 6 + 2                                       # v.len 28 with column 1: 72 bytes
    f = int(want.first[r])
    assert want.len[r] == 72
    for cap in (0, 1, f + 7, f + 25, f + 48 + 5, f + 72, f - 1, int(want.first[-1]) - 1):
        for oshift in (0, 5):
            for per_lane in (0, 1):
                U.same(host_get(payloads, adepths, req, keys, 2, 0, oshift, per_lane, out_cap=cap), want, cap)


def test_rule_order_and_itb_range(host_get):
    """status, then adepth, then the index table's presence, then the request's
    own checks; itb >= nitb is -EINVAL before any of them."""
    recs, adepths, status, req, keys = U.rule_order_case()
    want = agree(host_get, recs, adepths, req, keys, status=status)
    assert want.err.tolist() == [0, U.EINVAL, -6, -6, -5, -5, U.E_TRUNCATED, U.E_TRUNCATED] + [U.EINVAL] * 6


def test_random_tables(host_get):
    """Seeded random slots over KV entries -- every flag, entries and conflicts
    over all 15 bits now and then -- and payloads cut at random."""
    rng = np.random.default_rng(0x6B76)
    for t in range(10):
        n_ites = int(rng.integers(1, 41))
        adepth = int(rng.integers(1, 11))
        keys_of = [int(rng.integers(0, 1 << 62)) for _ in range(n_ites)]
        kv = {nr: dict(flags=int(rng.choice([U.KV_NORMAL, U.KV_STR, 0, 0xC000])) if rng.random() < 0.9 else 0,
                       klen=int(rng.integers(0, 12)), vlen=int(rng.choice(U.VLENS))) for nr in range(n_ites)}
        rec = U.make_table(8500 + t, n_ites, adepth, {}, {nr: dict(key=keys_of[nr], **kv[nr]) for nr in range(n_ites)})
        for off in range(2048):
            wild = rng.random() < 0.05
            U.set_slot(rec, U.H, off, int(rng.integers(0, 32768 if wild else n_ites)),
                       int(rng.integers(0, 32768 if wild else 2048)), int(rng.integers(0, 4)))
        blob, rows = U.Blob(), []
        for nr in range(n_ites):
            _, _, key, klen, value = U.kv_fields(rec, nr)
            col = int(rng.integers(0, 6))
            rows.append((key, 0, U.GET | (U.F_COLUMN if nr % 2 else 0), U.KV_NORMAL | col, 0, 0))
            rows.append((key, 0, U.GET, U.KV_STR | col, blob.put(value[:klen]), klen))
            rows.append((int(rng.integers(0, 1 << 62)), 0, U.GET, U.KV_NORMAL, 0, 0))
        if t % 3 == 0:
            cut = int(rng.integers(1, 700))
            rec = bytearray(rec[: len(U.payload_of(rec)) + U.H - cut])
            rec[240:244] = np.uint32(len(rec)).tobytes()
        agree(host_get, [rec], [adepth], U.rows_to_req(rows), bytes(blob.bytes))


def test_itb_kvget_check_passes():
    """The stand-alone checker (itb_kvget.h against its own naive walk, every
    payload, blob and capped output ending where its heap block ends; built
    with AddressSanitizer and UBSan where they link) exits 0."""
    r = subprocess.run([os.path.join(NATIVE, "itb_kvget_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_kvget_check: ok" in r.stdout


def test_requests_and_parse():
    req, blob = kvget.requests([dict(itb=0, key=7), dict(itb=1, key=8, skey=b"abc"),
                                dict(itb=2, key=9, skey=b"", flag=kvget.KG_KV | kvget.KG_COLUMN, kvflag=kvget.KV_STR | 3)])
    assert blob == b"abc" and req["sklen"].tolist() == [0, 3, 0] and req["skey_off"].tolist() == [0, 0, 3]
    assert req["kvflag"].tolist() == [0x8000, 0x4000, 0x4003] and req["flag"][0] == 0x40000010
    rec = bytes(range(20 + 9 + 24))
    rec = rec[:4] + (9).to_bytes(4, "little") + rec[8:]
    flags, ln, key, klen, value, column = kvget.parse(rec, column=True)
    assert (flags, ln, klen, value) == (0x03020100, 9, int.from_bytes(rec[16:20], "little"), rec[20:29])
    assert key == int.from_bytes(rec[8:16], "little")
    assert column == tuple(int.from_bytes(rec[29 + 8 * i: 37 + 8 * i], "little") for i in range(3))
    assert kvget.parse(rec[:29])[5] is None
    with pytest.raises(ValueError):
        kvget.parse(rec[:28])
    with pytest.raises(ValueError):
        kvget.parse(rec[:19])


def test_exports_are_declared():
    assert {"pom_kvget_dev", "pom_kvget_batch"} <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert hasattr(lib, "pom_kvget_dev") and hasattr(lib, "pom_kvget_batch")
    text = open(os.path.join(ROOT, "include", "pom_kvget.h")).read()
    assert re.search(r"\bint pom_kvget_dev\(", text) and re.search(r"\bint pom_kvget_batch\(", text)
    # the launcher and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_kvget", "pom_kvget_chunked"} & set(lzo.EXPORTS)


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_kvget_batch_refuses():
    recs, _, req, keys = U.family_handmade()
    res = None
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        res = kvget.kvget_batch(recs, req, keys)
    assert res is None
    # and the C call itself, with no request at all
    assert kvget._lib().pom_kvget_batch(None, None, 0, 0, None, 0, None, 0, None, 0, None, None, None, None, None,
                                        None) == lzo.LZO_E_ERROR
