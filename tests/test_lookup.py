"""CPU: the lookup (include/pom_lookup.h) without a GPU -- the header's layout
constants against the reference's structs, the shared walk and the wave's copy
plan (pomegranate_amd/csrc/itb_find.h, compiled as plain C++) against the
Python restatement of mds/itb.c:1769-1814 in lookup_util.py, the stand-alone
checker, the exports, and the refusal without a GPU."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import lookup_util as U
from conftest import ROOT
from pomegranate_amd import lookup, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"
POISON = 0xA5


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_lookup.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof / sizeof over the reference's own headers (LP64, its build
    flags), against every macro of pom_lookup.h; the bit-field packing of
    struct itb_index is read off words the reference's struct was filled into."""
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
static long word(unsigned entry, unsigned conflict, unsigned flag)
{
    struct itb_index ii;
    unsigned w;
    memset(&ii, 0, sizeof ii);
    ii.entry = entry;
    ii.conflict = conflict;
    ii.flag = flag;
    memcpy(&w, &ii, 4);
    return w;
}
int main(void)
{
    P("POM_ITB_INDEX_ENTRIES", sizeof(((struct itb *)0)->index) / sizeof(struct itb_index));
    P("POM_ITB_INDEX_SIZE", sizeof(struct itb_index));
    P("POM_IDX_FREE", ITB_INDEX_FREE);
    P("POM_IDX_UNIQUE", ITB_INDEX_UNIQUE);
    P("POM_IDX_CONFLICT", ITB_INDEX_CONFLICT);
    P("POM_IDX_OVERFLOW", ITB_INDEX_OVERFLOW);
    P("POM_ITE_HASH_OFF", offsetof(struct ite, hash));
    P("POM_ITE_MD_OFF", offsetof(struct ite, g));
    P("POM_MDU_SIZE", HVFS_MDU_SIZE);
    P("POM_MDU_DTIME_OFF", offsetof(struct ite, s.mdu.dtime) - offsetof(struct ite, g));
    P("POM_ITE_UNLINKED", ITE_UNLINKED);
    P("POM_ITE_SHADOW", ITE_SHADOW);
    P("POM_ITBH_FLAG_OFF", offsetof(struct itbh, flag));
    P("POM_ITBH_DEPTH_OFF", offsetof(struct itbh, depth));
    P("POM_ITBH_ITBID_OFF", offsetof(struct itbh, itbid));
    P("POM_ITB_JUST_SPLIT", ITB_JUST_SPLIT);
    P("POM_LK_BY_NAME", INDEX_BY_NAME);
    P("POM_LK_BY_UUID", INDEX_BY_UUID);
    P("POM_LK_LOOKUP", INDEX_LOOKUP);
    P("POM_LK_COLUMN", INDEX_COLUMN);
    P("POM_LK_ITE_ACTIVE", INDEX_ITE_ACTIVE);
    P("POM_LK_ITE_SHADOW", INDEX_ITE_SHADOW);
    P("POM_LK_REC_SIZE", sizeof(u64) + HVFS_MDU_SIZE + sizeof(struct column));
    P("POM_LK_E_NOENT", -ENOENT);
    P("POM_LK_E_SPLIT", -ESPLIT);
    P("total", 1 << (ITB_DEPTH + 1));
    P("itb_depth", ITB_DEPTH);
    P("s_off", offsetof(struct ite, s));
    P("v_off", offsetof(struct ite, v));
    P("ite_uuid_size", sizeof(((struct ite *)0)->uuid));
    P("hi_namelen_size", sizeof(((struct hvfs_index *)0)->namelen));
    P("itbid_size", sizeof(((struct itbh *)0)->itbid));
    P("depth_size", sizeof(((struct itbh *)0)->depth));
    P("w_entry_1", word(1, 0, 0));
    P("w_entry_max", word(0x7FFF, 0, 0));
    P("w_conflict_1", word(0, 1, 0));
    P("w_conflict_max", word(0, 0x7FFF, 0));
    P("w_flag_1", word(0, 0, 1));
    P("w_flag_3", word(0, 0, 3));
    P("w_mixed", word(0x1234, 0x4321, 2));
    return 0;
}
''')
    exe = tmp_path / "probe"
    inc = [f"-I{os.path.join(REFERENCE, d)}" for d in ("include", "lib", "mds", "xnet", "mdsl", "r2")]
    subprocess.run(["gcc", "-w", "-D__CORES__=8", "-DDISABLE_PYTHON=1", f"-I{tmp_path}", *inc,
                    str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert (got.pop("total"), got.pop("itb_depth")) == (2048, 10)
    assert got.pop("s_off") == got.pop("v_off") == got["POM_ITE_MD_OFF"]
    assert (got.pop("ite_uuid_size"), got.pop("hi_namelen_size"), got.pop("itbid_size"), got.pop("depth_size")) == \
        (8, 1, 8, 1)
    want = header_macros()
    assert (want.pop("POM_LK_E_LOOP"), want.pop("POM_LOOKUP_H")) == (-4100, 1)       # (the code, the include guard)
    # entry in bits 0 ... 14, conflict in bits 15 ... 29, flag in bits 30 ... 31
    bits, shift = want.pop("POM_IDX_ENTRY_BITS"), want.pop("POM_IDX_FLAG_SHIFT")
    assert (bits, shift) == (15, 30)
    assert (got.pop("w_entry_1"), got.pop("w_entry_max")) == (1, (1 << bits) - 1)
    assert (got.pop("w_conflict_1"), got.pop("w_conflict_max")) == (1 << bits, ((1 << bits) - 1) << bits)
    assert (got.pop("w_flag_1"), got.pop("w_flag_3")) == (1 << shift, 3 << shift)
    assert got.pop("w_mixed") == 0x1234 | 0x4321 << bits | 2 << shift
    assert want == got
    assert (got["POM_ITE_MD_OFF"], got["POM_MDU_SIZE"], got["POM_LK_REC_SIZE"]) == (24, 104, 136)
    # the test oracle's own constants are the reference's too
    assert (U.INDEX_ENTRIES, U.MD_OFF, U.MDU_SIZE, U.REC_SIZE, U.ESPLIT, U.ENOENT, U.ITBH_FLAG, U.ITBH_DEPTH,
            U.ITBH_ITBID, U.ITB_JUST_SPLIT) == tuple(got[k] for k in (
                "POM_ITB_INDEX_ENTRIES", "POM_ITE_MD_OFF", "POM_MDU_SIZE", "POM_LK_REC_SIZE", "POM_LK_E_SPLIT",
                "POM_LK_E_NOENT", "POM_ITBH_FLAG_OFF", "POM_ITBH_DEPTH_OFF", "POM_ITBH_ITBID_OFF",
                "POM_ITB_JUST_SPLIT"))


def test_lookup_py_mirrors_the_header():
    want = header_macros()
    names = {"POM_ITB_INDEX_ENTRIES": "ITB_INDEX_ENTRIES", "POM_ITB_INDEX_SIZE": "ITB_INDEX_SIZE",
             "POM_LK_E_LOOP": "E_LOOP", "POM_LK_E_NOENT": "ENOENT", "POM_LK_E_SPLIT": "ESPLIT",
             "POM_LK_REC_SIZE": "REC_SIZE"}
    del want["POM_LOOKUP_H"]
    for macro, value in want.items():
        mirror = names.get(macro, macro[4:])
        assert getattr(lookup, mirror) == value, macro
    assert lookup.REQ_DTYPE.itemsize == 32
    assert [lookup.REQ_DTYPE.fields[k][1] for k in ("hash", "uuid", "itb", "flag", "name_off", "namelen", "column")] \
        == [0, 8, 16, 20, 24, 28, 30]
    assert (lookup.E_TRUNCATED, lookup.EINVAL) == (-4097, -22)


# ---------------------------------------------------------------------------
# libitb_find_host.so (itb_find.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_find():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_find_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.itb_find_host.restype = ctypes.c_int
    lib.itb_find_host.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, vp]
    lib.itb_find_batch_host.restype = ctypes.c_int
    lib.itb_find_batch_host.argtypes = [vp] * 5 + [u32, vp, u32, vp, u32] + [vp] * 4 + [ctypes.c_int]

    def run(payloads, adepths, req, names, pshift=0, nshift=0, oshift=0, per_lane=0, status=None, single=False):
        """-> (err, nr, depth, out[nreq, 136]).  Payload b sits at residue
        (pshift + b) mod 16, the blob at nshift, the output at oshift, each in
        a buffer of its own; the outputs are poisoned around what is theirs."""
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
        blob = np.zeros(len(names) + 32, dtype=np.uint8)
        na = (-blob.ctypes.data) % 16 + nshift
        blob[na: na + len(names)] = np.frombuffer(names, dtype=np.uint8)
        out = np.full(lookup.REC_SIZE * nreq + 64, POISON, dtype=np.uint8)
        oa = (-out.ctypes.data) % 16 + oshift
        res = np.full((3, nreq + 2), 0x5A5A5A5A, dtype=np.uint32)
        req = np.ascontiguousarray(req)
        if single:
            assert n == 1 and status is None
            for r in range(nreq):
                q = req[r: r + 1].copy()
                res[0, 1 + r] = np.uint32(lib.itb_find_host(room.ctypes.data + base + off[0], len(payloads[0]),
                                                            adepths[0], q.ctypes.data, blob.ctypes.data + na,
                                                            len(names), res[1, 1 + r:].ctypes.data,
                                                            res[2, 1 + r:].ctypes.data,
                                                            out.ctypes.data + oa + lookup.REC_SIZE * r) & 0xFFFFFFFF)
        else:
            offs = np.array(off, dtype=np.uint64)
            lens = np.array([len(p) for p in payloads], dtype=np.uint32)
            ads = np.array(adepths, dtype=np.uint8)
            st = None if status is None else np.array(status, dtype=np.int32)
            assert lib.itb_find_batch_host(room.ctypes.data + base, offs.ctypes.data, lens.ctypes.data,
                                           None if st is None else st.ctypes.data, ads.ctypes.data, n,
                                           req.ctypes.data, nreq, blob.ctypes.data + na, len(names),
                                           res[0, 1:].ctypes.data, res[1, 1:].ctypes.data, res[2, 1:].ctypes.data,
                                           out.ctypes.data + oa, per_lane) == 0
        assert (res[:, 0] == 0x5A5A5A5A).all() and (res[:, -1] == 0x5A5A5A5A).all()
        assert (out[:oa] == POISON).all() and (out[oa + lookup.REC_SIZE * nreq:] == POISON).all()
        return (res[0, 1:-1].view(np.int32), res[1, 1:-1], res[2, 1:-1],
                out[oa: oa + lookup.REC_SIZE * nreq].reshape(nreq, lookup.REC_SIZE))
    return run


def same(got, want):
    for g, w, what in zip(got, want, ("err", "nr", "depth", "out")):
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert len(bad) == 0, f"{what}: request {int(bad[0])}: {g[bad[0]]} != {w[bad[0]]}"


def agree(host_find, recs, adepths, req, names, status=None, singles=True):
    """The batch as the kernel cuts it -- the granule copy, the byte copy, an
    unaligned output, shifted payloads and blob -- and, where there is one ITB,
    request by request.  Returns the oracle's answer."""
    payloads = [U.payload_of(r) for r in recs]
    want = U.expect(payloads, adepths, req, names, status)
    same(host_find(payloads, adepths, req, names, status=status), want)
    same(host_find(payloads, adepths, req, names, 3, 5, 0, 1, status=status), want)
    same(host_find(payloads, adepths, req, names, 8, 1, 9, status=status), want)
    if len(recs) == 1 and status is None and singles:
        same(host_find(payloads, adepths, req, names, 7, 3, 1, single=True), want)
    return want


def test_mixed_batch(host_find):
    recs, adepths, items = U.family_mixed()
    req, names = lookup.requests(items)
    order = np.random.default_rng(5).permutation(len(req))
    err, nr, depth, out = agree(host_find, recs, adepths, req[order], names)
    assert (err == 0).sum() > 700 and (err == U.ENOENT).sum() > 400 and set(err.tolist()) == {0, U.ENOENT}
    assert depth.max() >= 3
    # a hit's record: the ITE's uuid, then 104 bytes from byte 24, no column
    r = int(np.flatnonzero(err == 0)[0])
    q = req[order][r]
    ite = U.H + U.ITE_OFF + U.ITE_SIZE * int(nr[r])
    rec = recs[int(q["itb"])]
    assert out[r].tobytes() == bytes(rec[ite + 8: ite + 16]) + bytes(rec[ite + 24: ite + 128]) + bytes(24)
    uuid, mdu, column = lookup.parse(out[r])
    assert uuid == U.ite_fields(rec, U.H, int(nr[r]))[1] and len(mdu) == 104 and column == (0, 0, 0)


def test_chains(host_find):
    recs, adepths, items = U.family_chains()
    req, names = lookup.requests(items)
    err, nr, depth, _ = agree(host_find, recs, adepths, req, names)
    # the second entry goes behind the first, every later one to the head: 7, 6, 5, 4, 3, 2, 0, 1
    by_name_short = {int(nr[r]): int(depth[r]) for r in range(16) if err[r] == 0 and req[r]["flag"] & U.BY_NAME}
    assert by_name_short == {7: 1, 6: 2, 5: 3, 4: 4, 3: 5, 2: 6, 0: 7, 1: 8}
    assert depth.max() == 1024 and (err[req["itb"] == 1] == 0).sum() > 50


def test_handmade_tables(host_find):
    recs, adepths, items = U.family_handmade()
    req, names = lookup.requests(items)
    err, nr, depth, out = agree(host_find, recs, adepths, req, names)
    e, d = err.tolist(), depth.tolist()
    assert (e[0], d[0], e[1], d[1]) == (0, 1, U.ENOENT, 1)                       # A
    assert (e[2:5], d[2:5], nr[3]) == ([0, 0, U.ENOENT], [1, 2, 2], 3)           # B
    assert e[5:9] == [0, U.ENOENT, 0, U.ENOENT] and d[5:9] == [1, 1, 1, 1]       # C
    assert (e[9], d[9], e[10], d[10]) == (0, 1, U.E_LOOP, 2048)                  # D: the self-loop
    assert e[11:15] == [0, 0, U.E_LOOP, U.E_LOOP] and d[11:15] == [1, 2, 2048, 2048]
    assert e[15:19] == [U.E_TRUNCATED] * 4 and d[15:19] == [1, 1, 1, 1]          # E
    # one byte short: ITE 7 is cut for the requests that reach it, ITE 6 before it is whole
    assert e[19 + 11] == 0 and e[19 + 12] == U.E_TRUNCATED and d[19 + 12] == 2
    assert (e[19 + 15], e[19 + 16]) == (U.E_TRUNCATED, U.E_TRUNCATED)
    assert not out[err != 0].any() and not nr[err != 0].any()


def test_states(host_find):
    recs, adepths, items = U.family_states()
    req, names = lookup.requests(items)
    err, nr, depth, _ = agree(host_find, recs, adepths, req, names)
    found = {}
    for r in range(len(req)):
        extra = int(req[r]["flag"]) & (U.F_ACTIVE | U.F_SHADOW)
        if req[r]["flag"] & U.BY_UUID and err[r] == 0:
            found.setdefault(extra, set()).add(int(nr[r]))
    assert found[0] == {0, 2, 3, 4, 5, 6, 8}                        # UNLINKED is excluded
    assert found[U.F_ACTIVE] == {0, 4, 5, 6, 8}
    assert found[U.F_SHADOW] == {1, 3, 7}
    assert U.F_ACTIVE | U.F_SHADOW not in found                      # nothing is both
    # the duplicate names: the first in chain order wins
    by_name = {(int(req[r]["flag"]) & (U.F_ACTIVE | U.F_SHADOW), r % 18 // 2): int(nr[r])
               for r in range(len(req)) if req[r]["flag"] & U.BY_NAME and err[r] == 0}
    assert by_name[(0, 4)] == by_name[(0, 6)] == 6
    assert by_name[(0, 7)] == by_name[(0, 8)] == 8 and by_name[(U.F_SHADOW, 8)] == 7


def test_names_columns_and_refusals(host_find):
    recs, adepths, req, blob = U.family_names()
    for shift in range(8):
        payloads = [U.payload_of(recs[0])]
        want = U.expect(payloads, adepths, req, blob)
        same(host_find(payloads, adepths, req, blob, shift, shift, 0), want)
        same(host_find(payloads, adepths, req, blob, (3 * shift) % 16, 7 - shift, shift + 1, single=True), want)
    err, nr, _, out = want
    assert (err[:8] == 0).all() and (nr[:8] == 0).all()                 # the empty name, at every residue
    cols = [r for r in range(len(req)) if req[r]["flag"] & U.COLUMN]
    assert [int(err[r]) for r in cols] == [0, 0] * 6 + [U.EINVAL] * 2
    rec, ite = recs[0], U.H + U.ITE_OFF + U.ITE_SIZE * 5
    for r in cols[:12]:
        c = int(req[r]["column"])
        assert out[r, 112:].tobytes() == bytes(rec[ite + 368 + 24 * c: ite + 392 + 24 * c])
    assert (err == U.EINVAL).sum() == 15


def test_rule_order_and_itb_range(host_find):
    """status, then adepth, then the index table's presence, then the request's
    own checks; itb >= nitb is -EINVAL before any of them."""
    recs, adepths, items = U.family_chains()
    rec = recs[0]
    hsh, _, _, _, name = U.ite_fields(rec, U.H, 2)
    good = dict(hash=hsh, flag=U.BY_NAME, name=name)
    bad = dict(hash=hsh, flag=U.BY_NAME | 0x4, name=name)
    items = [dict(itb=b, **q) for b in range(6) for q in (good, bad)]
    req, names = lookup.requests(items)
    short = bytearray(rec[: U.H + U.ITE_OFF - 1])
    recs6 = [rec, rec, rec, short, rec]
    err, _, _, _ = agree(host_find, recs6, [3, 3, 0, 3, 11], req, names, status=[0, -6, -5, 0, 0])
    assert err.tolist() == [0, U.EINVAL, -6, -6, -5, -5, U.E_TRUNCATED, U.E_TRUNCATED, U.EINVAL, U.EINVAL,
                            U.EINVAL, U.EINVAL]


def test_random_tables(host_find):
    """Seeded random slots over real ITEs -- every flag, entries and conflicts
    over all 15 bits now and then -- and payloads cut at random."""
    rng = np.random.default_rng(0x10C)
    for t in range(12):
        n_ites = int(rng.integers(1, 40))
        adepth = int(rng.integers(1, 11))
        rec = U.make_record(7500 + t, n_ites, adepth, {})
        for nr in range(min(n_ites, 1024)):
            U.set_hash(rec, nr, int(rng.integers(0, 1 << 62)))
        for off in range(2048):
            wild = rng.random() < 0.05
            U.set_slot(rec, U.H, off, int(rng.integers(0, 32768 if wild else n_ites)),
                       int(rng.integers(0, 32768 if wild else 2048)), int(rng.integers(0, 4)))
        items = U.hits_for(rec, 0, range(n_ites)) + [q for nr in range(0, n_ites, 3) for q in U.misses_for(rec, 0, nr)]
        for q in items:                                     # send them down random chains
            if rng.random() < 0.5:
                q["hash"] = int(rng.integers(0, 1 << 62))
        req, names = lookup.requests(items)
        if t % 3 == 0:
            cut = int(rng.integers(1, 700))
            rec = bytearray(rec[: len(U.payload_of(rec)) + U.H - cut])
            rec[240:244] = np.uint32(len(rec)).tobytes()
        agree(host_find, [rec], [adepth], req, names, singles=t % 4 == 0)


def test_itb_find_check_passes():
    """The stand-alone checker (itb_find.h against its own naive walk, every
    payload and blob ending where its heap block ends; built with
    AddressSanitizer and UBSan where they link) exits 0."""
    r = subprocess.run([os.path.join(NATIVE, "itb_find_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_find_check: ok" in r.stdout


def test_add_index_builds_what_the_reference_builds():
    """FREE -> UNIQUE; UNIQUE -> CONFLICT with a slot of the overflow half found
    through h.inf; CONFLICT inserts at the head."""
    rec = U.make_record(7600, 4, 2, {})
    U.add_index(rec, 1, 0)
    assert U.get_slot(rec, U.H, 1) == (0, 0, U.IDX_UNIQUE)
    U.add_index(rec, 1, 1)
    assert U.get_slot(rec, U.H, 1) == (0, 4, U.IDX_CONFLICT) and U.get_slot(rec, U.H, 4) == (1, 0, U.IDX_UNIQUE)
    U.add_index(rec, 1, 2)
    assert U.get_slot(rec, U.H, 1) == (2, 5, U.IDX_CONFLICT) and U.get_slot(rec, U.H, 5) == (0, 4, U.IDX_CONFLICT)
    assert tuple(rec[U.ITBH_INF: U.ITBH_INF + 4]) == (2, 0, 2, 0)            # h.inf, h.itu


def test_parse():
    rec = bytes(range(136))
    uuid, mdu, column = lookup.parse(rec)
    assert uuid == int.from_bytes(rec[:8], "little") and mdu == rec[8:112]
    assert column == tuple(int.from_bytes(rec[112 + 8 * i: 120 + 8 * i], "little") for i in range(3))
    with pytest.raises(ValueError):
        lookup.parse(rec[:135])


def test_exports_are_declared():
    assert {"pom_lookup_dev", "pom_lookup_batch"} <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert hasattr(lib, "pom_lookup_dev") and hasattr(lib, "pom_lookup_batch")
    text = open(os.path.join(ROOT, "include", "pom_lookup.h")).read()
    assert re.search(r"\bint pom_lookup_dev\(", text) and re.search(r"\bint pom_lookup_batch\(", text)
    assert '#include "pom_readdir.h"' in text
    # the launcher and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_lookup", "pom_lookup_chunked"} & set(lzo.EXPORTS)


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_lookup_batch_refuses():
    recs, _, items = U.family_handmade()
    req, names = lookup.requests(items)
    res = None
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        res = lookup.lookup_batch(recs, req, names)
    assert res is None
    # and the C call itself, with no request at all
    assert lookup._lib().pom_lookup_batch(None, None, 0, 0, None, 0, None, 0, None, None, None, None) == \
        lzo.LZO_E_ERROR
