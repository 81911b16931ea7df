"""CPU: the ITB check (include/pom_check.h) without a GPU -- the header's layout
macros against the reference's structs, the rules (pomegranate_amd/csrc/
itb_check.h, compiled as plain C++) against the Python restatement in
check_util.py over tables built the way the MDS builds them, hand-made tables
for every kind, fuzzed tables and the error rules; directed tables with
closed-form answers at the word, half, count and walk edges; the stand-alone
checkers, the exports, and the refusal without a GPU."""
from __future__ import annotations

import ctypes
import hashlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import check_util as C
from conftest import ROOT
from pomegranate_amd import check, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_check.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof / sizeof over the reference's own headers (LP64, its build
    flags) against the layout macros of pom_check.h, and the fields' widths
    against struct pom_check_hdr's."""
    (tmp_path / "attr").mkdir()
    (tmp_path / "attr" / "xattr.h").write_text("/* stub: the probe needs no xattr call */\n")
    probe = tmp_path / "probe.c"
    probe.write_text(r'''
#include "hvfs.h"
#include "xtable.h"
#include "ite.h"
#include <stddef.h>
#include <stdio.h>
#define P(name, v) printf("%s %ld\n", name, (long)(v))
#define W(f) sizeof(((struct itbh *)0)->f)
int main(void)
{
    P("POM_ITBH_MAX_OFFSET_OFF", offsetof(struct itbh, max_offset));
    P("POM_ITBH_PSEUDO_CONFLICTS_OFF", offsetof(struct itbh, pseudo_conflicts));
    P("POM_ITBH_INF_OFF", offsetof(struct itbh, inf));
    P("POM_ITBH_ITU_OFF", offsetof(struct itbh, itu));
    P("POM_ITB_SIZE", sizeof(struct itb));
    P("itbh", sizeof(struct itbh));
    P("ite", sizeof(struct ite));
    P("ite_off", offsetof(struct itb, ite));
    P("entries_off", offsetof(struct itbh, entries));
    P("w_entries", W(entries));
    P("w_max_offset", W(max_offset));
    P("w_pseudo", W(pseudo_conflicts));
    P("w_len", W(len));
    P("w_inf", W(inf));
    P("w_itu", W(itu));
    P("w_depth", W(depth));
    P("w_itbid", W(itbid));
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
    for macro in ("POM_ITBH_MAX_OFFSET_OFF", "POM_ITBH_PSEUDO_CONFLICTS_OFF", "POM_ITBH_INF_OFF", "POM_ITBH_ITU_OFF",
                  "POM_ITB_SIZE"):
        assert want[macro] == got[macro], macro
    assert (want["POM_ITBH_MAX_OFFSET_OFF"], want["POM_ITBH_PSEUDO_CONFLICTS_OFF"], want["POM_ITBH_INF_OFF"],
            want["POM_ITBH_ITU_OFF"]) == (8, 16, 250, 252)
    # sizeof(struct itb) - 264 is POM_ITB_ITE_OFF, where the ITEs start
    assert got["POM_ITB_SIZE"] - got["itbh"] == 11904 and got["ite_off"] == got["POM_ITB_SIZE"] and got["ite"] == 512
    assert (got["w_entries"], got["w_max_offset"], got["w_pseudo"], got["w_len"], got["w_inf"], got["w_itu"],
            got["w_depth"], got["w_itbid"]) == (4, 4, 4, 4, 2, 2, 1, 8)
    # the test builders' own constants are the reference's too
    assert (C.ITBH_ENTRIES, C.ITBH_MAX_OFFSET, C.ITBH_PSEUDO, C.ITBH_INF, C.ITBH_ITU, C.ITB_SIZE) == \
        (got["entries_off"], got["POM_ITBH_MAX_OFFSET_OFF"], got["POM_ITBH_PSEUDO_CONFLICTS_OFF"],
         got["POM_ITBH_INF_OFF"], got["POM_ITBH_ITU_OFF"], got["POM_ITB_SIZE"])


def test_check_py_mirrors_the_header():
    want = header_macros()
    del want["POM_CHECK_H"]
    for macro, value in want.items():
        assert getattr(check, macro[4:]) == value, macro
    assert [want["POM_CK_" + name] for name in check.KINDS] == list(range(22)) and want["POM_CK_KINDS"] == 22
    assert [check.HDR_DTYPE.fields[k][1] for k in ("entries", "max_offset", "pseudo_conflicts", "ulen", "inf", "itu",
                                                   "depth", "itbid")] == [0, 4, 8, 12, 16, 18, 20, 24]
    assert [check.REPORT_DTYPE.fields[k][1] for k in ("findings", "live", "used_home", "used_over", "reached",
                                                      "longest", "count")] == [0, 4, 8, 10, 12, 14, 16]
    assert (check.E_TRUNCATED, check.EINVAL) == (-4097, -22)
    # the oracle's own kind numbers and header packing agree with the binding's
    assert [getattr(C, name) for name in check.KINDS] == list(range(22))
    rec = C.base_table().record()
    assert check.header_facts(rec).tobytes() == C.hdr_bytes(C.hdr_of(rec))
    r = check.Report.parse(C.check(C.payload_of(C.kind_tables()["shared_loop"][0]), 2)[1])
    assert r.kinds == ("S_SHARED", "S_LOOP") and r.count[7] == r.count[10] == 1 and (r.live, r.longest) == (2, 0)
    with pytest.raises(ValueError):
        check.Report.parse(bytes(47))


# ---------------------------------------------------------------------------
# libitb_check_host.so (itb_check.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_check_host.so"))
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.itb_check_host.restype = ctypes.c_int
    lib.itb_check_host.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp]
    lib.itb_check_batch_host.restype = None
    lib.itb_check_batch_host.argtypes = [vp] * 6 + [u32, u32] + [vp] * 4

    def run(payloads, adepths, hdrs=None, flags=0, shift=0, masks=True, status=None, single=False):
        """-> (err, reports [n, 48], slot masks [n, 32], ITE masks [n, 16]);
        the masks are None without `masks`.  Payload b sits at residue (shift +
        b) mod 8 in a buffer of its own that ends where the payload ends."""
        n = len(payloads)
        bufs, ptrs = [], []
        for b, p in enumerate(payloads):
            s = (shift + b) % 8
            buf = np.zeros(len(p) + 16 + s, dtype=np.uint8)
            at = (-buf.ctypes.data) % 8 + s
            buf = buf[: at + len(p)]
            buf[at:] = np.frombuffer(bytes(p), dtype=np.uint8)
            bufs.append(buf)
            ptrs.append(buf.ctypes.data + at)
        rep = np.full((n + 2, 48), 0x5A, dtype=np.uint8)
        sm = np.full((n + 2, 32), 0x5A5A, dtype=np.uint64)
        im = np.full((n + 2, 16), 0x5A5A, dtype=np.uint64)
        err = np.full(n + 2, 0x5A5A, dtype=np.int32)
        hd = None if hdrs is None else np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy()
        if single:
            assert status is None
            for b in range(n):
                err[1 + b] = lib.itb_check_host(ptrs[b], len(payloads[b]), adepths[b],
                                                None if hd is None else hd.ctypes.data + 32 * b, flags,
                                                rep[1 + b:].ctypes.data, sm[1 + b:].ctypes.data if masks else None,
                                                im[1 + b:].ctypes.data if masks else None)
        else:
            base = min(ptrs)
            offs = np.array([p - base for p in ptrs], dtype=np.uint64)
            lens = np.array([len(p) for p in payloads], dtype=np.uint32)
            ads = np.array(adepths, dtype=np.uint8)
            st = None if status is None else np.array(status, dtype=np.int32)
            lib.itb_check_batch_host(base, offs.ctypes.data, lens.ctypes.data, None if st is None else st.ctypes.data,
                                     ads.ctypes.data, None if hd is None else hd.ctypes.data, n, flags,
                                     rep[1:].ctypes.data, sm[1:].ctypes.data if masks else None,
                                     im[1:].ctypes.data if masks else None, err[1:].ctypes.data)
        for a in (rep, sm, im, err):
            assert (a[0] == a.dtype.type(0x5A5A if a.dtype != np.uint8 else 0x5A)).all() and (a[-1] == a[0]).all()
        if not masks:
            assert (sm == 0x5A5A).all() and (im == 0x5A5A).all()
        return err[1:-1], rep[1:-1], sm[1:-1] if masks else None, im[1:-1] if masks else None
    return run


def same(got, want, what=""):
    """err, all 48 report bytes and both masks, ITB by ITB."""
    names = ("err", "report", "slot_mask", "ite_mask")
    for g, w, name in zip(got, want, names):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        if len(bad):
            b = int(bad[0])
            detail = f"{C.report_fields(g[b])} != {C.report_fields(w[b])}" if name == "report" else f"{g[b]} != {w[b]}"
            raise AssertionError(f"{what}{name}: ITB {b}: {detail}")


def agree(host_check, recs, adepths, flags=C.CK_ITBID, status=None):
    """With the header facts and without, with masks and without, at payload
    residues 0 and 5, as a batch and one by one.  Returns the oracle's answer
    with the header facts."""
    payloads = [C.payload_of(r) for r in recs]
    hdrs = [C.hdr_of(r) for r in recs]
    want = C.expect(payloads, adepths, hdrs, flags, status)
    same(host_check(payloads, adepths, hdrs, flags, 0, status=status), want)
    same(host_check(payloads, adepths, hdrs, flags, 5, masks=False, status=status), want)
    same(host_check(payloads, adepths, None, flags, 3, status=status), C.expect(payloads, adepths, None, flags, status),
         "hdr NULL: ")
    if status is None:
        same(host_check(payloads, adepths, hdrs, flags, 1, single=True), want)
    return want


@pytest.mark.parametrize("adepth", [1, 2, 3, 6, 10])
def test_no_false_alarm(host_check, adepth):
    """A condition, not a measurement: after every tenth of 2,000 random adds
    and deletes -- hashes collide on purpose, tables run full -- a table the
    reference's functions built reports nothing, and live, used_home,
    used_over and reached are the builder's own bookkeeping."""
    rng = np.random.default_rng(100 + adepth)
    depth, itbid = 3, 5
    t = C.Table(adepth, adepth, depth, itbid)
    d = t.d
    full = 0
    recs = []
    for step in range(2000):
        # fill towards full for a while, then drain, so both ends are met
        p_del = 0.25 if (step // 250) % 2 == 0 else 0.65
        if t.hashes and rng.random() < p_del:
            t.delete(int(rng.choice(sorted(t.hashes))))
        else:
            low = int(rng.integers(0, max(1, d // 4) if rng.random() < 0.6 else d))
            full += t.add(low | itbid << 10 | int(rng.integers(0, 1 << 30)) << 13) is None
        if step % 10 == 9:
            rec = t.record()
            e, rep, sm, im = C.check(C.payload_of(rec), adepth, C.hdr_of(rec), C.CK_ITBID)
            f = C.report_fields(rep)
            assert e == 0 and f["findings"] == 0 and not any(f["count"]) and not any(sm) and not any(im), (step, f)
            assert {k: f[k] for k in ("live", "used_home", "used_over", "reached")} == t.bookkeeping(), step
            recs.append(rec)
    assert full > 0 or adepth == 10                      # the small tables ran full
    assert max(len(r) for r in recs) > C.ITB_SIZE + 512
    # itb_check.h agrees with the oracle field for field (every fourth snapshot: 50 tables)
    want = agree(host_check, recs[::4], [adepth] * len(recs[::4]))
    assert not want[1][:, :4].any() and (want[0] == 0).all()


def test_one_table_per_kind(host_check):
    """Exactly the kinds check_util.kind_tables names, with their exact counts
    and mask bits (hdr NULL: a hand-made table's header counters are the valid
    base table's); which kinds cannot stand alone, and why, is said there."""
    tables = C.kind_tables()
    covered = set()
    for name, (rec, kinds, slots, ites) in tables.items():
        got = host_check([C.payload_of(rec)], [2], None, 0, shift=3)
        f = C.report_fields(got[1][0])
        assert got[0][0] == 0, name
        assert f["findings"] == sum(1 << k for k in kinds), (name, f)
        assert f["count"] == [kinds.get(k, 0) for k in range(16)], (name, f)
        assert got[2][0].tolist() == C.masks_of(slots, 32) and got[3][0].tolist() == C.masks_of(ites, 16), name
        covered |= set(kinds)
    assert covered == set(range(15))
    recs = [rec for rec, _, _, _ in tables.values()]
    agree(host_check, recs, [2] * len(recs))
    # E_MISPLACED and the header's kinds, each alone, on the valid table
    base = tables["valid"][0]
    payload, hdr = C.payload_of(base), C.hdr_of(base)
    wrong = bytearray(base)
    C.set_hash(wrong, 1, 5 | 2 << 10)                    # itbid 2 at depth 2, still home slot 1
    high = bytearray(base)
    C.set_hash(high, 1, 5 | 1 << 10 | 1 << 63)           # bit 53 of hash >> 10: kept from depth 54 on
    cases = [(bytes(wrong[C.H:]), hdr, C.CK_ITBID, 1 << C.E_MISPLACED),
             (bytes(wrong[C.H:]), hdr, 0, 0),
             (bytes(high[C.H:]), dict(hdr, depth=53), C.CK_ITBID, 0),
             (bytes(high[C.H:]), dict(hdr, depth=54), C.CK_ITBID, 1 << C.E_MISPLACED),
             (bytes(high[C.H:]), dict(hdr, depth=63), C.CK_ITBID, 1 << C.E_MISPLACED),
             (bytes(high[C.H:]), dict(hdr, depth=64), C.CK_ITBID, 1 << C.E_MISPLACED),
             (bytes(high[C.H:]), dict(hdr, depth=255), C.CK_ITBID, 1 << C.E_MISPLACED),
             (payload, dict(hdr, depth=0, itbid=0), C.CK_ITBID, 0),
             (payload, dict(hdr, entries=3), 0, 1 << C.H_ENTRIES),
             (payload, dict(hdr, entries=-2), 0, 1 << C.H_ENTRIES),
             (payload, dict(hdr, itu=2), 0, 1 << C.H_ITU),
             (payload, dict(hdr, pseudo_conflicts=0), 0, 1 << C.H_PSEUDO),
             (payload, dict(hdr, max_offset=0, ulen=C.ITB_SIZE + 512), 0, 1 << C.H_MAXOFF),
             (payload, dict(hdr, max_offset=-1, ulen=C.ITB_SIZE), 0, 1 << C.H_MAXOFF),
             (payload, dict(hdr, ulen=hdr["ulen"] + 1), 0, 1 << C.H_LEN),
             (payload, dict(hdr, max_offset=2), 0, 1 << C.H_LEN),
             (payload, dict(hdr, inf=5), 0, 1 << C.H_INF),
             (payload, dict(hdr, inf=4), 0, 0)]
    for p, h, flags, findings in cases:
        got = host_check([p], [2], [h], flags)
        same(got, C.expect([p], [2], [h], flags))
        f = C.report_fields(got[1][0])
        assert f["findings"] == findings, (h, flags, f)
    got = host_check([bytes(wrong[C.H:])], [2], [hdr], C.CK_ITBID)
    assert C.report_fields(got[1][0])["count"][15] == 1 and got[3][0].tolist() == C.masks_of([1], 16)
    # without hdr the flag alone turns nothing on
    assert not host_check([bytes(wrong[C.H:])], [2], None, C.CK_ITBID)[1][0][:4].any()


# ---------------------------------------------------------------------------
# Directed tables (check_util.directed): the closed-form answers judge the
# oracle and itb_check.h alike
# ---------------------------------------------------------------------------
def directed_agree(host_check, tables):
    """agree() over the tables, then their closed-form values against the
    oracle's answer and against itb_check.h's with hdr NULL."""
    recs, adepths = [t.rec for t in tables], [t.adepth for t in tables]
    want = agree(host_check, recs, adepths)
    bare = host_check([C.payload_of(r) for r in recs], adepths, None, 0, shift=3)
    for b, t in enumerate(tables):
        C.assert_directed(t, want[0][b], want[1][b], want[2][b], want[3][b])
        C.assert_directed(t, bare[0][b], bare[1][b], bare[2][b], bare[3][b])
        assert not bare[1][b][:4].view("<u4")[0] >> 15, t.name
    return want


# kind_tables(adepth, where) leaves these out: they need a third ITE or a third overflow slot
KIND_CASES_LEFT_OUT = [
    (1, "low", "entry_dead_orphan"), (1, "low", "shared_misfiled"), (1, "low", "leaked"), (1, "low", "island"),
    (1, "low", "leaked_island"), (1, "low", "orphan"),
    (1, "high", "entry_dead_orphan"), (1, "high", "shared_misfiled"), (1, "high", "leaked"), (1, "high", "island"),
    (1, "high", "leaked_island"), (1, "high", "orphan")]


def test_kind_tables_are_the_first_ones():
    """kind_tables() and base_table() called as before return the bytes they
    returned before they took an adepth and a position."""
    h = hashlib.sha256()
    for name, (rec, kinds, slots, ites) in C.kind_tables().items():
        h.update(name.encode())
        h.update(bytes(rec))
        h.update(repr((kinds, slots, ites)).encode())
    assert h.hexdigest() == "587b74f91d6c045f7cf2a7682d11804a635351aa790487d0f7f13412ec45d2d1"
    assert {k: bytes(v[0]) for k, v in C.kind_tables(2, "low").items()} == \
        {k: bytes(v[0]) for k, v in C.kind_tables().items()}
    assert bytes(C.base_table().record()) == bytes(C.kind_tables()["valid"][0])


@pytest.mark.parametrize("adepth", range(1, 11))
def test_directed_kind_tables(host_check, adepth):
    """A condition, not a measurement: one table per kind with its ITEs, slots
    and the defect's value at the low and at the high end of their ranges.
    Every kind 0 ... 14 appears at both positions of every adepth from 2 up;
    at adepth 10 no slot lies outside and no bit is stray, and the two tables
    that would show them report nothing.  What adepth 1 cannot hold is named in
    KIND_CASES_LEFT_OUT."""
    assert all(ad == 1 for ad, _, _ in KIND_CASES_LEFT_OUT)
    names = list(C.kind_tables())
    for where in C.WHERES:
        tables = C.kind_tables(adepth, where)
        left_out = {name for ad, wh, name in KIND_CASES_LEFT_OUT if (ad, wh) == (adepth, where)}
        assert list(tables) == [name for name in names if name not in left_out]
        covered = set()
        for _, kinds, _, _ in tables.values():
            covered |= set(kinds)
        if adepth == 10:
            assert tables["outside"][1] == tables["stray"][1] == {}
            assert tables["outside"][0] == tables["stray"][0] == tables["valid"][0]
            assert covered == set(range(15)) - {C.S_OUTSIDE, C.E_STRAY}
        elif adepth >= 2:
            assert covered == set(range(15))
        if where == "high":
            assert all(len(rec) == C.ITB_SIZE + 512 * (1 << adepth) for rec, _, _, _ in tables.values())
    tables = C.directed("kinds", [adepth])
    want = directed_agree(host_check, tables)
    valid = [b for b, t in enumerate(tables) if not t.kinds]
    assert len(valid) == (6 if adepth == 10 else 2) and not want[1][valid, :4].any()   # with the header, too


def test_directed_combs(host_check):
    """Findings at bit 0 and bit 63 of every word of both halves and of the ITE
    bitmap (adepth 6 ... 10): each ballot word, and each span mask of one,
    keeps its first and last bit and no other."""
    tables = C.directed("combs")
    assert [t.adepth for t in tables] == [6, 6, 7, 7, 8, 8, 9, 9, 10, 10]
    directed_agree(host_check, tables)
    slot, ite = tables[-2], tables[-1]
    assert slot.kinds == {C.S_LINK_FREE: 32, C.S_ENTRY_RANGE: 32, C.S_LEAKED: 32} and len(slot.slots) == 64
    assert ite.kinds == {C.E_ORPHAN: 32, C.E_STRAY: 0} and tables[1].kinds == {C.E_ORPHAN: 2, C.E_STRAY: 30}


def test_directed_counts(host_check):
    """indeg 1 beside indeg 2 along the whole overflow half, indeg d on one
    slot, refs 2d on one ITE."""
    tables = C.directed("counts")
    directed_agree(host_check, tables)
    shared = [t.kinds[C.S_SHARED] for t in tables if t.name.startswith("alternating")]
    assert shared == [1, 2, 5, 10, 21, 42, 85, 170, 341]             # adepth 2 ... 10: one per j with 3j + 2 < d
    assert len(tables) == 29


def test_directed_walk(host_check):
    """The walk's bound: a path of d + 1 slots is the longest a table has and
    is no loop; one more good link is.  Every adepth, ascending and permuted
    chains (1,024 walks of 1,025 slots in the adepth-10 fan)."""
    tables = C.directed("walk")
    assert len(tables) == 100
    want = directed_agree(host_check, tables)
    for b, t in enumerate(tables):
        d, f = 1 << t.adepth, C.report_fields(want[1][b])
        variant = t.name.split("@")[0]
        assert (f["longest"], f["count"][C.S_LOOP]) == {"line": (d + 1, 0), "short": (d, 0), "cycle": (0, 1),
                                                        "self": (0, 1), "fan": (d + 1, 0)}[variant], t.name


def test_funnel(host_check):
    """All 1,024 home slots of an adepth-10 table link into one cycle of the
    whole overflow half: every one of them is S_LOOP, no path is left to be
    the longest, and the walks' bound (d + 1 slots) ends each of them."""
    rec = C.funnel()
    want = agree(host_check, [rec], [10])
    f = C.report_fields(want[1][0])
    assert f["count"][C.S_LOOP] == 1024 and f["longest"] == 0 and f["reached"] == 2048
    assert f["count"][C.S_SHARED] == 1024 and f["count"][C.E_DUP] == 1024


def test_fuzzed_tables(host_check):
    """300 valid tables, each with 1 ... 8 flips of index words, bitmap bits,
    ITE hashes and header fields."""
    recs, adepths = zip(*(C.fuzzed(s) for s in range(300)))
    want = agree(host_check, list(recs), list(adepths))
    findings = want[1][:, :4].copy().view("<u4").ravel()
    assert (want[0] == 0).sum() > 250 and (findings != 0).sum() > 200
    seen = 0
    for f in findings:
        seen |= int(f)
    assert bin(seen).count("1") >= 18, bin(seen)


@pytest.mark.parametrize("shift", range(8))
def test_error_rules(host_check, shift):
    """A status code, adepth 0 and 11, n = 11903, and a live ITE cut one byte
    short (live is kept), each before the next; a whole table beside them."""
    t = C.random_table(9, 3, 40)
    rec = t.record()
    payload = C.payload_of(rec)
    hdr = C.hdr_of(rec)
    top = max(t.hashes)
    cut = payload[: C.ITE_OFF + C.ITE_SIZE * (top + 1) - 1]
    payloads = [payload, payload, payload, payload, payload[: C.ITE_OFF - 1], cut, cut, payload[: C.ITE_OFF - 1],
                payload[: C.ITE_OFF + C.ITE_SIZE * (top + 1)]]
    adepths = [3, 3, 0, 11, 3, 3, 0, 11, 3]
    status = [0, -6, 0, 0, 0, 0, -4, 0, 0]
    want = C.expect(payloads, adepths, [hdr] * 9, 0, status)
    assert want[0].tolist() == [0, -6, C.EINVAL, C.EINVAL, C.E_TRUNCATED, C.E_TRUNCATED, -4, C.EINVAL, 0]
    lives = [C.report_fields(r)["live"] for r in want[1]]
    assert lives == [len(t.hashes), 0, 0, 0, 0, len(t.hashes), 0, 0, len(t.hashes)]
    assert not want[1][1:8, :4].any() and not want[1][1:8, 8:].any() and not want[2][1:8].any()
    same(host_check(payloads, adepths, [hdr] * 9, 0, shift, status=status), want)
    one = [i for i in range(9) if status[i] == 0]
    same(host_check([payloads[i] for i in one], [adepths[i] for i in one], [hdr] * len(one), 0, shift, single=True),
         tuple(w[one] for w in want))


def test_standalone_checkers_pass():
    """itb_check_check (itb_check.h over random tables, every payload ending
    where its heap block ends) and check_layout_check (the check's staging
    layout), both built with AddressSanitizer and UBSan where they link."""
    for exe in ("itb_check_check", "check_layout_check"):
        r = subprocess.run([os.path.join(NATIVE, exe)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{exe}: ok" in r.stdout


def test_table_builder_restates_the_reference():
    """add: FREE -> UNIQUE, UNIQUE -> CONFLICT, CONFLICT inserts at the head,
    with pseudo_conflicts, itu, max_offset and len; delete: the head of a chain
    swaps entries with the second slot and frees that one, a tail makes its
    predecessor UNIQUE, the last entry resets max_offset and len."""
    t = C.Table(2)
    i32 = lambda off: struct.unpack_from("<i", t.rec, off)[0]
    assert [t.add(h) for h in (1, 5, 9)] == [0, 1, 2]
    g = lambda o: C.get_slot(t.rec, C.H, o)
    assert g(1) == (2, 5, C.IDX_CONFLICT) and g(5) == (0, 4, C.IDX_CONFLICT) and g(4)[::2] == (1, C.IDX_UNIQUE)
    assert (i32(C.ITBH_ENTRIES), i32(C.ITBH_MAX_OFFSET), i32(C.ITBH_PSEUDO), i32(C.ITBH_LEN)) == \
        (3, 2, 2, C.ITB_SIZE + 3 * 512)
    t.delete(2)                                         # the head: entry 0 moves up, slot 5 goes
    assert g(1) == (0, 4, C.IDX_CONFLICT) and g(5)[2] == C.IDX_FREE and g(4)[::2] == (1, C.IDX_UNIQUE)
    assert (i32(C.ITBH_ENTRIES), i32(C.ITBH_MAX_OFFSET), i32(C.ITBH_PSEUDO), i32(C.ITBH_LEN)) == \
        (2, 1, 1, C.ITB_SIZE + 2 * 512)
    t.delete(1)                                         # the tail
    assert g(1)[::2] == (0, C.IDX_UNIQUE) and g(4)[2] == C.IDX_FREE
    t.delete(0)
    assert g(1)[2] == C.IDX_FREE and not t.hashes
    assert (i32(C.ITBH_ENTRIES), i32(C.ITBH_MAX_OFFSET), i32(C.ITBH_PSEUDO), i32(C.ITBH_LEN)) == (0, 0, 0, C.ITB_SIZE)
    assert struct.unpack_from("<HH", t.rec, C.ITBH_INF) == (2, 0)
    for h in range(4):
        assert t.add(h) == h
    assert t.add(7) is None and i32(C.ITBH_ENTRIES) == 4        # full: the MDS would split


def test_exports_are_declared():
    assert {"pom_itb_check_dev", "pom_itb_check_batch"} <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert hasattr(lib, "pom_itb_check_dev") and hasattr(lib, "pom_itb_check_batch")
    text = open(os.path.join(ROOT, "include", "pom_check.h")).read()
    assert re.search(r"\bint pom_itb_check_dev\(", text) and re.search(r"\bint pom_itb_check_batch\(", text)
    # the launcher and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_itb_check", "pom_itb_check_chunked"} & set(lzo.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", lzo.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines()}
    assert {"pom_itb_check_dev", "pom_itb_check_batch"} <= defined


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_check_batch_refuses():
    recs = [C.base_table().record()]
    res = None
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        res = check.check_batch(recs, masks=True)
    assert res is None
    # and the C call itself, with no record at all and with a bad flag
    assert check._lib().pom_itb_check_batch(None, None, 0, 0, None, None, None, None, None) == lzo.LZO_E_ERROR
    assert check._lib().pom_itb_check_batch(None, None, 0, 2, None, None, None, None, None) == lzo.LZO_E_ERROR
