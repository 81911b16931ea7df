"""CPU: the ITB split (include/pom_split.h) without a GPU -- the header's layout
macros against the reference's structs, the rules (pomegranate_amd/csrc/
itb_split.h, compiled as plain C++) against the Python restatement of the
reference's loop in itb_split_util.py over random and directed tables, the
invariants the contract relies on, the error rules, the header builder byte
for byte, the stand-alone sanitizer check and the exports."""
from __future__ import annotations

import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import check_util as C
import itb_split_util as S
from conftest import ROOT
from pomegranate_amd import itbsplit, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_split.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_layout_constants_match_reference_structs(tmp_path):
    """offsetof over the reference's own headers (LP64, its build flags) and
    its flag values against the macros of pom_split.h and the oracle's."""
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
    P("POM_ITBH_STATE_OFF", offsetof(struct itbh, state));
    P("POM_ITBH_CONFLICTS_OFF", offsetof(struct itbh, conflicts));
    P("POM_ITBH_TWIN_OFF", offsetof(struct itbh, twin));
    P("POM_ITBH_SPLIT_RLINK_OFF", offsetof(struct itbh, split_rlink));
    P("POM_ITB_STATE_DIRTY", ITB_STATE_DIRTY);
    P("flag_off", offsetof(struct itbh, flag));
    P("just_split", ITB_JUST_SPLIT);
    P("w_flag", W(flag));
    P("w_state", W(state));
    P("w_conflicts", W(conflicts));
    P("w_twin", W(twin));
    P("w_split_rlink", W(split_rlink));
    P("itb_depth", ITB_DEPTH);
    P("lock_region", offsetof(struct itb, bitmap) - sizeof(struct itbh));
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
    for macro in ("POM_ITBH_STATE_OFF", "POM_ITBH_CONFLICTS_OFF", "POM_ITBH_TWIN_OFF", "POM_ITBH_SPLIT_RLINK_OFF",
                  "POM_ITB_STATE_DIRTY"):
        assert want[macro] == got[macro], macro
    assert (got["flag_off"], got["just_split"]) == (S.ITBH_FLAG, S.ITB_JUST_SPLIT) == (0, 2)
    assert (got["w_flag"], got["w_state"], got["w_conflicts"], got["w_twin"], got["w_split_rlink"]) == (1, 1, 4, 8, 8)
    assert (got["itb_depth"], got["lock_region"]) == (10, C.BITMAP_OFF)
    assert (S.ITBH_STATE, S.ITBH_CONFLICTS, S.ITBH_TWIN, S.ITBH_SPLIT_RLINK, S.ITB_STATE_DIRTY) == \
        tuple(got[m] for m in ("POM_ITBH_STATE_OFF", "POM_ITBH_CONFLICTS_OFF", "POM_ITBH_TWIN_OFF",
                               "POM_ITBH_SPLIT_RLINK_OFF", "POM_ITB_STATE_DIRTY"))


def test_itbsplit_py_mirrors_the_header():
    want = header_macros()
    del want["POM_SPLIT_H"]
    for macro, value in want.items():
        assert getattr(itbsplit, macro[4:]) == value, macro
    assert want["POM_SPLIT_E_DAMAGED"] == S.E_DAMAGED and want["POM_SPLIT_DEPTH_MAX"] == S.DEPTH_MAX
    # distinct from every code in use
    codes = set()
    for name in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", name)).read()
        codes |= {(m.group(1), int(m.group(2))) for m in re.finditer(r"#define (\w+_E_\w+) \((-\d+)\)", text)}
    assert [n for n, v in codes if v == S.E_DAMAGED] == ["POM_SPLIT_E_DAMAGED"]
    assert [itbsplit.RESULT_DTYPE.fields[k][1] for k in S.RESULT_FIELDS] == \
        [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 42, 44, 46]
    r = itbsplit.Result.parse(S.RESULT.pack(*range(14)))
    assert tuple(r) == tuple(range(14)) and r._fields == S.RESULT_FIELDS
    with pytest.raises(ValueError):
        itbsplit.Result.parse(bytes(47))


# ---------------------------------------------------------------------------
# libitb_split_host.so (itb_split.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_split():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_split_host.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.itb_split_host.restype = ctypes.c_int
    lib.itb_split_host.argtypes = [vp, u32, u32, vp, u32, u64, u64, vp, u32, vp, vp]
    lib.itb_split_batch_host.restype = None
    lib.itb_split_batch_host.argtypes = [vp] * 7 + [u32] + [vp] * 5

    def run(payloads, adepths, hdrs, sds=None, new_caps=None, status=None, off_residue=None, single=False):
        """-> [(result 48 bytes, payload after, the new payload's room after,
        steps)].  Payload b and its new payload's room lie in two arenas of
        0x5A, 64 guard bytes around each, at multiples of 16 plus
        off_residue[b] (both offsets); the guards must keep their fill."""
        n = len(payloads)
        caps = [len(p) for p in payloads] if new_caps is None else list(new_caps)
        res = [0] * n if off_residue is None else list(off_residue)
        offs, noffs, at, nat = [], [], 64, 64
        for b in range(n):
            offs.append(at + res[b])
            noffs.append(nat + res[b])
            at = (at + res[b] + len(payloads[b]) + 64 + 15) // 16 * 16
            nat = (nat + res[b] + caps[b] + 64 + 15) // 16 * 16
        raw, nraw = np.full(at + 32, 0x5A, np.uint8), np.full(nat + 32, 0x5A, np.uint8)
        skew, nskew = (-raw.ctypes.data) % 16, (-nraw.ctypes.data) % 16
        arena, narena = raw[skew:], nraw[nskew:]
        for b, p in enumerate(payloads):
            arena[offs[b]: offs[b] + len(p)] = np.frombuffer(bytes(p), np.uint8)
        before = arena.copy()
        hd = np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy()
        result = np.full((n + 2, 48), 0x5A, np.uint8)
        steps = np.zeros(n, np.uint32)
        o64 = np.array(offs, np.uint64)
        n64 = np.array(noffs, np.uint64)
        lens = np.array([len(p) for p in payloads], np.uint32)
        cp = np.array(caps, np.uint32)
        ads = np.array(adepths, np.uint8)
        sd8 = None if sds is None else np.array(sds, np.uint8)
        st = None if status is None else np.array(status, np.int32)
        if single:
            assert status is None and sds is not None
            for b in range(n):
                rc = lib.itb_split_host(arena.ctypes.data + offs[b], len(payloads[b]), adepths[b],
                                        hd.ctypes.data + 32 * b, sds[b], offs[b], noffs[b],
                                        narena.ctypes.data + noffs[b], caps[b], result[1 + b:].ctypes.data,
                                        steps[b:].ctypes.data)
                assert rc == struct.unpack_from("<i", result[1 + b].tobytes())[0]
        else:
            lib.itb_split_batch_host(arena.ctypes.data, o64.ctypes.data, lens.ctypes.data,
                                     None if st is None else st.ctypes.data, ads.ctypes.data, hd.ctypes.data,
                                     None if sd8 is None else sd8.ctypes.data, n, narena.ctypes.data, n64.ctypes.data,
                                     cp.ctypes.data, result[1:].ctypes.data, steps.ctypes.data)
        assert (result[0] == 0x5A).all() and (result[-1] == 0x5A).all()
        keep, nkeep = np.ones(len(arena), bool), np.ones(len(narena), bool)
        for b in range(n):
            keep[offs[b]: offs[b] + len(payloads[b])] = False
            nkeep[noffs[b]: noffs[b] + caps[b]] = False
        assert (arena[keep] == before[keep]).all() and (narena[nkeep] == 0x5A).all(), "a guard byte changed"
        return [(result[1 + b].tobytes(), arena[offs[b]: offs[b] + len(payloads[b])].tobytes(),
                 narena[noffs[b]: noffs[b] + caps[b]].tobytes(), int(steps[b])) for b in range(n)]
    return run


same = S.assert_same


def agree(host_split, recs, adepths, sds, names=None, invariants=True):
    """As a batch and one by one; the invariants for every split that produced
    something.  Returns the oracle's answers."""
    payloads = [C.payload_of(r) for r in recs]
    hdrs = [C.hdr_of(r) for r in recs]
    want = S.expect(payloads, adepths, hdrs, sds)
    same(host_split(payloads, adepths, hdrs, sds), want, payloads, names)
    same(host_split(payloads, adepths, hdrs, sds, single=True), want, payloads, names)
    if invariants:
        for b, w in enumerate(want):
            if w.new_payload is not None:
                S.invariants(payloads[b], adepths[b], hdrs[b], sds[b], w)
    return want


@pytest.mark.parametrize("adepth", [1, 2, 3, 5, 8, 10])
def test_random_tables(host_split, adepth):
    """Tables built by random adds and deletes at depths 0 ... 2, split at
    depth + 1: itb_split.h equals the restated loop in every byte, and every
    invariant holds."""
    count = 24 if adepth < 8 else 6
    recs, sds = [], []
    for k in range(count):
        depth = k % 3
        recs.append(S.random_split_table(7000 + 31 * adepth + k, adepth, depth).record())
        sds.append(depth + 1)
    want = agree(host_split, recs, [adepth] * count, sds)
    produced = [w for w in want if w.new_payload is not None]
    # (the inputs' own coverage: an adepth-1 table holds 0 ... 2 ITEs, each moving with probability 1/2)
    assert len(produced) >= count // 3 and all(w.fields["err"] == 0 for w in want)
    if adepth >= 3:
        assert any(w.fields["old_pseudo"] and w.fields["new_pseudo"] for w in produced)
    # split_depth NULL is hdr.depth + 1
    payloads, hdrs = [C.payload_of(r) for r in recs], [C.hdr_of(r) for r in recs]
    same(host_split(payloads, [adepth] * count, hdrs, None), want, payloads)


@pytest.mark.parametrize("adepth", [1, 2, 3, 10])
def test_directed_tables(host_split, adepth):
    """One table per piece of the loop's machinery (itb_split_util.directed),
    with what each must show stated here in closed form."""
    tables = S.directed(adepth)
    d = 1 << adepth
    names = [t[0] for t in tables]
    want = agree(host_split, [t[1] for t in tables], [adepth] * len(tables), [t[2] for t in tables], names,
                 invariants=False)
    for (name, rec, sd), x in zip(tables, want):
        if x.new_payload is not None:
            # (sd50's hashes differ below the split bit on purpose: no itbid fits both kinds)
            S.invariants(C.payload_of(rec), adepth, C.hdr_of(rec), sd, x, itbid=not name.startswith("sd50"))
    w = {name.split("@")[0]: x for name, x in zip(names, want)}
    f = {k: v.fields for k, v in w.items()}
    assert f["none"] == dict.fromkeys(S.RESULT_FIELDS, 0) and w["none"].new_payload is None
    assert (f["all"]["moved"], f["all"]["old_entries"], f["all"]["old_len"], f["all"]["old_max_offset"]) == \
        (d, 0, C.ITB_SIZE, 0)
    assert f["all"]["old_pseudo"] == f["all"]["old_itu"] == 0 and f["all"]["new_len"] == C.ITB_SIZE + 512 * d
    assert f["alternate"]["moved"] == d // 2 and f["alternate"]["new_pseudo"] == d // 2 - 1
    assert f["alternate"]["old_pseudo"] == d // 2 - 1
    assert f["head"]["moved"] == f["tail"]["moved"] == 1 and f["head"]["old_entries"] == d - 1
    assert f["stale"]["moved"] == (2 if d > 2 else 1)
    assert f["one_home"]["moved"] == d // 2 and f["one_home"]["new_itu"] == f["one_home"]["new_inf"] == d // 2 - 1
    assert f["maxoff"]["moved"] == 1
    if d > 2:                       # the highest ITE left, the one below it is dead: max_offset-- stops on it
        assert f["maxoff"]["old_max_offset"] == d - 2 and f["maxoff"]["old_len"] == C.ITB_SIZE + 512 * (d - 1)
    assert f["sd1"]["moved"] == f["sd50"]["moved"] == d // 2
    # a rescan happened where a head moved off a chain that goes on
    assert w["alternate"].steps > d // 2 or d == 2


def test_moved_nothing_then_deeper(host_split):
    """moved == 0 is a result: nothing is produced, and the caller's retry one
    depth deeper finds the ITEs."""
    t = S._built(4, 11, [i % 16 | 1 << 11 | i << 20 for i in range(12)])
    rec = t.record()
    want = agree(host_split, [rec, rec], [4, 4], [1, 2])
    assert want[0].fields == dict.fromkeys(S.RESULT_FIELDS, 0) and want[1].fields["moved"] == 12


def test_error_rules(host_split):
    """Each rule before the next: a decoder's code, adepth 0 and 11, n = 11903,
    a live ITE cut short, sd 0 and 51, offsets at residues 1 and 8, damage,
    new_cap one byte short; a whole table beside them splits as ever."""
    t = S.random_split_table(9, 3, 0)
    rec = t.record()
    payload, hdr = C.payload_of(rec), C.hdr_of(rec)
    moved = sum(S.moves(h, 1) for h in t.hashes.values())
    assert 0 < moved < len(t.hashes)
    top = max(t.hashes)
    cut = payload[: C.ITE_OFF + C.ITE_SIZE * (top + 1) - 1]
    damaged = C.payload_of(C.kind_tables(3)["dup"][0])
    dhdr = C.hdr_of(C.kind_tables(3)["dup"][0])
    need = C.ITE_OFF + 512 * moved
    #        payload, adepth, hdr, sd, status, residue, new_cap
    cases = [(payload, 3, hdr, 1, 0, 0, None, 0),
             (payload, 3, hdr, 1, -6, 0, None, -6),
             (payload, 0, hdr, 0, 0, 1, None, C.EINVAL),
             (payload, 11, hdr, 1, 0, 0, None, C.EINVAL),
             (payload[: C.ITE_OFF - 1], 3, hdr, 51, 0, 8, None, C.E_TRUNCATED),
             (cut, 3, hdr, 1, 0, 0, None, C.E_TRUNCATED),
             (payload, 3, hdr, 0, 0, 0, None, C.EINVAL),
             (payload, 3, hdr, 51, 0, 8, None, C.EINVAL),
             (payload, 3, hdr, 1, 0, 1, None, C.EINVAL),
             (payload, 3, hdr, 50, 0, 8, None, C.EINVAL),
             (damaged, 3, dhdr, 1, 0, 8, None, C.EINVAL),
             (damaged, 3, dhdr, 1, 0, 0, 0, S.E_DAMAGED),
             (payload, 3, dict(hdr, entries=hdr["entries"] + 1), 1, 0, 0, None, S.E_DAMAGED),
             (payload, 3, hdr, 1, 0, 0, need - 1, S.E_OUTPUT_OVERRUN),
             (payload, 3, hdr, 1, 0, 0, need, 0)]
    payloads, adepths, hdrs, sds, status, res, caps, errs = (list(x) for x in zip(*cases))
    caps = [len(p) if c is None else c for p, c in zip(payloads, caps)]
    offs = [16 * 4 + r for r in res]
    want = S.expect(payloads, adepths, hdrs, sds, offs, offs, caps, status)
    assert [w.fields["err"] for w in want] == errs
    assert want[13].fields["moved"] == moved and want[13].new_payload is None
    assert all(w.fields["moved"] == 0 for w in want[1:13])
    got = host_split(payloads, adepths, hdrs, sds, caps, status, res)
    same(got, want, payloads)
    assert got[0][1] != payload and got[-1][0] == got[0][0]


def test_damaged_tables_are_never_walked(host_split):
    """Each table of kind_tables() except `valid`, and the funnel:
    POM_SPLIT_E_DAMAGED, with no byte of the payload changed."""
    tables = S.damaged_tables()
    assert len(tables) == len(C.kind_tables()) - 1 + 1
    recs = [t[1] for t in tables]
    want = agree(host_split, recs, [t[2] for t in tables], [1] * len(tables), [t[0] for t in tables])
    assert [w.fields["err"] for w in want] == [S.E_DAMAGED] * len(tables)


def test_oracle_loop_invariants_over_many_tables():
    """The restated loop alone (no product code): the invariants over more
    tables than the comparison above takes, and two all-collide chains."""
    n = 0
    for adepth in (1, 2, 3, 5):
        for k in range(40):
            depth = k % 3
            rec = S.random_split_table(100 + k, adepth, depth).record()
            payload, hdr = C.payload_of(rec), C.hdr_of(rec)
            w = S.expect_one(payload, adepth, hdr, depth + 1)
            if w.new_payload is not None:
                S.invariants(payload, adepth, hdr, depth + 1, w)
                n += 1
    for adepth in (3, 6):
        d = 1 << adepth
        rec = S._built(adepth, 5, [(d - 1) | int(x) << 10 | i << 20
                                   for i, x in enumerate(np.random.default_rng(adepth).integers(0, 2, d))]).record()
        w = S.expect_one(C.payload_of(rec), adepth, C.hdr_of(rec), 1)
        S.invariants(C.payload_of(rec), adepth, C.hdr_of(rec), 1, w)
        n += 1
    assert n > 100


# ---------------------------------------------------------------------------
# The header builder
# ---------------------------------------------------------------------------
def test_headers_byte_for_byte():
    """pom_itb_split_headers against the oracle's headers(): of the 264 bytes
    only the named fields differ from O's header, in O's copy and in N's."""
    t = S.random_split_table(21, 4, 2)
    rec = bytearray(t.record())
    rec[:C.H] = np.random.default_rng(3).integers(0, 256, C.H, dtype=np.uint8).tobytes()      # pointers, locks, txg
    rec[S.ITBH_ADEPTH], rec[S.ITBH_DEPTH] = 4, 2
    struct.pack_into("<Q", rec, S.ITBH_ITBID, 2)
    struct.pack_into("<H", rec, S.ITBH_ALGO, 1)
    struct.pack_into("<H", rec, C.ITBH_INF, C.hdr_of(t.record())["inf"])    # O's inf is O's own: a split keeps it
    sd = 3
    w = S.expect_one(C.payload_of(t.record()), 4, C.hdr_of(t.record()), sd)
    assert w.fields["moved"] > 0
    o, n, bits = itbsplit.split_headers(rec[:C.H], sd, w.result)
    assert (o, n, bits) == S.headers(rec[:C.H], sd, w.result) and bits == 0
    diff = lambda a, b: {i for i in range(C.H) if a[i] != b[i]}
    span = lambda off, size: set(range(off, off + size))
    o_fields = span(S.ITBH_DEPTH, 1) | span(C.ITBH_ENTRIES, 8) | span(C.ITBH_PSEUDO, 4) | span(C.ITBH_ITU, 2) | \
        span(C.ITBH_LEN, 8) | span(S.ITBH_ALGO, 2)
    n_fields = o_fields | span(0, 2) | span(S.ITBH_ITBID, 8) | span(S.ITBH_CONFLICTS, 4) | span(C.ITBH_INF, 2) | \
        span(S.ITBH_TWIN, 16)
    assert diff(o, rec) <= o_fields and diff(n, rec) <= n_fields
    f = w.fields
    assert C.hdr_of(o) == dict(entries=f["old_entries"], max_offset=f["old_max_offset"],
                               pseudo_conflicts=f["old_pseudo"], ulen=f["old_len"], inf=f["old_inf"],
                               itu=f["old_itu"], depth=sd, itbid=2)
    assert C.hdr_of(n) == dict(entries=f["new_entries"], max_offset=f["new_max_offset"],
                               pseudo_conflicts=f["new_pseudo"], ulen=f["new_len"], inf=f["new_inf"],
                               itu=f["new_itu"], depth=sd, itbid=2 | 1 << (sd - 1))
    assert (n[0], n[1]) == (2, 1) and n[S.ITBH_TWIN: S.ITBH_TWIN + 16] == bytes(16)
    assert n[S.ITBH_CONFLICTS: S.ITBH_CONFLICTS + 4] == bytes(4)
    # sd 50 sets itbid bit 49; what is refused writes nothing
    _, n50, _ = itbsplit.split_headers(rec[:C.H], 50, w.result)
    assert struct.unpack_from("<Q", n50, S.ITBH_ITBID)[0] == 2 | 1 << 49
    for bad_sd, res in ((0, w.result), (51, w.result), (3, S._only(S.E_DAMAGED)), (3, S._only(0))):
        with pytest.raises(ValueError):
            itbsplit.split_headers(rec[:C.H], bad_sd, res)


def test_not_smaller_rule_at_its_tie(oracle):
    """itb_lzo_compress keeps a stream only when it is smaller than the payload.
    record_util's tie sizes and differences applied to each half's payload
    length: a stream one byte longer, as long, one and two bytes shorter; then
    real payloads of the tie sizes whose oracle streams have those lengths."""
    import record_util as R
    t = S.random_split_table(21, 4, 2)
    rec = t.record()
    w = S.expect_one(C.payload_of(rec), 4, C.hdr_of(rec), 3)
    f = w.fields
    for diff in R.TIE_DIFFS:
        zo, zn = f["old_len"] - C.H + diff, f["new_len"] - C.H + diff
        o, n, bits = itbsplit.split_headers(rec[:C.H], 3, w.result, zo, zn)
        assert (o, n, bits) == S.headers(rec[:C.H], 3, w.result, zo, zn), diff
        assert bits == (3 if diff < 0 else 0), diff
        ln, zlen, algo = struct.unpack_from("<IIH", o, C.ITBH_LEN)
        assert (ln, zlen, algo) == ((C.H + zo, f["old_len"], 1) if diff < 0 else (f["old_len"], 0, 0)), diff
        ln, zlen, algo = struct.unpack_from("<IIH", n, C.ITBH_LEN)
        assert (ln, zlen, algo) == ((C.H + zn, f["new_len"], 1) if diff < 0 else (f["new_len"], 0, 0)), diff
        # one half above the tie, the other below
        _, _, mixed = itbsplit.split_headers(rec[:C.H], 3, w.result, f["old_len"] - C.H - 1, f["new_len"] - C.H)
        assert mixed == 1
    for size in R.TIE_SIZES:
        for diff, payload in R.tie_search(oracle, size, R.TIE_DIFFS, 77).items():
            z = len(oracle.compress(payload))
            assert z - len(payload) == diff
            res = S.RESULT.pack(0, 1, C.H + len(payload), C.ITB_SIZE, *([0] * 10))
            o, _, bits = itbsplit.split_headers(rec[:C.H], 3, res, z, itbsplit.SPLIT_NO_STREAM)
            assert bits == (1 if diff < 0 else 0), (size, diff)
            assert o == S.headers(rec[:C.H], 3, res, z, None)[0]


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_split_batch_refuses():
    """LZO_E_ERROR, with every output as the caller left it."""
    rec = S.directed(2)[1][1]
    res = None
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        res = itbsplit.split_batch([rec])
    assert res is None
    n = 1
    buf = np.frombuffer(bytes(rec), dtype=np.uint8)
    ptrs, lens = (ctypes.c_void_p * n)(buf.ctypes.data), (ctypes.c_size_t * n)(buf.size)
    old, new = np.full(len(rec), 7, np.uint8), np.full(len(rec), 7, np.uint8)
    optr, nptr = (ctypes.c_void_p * n)(old.ctypes.data), (ctypes.c_void_p * n)(new.ctypes.data)
    caps = (ctypes.c_size_t * n)(len(rec))
    ol, nl = (ctypes.c_size_t * n)(7), (ctypes.c_size_t * n)(7)
    result = np.full(48, 7, np.uint8)
    err, ok = np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    rc = itbsplit._lib().pom_itb_split_batch(ptrs, lens, n, None, optr, nptr, caps, ol, nl, result.ctypes.data,
                                             err.ctypes.data, ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    assert (old == 7).all() and (new == 7).all() and (result == 7).all() and err[0] == 7 and ok[0] == 7
    assert (ol[0], nl[0]) == (7, 7)
    assert itbsplit._lib().pom_itb_split_batch(None, None, 0, None, None, None, None, None, None, None, None,
                                               None) == lzo.LZO_E_ERROR


# ---------------------------------------------------------------------------
# The stand-alone program, the exports
# ---------------------------------------------------------------------------
def test_standalone_check_passes():
    """itb_split_check: itb_split.h over seeded tables and flipped ones, every
    payload and new payload a heap block of exactly its length, built with
    AddressSanitizer and UBSan where they link."""
    r = subprocess.run([os.path.join(NATIVE, "itb_split_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_split_check: ok" in r.stdout


def test_exports_are_declared():
    names = {"pom_itb_split_dev", "pom_itb_split_scratch", "pom_itb_split_headers", "pom_itb_split_batch"}
    assert names <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert all(hasattr(lib, name) for name in names)
    text = open(os.path.join(ROOT, "include", "pom_split.h")).read()
    assert all(re.search(rf"\b{name}\(", text) for name in names)
    # the launchers and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_itb_split", "lzo_mi355x_launch_itb_split_lens", "pom_itb_split_chunked"} & \
        set(lzo.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", lzo.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines()}
    assert itbsplit.split_scratch_bytes(0) == 0 and itbsplit.split_scratch_bytes(5) >= 5 * 52
    # the device entry refuses a NULL hdr and a misaligned arena before it queues anything
    dev = itbsplit._lib().pom_itb_split_dev
    assert dev(None, None, None, None, None, None, None, 0, None, None, None, None, None, None) == C.EINVAL
    assert dev(8, None, None, None, None, 8, None, 0, None, None, None, None, None, None) == C.EINVAL
