"""CPU: the ITB sweep (include/pom_sweep.h) without a GPU -- the rules
(pomegranate_amd/csrc/itb_sweep.h, compiled as plain C++: the serial loop and
the chain / count / fold pieces the kernel uses) against the Python restatement
of the reference's loop in itb_sweep_util.py over directed, random and damaged
tables, the invariants the contract relies on, the error rules, the header
builder byte for byte, the stand-alone sanitizer check and the exports."""
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
import itb_sweep_util as W
from conftest import ROOT
from pomegranate_amd import itbsweep, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
REFERENCE = "/root/reference"


def header_macros():
    text = open(os.path.join(ROOT, "include", "pom_sweep.h")).read()
    return {m.group(1): int(m.group(2), 0) for m in
            re.finditer(r"^#define (POM_\w+) \(?(-?(?:0x[0-9A-Fa-f]+|\d+))u?\)?", text, re.M)}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference sources are not on this machine")
def test_flag_constants_match_reference_structs(tmp_path):
    """offsetof(struct ite, flag) and the state values over the reference's
    own headers against the macros the sweep uses and the oracle's."""
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
int main(void)
{
    P("flag_off", offsetof(struct ite, flag));
    P("w_flag", sizeof(((struct ite *)0)->flag));
    P("mask", ITE_STATE_MASK);
    P("unlinked", ITE_UNLINKED);
    P("shadow", ITE_SHADOW);
    P("active", ITE_ACTIVE);
    P("state_off", offsetof(struct itbh, state));
    return 0;
}
''')
    exe = tmp_path / "probe"
    inc = [f"-I{os.path.join(REFERENCE, d)}" for d in ("include", "lib", "mds", "xnet", "mdsl", "r2")]
    subprocess.run(["gcc", "-w", "-D__CORES__=8", "-DDISABLE_PYTHON=1", f"-I{tmp_path}", *inc,
                    str(probe), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}
    assert (got["flag_off"], got["w_flag"], got["mask"], got["unlinked"], got["shadow"], got["active"]) == \
        (W.ITE_FLAG_OFF, 4, W.STATE_MASK, W.UNLINKED, W.SHADOW, 0)
    assert (itbsweep.ITE_STATE_MASK, itbsweep.ITE_UNLINKED) == (got["mask"], got["unlinked"])
    assert got["state_off"] == S.ITBH_STATE
    macros = {}
    for name in ("pom_readdir.h", "pom_lookup.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        macros.update({m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define (POM_ITE_\w+) (0x[0-9A-Fa-f]+|\d+)u", text)})
    assert (macros["POM_ITE_FLAG_OFF"], macros["POM_ITE_STATE_MASK"], macros["POM_ITE_UNLINKED"]) == \
        (got["flag_off"], got["mask"], got["unlinked"])


def test_itbsweep_py_mirrors_the_header():
    want = header_macros()
    del want["POM_SWEEP_H"]
    assert want == {"POM_SWEEP_NO_BUDGET": 0xFFFFFFFF}
    assert itbsweep.SWEEP_NO_BUDGET == W.NO_BUDGET == want["POM_SWEEP_NO_BUDGET"]
    assert itbsweep.SPLIT_E_DAMAGED == W.E_DAMAGED
    assert [itbsweep.RESULT_DTYPE.fields[k][1] for k in W.RESULT_FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28, 30]
    r = itbsweep.Result.parse(W.RESULT.pack(*range(9)))
    assert tuple(r) == tuple(range(9)) and r._fields == W.RESULT_FIELDS
    with pytest.raises(ValueError):
        itbsweep.Result.parse(bytes(31))


# ---------------------------------------------------------------------------
# libitb_sweep_host.so (itb_sweep.h as plain C++) against the Python oracle
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_sweep():
    lib = ctypes.CDLL(os.path.join(NATIVE, "libitb_sweep_host.so"))
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.itb_sweep_host.restype = ctypes.c_int
    lib.itb_sweep_host.argtypes = [vp, u32, u32, vp, u32, u64, ctypes.c_int, vp, vp]
    lib.itb_sweep_batch_host.restype = None
    lib.itb_sweep_batch_host.argtypes = [vp] * 7 + [u32, ctypes.c_int] + [vp] * 2

    def run(payloads, adepths, hdrs, budgets=None, status=None, off_residue=None, parts=False, single=False):
        """-> [(result 32 bytes, payload after, steps or None)].  Payload b lies
        in an arena of 0x5A, 64 guard bytes around it, at a multiple of 16 plus
        off_residue[b]; the guards must keep their fill.  parts: the kernel's
        pieces instead of the serial loop (no step count then)."""
        n = len(payloads)
        res = [0] * n if off_residue is None else list(off_residue)
        offs, at = [], 64
        for b in range(n):
            offs.append(at + res[b])
            at = (at + res[b] + len(payloads[b]) + 64 + 15) // 16 * 16
        raw = np.full(at + 32, 0x5A, np.uint8)
        arena = raw[(-raw.ctypes.data) % 16:]
        for b, p in enumerate(payloads):
            arena[offs[b]: offs[b] + len(p)] = np.frombuffer(bytes(p), np.uint8)
        before = arena.copy()
        hd = np.frombuffer(b"".join(C.hdr_bytes(h) for h in hdrs), dtype=np.uint8).copy()
        result = np.full((n + 2, 32), 0x5A, np.uint8)
        steps = np.zeros(n, np.uint32)
        o64 = np.array(offs, np.uint64)
        lens = np.array([len(p) for p in payloads], np.uint32)
        ads = np.array(adepths, np.uint8)
        bud = None if budgets is None else np.array([W.NO_BUDGET if x is None else x for x in budgets], np.uint32)
        st = None if status is None else np.array(status, np.int32)
        if single:
            assert status is None
            for b in range(n):
                rc = lib.itb_sweep_host(arena.ctypes.data + offs[b], len(payloads[b]), adepths[b],
                                        hd.ctypes.data + 32 * b, W.NO_BUDGET if bud is None else int(bud[b]), offs[b],
                                        int(parts), result[1 + b:].ctypes.data, steps[b:].ctypes.data)
                assert rc == struct.unpack_from("<i", result[1 + b].tobytes())[0]
        else:
            lib.itb_sweep_batch_host(arena.ctypes.data, o64.ctypes.data, lens.ctypes.data,
                                     None if st is None else st.ctypes.data, ads.ctypes.data, hd.ctypes.data,
                                     None if bud is None else bud.ctypes.data, n, int(parts), result[1:].ctypes.data,
                                     steps.ctypes.data)
        assert (result[0] == 0x5A).all() and (result[-1] == 0x5A).all()
        keep = np.ones(len(arena), bool)
        for b in range(n):
            keep[offs[b]: offs[b] + len(payloads[b])] = False
        assert (arena[keep] == before[keep]).all(), "a guard byte changed"
        return [(result[1 + b].tobytes(), arena[offs[b]: offs[b] + len(payloads[b])].tobytes(),
                 None if parts else int(steps[b])) for b in range(n)]
    return run


same = W.assert_same


def agree(host_sweep, recs, adepths, budgets=None, names=None, invariants=True):
    """The serial loop and the pieces, as a batch and one by one, against the
    oracle; the invariants for every sweep that removed something.  Returns the
    oracle's answers."""
    payloads = [C.payload_of(r) for r in recs]
    hdrs = [C.hdr_of(r) for r in recs]
    want = W.expect(payloads, adepths, hdrs, budgets)
    for parts in (False, True):
        same(host_sweep(payloads, adepths, hdrs, budgets, parts=parts), want, payloads, names)
        same(host_sweep(payloads, adepths, hdrs, budgets, parts=parts, single=True), want, payloads, names)
    if invariants:
        for b, w in enumerate(want):
            if w.produced:
                W.invariants(payloads[b], adepths[b], hdrs[b], w)
    return want


@pytest.fixture(scope="module")
def chains():
    return W.directed_chains()


def test_directed_chains(host_sweep, chains):
    """U / L chains at adepth 1, 2 and 10, low and high, and every chain of all
    four ITEs at adepth 2, with what each must show in closed form: removed is
    the number of U, dc one more when the head is U and an L follows, a swept
    chain keeps its L members in order."""
    names = [c[0] for c in chains]
    want = agree(host_sweep, [c[1] for c in chains], [c[2] for c in chains], None, names)
    assert {n.split("@")[0] for n in names} >= set(W.PATTERNS) and len(names) >= 13 * 4 + 6 + 16
    for (name, rec, adepth), w in zip(chains, want):
        pattern, f = name.split("@")[0], w.fields
        u = pattern.count("U")
        swap = int(pattern[0] == "U" and "L" in pattern)
        assert (f["removed"], f["dc"]) == ((u, u + swap) if u else (0, 0)), name
        if u:
            assert w.facts["swaps"] == swap and f["visited"] == 1 << adepth, name
            assert f["entries"] == C.hdr_of(rec)["entries"] - u, name
            home = 0 if name.endswith(("low", "all")) else (1 << adepth) - 1
            t = W.table_of(w.payload, adepth, W.swept_hdr(C.hdr_of(rec), f))
            before = S._chain(W.table_of(C.payload_of(rec), adepth, C.hdr_of(rec)), home)
            lives = [nr for nr, c in zip(before, pattern) if c == "L"]
            if lives:
                assert S._chain(t, home) == lives, name
            else:
                assert C.get_slot(t.rec, C.H, home)[2] == C.IDX_FREE, name
    by = dict(zip(names, want))
    # swap then tail, swap then middle, head freed last
    assert by["UL@2low"].facts["deleted"] and by["ULL@2low"].fields["dc"] == 2 and by["UUU@10high"].fields["dc"] == 3
    assert by["UUUU@2all"].fields["len"] == C.ITB_SIZE and by["UUUU@2all"].fields["max_offset"] == 0


@pytest.mark.parametrize("state", [0, 1, 2, 3, 5, 7])
def test_states(host_sweep, state):
    """Only state 1 sweeps, with any high bits; 0, 2, 3 (SHADOW), 5 and 7
    never do."""
    recs = []
    for high in (0, 0xFFFFFFF8, 0x01000000, 0xA5A5A5A0):
        t = S._built(3, 80, [i % 4 | i << 20 for i in range(8)])
        for nr in t.hashes:
            struct.pack_into("<I", t.rec, C.H + C.ITE_OFF + C.ITE_SIZE * nr + W.ITE_FLAG_OFF, high | state)
        recs.append(t.record())
    want = agree(host_sweep, recs, [3] * len(recs))
    assert [w.fields["removed"] for w in want] == [8 if state == 1 else 0] * len(recs)


def test_max_offset(host_sweep):
    """The highest ITE deleted first, last (stale), not at all, a descending
    run, a chain whose order disagrees with the ITEs', and a table swept
    empty."""
    tables = W.max_offset_tables()
    want = agree(host_sweep, [t[1] for t in tables], [t[2] for t in tables], None, [t[0] for t in tables])
    for (name, rec, adepth, (mo, ln)), w in zip(tables, want):
        assert (w.fields["max_offset"], w.fields["len"]) == (mo, ln), name
    assert want[-1].fields["entries"] == 0 and want[-1].fields["len"] == 12168


def test_budget(host_sweep):
    """budget_table at 0, 1, 2, one less than the total dc, the total, more and
    NULL: the stop right after the swap chain, where dc passes the budget one
    delete early; FREE home slots before and after the stop; visited."""
    rec = W.budget_table().record()
    budgets = [0, 1, 2, 3, 4, 5, 6, None]
    want = agree(host_sweep, [rec] * len(budgets), [4] * len(budgets), budgets, [f"budget {x}" for x in budgets])
    got = [(w.fields["removed"], w.fields["dc"], w.fields["visited"]) for w in want]
    #                 0: the first used slot is still swept; 2: the swap chain's dc alone reaches it
    assert got == [(1, 2, 2), (1, 2, 2), (1, 2, 2), (2, 3, 4), (3, 4, 6), (4, 5, 10), (4, 5, 16), (4, 5, 16)]
    # a budget the first used chain does not use up: nothing removed there is still a result
    live_first = W.with_states(S._built(4, 81, [2, 7, 9]), {1: W.UNLINKED})
    want = agree(host_sweep, [live_first.record()] * 3, [4] * 3, [0, 1, None])
    assert [w.fields for w in want[:1]] == [dict.fromkeys(W.RESULT_FIELDS, 0)]
    assert [(w.fields["removed"], w.fields["visited"]) for w in want[1:]] == [(1, 8), (1, 16)]


@pytest.mark.parametrize("adepth", range(1, 11))
def test_random_tables(host_sweep, adepth):
    """Tables built by random adds and deletes, marked at fractions 0, 0.1,
    0.5, 0.9 and 1, some with a budget: itb_sweep.h equals the restated loop
    in every byte, every invariant holds, and a second sweep removes nothing."""
    fractions = (0.0, 0.1, 0.5, 0.9, 1.0)
    count = 10 if adepth < 8 else 5
    recs, budgets = [], []
    rng = np.random.default_rng(adepth)
    for k in range(count):
        recs.append(W.random_sweep_table(6000 + 31 * adepth + k, adepth, fractions[k % 5]).record())
        budgets.append(None if k < 5 else int(rng.integers(0, 1 << adepth)))
    want = agree(host_sweep, recs, [adepth] * count, budgets)
    assert all(w.fields["err"] == 0 for w in want) and want[0].fields["removed"] == 0
    assert adepth == 1 or any(w.produced for w in want)
    again = [(w.payload[: w.fields["len"] - C.H], W.swept_hdr(C.hdr_of(r), w.fields))
             for r, w, b in zip(recs, want, budgets) if w.produced and b is None]
    if again:
        w2 = W.expect([a[0] for a in again], [adepth] * len(again), [a[1] for a in again])
        assert all(w.fields == dict.fromkeys(W.RESULT_FIELDS, 0) for w in w2)
        same(host_sweep([a[0] for a in again], [adepth] * len(again), [a[1] for a in again], parts=True), w2,
             [a[0] for a in again])


def test_damaged_and_fuzzed_tables_are_never_walked(host_sweep):
    """Each table of kind_tables() except `valid`, the funnel, and 60 fuzzed
    tables, every ITE marked: what the check has a finding for is
    POM_SPLIT_E_DAMAGED with no byte changed; the rest sweep as the oracle
    says."""
    tables = [(name, bytearray(rec), adepth) for name, rec, adepth in W.damaged_tables()]
    ndamaged = len(tables)
    for seed in range(60):
        rec, adepth = C.fuzzed(9100 + seed, 1 + seed % 6)
        tables.append((f"fuzzed {seed}", rec, adepth))
    for name, rec, adepth in tables:
        for nr in range(min(1 << adepth, (len(rec) - C.ITB_SIZE) // C.ITE_SIZE)):
            W.set_state(rec, nr, W.UNLINKED)
    want = agree(host_sweep, [t[1] for t in tables], [t[2] for t in tables], None, [t[0] for t in tables],
                 invariants=False)
    errs = [w.fields["err"] for w in want]
    assert errs[:ndamaged] == [W.E_DAMAGED] * ndamaged and errs[ndamaged:].count(W.E_DAMAGED) >= 20


def test_error_rules(host_sweep):
    """Each rule before the next: a decoder's code, adepth 0 and 11, n = 11903,
    a live ITE cut short, an offset at residues 1 and 8, damage, nothing
    marked; a whole table beside them sweeps as ever."""
    t = W.random_sweep_table(9, 3, 0.5)
    rec = t.record()
    payload, hdr = C.payload_of(rec), C.hdr_of(rec)
    cut = payload[: C.ITE_OFF + C.ITE_SIZE * (max(t.hashes) + 1) - 1]
    drec = bytearray(C.kind_tables(3)["dup"][0])
    damaged, dhdr = C.payload_of(drec), C.hdr_of(drec)
    clean = C.payload_of(W.random_sweep_table(9, 3, 0.0).record())
    #        payload, adepth, hdr, status, residue, err
    cases = [(payload, 3, hdr, 0, 0, 0),
             (payload, 3, hdr, -6, 0, -6),
             (payload, 0, hdr, -4, 8, -4),
             (payload, 0, hdr, 0, 1, C.EINVAL),
             (payload, 11, hdr, 0, 0, C.EINVAL),
             (payload[: C.ITE_OFF - 1], 3, hdr, 0, 8, C.E_TRUNCATED),
             (cut, 3, hdr, 0, 0, C.E_TRUNCATED),
             (payload, 3, hdr, 0, 1, C.EINVAL),
             (payload, 3, hdr, 0, 8, C.EINVAL),
             (damaged, 3, dhdr, 0, 8, C.EINVAL),
             (damaged, 3, dhdr, 0, 0, W.E_DAMAGED),
             (payload, 3, dict(hdr, entries=hdr["entries"] + 1), 0, 0, W.E_DAMAGED),
             (clean, 3, hdr, 0, 0, 0),
             (payload, 3, hdr, 0, 0, 0)]
    payloads, adepths, hdrs, status, res, errs = (list(x) for x in zip(*cases))
    offs = [64 + r for r in res]
    want = W.expect(payloads, adepths, hdrs, None, offs, status)
    assert [w.fields["err"] for w in want] == errs
    assert want[0].produced and not want[12].produced and all(not w.produced for w in want[1:12])
    for parts in (False, True):
        got = host_sweep(payloads, adepths, hdrs, None, status, res, parts=parts)
        same(got, want, payloads)
        assert got[0][1] != payload and got[-1][0] == got[0][0]


def test_oracle_loop_invariants_over_many_tables():
    """The restated loop alone (no product code): the invariants over more
    tables than the comparison above takes."""
    n = 0
    for adepth in (1, 2, 3, 5):
        for k in range(40):
            rec = W.random_sweep_table(100 + k, adepth, (0.1, 0.5, 0.9, 1.0)[k % 4]).record()
            payload, hdr = C.payload_of(rec), C.hdr_of(rec)
            w = W.expect_one(payload, adepth, hdr, None if k % 3 else k % 7)
            if w.produced:
                W.invariants(payload, adepth, hdr, w)
                n += 1
    assert n > 100


# ---------------------------------------------------------------------------
# The header builder
# ---------------------------------------------------------------------------
def swept_example():
    t = W.random_sweep_table(21, 4, 0.5)
    rec = bytearray(t.record())
    w = W.expect_one(C.payload_of(rec), 4, C.hdr_of(rec))
    assert w.produced
    rec[:C.H] = np.random.default_rng(3).integers(0, 256, C.H, dtype=np.uint8).tobytes()      # pointers, locks, txg
    return rec, w


def test_header_byte_for_byte():
    """pom_itb_sweep_header against the oracle's header(): of the 264 bytes
    only the named fields differ from the old header; `state` stays."""
    rec, w = swept_example()
    f = w.fields
    for state in (0, 1, 4):
        rec[S.ITBH_STATE] = state
        h, lzo_ = itbsweep.sweep_header(rec[:C.H], w.result)
        assert (h, lzo_) == W.header(rec[:C.H], w.result) and lzo_ == 0 and h[S.ITBH_STATE] == state
        span = lambda off, size: set(range(off, off + size))
        fields = span(C.ITBH_ENTRIES, 8) | span(C.ITBH_PSEUDO, 4) | span(C.ITBH_ITU, 2) | span(C.ITBH_LEN, 8) | \
            span(S.ITBH_ALGO, 2)
        assert {i for i in range(C.H) if h[i] != rec[i]} <= fields
        got = C.hdr_of(h)
        assert (got["entries"], got["max_offset"], got["pseudo_conflicts"], got["itu"], got["ulen"]) == \
            (f["entries"], f["max_offset"], f["pseudo_conflicts"], f["itu"], f["len"])
    for res in (W._only(W.E_DAMAGED), W._only(0), W.RESULT.pack(0, 1, 1, 263, 0, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            itbsweep.sweep_header(rec[:C.H], res)


def test_not_smaller_rule_at_its_tie(oracle):
    """itb_lzo_compress keeps a stream only when it is smaller than the
    payload: a stream one byte longer, as long, one and two bytes shorter;
    then real payloads of the tie sizes whose oracle streams have those
    lengths.  The rule is the split's own function."""
    import record_util as R
    rec, w = swept_example()
    f = w.fields
    for diff in R.TIE_DIFFS:
        z = f["len"] - C.H + diff
        h, lzo_ = itbsweep.sweep_header(rec[:C.H], w.result, z)
        assert (h, lzo_) == W.header(rec[:C.H], w.result, z), diff
        assert lzo_ == int(diff < 0), diff
        ln, zlen, algo = struct.unpack_from("<IIH", h, C.ITBH_LEN)
        assert (ln, zlen, algo) == ((C.H + z, f["len"], 1) if diff < 0 else (f["len"], 0, 0)), diff
    for size in R.TIE_SIZES:
        for diff, payload in R.tie_search(oracle, size, R.TIE_DIFFS, 77).items():
            z = len(oracle.compress(payload))
            res = W.RESULT.pack(0, 1, 1, C.H + len(payload), 1, 0, 0, 0, 1)
            h, lzo_ = itbsweep.sweep_header(rec[:C.H], res, z)
            assert lzo_ == int(diff < 0) and h == W.header(rec[:C.H], res, z)[0], (size, diff)
    text = open(os.path.join(ROOT, "pomegranate_amd", "csrc", "itbsweep.c")).read()
    assert "pom_itb_stored_as(" in text and "POM_COMPR_LZO" not in text


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_no_gpu_sweep_batch_refuses():
    """LZO_E_ERROR, with every output as the caller left it."""
    rec = bytes(W.chain_table(2, "low", "UL").record())
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        itbsweep.sweep_batch([rec])
    buf = np.frombuffer(rec, dtype=np.uint8)
    ptrs, lens = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(buf.size)
    out = np.full(len(rec), 7, np.uint8)
    optr, caps, ol = (ctypes.c_void_p * 1)(out.ctypes.data), (ctypes.c_size_t * 1)(len(rec)), (ctypes.c_size_t * 1)(7)
    result = np.full(32, 7, np.uint8)
    err, ok = np.full(1, 7, np.int32), np.full(1, 7, np.int32)
    rc = itbsweep._lib().pom_itb_sweep_batch(ptrs, lens, 1, None, optr, caps, ol, result.ctypes.data, err.ctypes.data,
                                             ok.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    assert (out == 7).all() and (result == 7).all() and (err[0], ok[0], ol[0]) == (7, 7, 7)
    assert itbsweep._lib().pom_itb_sweep_batch(None, None, 0, None, None, None, None, None, None, None) == lzo.LZO_E_ERROR


# ---------------------------------------------------------------------------
# The stand-alone program, the exports
# ---------------------------------------------------------------------------
def test_standalone_check_passes():
    """itb_sweep_check: both forms of itb_sweep.h over seeded tables and
    flipped ones, every payload a heap block of exactly its length, built with
    AddressSanitizer and UBSan where they link."""
    r = subprocess.run([os.path.join(NATIVE, "itb_sweep_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "itb_sweep_check: ok" in r.stdout


def test_exports_are_declared():
    names = {"pom_itb_sweep_dev", "pom_itb_sweep_scratch", "pom_itb_sweep_header", "pom_itb_sweep_batch"}
    assert names <= set(lzo.EXPORTS)
    lib = lzo.load()
    assert all(hasattr(lib, name) for name in names)
    text = open(os.path.join(ROOT, "include", "pom_sweep.h")).read()
    assert all(re.search(rf"\b{name}\(", text) for name in names)
    # the launchers and the host pipeline's pieces are internal
    assert not {"lzo_mi355x_launch_itb_sweep", "lzo_mi355x_launch_itb_sweep_lens", "pom_itb_sweep_chunked",
                "pom_itb_stored_as"} & set(lzo.EXPORTS)
    out = subprocess.run(["nm", "-D", "--defined-only", lzo.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert names <= {ln.split()[-1] for ln in out.splitlines()}
    assert itbsweep.sweep_scratch_bytes(0) == 0 and itbsweep.sweep_scratch_bytes(5) >= 5 * 52
    # the device entry refuses a NULL hdr and a misaligned arena before it queues anything
    dev = itbsweep._lib().pom_itb_sweep_dev
    assert dev(None, None, None, None, None, None, None, 0, None, None, None) == C.EINVAL
    assert dev(8, None, None, None, None, 8, None, 0, None, None, None) == C.EINVAL
