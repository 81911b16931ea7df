"""The directed stream builder (tests/lzo_directed.py) and its families
(tests/lzo_families.py) on the CPU: the builder against the random
generator and the oracle decoder, every family block through the oracle (the
builder's output at room n, OUTPUT_OVERRUN at n - 1) and through the shared
instruction grammar in all eight modes of test_grammar.py.  The families'
own coverage asserts run when they are built."""
from __future__ import annotations

import numpy as np
import pytest

import lzo_directed as ld
import lzo_families as lf
import lzo_streams
from grammar_util import DONE, MODES, REFUSED, decode, load

OK, E_OUTPUT_OVERRUN, E_LOOKBEHIND_OVERRUN = 0, -5, -6


@pytest.fixture(scope="module")
def harness():
    return load()


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lf.FAMILIES[name]()
            print(f"family {name}: {lf.summary(cache[name])}")
        return cache[name]
    return get


# ---------------------------------------------------------------------------
# The builder
# ---------------------------------------------------------------------------
def test_round_trip():
    """parse(assemble(ops)) is the merged op list with every form named."""
    a = bytes(range(1, 41))
    ops = [("L", a[:2]), ("L", a[2:3]),                   # merged: 3 first-byte literals, state C
           ("M", 2, 2),                                   # 2 bytes in state C: M1
           ("L", b"x"), ("M", 4, 2, "M1"), ("M", 1, 3), ("L", b""), ("L", a[:3]), ("L", a[3:9]),
           ("M", 9, 8), ("M", 9, 9), ("M", 2, 300), ("M", 20, 3, "M3"), ("L", b"yz"),
           ("M", 2, 3), ("L", a * 80),                    # 3200 bytes: an extended run, state B
           ("M", 0x801, 3, "M1"), ("L", a * 40), ("M", 0xC00, 3, "M1"), ("M", 0xC00, 3),
           ("L", a * 500),                                # past 0x4000 of output
           ("M", 0x4000, 3), ("M", 0x4001, 3), ("M", 0x4001, 10), ("M", 0x4001, 9 + 255 + 1),
           ("M", 0x3FFF, 33 + 255), ("M", 2048, 8), ("M", 2049, 8)]
    z, out = ld.assemble(ops)
    want = [("L", a[:3]), ("M", 2, 2, "M1"), ("L", b"x"), ("M", 4, 2, "M1"), ("M", 1, 3, "M2"),
            ("L", a[:9]), ("M", 9, 8, "M2"), ("M", 9, 9, "M3"), ("M", 2, 300, "M3"), ("M", 20, 3, "M3"),
            ("L", b"yz"), ("M", 2, 3, "M2"), ("L", a * 80), ("M", 0x801, 3, "M1"), ("L", a * 40),
            ("M", 0xC00, 3, "M1"), ("M", 0xC00, 3, "M3"), ("L", a * 500), ("M", 0x4000, 3, "M3"),
            ("M", 0x4001, 3, "M4"), ("M", 0x4001, 10, "M4"), ("M", 0x4001, 265, "M4"),
            ("M", 0x3FFF, 288, "M3"), ("M", 2048, 8, "M2"), ("M", 2049, 8, "M3")]
    assert ld.normalise(ops) == want
    got, offs = ld.parse(z)
    assert got == want
    assert offs == list(np.cumsum([0] + [len(o[1]) if o[0] == "L" else o[2] for o in want])[:-1])
    assert len(out) == ld.output_length(ops) and z.endswith(ld.EOF)
    assert ld.assemble(got) == (z, out)
    # a first literal too long for the first-byte form is an ordinary run
    z2, out2 = ld.assemble([("L", a * 6), ("M", 240, 5)])
    assert z2[:2] == bytes([0, 240 - 18]) and ld.parse(z2)[0] == [("L", a * 6), ("M", 240, 5, "M2")]


def test_builder_with_oracle(oracle):
    z, out = ld.assemble([("L", b"abcdefgh"), ("M", 3, 10), ("L", b"Q"), ("M", 1, 2), ("M", 12, 12),
                          ("L", b"0123456789" * 30), ("M", 300, 40, "M3")])
    assert out[:19] == b"abcdefgh" + b"fghfghfghf" + b"Q" and out[19:21] == b"QQ"
    assert oracle.decompress_safe(z, len(out)) == (OK, out)


@pytest.mark.parametrize("ops", [
    [("M", 1, 3)],                                        # no output yet
    [("L", b"abcd"), ("M", 5, 3)],                        # before the output
    [("L", b"abcd"), ("M", 1, 2)],                        # 2 bytes: only after trailing literals
    [("L", b"abc"), ("M", 1, 3, "M1")],
    [("L", b"abcd"), ("M", 1, 3, "M1")],                  # state B: distance 0x801..0xC00
    [("L", b"abcd"), ("M", 1, 9, "M2")],
    [("L", b"abcd"), ("M", 1, 3, "M4")],
    [("L", bytes(0x5000)), ("M", 0x4001, 3, "M3")],
    [("L", bytes(0x5000)), ("M", 0x4000, 3, "M4")],       # (would be the EOF marker)
    [("L", b"abcd"), ("M", 0xC000, 3)],
    [("L", b"abcd"), ("M", 0, 3)],
    [("L", b"abcd"), ("M", 2, 1)],
    [("L", b"abcd"), ("M", 2, 3, "M5")],
    [("L", b"abcd"), ("X", 2)],
    [("L", b"")],
])
def test_builder_raises(ops):
    with pytest.raises(ValueError):
        ld.assemble(ops)


def test_builder_against_generator():
    """Streams of the random full-grammar generator, parsed and assembled
    again with their forms: the same bytes."""
    forms = set()
    for n in (1, 50, 3000, 70000):
        for seed in range(12):
            z, out = lzo_streams.stream(4200 + 100 * seed + n, n)
            ops, offs = ld.parse(z)
            assert ld.assemble(ops) == (z, out), (seed, n)
            forms |= {(o[3], o[2] == 2) for o in ops if o[0] == "M"}
    assert forms == {("M1", True), ("M1", False), ("M2", False), ("M3", False), ("M4", False)}


def test_chain_depth():
    ops = [("L", b"abcd"), ("M", 2, 5), ("L", b"x"), ("M", 3, 2), ("M", 12, 12)]
    #        a b c d | c d c d c | x | d c | a b c d c d c d c x d c
    assert ld.chain_depth(ops).tolist() == [0, 0, 0, 0, 1, 1, 2, 2, 3, 0, 3, 4,
                                            1, 1, 1, 1, 2, 2, 3, 3, 4, 1, 4, 5]
    with pytest.raises(ValueError):
        ld.chain_depth([("L", b"a"), ("M", 2, 3)])


# ---------------------------------------------------------------------------
# The families
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lf.FAMILIES))
def test_family_oracle(oracle, built, name):
    """The oracle decodes every block to the builder's output, and answers
    OUTPUT_OVERRUN with one byte less room."""
    for b in built(name):
        assert b.rc == OK and b.cap == len(b.output) and b.cap > 0
        assert oracle.decompress_safe(b.stream, b.cap) == (OK, b.output), b.name
        rc, part = oracle.decompress_safe(b.stream, b.cap - 1)
        assert rc == E_OUTPUT_OVERRUN and part == b.output[:len(part)], b.name
        # no decoder's zero-run cap applies, but to the 70,000-byte matches of W
        zeros = ld.extension_zeros(b.stream)
        assert (zeros >= 62) == (bytes(62) in b.stream), b.name
        assert zeros < 62 or (name in ("W", "W64") and zeros == (70000 - 33 - 1) // 255) or \
            (name == "Z" and zeros in (63, 64)), (b.name, zeros)


@pytest.mark.parametrize("name", list(lf.FAMILIES))
def test_family_grammar(harness, built, name):
    """The shared instruction grammar, in every mode: DONE and the same bytes.
    A refusal only from a policy with a zero-run cap, on exactly the blocks
    whose longest length extension reaches it (W's 70,000-byte matches, and
    Z's 64 zero bytes under the latency decoder's policy)."""
    refused = 0
    for b in built(name):
        zeros = ld.extension_zeros(b.stream)
        for mname, mode, limit in MODES:
            rc, got = decode(harness, b.stream, b.cap, mode)
            if limit is not None and zeros >= limit:
                assert rc == REFUSED and got == b.output[:len(got)], (b.name, mname, rc)
                refused += 1
            else:
                assert rc == DONE and got == b.output, (b.name, mname, rc, len(got))
    assert (refused > 0) == (name in ("W", "W64", "Z"))


def test_family_block_names(built):
    names = [b.name for name in lf.FAMILIES for b in built(name)]
    assert len(set(names)) == len(names)
    thin = lf.family_p(lf.P_THIN)
    full = {b.name: b for b in built("P")}
    assert all(full[b.name] == b for b in thin) and len(thin) == 8


def test_lookbehind_streams(oracle, harness):
    """One byte before the output: the oracle's LOOKBEHIND_OVERRUN and the
    literals before the match; the grammar harness stops at the same op."""
    from grammar_util import LOOKBEHIND
    blocks = lf.family_e_lookbehind()
    valid = {b.name: b for b in lf.family_e()}
    for b in blocks:
        rc, part = oracle.decompress_safe(b.stream, b.cap)
        assert (rc, part) == (E_LOOKBEHIND_OVERRUN, b.output) == (b.rc, b.output), b.name
        twin = valid[b.name.replace("lookbehind", "byte0")]
        assert part == twin.output[:len(part)] and b.cap == twin.cap
        for mname, mode, _ in MODES:
            assert decode(harness, b.stream, b.cap, mode) == (LOOKBEHIND, b.output), (b.name, mname)
