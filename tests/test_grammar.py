"""The speculative decoders' instruction grammar
(pomegranate_amd/csrc/lzo1x_grammar.h) on the CPU, through
tests/native/grammar_host.cc: grammar_check compares the branch-free form
with the general form over instruction words, and libgrammar_host.so steps
through whole streams with the shared functions, in every mode (branch-free
with the general form where it asks for it, or the general form alone; each
decoder's zero-run policy), against the stream generator and the oracle's
recorded results."""
from __future__ import annotations

import subprocess

import pytest

from tests import lzo_streams
from tests.grammar_util import (CAPACITY, CHECK, DONE, GENERAL, MODES, POLICIES, REFUSED, decode,
                                load)


@pytest.fixture(scope="module")
def harness():
    return load()


def may_refuse(z: bytes, limit) -> bool:
    """A capped policy may refuse a stream that holds a zero run of its limit."""
    return limit is not None and bytes(limit) in z


def test_grammar_check_program(harness):
    """Branch-free form == general form, field for field, wherever it does not
    ask for the general form; both bit-field extraction variants agree."""
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grammar_check: ok" in r.stdout


@pytest.fixture(scope="module")
def valid_streams(edge, oracle):
    """(name, stream, output): generated full-grammar streams (the generator
    knows the output; 70,000 crosses the kernels' 2 KiB piece and 64 KiB ring
    sizes) and the oracle's streams of edge.npz."""
    out = []
    for n in (200, 5000, 70000):
        for seed in range(4):
            z, want = lzo_streams.stream(1000 * seed + n, n)
            out.append((f"stream({1000 * seed + n}, {n})", z, want))
    for name, data, z in zip(edge["names"], edge["inputs"], edge["comps"]):
        out.append((f"edge[{name}]", z, data))
    return out


@pytest.mark.parametrize("name,mode,limit", MODES, ids=[m[0] for m in MODES])
def test_valid_streams(harness, valid_streams, name, mode, limit):
    refused = []
    for sname, z, want in valid_streams:
        rc, got = decode(harness, z, len(want), mode)
        if rc == REFUSED and may_refuse(z, limit):
            refused.append(sname)
            continue
        assert rc == DONE and got == want, (sname, rc, len(got), len(want))
    assert limit is not None or not refused, f"{len(refused)} streams refused without a cap: {refused[:5]}"
    # (capped policies: only streams with a zero run of the cap or more)
    print(f"{name}: {len(refused)} of {len(valid_streams)} streams refused")


@pytest.mark.parametrize("name,mode,limit", MODES, ids=[m[0] for m in MODES])
def test_malformed_streams(harness, malformed, name, mode, limit):
    """At the recorded room: where the reference decodes (code 0), so does the
    harness, to the same bytes; where it does not, the harness refuses or
    stops (and never writes past the room: decode() checks)."""
    refused = 0
    for i, (z, cap, code, want) in enumerate(zip(malformed["streams"], malformed["caps"],
                                                 malformed["rc"], malformed["outs"])):
        rc, got = decode(harness, z, cap, mode)
        if code != 0:
            assert rc != DONE, (i, code)
        elif rc == REFUSED and may_refuse(z, limit):
            refused += 1
        else:
            assert rc == DONE and got == want, (i, rc, len(got), len(want))
    assert limit is not None or refused == 0
    print(f"{name}: {refused} decodable streams refused for a capped zero run")


def test_long_zero_runs(harness, longext):
    """Length extensions of ~16.8 M zero bytes, general form only.  The
    windowed decoder's true path refuses from 2^24 zeros on (the u32 length
    would wrap from 16,843,009 on); its speculative lanes and the latency
    decoder refuse much earlier.  The uncapped policy keeps a u32 length that
    wraps, as its kernel does: only that it stays inside the room is checked."""
    from tests.golden.make_golden import longext_stream
    for c in longext:
        z = c["stream"]
        assert c["zeros"] >= 1 << 24
        for pol in ("win_true", "win_spec", "lat"):
            rc, _ = decode(harness, z, c["cap"], POLICIES[pol][0] | GENERAL)
            assert rc == REFUSED, (c["kind"], c["zeros"], pol, rc)
        decode(harness, z, c["cap"], POLICIES["fast"][0] | GENERAL)
    # the cap itself: an M3 whose extension has one zero fewer is taken (its
    # length, 4,278,189,859, is still a u32: the match then finds no room),
    # one of 2^24 zeros is refused
    for zeros, want in (((1 << 24) - 1, CAPACITY), (1 << 24, REFUSED)):
        rc, got = decode(harness, longext_stream("m3", zeros), 1 << 20, POLICIES["win_true"][0] | GENERAL)
        assert rc == want and got == b"ABCD", (zeros, rc)
