"""The directed stream families (tests/lzo_families.py) on every decoder
path: the exact decoder, the windowed and the op-set throughput decoder with
the exact one behind them and alone, the latency decoder one block at a time
and eight side by side.  Sources sit at (5 i) mod 16, destinations are
guarded arenas (gpu_util.guarded_batch) with room for exactly the output.

Every path: status, out_len and bytes equal the builder's output and no
guard byte changes (gpu_util.check_decoded).  And include/lzo_mi355x.h's
"every valid stream with a 16-byte aligned destination stays on the
throughput decoders" as counts: the stand-alone throughput decoders hand
over nothing and launch everything, the paths with the exact decoder behind
them count 0 fallbacks.  The exceptions are exact: the look-behind streams of
family E (not valid: every path reports or hands over what the oracle
answers), and on the latency decoder the blocks with a length extension of
64 or more zero bytes (W's 70,000-byte matches; family Z stands on both
sides of that cap), which it hands over by design (lzo1x_decode_lat.hip
decode_at; stated in include/lzo_mi355x.h)."""
from __future__ import annotations

import pytest

import lzo_directed as ld
import lzo_families as lf
from gpu_util import FILL, HANDED, OK, PATHS, check_decoded, guarded_batch, run_path
from pomegranate_amd import lzo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAT_ZEROS = 64               # kLzoZerosLat (lzo1x_grammar.h)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


@pytest.fixture(scope="module")
def built(oracle):
    """family name -> its blocks, built once; E with its look-behind streams
    behind the valid ones.  Every block is what the oracle says it is."""
    cache = {}

    def get(name):
        if name not in cache:
            blocks = lf.FAMILIES[name]()
            if name == "E":
                blocks = blocks + lf.family_e_lookbehind()
            for b in blocks:
                assert oracle.decompress_safe(b.stream, b.cap) == (b.rc, b.output), b.name
            cache[name] = blocks
        return cache[name]
    return get


def decode_and_check(dev, debug_env, blocks, path, shift):
    """Launches `path` on the blocks (every destination at `shift` mod 16) and
    holds it to the module's rules; -> (status, handed, fallback count)."""
    names = [b.name for b in blocks]
    comps = [b.stream for b in blocks]
    caps = [b.cap for b in blocks]
    want = [(b.rc, b.output) for b in blocks]
    n = len(blocks)
    print(f"{path}: {lf.summary(blocks)}")
    src = guarded_batch(torch, comps, dev, [(5 * i) % 16 for i in range(n)], 0, neighbours="ff")
    dst = guarded_batch(torch, caps, dev, [shift] * n, FILL)
    olen, st, handed, fb = run_path(torch, path, dev, debug_env, comps, caps, src, dst)
    check_decoded(names, want, caps, olen, st, handed, dst)
    return st, handed, fb


def expected_handed(blocks, path, shift):
    """The ids a path may hand over -- and must: not valid (the look-behind
    streams), a destination alignment the decoder does not take, or, on the
    latency decoder, a zero run of its cap."""
    out = []
    for i, b in enumerate(blocks):
        misaligned = shift % {"win": 8, "fast": 16}.get(path.split("+")[0], 1) != 0
        capped = path.startswith("lat") and ld.extension_zeros(b.stream) >= LAT_ZEROS
        if b.rc != OK or misaligned or capped:
            out.append(i)
    return out


def hold_to_promise(blocks, path, shift, st, handed, fb):
    n = len(blocks)
    expect = expected_handed(blocks, path, shift)
    if handed is None:                                   # the exact decoder behind (or alone)
        assert st == [b.rc for b in blocks]
        assert fb == (None if path == "exact" else len(expect)), f"{fb} fallbacks, expected {len(expect)}"
        return
    assert None not in st, [blocks[i].name for i in range(n) if st[i] is None][:6]
    names = lambda ids: [blocks[i].name for i in ids][:6]
    assert handed == expect, (f"handed over but not expected: {names(sorted(set(handed) - set(expect)))}; "
                              f"expected but decoded: {names(sorted(set(expect) - set(handed)))}")
    assert [i for i in range(n) if st[i] == HANDED] == expect
    assert all(st[i] == OK for i in range(n) if i not in set(expect))


def for_path(built, family, path):
    """The latency paths launch from Python per block or group: they take P
    thinned to lf.P_THIN."""
    blocks = built(family)
    if family == "P" and path.startswith("lat"):
        keep = {f"P/d={d}" for d in lf.P_THIN}
        blocks = [b for b in blocks if b.name in keep]
        assert len(blocks) == len(lf.P_THIN)
    return blocks


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("family", list(lf.FAMILIES))
def test_directed(dev, debug_env, built, family, path):
    blocks = for_path(built, family, path)
    st, handed, fb = decode_and_check(dev, debug_env, blocks, path, 0)
    hold_to_promise(blocks, path, 0, st, handed, fb)
    if family in ("W", "W64", "Z") and path.startswith("lat"):
        # (the latency decoder's limit, exactly: the blocks with a 70,000-byte
        # match, and those of Z with 64 zero bytes, not those with 63)
        mark = "zeros=64" if family == "Z" else "L=70000"
        assert [blocks[i].name for i in handed] == [b.name for b in blocks if mark in b.name]
        assert 0 < len(handed) < len(blocks)
    elif family != "E":
        assert handed in (None, []) and fb in (None, 0)


@pytest.mark.parametrize("path", PATHS)
def test_ends_at_residue_8(dev, debug_env, built, path):
    """Family E with every destination at 8 mod 16: the windowed decoder takes
    it, the op-set decoder hands every block over -- and writes nothing
    outside the blocks on the way."""
    blocks = built("E")
    st, handed, fb = decode_and_check(dev, debug_env, blocks, path, 8)
    hold_to_promise(blocks, path, 8, st, handed, fb)
    if path == "fast":
        assert handed == list(range(len(blocks)))
    elif path == "win":
        assert handed == [i for i, b in enumerate(blocks) if b.rc != OK] and 0 < len(handed) < 16
