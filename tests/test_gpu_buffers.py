"""The device ABI's buffer contract (include/lzo_mi355x.h): "block b reads
src + src_off[b] .. + src_len[b] and writes at most dst_cap[b] bytes at
dst + dst_off[b]", at every alignment mod 16, at capacities around every
edge, and with hostile bytes right behind each source block.

Every batch is a guarded arena (gpu_util.guarded_batch): one allocation, the
blocks at chosen residues mod 16, guard bytes between them and 4 KiB at both
ends, so a stray access lands in memory the test owns and shows as a changed
guard byte or a changed result -- never as a fault.  Everything is bit-exact
against the oracle (oracle/lzo1x_oracle.c).

The builders (alignment_streams, capacity_cases, prefix_cases, encoder_cases,
concat_cases) need only the oracle, and assert what the fixtures must hold
("no proper prefix decodes OK", "OK iff cap >= n", the `need` values); they
run without a GPU when called directly.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from gpu_util import (E_EOF_NOT_FOUND, E_INPUT_NOT_CONSUMED, E_INPUT_OVERRUN, E_OUTPUT_OVERRUN, FILL,
                      FILL_ENC, OK, PATHS, check_decoded, run_path)
from pomegranate_amd import lzo, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ["zero", "ff", "random", "continuation"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def gu():
    import gpu_util
    return gpu_util


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


# ---------------------------------------------------------------------------
# Builders (CPU only)
# ---------------------------------------------------------------------------
def _text3(oracle):
    """The oracle streams of TEXT, LZLIKE and ALPHA4 at 4096 B."""
    out = []
    for model, seed in ((synth.TEXT, 4401), (synth.LZLIKE, 4402), (synth.ALPHA4, 4403)):
        d = synth.block(model, seed, 4096)
        out.append((synth.MODEL_NAMES[model], d, oracle.compress(d)))
    return out


def alignment_streams(oracle):
    """A: 48 valid streams (data, stream), 8 of each kind: TEXT, LZLIKE, ALPHA4
    at 4096 B, ITB at 65,536 B, 13/14-byte blocks, 70,000 zero bytes.  Block i
    decodes to off % 16 == i % 16; the three 16-aligned places go to ITB, the
    zero block and TEXT, the three 8-but-not-16 ones to ITB, ALPHA4 and a
    14-byte block, the rest in turn."""
    kinds = ["text", "lzlike", "alpha4", "itb", "tiny", "zeros"]
    place = {0: "itb", 16: "zeros", 32: "text", 8: "itb", 24: "alpha4", 40: "tiny"}
    left = {k: 8 for k in kinds}
    for k in place.values():
        left[k] -= 1
    order, turn = [], 0
    for i in range(48):
        if i in place:
            order.append(place[i])
            continue
        while left[kinds[turn % 6]] == 0:
            turn += 1
        order.append(kinds[turn % 6])
        left[kinds[turn % 6]] -= 1
        turn += 1
    assert sorted(order) == sorted(kinds * 8)
    model = {"text": synth.TEXT, "lzlike": synth.LZLIKE, "alpha4": synth.ALPHA4, "itb": synth.ITB}
    out = []
    for i, k in enumerate(order):
        if k == "zeros":
            d = bytes(70000)
        elif k == "tiny":
            d = synth.block(synth.ITB, 4500 + i, 13 + (i >> 3 & 1))      # (i = 40: 14 bytes)
        else:
            d = synth.block(model[k], 4500 + i, 65536 if k == "itb" else 4096)
        z = oracle.compress(d)
        assert oracle.decompress_safe(z, len(d)) == (OK, d)
        out.append((f"{k}[{i}]", d, z))
    return out


def capacity_list(n):
    caps = [n - k for k in range(18)] + [n // 2, 2049, 2048, 2047, 65, 64, 63, 16, 9, 8, 7, 1, 0]
    seen, out = set(), []
    for c in caps:
        if 0 <= c <= n and c not in seen:
            seen.add(c)
            out.append(c)
    return out


def capacity_cases(oracle):
    """B: (name, stream, cap, destination shift, oracle result) over one TEXT
    4096 B stream, one ITB 65,536 B stream and one full-grammar stream (M1
    matches, long extensions; an output length that is no multiple of 8), each
    at capacities n .. n-17, n/2, around the windowed decoder's 2048-byte piece
    and down to 0.  Destination shifts cycle through 0-15 over the cases; each
    case stands twice more, at shifts 0 and 8, because the throughput
    decoders take only aligned destinations and it is their capacity edges
    that matter."""
    import lzo_streams
    d1 = synth.block(synth.TEXT, 4401, 4096)
    d2 = synth.block(synth.ITB, 4411, 65536)
    z3, d3 = lzo_streams.stream(3001, 6000)
    assert len(d3) % 8 and bytes(2) in z3
    streams = [("text", oracle.compress(d1), d1), ("itb", oracle.compress(d2), d2), ("grammar", z3, d3)]
    out, i = [], 0
    for name, z, d in streams:
        n = len(d)
        for cap in capacity_list(n):
            want = oracle.decompress_safe(z, cap)
            # the fixture cannot quietly become all-OK: OK iff cap >= n
            assert want[0] == (OK if cap >= n else E_OUTPUT_OVERRUN), (name, cap, want[0])
            assert want[1] == d[:len(want[1])]
            for shift in (i % 16, 0, 8):
                out.append((f"{name}/cap={cap}/shift={shift}", z, cap, shift, want))
            i += 1
    return out


def prefix_cases(oracle, malformed):
    """C: (name, stream, cap, continuation, oracle result): every prefix z[:k],
    k = 0..len(z), of the TEXT / LZLIKE / ALPHA4 4096 B streams and of the
    stream of ITB(300) + 70,000 zero bytes + ITB(300) (289 B: its length
    extension is a run of about 270 zero bytes, so the cuts land inside the
    run at every residue mod 16), then the first 300 malformed streams with
    their own capacities.  The continuation of a prefix is the rest of its own
    valid stream: a decoder that ignores src_len decodes a perfect block."""
    base = [(name, d, z) for name, d, z in _text3(oracle)]
    dz = synth.block(synth.ITB, 4421, 300) + bytes(70000) + synth.block(synth.ITB, 4422, 300)
    zz = oracle.compress(dz)
    assert bytes(256) in zz and len(zz) < 320
    base.append(("zrun", dz, zz))
    out = []
    for name, d, z in base:
        assert oracle.decompress_safe(z, len(d)) == (OK, d)
        for k in range(len(z) + 1):
            want = oracle.decompress_safe(z[:k], len(d))
            if k < len(z):                       # no proper prefix decodes OK
                assert want[0] in (E_INPUT_OVERRUN, E_EOF_NOT_FOUND), (name, k, want[0])
            out.append((f"{name}[:{k}]", z[:k], len(d), z[k:], want))
    nprefix = len(out)
    hostile = base[0][2]                         # a whole valid stream behind each malformed one
    for i in range(300):
        z, cap = malformed["streams"][i], malformed["caps"][i]
        want = oracle.decompress_safe(z, cap)
        assert want == (malformed["rc"][i], malformed["outs"][i])
        out.append((f"malformed[{i}]", z, cap, hostile, want))
    return out, nprefix


def encoder_cases(oracle):
    """E: (name, data, cap, need, oracle stream) for TEXT, ALPHA4 and RANDOM at
    4096 B, ITB at 65,536 and 70,000 B and blocks of 0, 1, 13 and 14 bytes, at
    capacities worst_compress(n), need+1 .. need-3 (the two bytes the emitter
    keeps staged, the 3-byte EOF marker), need/2, 3, 2, 1, 0."""
    blocks = [("text", synth.block(synth.TEXT, 4431, 4096)),
              ("alpha4", synth.block(synth.ALPHA4, 4432, 4096)),
              ("random", synth.block(synth.RANDOM, 4433, 4096)),
              ("itb64k", synth.block(synth.ITB, 4434, 65536)),
              ("itb70000", synth.block(synth.ITB, 4435, 70000))]
    blocks += [(f"tiny{n}", synth.block(synth.ITB, 4436 + n, n)) for n in (0, 1, 13, 14)]
    out = []
    for name, d in blocks:
        z = oracle.compress(d)
        need = len(z)
        assert 3 <= need <= lzo.worst_compress(len(d))
        caps, seen = [], set()
        for c in [lzo.worst_compress(len(d)), need + 1, need, need - 1, need - 2, need - 3,
                  need // 2, 3, 2, 1, 0]:
            if c >= 0 and c not in seen:
                seen.add(c)
                caps.append(c)
        out += [(f"{name}/cap={c}", d, c, need, z) for c in caps]
    return out


def concat_oracle(oracle, streams, cut, cap):
    """The header's rule for a block of consecutive streams, as a loop of
    lzo1x_decompress_safe calls: each stream decodes right after the previous
    one's output in what room is left; INPUT_NOT_CONSUMED goes on to the next
    stream, the last code wins."""
    z = b"".join(streams)[:cut]
    pos, produced, rc = 0, b"", None
    for s in streams:
        rc, out = oracle.decompress_safe(z[pos:], cap - len(produced))
        produced += out
        if rc != E_INPUT_NOT_CONSUMED:
            break
        # the stream that ended before the input did is `s`, whole
        assert oracle.decompress_safe(z[pos: pos + len(s)], cap - len(produced) + len(out))[0] == OK
        pos += len(s)
    assert rc != E_INPUT_NOT_CONSUMED            # (the cases carry no trailing bytes)
    return rc, produced


def concat_cases(oracle, columns):
    """F: (name, block, cap, continuation, oracle result).  The column.npz
    payloads whole (one reference stream per iovec, back to back), those of up
    to 8 KiB of data also cut at every 8th byte; a block of two TEXT streams
    cut at every 8th byte; and that block whole at capacities that end inside
    the second stream."""
    out = []

    def add(name, streams, cuts, cap):
        z = b"".join(streams)
        for cut in cuts:
            out.append((f"{name}[:{cut}]/cap={cap}", z[:cut], cap, z[cut:],
                        concat_oracle(oracle, streams, cut, cap)))

    for name, data, zipped, iov in zip(columns["names"], columns["data"], columns["zips"],
                                       columns["iov_len"]):
        payload, streams, at = zipped[8:], [], 0
        for n in iov:
            streams.append(oracle.compress(data[at: at + n]))
            at += n
        assert b"".join(streams) == payload and at == len(data)
        cuts = [len(payload)]
        if len(data) <= 8192:
            cuts = list(range(0, len(payload), 8)) + cuts
        add(name, streams, cuts, len(data))
        assert out[-1][4] == (OK, data)
    d = synth.block(synth.TEXT, 4401, 4096)
    z = oracle.compress(d)
    add("text2", [z, z], list(range(0, 2 * len(z), 8)) + [2 * len(z)], 8192)
    assert out[-1][4] == (OK, d + d)
    for cap in (8191, 8190, 8185, 8184, 8183, 6145, 6144, 6143, 4112, 4104, 4100, 4097, 4096, 4095, 1):
        add("text2", [z, z], [2 * len(z)], cap)
        assert out[-1][4][0] == E_OUTPUT_OVERRUN and len(out[-1][4][1]) <= cap
    return out


# ---------------------------------------------------------------------------
# The decoder paths: gpu_util.run_path, gpu_util.check_decoded
# ---------------------------------------------------------------------------


def long_extension(z):
    """The latency decoder hands over streams with 64 or more zero bytes of
    length extension (a zero run then costs linear time), and no others."""
    return bytes(64) in z


# ---------------------------------------------------------------------------
# A. Destination alignment
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def align_fx(oracle):
    return alignment_streams(oracle)


@pytest.mark.parametrize("path", PATHS)
def test_destination_alignment(dev, gu, debug_env, align_fx, path):
    """Every residue of the destination mod 16 in one batch (sources at
    (5 i) mod 16): exact bytes on every path, and the header's sentence "every
    valid stream with a 16-byte aligned destination stays on the throughput
    decoders (8 for the windowed one)" as counts: the windowed decoder hands
    over precisely the blocks with off % 8 != 0, the op-set decoder those with
    off % 16 != 0, the latency decoder none for alignment."""
    names = [n for n, _, _ in align_fx]
    comps = [z for _, _, z in align_fx]
    caps = [len(d) for _, d, _ in align_fx]
    want = [(OK, d) for _, d, _ in align_fx]
    n = len(comps)
    src = gu.guarded_batch(torch, comps, dev, [(5 * i) % 16 for i in range(n)], 0, neighbours="ff")
    dst = gu.guarded_batch(torch, caps, dev, [i % 16 for i in range(n)], FILL)
    assert sorted(set((dst.host_off % 16).tolist())) == list(range(16))
    olen, st, handed, fb = run_path(torch, path, dev, debug_env, comps, caps, src, dst)
    check_decoded(names, want, caps, olen, st, handed, dst)
    off8 = [i for i in range(n) if dst.host_off[i] % 8]
    off16 = [i for i in range(n) if dst.host_off[i] % 16]
    if path == "exact":
        assert st == [OK] * n
    elif path == "win+exact":
        assert st == [OK] * n and fb == len(off8) == 42
    elif path == "fast+exact":
        assert st == [OK] * n and fb == len(off16) == 45
    elif path == "win":
        assert handed == off8
    elif path == "fast":
        assert handed == off16
    else:
        assert set(handed) <= {i for i in range(n) if long_extension(comps[i])}, handed
        assert all(s == OK for i, s in enumerate(st) if i not in set(handed))


# ---------------------------------------------------------------------------
# B. Destination capacity
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capacity_fx(oracle):
    return capacity_cases(oracle)


@pytest.mark.parametrize("path", PATHS)
def test_destination_capacity(dev, gu, debug_env, capacity_fx, path):
    """Capacities n .. n-17, n/2, 2049 .. 2047, 65 .. 0 at destination shifts
    0-15: the oracle's code, length and bytes, and not one byte past the room
    -- also from the throughput decoders, which write before they know that a
    block fits."""
    names = [c[0] for c in capacity_fx]
    comps = [c[1] for c in capacity_fx]
    caps = [c[2] for c in capacity_fx]
    want = [c[4] for c in capacity_fx]
    n = len(comps)
    src = gu.guarded_batch(torch, comps, dev, [(3 * i) % 16 for i in range(n)], 0, neighbours="ff")
    dst = gu.guarded_batch(torch, caps, dev, [c[3] for c in capacity_fx], FILL)
    olen, st, handed, _ = run_path(torch, path, dev, debug_env, comps, caps, src, dst)
    check_decoded(names, want, caps, olen, st, handed, dst)


# ---------------------------------------------------------------------------
# C. Source bounds (hostile neighbours)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prefix_fx(oracle, malformed):
    cases, nprefix = prefix_cases(oracle, malformed)
    return {"all": cases, "lat": cases[:nprefix][::16], "seen": {}}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", PATHS)
def test_source_bounds(dev, gu, debug_env, prefix_fx, path, mode):
    """Truncated streams with zeros, 0xFF, random bytes or the valid rest of
    their own stream right behind them in memory (sources at every residue mod
    16): the oracle's result on the stream alone, whatever the neighbours --
    and the same status and out_len in all four neighbourhoods, also from the
    stand-alone throughput decoders.  The latency decoder (a launch per block
    or per group of 8 from Python) takes every 16th prefix."""
    cases = prefix_fx["lat" if path.startswith("lat") else "all"]
    names = [c[0] for c in cases]
    comps = [c[1] for c in cases]
    caps = [c[2] for c in cases]
    want = [c[4] for c in cases]
    n = len(comps)
    src = gu.guarded_batch(torch, comps, dev, [i % 16 for i in range(n)], 0, neighbours=mode,
                           continuation=[c[3] for c in cases] if mode == "continuation" else None)
    dst = gu.guarded_batch(torch, caps, dev, [0] * n, FILL)
    olen, st, handed, _ = run_path(torch, path, dev, debug_env, comps, caps, src, dst)
    check_decoded(names, want, caps, olen, st, handed, dst)
    # identical across the neighbourhoods (handed-over blocks: their status)
    mine = [(s, o if s == OK else None) for s, o in zip(st, olen)] if handed is not None else list(zip(st, olen))
    first_mode, first = prefix_fx["seen"].setdefault(path, (mode, mine))
    diff = [names[i] for i in range(n) if mine[i] != first[i]]
    assert not diff, f"{len(diff)} blocks differ between neighbours {first_mode!r} and {mode!r}: {diff[:6]}"


# ---------------------------------------------------------------------------
# D. decoded_length_dev
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ff", "continuation"])
def test_decoded_length_dev(dev, gu, oracle, unchecked, align_fx, prefix_fx, mode):
    """lzo_mi355x_decoded_length_dev (the unchecked decoder's view, no
    output): status and out_len equal oracle.decompress_unchecked's -- and the
    reference's recorded rc / out_len on the unchecked.npz streams (valid,
    trailing bytes, concatenated, EOF-cut) -- on the valid streams of A and on
    every 8th prefix of C.  Both read bytes past the end as zero and stop 64
    bytes past it, so the neighbours must not change the answer."""
    cases = []                                   # (name, stream, continuation, rc, out_len)
    for i, (k, s, rc, n) in enumerate(zip(unchecked["kinds"], unchecked["streams"], unchecked["rc"],
                                          unchecked["out_len"])):
        got = oracle.decompress_unchecked(s)
        assert (got[0], len(got[1])) == (rc, n), (i, k)
        cases.append((f"unchecked[{i}]:{k}", s, b"\x11\x00\x00", rc, n))
    for name, d, z in align_fx:
        cases.append((name, z, z, OK, len(d)))
    npre = len(prefix_fx["all"]) - 300
    for name, z, cap, cont, _ in prefix_fx["all"][:npre][::8]:
        rc, out = oracle.decompress_unchecked(z, room=1 << 20)
        cases.append((name, z, cont, rc, len(out)))
    comps = [c[1] for c in cases]
    n = len(comps)
    src = gu.guarded_batch(torch, comps, dev, [i % 16 for i in range(n)], 0, neighbours=mode,
                           continuation=[c[2] for c in cases] if mode == "continuation" else None)
    olen = torch.full((n,), 77, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    lzo.decoded_length_dev(src, olen, st)
    torch.cuda.synchronize()
    got = list(zip(st.cpu().numpy().tolist(), olen.cpu().numpy().view(np.uint32).tolist()))
    bad = [(c[0], g, (c[3], c[4])) for c, g in zip(cases, got) if g != (c[3], c[4])]
    assert not bad, f"{len(bad)} of {n} differ (name, got, oracle): {bad[:6]}"


# ---------------------------------------------------------------------------
# E. Encoder capacity and destination alignment
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder_fx(oracle):
    return encoder_cases(oracle)


@pytest.mark.parametrize("kernel", ["lds", "gdict_one_wave", "gdict_two_wave", "general"])
def test_encoder_capacity(dev, gu, debug_env, encoder_fx, kernel):
    """All four encoder kernels at capacities around the needed length,
    destinations at every residue mod 16 (sources at (7 i) mod 16): OK iff
    cap >= need, then the oracle's bytes; otherwise OUTPUT_OVERRUN with
    out_len == need (the length the block would have needed); and never a
    byte past the room.  The general one-wave encoder, which the public API
    reaches only past 16 MiB, is launched directly."""
    names = [c[0] for c in encoder_fx]
    blocks = [c[1] for c in encoder_fx]
    caps = [c[2] for c in encoder_fx]
    n = len(blocks)
    src = gu.guarded_batch(torch, blocks, dev, [(7 * i) % 16 for i in range(n)], 0, neighbours="ff")
    # (end guards that hold a whole unclipped stream: an encoder that lost its
    # clip still writes only into memory this test owns)
    dst = gu.guarded_batch(torch, caps, dev, [i % 16 for i in range(n)], FILL_ENC,
                           ends=(max(caps) + 4096 + 15) // 16 * 16)
    olen = torch.full((n,), 77, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    if kernel == "general":
        fn = lzo.load().lzo_mi355x_launch_compress
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        p = lambda t: t.data_ptr()
        assert fn(p(src.arena), p(src.off), p(src.length), p(dst.arena), p(dst.off), p(dst.length),
                  p(olen), p(st), n, 0, torch.cuda.current_stream().cuda_stream) == 0
    elif kernel == "lds":
        lzo.compress_dev(src, dst, olen, st, scratch=None)
    else:
        debug_env("enc_waves=2" if kernel == "gdict_two_wave" else "enc_waves=1")
        scr = torch.full((lzo.compress_scratch_bytes(n),), 0x5A, dtype=torch.uint8, device=dev)
        lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    st = st.cpu().numpy().tolist()
    olen = olen.cpu().numpy().view(np.uint32).tolist()
    written = [min(o, c) for o, c in zip(olen, caps)]
    problems = []
    try:
        arena = gu.assert_guards(dst, written, FILL_ENC)
    except AssertionError as e:
        problems.append(str(e))
        arena = dst.arena.cpu().numpy()
    bad = []
    for i, (name, d, cap, need, z) in enumerate(encoder_fx):
        o = int(dst.host_off[i])
        if cap >= need:
            good = (st[i], olen[i]) == (OK, need) and arena[o: o + need].tobytes() == z
        else:
            good = (st[i], olen[i]) == (E_OUTPUT_OVERRUN, need)
        if not good:
            bad.append((name, st[i], olen[i], need))
    if bad:
        problems.append(f"{len(bad)} of {n} wrong (name, status, out_len, need): {bad[:6]}")
    assert not problems, "\n".join(problems)


# ---------------------------------------------------------------------------
# F. Concatenated streams
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def concat_fx(oracle, fwritev_columns):
    return concat_cases(oracle, fwritev_columns)


@pytest.mark.parametrize("mode", ["ff", "continuation"])
def test_concat_streams(dev, gu, concat_fx, mode):
    """lzo_mi355x_launch_decompress_concat on guarded batches: the total
    out_len, the status and the bytes of a per-stream loop of
    lzo1x_decompress_safe (go on after INPUT_NOT_CONSUMED, the last code
    wins), whatever lies behind the block, and not a byte past the room."""
    names = [c[0] for c in concat_fx]
    comps = [c[1] for c in concat_fx]
    caps = [c[2] for c in concat_fx]
    want = [c[4] for c in concat_fx]
    n = len(comps)
    src = gu.guarded_batch(torch, comps, dev, [i % 16 for i in range(n)], 0, neighbours=mode,
                           continuation=[c[3] for c in concat_fx] if mode == "continuation" else None)
    dst = gu.guarded_batch(torch, caps, dev, [(11 * i) % 16 for i in range(n)], FILL)
    fn = lzo.load().lzo_mi355x_launch_decompress_concat
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_uint32, ctypes.c_void_p]
    olen = torch.full((n,), 77, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    assert fn(p(src.arena), p(src.off), p(src.length), p(dst.arena), p(dst.off), p(dst.length),
              p(olen), p(st), n, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    check_decoded(names, want, caps, olen.cpu().numpy().view(np.uint32).tolist(),
                  st.cpu().numpy().tolist(), None, dst)
