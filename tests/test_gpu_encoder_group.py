"""GPU: the grouped global-dictionary encoder (lzo1x_encode_fast.hip,
enc_group_body: eight parse waves and two emit waves to a workgroup), forced
with the debug key enc_group=82 on batches of a few blocks: compressed bytes,
lengths and statuses against the oracle for partly filled groups, mixed sizes
in one group, block tickets (hand-overs of a slot), full and nearly idle token
queues, a capacity one byte short, and the adversarial claim inputs of
tests/test_encoder_claims.py.  And both sides of the rule that picks between
it and the one-wave kernel (lzo1x_enc_group.h, enc_group_use)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from gpu_util import E_OUTPUT_OVERRUN, FILL_ENC, OK
from pomegranate_amd import lzo, synth
from test_encoder_claims import claim_blocks

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GROUP = "enc_group=82"         # the default shape, whatever the batch
ONE, GROUPED, G = 1, 82, 8     # lzo_mi355x_debug_enc_kernel; parse waves per workgroup


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


def enc_kernel(nblocks: int) -> int:
    """The encoder a batch of nblocks with its scratch takes under the current debug keys."""
    fn = lzo.load().lzo_mi355x_debug_enc_kernel
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_size_t]
    return fn(nblocks, 1, lzo.compress_scratch_bytes(nblocks))


def run(gu, dev, blocks):
    """Device-batch compress with a dirty scratch -> streams, statuses."""
    src = gu.device_batch(torch, blocks, dev, shift=3)
    dst = gu.empty_batch(torch, [lzo.worst_compress(len(b)) for b in blocks], dev, fill=FILL_ENC)
    n = len(blocks)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    scr = torch.full((lzo.compress_scratch_bytes(n),), 0x5A, dtype=torch.uint8, device=dev)
    lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    return gu.fetch(dst, olen), st.cpu().numpy().tolist()


def check(oracle, blocks, comps, st):
    assert st == [OK] * len(blocks)
    bad = [(i, len(b)) for i, (b, c) in enumerate(zip(blocks, comps)) if c != oracle.compress(b)]
    assert not bad, f"{len(bad)} of {len(blocks)} differ from the oracle (index, size): {bad[:8]}"


MIXED = [1, 13, 14, 4096, 65536, 65549, 300000]


def mixed_blocks(count, seed):
    """count ITB blocks of the MIXED sizes in turn: 1 and 13 are a tail token
    alone, 65,549 is the first size that re-bases, 300,000 re-bases many times
    while its neighbours finish and exit."""
    return [synth.block(synth.ITB, seed + i, MIXED[i % len(MIXED)]) for i in range(count)]


SHAPES = [41, 81, 82, 84]      # 4 + 1, 8 + 1, 8 + 2 (the default), 8 + 4


@pytest.mark.parametrize("nblocks", [1, 3, 4, 5, 9, 17])
@pytest.mark.parametrize("shape", SHAPES)
def test_partial_groups(dev, gu, oracle, debug_env, shape, nblocks):
    """Idle parse waves, and a last workgroup that is partly filled."""
    debug_env(f"enc_group={shape}")
    assert enc_kernel(nblocks) == shape
    blocks = [synth.block(synth.ITB, 700 + i, 20000 + 4001 * i) for i in range(nblocks)]
    check(oracle, blocks, *run(gu, dev, blocks))


def test_mixed_sizes_in_one_group(dev, gu, oracle, debug_env):
    debug_env(GROUP)
    blocks = mixed_blocks(len(MIXED), 720)
    check(oracle, blocks, *run(gu, dev, blocks))


@pytest.mark.parametrize("grid", [5, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_ticket_mode(dev, gu, oracle, debug_env, shape, grid):
    """23 mixed-size blocks over 5 regions (4 + 1: two workgroups, one with a
    single live parse wave; 8 + E: one with three idle ones) and over 4 (one
    workgroup, every slot handing over several times)."""
    debug_env(f"enc_group={shape},enc_grid={grid}")
    assert enc_kernel(23) == shape
    blocks = mixed_blocks(23, 740)
    check(oracle, blocks, *run(gu, dev, blocks))


def test_queue_pressure(dev, gu, oracle, debug_env):
    """alpha4: many short tokens a window, the queue fills and the parse wave
    waits for room; zeros: one long match, an idle emitter, then the tail."""
    debug_env(GROUP)
    blocks = [synth.block(synth.ALPHA4, 760, 65536), synth.block(synth.ZEROS, 761, 65536),
              synth.block(synth.ALPHA4, 762, 65536), synth.block(synth.ZEROS, 763, 65536),
              synth.block(synth.ALPHA4, 764, 65536)]
    check(oracle, blocks, *run(gu, dev, blocks))


@pytest.mark.parametrize("short", [0, 3])
def test_capacity_one_byte_short(dev, gu, oracle, debug_env, short):
    """One block of a group with a dst_cap one byte short: -5 with out_len the
    needed length, its three neighbours exact, nothing past any capacity."""
    debug_env(GROUP)
    blocks = [synth.block(synth.ITB, 780 + i, 30000 + 1111 * i) for i in range(4)]
    want = [oracle.compress(b) for b in blocks]
    caps = [len(z) - 1 if i == short else lzo.worst_compress(len(b))
            for i, (b, z) in enumerate(zip(blocks, want))]
    src = gu.guarded_batch(torch, blocks, dev, [(7 * i) % 16 for i in range(4)], 0, neighbours="ff")
    dst = gu.guarded_batch(torch, caps, dev, [(5 * i + 1) % 16 for i in range(4)], FILL_ENC,
                           ends=(max(caps) + 4096 + 15) // 16 * 16)
    olen = torch.full((4,), 77, dtype=torch.int32, device=dev)
    st = torch.full((4,), 99, dtype=torch.int32, device=dev)
    scr = torch.full((lzo.compress_scratch_bytes(4),), 0x5A, dtype=torch.uint8, device=dev)
    lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    st = st.cpu().numpy().tolist()
    olen = olen.cpu().numpy().view(np.uint32).tolist()
    arena = gu.assert_guards(dst, [min(o, c) for o, c in zip(olen, caps)], FILL_ENC)
    assert st == [E_OUTPUT_OVERRUN if i == short else OK for i in range(4)]
    assert olen == [len(z) for z in want]
    for i, z in enumerate(want):
        if i != short:
            o = int(dst.host_off[i])
            assert arena[o: o + len(z)].tobytes() == z, i


def test_adversarial_claims(dev, gu, oracle, debug_env):
    debug_env(GROUP)
    blocks = [b for _, b in claim_blocks()]
    check(oracle, blocks, *run(gu, dev, blocks))


def test_selection_rule(dev, gu, oracle, debug_env):
    """Without debug keys: a batch whose groups do not reach every CU stays
    with the one-wave kernel, one that does takes the grouped kernel; the keys
    enc_waves=1 / 2 still select the kernels they name.  Both sides against
    the oracle."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    few, many = G * (cus - 1), G * (cus - 1) + 1
    assert (enc_kernel(1), enc_kernel(G), enc_kernel(few), enc_kernel(many)) == (ONE, ONE, ONE, GROUPED)
    blocks = [synth.block(synth.ITB, 800 + i, 200 + (37 * i) % 1800) for i in range(many)]
    want = [oracle.compress(b) for b in blocks]
    for n in (few, many):
        comps, st = run(gu, dev, blocks[:n])
        assert st == [OK] * n and comps == want[:n], n
    debug_env("enc_waves=1")
    assert enc_kernel(many) == ONE
    debug_env("enc_waves=2")
    assert enc_kernel(many) == 2
