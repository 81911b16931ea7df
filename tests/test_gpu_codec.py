"""GPU parity: the HIP kernels through the C-ABI against the reference's golden
vectors and the oracle.  Bit-exact everywhere (integer/byte work):
  - compressed bytes identical to lib/minilzo.c with a zero-filled wrkmem,
  - decompressed bytes identical to the input,
  - lzo1x_decompress_safe return codes, produced lengths and produced bytes
    identical on malformed streams.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import pytest

from conftest import batch_sizes
from pomegranate_amd import lzo, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


@pytest.mark.parametrize("shift", [0, 1, 3])
def test_compress_edge_vectors_bit_exact(dev, gu, edge, shift):
    outs, st = gu.gpu_compress(torch, edge["inputs"], dev, shift=shift)
    assert all(s == 0 for s in st)
    bad = [n for n, o, z in zip(edge["names"], outs, edge["comps"]) if o != z]
    assert not bad, f"{len(bad)} mismatches, first {bad[:5]}"


@pytest.mark.parametrize("shift", [0, 1, 2])
def test_decompress_edge_vectors(dev, gu, edge, shift):
    caps = [len(d) for d in edge["inputs"]]
    outs, st, _ = gu.gpu_decompress(torch, edge["comps"], caps, dev, shift=shift)
    assert all(s == 0 for s in st), [n for n, s in zip(edge["names"], st) if s][:5]
    bad = [n for n, o, d in zip(edge["names"], outs, edge["inputs"]) if o != d]
    assert not bad, f"{len(bad)} mismatches, first {bad[:5]}"


def test_decompress_malformed_error_codes(dev, gu, malformed):
    outs, st, _ = gu.gpu_decompress(torch, malformed["streams"], malformed["caps"], dev)
    bad = [i for i in range(len(st))
           if st[i] != malformed["rc"][i] or outs[i] != malformed["outs"][i]]
    assert not bad, [(i, st[i], malformed["rc"][i]) for i in bad[:8]]


def test_decompress_respects_capacity(dev, gu):
    """Bytes past dst_cap are never written (lib/minilzo.c:3740 NEED_OP)."""
    d = synth.block(synth.ITB, 3, 65536)
    z = lzo_oracle_free_compress(dev, gu, d)
    outs, st, dst = gu.gpu_decompress(torch, [z, z], [1000, 65536], dev)
    assert st == [lzo.LZO_E_OUTPUT_OVERRUN, 0]
    arena = dst.arena.cpu().numpy()
    off = dst.off.cpu().numpy()
    assert (arena[1000: int(off[1])] == 0x5A).all()
    assert outs[0] == d[:len(outs[0])]


def lzo_oracle_free_compress(dev, gu, d):
    outs, st = gu.gpu_compress(torch, [d], dev)
    assert st == [0]
    return outs[0]


@pytest.mark.parametrize("name", ["C1", "C2C3", "C4_sample", "C4_order", "itb_max", "random_300k",
                                  "models64k_random", "models64k_itb", "models64k_zeros",
                                  "models64k_alpha4", "models64k_lzlike", "models64k_text"])
def test_manifest_batches_round_trip(dev, gu, manifest, name):
    """Full-size batches: GPU compressed stream hashes to the reference's; the
    GPU decode of it reproduces the input hash."""
    entry = next(e for e in manifest if e["name"] == name)
    arena, offs, lens = synth.batch(entry["model_id"], entry["seed0"], batch_sizes(entry))
    blocks = [arena[int(offs[b]): int(offs[b]) + int(lens[b])].tobytes()
              for b in range(len(lens))]
    comps, st = gu.gpu_compress(torch, blocks, dev)
    assert all(s == 0 for s in st)
    assert [len(c) for c in comps] == entry["zlens"]
    assert hashlib.sha256(b"".join(comps)).hexdigest() == entry["sha256_z"]
    outs, st2, _ = gu.gpu_decompress(torch, comps, [len(b) for b in blocks], dev)
    assert all(s == 0 for s in st2)
    assert hashlib.sha256(b"".join(outs)).hexdigest() == entry["sha256_input"]


@pytest.mark.parametrize("name", ["C1", "C2C3", "C4_sample", "C4_order", "itb_max", "random_300k"])
def test_manifest_batches_bench_encoder(dev, gu, manifest, name):
    """The same full-size batches through the encoder the bench times (device
    batch with scratch: lzo1x_encode_gdict1_kernel, global dictionaries,
    block tickets on C4's mixed sizes): compressed stream hashes to the
    reference's.  C4_order has more blocks than one
    resident round, so the batch starts largest first (lzo1x_order_kernel),
    the C4 regime."""
    entry = next(e for e in manifest if e["name"] == name)
    if name == "C4_order":
        import ctypes
        lib = lzo.load()
        lib.lzo_mi355x_fast_resident_blocks.restype = ctypes.c_uint32
        assert entry["nblocks"] > lib.lzo_mi355x_fast_resident_blocks()
    arena, offs, lens = synth.batch(entry["model_id"], entry["seed0"], batch_sizes(entry))
    blocks = [arena[int(offs[b]): int(offs[b]) + int(lens[b])].tobytes()
              for b in range(len(lens))]
    comps, st = gu.gpu_compress(torch, blocks, dev, scratch=True)
    assert all(s == 0 for s in st)
    assert [len(c) for c in comps] == entry["zlens"]
    assert hashlib.sha256(b"".join(comps)).hexdigest() == entry["sha256_z"]


def test_bench_encoder_dirty_scratch_reused_dictionaries(dev, gu, oracle):
    """The bench encoder's dictionaries need no zeroing (round 6: a per-block
    LDS bitmap of written slots, EncLdsT::occ).  Twice as many blocks as
    resident workgroups, so each workgroup codes a second block in the region
    its first one filled, and every block is a copy of one of two contents:
    a stale entry of the earlier block would point at equal bytes and turn
    literals into matches the reference (a zero-filled wrkmem,
    lib/minilzo.c:2878-2883, 3167-3173) never finds.  The scratch starts
    filled with 0x5A, not zeros."""
    lib = lzo.load()
    lib.lzo_mi355x_fast_resident_blocks.restype = ctypes.c_uint32
    n = 2 * int(lib.lzo_mi355x_fast_resident_blocks())
    a = synth.block(synth.ITB, 4242, 8192)
    b = synth.block(synth.ALPHA4, 4243, 8192)
    blocks = [a if i % 2 == 0 else b for i in range(n)]
    src = gu.device_batch(torch, blocks, dev)
    dst = gu.empty_batch(torch, [lzo.worst_compress(len(x)) for x in blocks], dev, fill=0xA5)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    scr = torch.full((lzo.compress_scratch_bytes(n),), 0x5A, dtype=torch.uint8, device=dev)
    lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    comps = gu.fetch(dst, olen)
    assert st.cpu().numpy().tolist() == [0] * n
    want = [oracle.compress(a), oracle.compress(b)]
    bad = [i for i in range(n) if comps[i] != want[i % 2]]
    assert not bad, f"{len(bad)} of {n} blocks differ, first {bad[:8]}"


def test_long_extensions_past_32_bits(dev, longext):
    """Length extensions of 16,843,008-16,843,010 zero bytes (255 per zero
    passes 2^32 from 16,843,009 on): lzo1x_decompress_safe and a host batch
    return the reference's code, length and bytes (tests/golden/longext.json,
    from lib/minilzo.c: OUTPUT_OVERRUN -- a 32-bit sum wraps to a small length
    and would decode the rest of the stream as valid)."""
    import time
    for c in longext:
        t0 = time.perf_counter()
        rc, out = lzo.lzo1x_decompress_safe(c["stream"], c["cap"])
        dt = time.perf_counter() - t0
        print(f"{c['kind']} zeros={c['zeros']}: rc={rc} out={len(out)} {dt * 1e3:.1f} ms")
        assert (rc, len(out), hashlib.sha256(out).hexdigest()) == \
            (c["rc"], c["out_len"], c["out_sha256"]), (c["kind"], c["zeros"])
    sel = [c for c in longext if c["zeros"] == 16843009]
    rc, status, outs = lzo.decompress_batch([c["stream"] for c in sel], [c["cap"] for c in sel])
    assert rc == 0
    for c, s, o in zip(sel, status, outs):
        assert s == c["rc"], (c["kind"], s)


def test_random_sizes_vs_oracle(dev, gu, oracle):
    rng = np.random.default_rng(5)
    blocks = [synth.block(int(rng.integers(0, 6)), 80000 + i, int(rng.integers(0, 140000)))
              for i in range(96)]
    comps, st = gu.gpu_compress(torch, blocks, dev, shift=5)
    assert all(s == 0 for s in st)
    for i, (b, c) in enumerate(zip(blocks, comps)):
        assert c == oracle.compress(b), i
    outs, st2, _ = gu.gpu_decompress(torch, comps, [len(b) for b in blocks], dev, shift=7)
    assert all(s == 0 for s in st2) and outs == blocks


def test_single_call_api(dev, edge):
    """The minilzo.h surface itself (what mds/itb.c and api/api.c call)."""
    assert lzo.lzo_init() == lzo.LZO_E_OK
    for d, z in list(zip(edge["inputs"], edge["comps"]))[::97] + [(b"", edge["comps"][0])]:
        if not d:
            continue
        rc, got = lzo.lzo1x_1_compress(d)
        assert rc == 0 and got == z
        rc, back = lzo.lzo1x_decompress(z)
        assert rc == 0 and back == d
        rc, back = lzo.lzo1x_decompress_safe(z, len(d))
        assert rc == 0 and back == d
    rc, got = lzo.lzo1x_1_compress(b"")
    assert rc == 0 and got == bytes([0x11, 0, 0])


def test_unchecked_decompress_codes(dev, unchecked):
    """The unchecked lzo1x_decompress of the drop-in (what mds/itb.c:2964,
    mdsl/gc.c:770 and api/api.c:6438 call) against the reference's own
    unchecked decoder: return code, *out_len and bytes on valid streams,
    trailing bytes, concatenated per-iovec streams and EOF-cut streams
    (lib/minilzo.c:3676-3680)."""
    bad = []
    for i, (k, s, rc, n, sha) in enumerate(zip(unchecked["kinds"], unchecked["streams"],
                                               unchecked["rc"], unchecked["out_len"],
                                               unchecked["sha"])):
        got_rc, got = lzo.lzo1x_decompress(s)
        if (got_rc, len(got), hashlib.sha256(got).hexdigest()) != (rc, n, sha):
            bad.append((i, k, got_rc, rc, len(got), n))
    assert not bad, bad[:8]


def test_single_calls_from_many_threads(dev, oracle):
    """Single calls arriving together from several threads (the MDS commit and
    service threads, mds/txg.c:1010-1011, mds/itb.c:2964) are combined into
    shared launches (single_queue.c, host_single.c); every caller still gets exactly
    its own bytes, length and return code, whatever else shares its launch."""
    from concurrent.futures import ThreadPoolExecutor
    sizes = [12416, 65536, 100, 300000, 4096, 1, 70000, 536192] * 4
    blocks = [synth.block(synth.ITB if i % 3 else synth.TEXT, 4242 + i, n) for i, n in enumerate(sizes)]
    want = [oracle.compress(b) for b in blocks]

    def work(i):
        d, z = blocks[i], want[i]
        out = []
        for _ in range(3):
            rc, got = lzo.lzo1x_1_compress(d)
            out.append(rc == 0 and got == z)
            rc, back = lzo.lzo1x_decompress(z)
            out.append(rc == 0 and back == d)
            rc, back = lzo.lzo1x_decompress_safe(z, len(d))
            out.append(rc == 0 and back == d)
            rc, _ = lzo.lzo1x_decompress_safe(z, len(d) - 1)      # one byte short
            out.append(rc == lzo.LZO_E_OUTPUT_OVERRUN)
        return i, out

    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map(work, range(len(blocks))))
    bad = [(i, o) for i, o in res if not all(o)]
    assert not bad, bad[:4]


@pytest.mark.parametrize("n", [65536, 262145, 536192, (2 << 20) + 7])
def test_unchecked_single_call_large_output(dev, oracle, n):
    """Outputs beyond the single call's first guess (16x the input, at least
    256 KiB) take the second round trip; bytes and length stay exact."""
    d = synth.block(synth.ITB, 31337 + n, n)
    z = oracle.compress(d)
    rc, back = lzo.lzo1x_decompress(z)
    assert rc == 0 and back == d


def test_host_batch_api(dev, edge, malformed):
    rc, st, comps = lzo.compress_batch(edge["inputs"][:300])
    assert rc == 0 and all(s == 0 for s in st)
    assert comps == edge["comps"][:300]
    rc, st, outs = lzo.decompress_batch(malformed["streams"], malformed["caps"])
    assert rc == 0
    assert st == malformed["rc"]
    assert outs == [o[:c] for o, c in zip(malformed["outs"], malformed["caps"])]


def _adversarial_blocks():
    """Inputs aimed at the throughput encoder's windowing
    (lzo1x_encode_fast.hip): short periods (every lane of a window hashes to
    the same few slots), periods around the 64-lane window, 4-byte patterns
    that collide in the 16384-slot dictionary, long matches (the 32-byte
    first compare and the wave-parallel extension), matches running into the
    block end, sizes around 64 KiB (where the u16 dictionary first re-bases),
    and the 14..17-byte blocks whose first probe lies at or past ip_end."""
    rng = np.random.default_rng(11)
    out = []
    for period in (1, 2, 3, 4, 5, 7, 8, 13, 31, 32, 33, 63, 64, 65, 67, 127, 128, 129, 255):
        unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        out.append((unit * (4096 // period + 1))[:4096])
    # many positions hashing alike: few distinct 4-byte words, shuffled
    words = rng.integers(0, 2**32, 24, dtype=np.uint64).astype(np.uint32)
    out.append(words[rng.integers(0, 24, 8192)].tobytes())
    # random data with long repeats at assorted distances, some to the end
    base = rng.integers(0, 256, 30000, dtype=np.uint8).tobytes()
    mix = bytearray(base)
    for k in range(40):
        a = int(rng.integers(0, len(mix) - 600)); L = int(rng.integers(4, 600))
        b = int(rng.integers(a + 1, len(mix) - L))
        mix[b:b + L] = mix[a:a + L]
    mix += mix[-5000:]
    out.append(bytes(mix))
    for n in (14, 15, 16, 17, 18, 29, 65535, 65536, 65537):
        d = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
        out.append(d)
    out.append(bytes(65536))                          # one long match to the end
    out.append(bytes(70000))                          # the same past 64 KiB
    return out


def _slot_primary(w):
    b0, b1, b2, b3 = w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24
    v = ((((b3 << 6) ^ b2) << 5) ^ b1)
    v = (v << 5) ^ b0
    return ((v * 33) >> 5) & 0x3FFF


def _claim_blocks():
    """Inputs aimed at the encoder's claim table and token writes:
    words whose dictionary slots differ but share a claim-table entry
    ((slot ^ slot >> 9) & 1023: aliases cut windows early, never wrongly);
    windows full of 3-5 byte matches (many tokens per window, token-queue
    back-pressure); and blocks past 64 KiB with repeats at distances
    0xBFFF / 0xC000 across the dictionary re-bases (every 8 KiB)."""
    rng = np.random.default_rng(23)
    words = rng.integers(0, 2**32, 20000, dtype=np.uint64).astype(np.uint32)
    groups = {}
    for w in words.tolist():
        s = _slot_primary(w)
        groups.setdefault((s ^ (s >> 9)) & 1023, {}).setdefault(s, w)
    alias = max(groups.values(), key=len)            # distinct slots, one claim entry
    aw = np.array(list(alias.values()), dtype=np.uint32)
    out = [aw[rng.integers(0, len(aw), 16384)].tobytes()]
    # many short matches: a 5-byte motif with one varying byte
    motif = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
    out.append(b"".join(motif[:3] + bytes([int(x)]) + motif[3:] for x in rng.integers(0, 7, 13000)))
    for n in (90000, 200000):
        d = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        for dist in (0xBFFE, 0xBFFF, 0xC000, 0xC001):
            for at in range(dist + 5, n - 300, 24571):
                L = int(rng.integers(3, 200))
                d[at: at + L] = d[at - dist: at - dist + L]
        out.append(bytes(d))
    return out


def test_encoder_adversarial_vs_oracle(dev, gu, oracle):
    blocks = _adversarial_blocks() + _claim_blocks()
    comps, st = gu.gpu_compress(torch, blocks, dev, shift=3)
    assert all(s == 0 for s in st)
    for i, (b, c) in enumerate(zip(blocks, comps)):
        assert c == oracle.compress(b), (i, len(b))
    outs, st2, _ = gu.gpu_decompress(torch, comps, [len(b) for b in blocks], dev, shift=1)
    assert all(s == 0 for s in st2) and outs == blocks


def _long_literal_prefix_blocks():
    """Streams whose first instruction is a long literal run: n >= 239 takes
    the extension form, n >= 273 its 255-chunk continuation (the first
    instruction of the block then needs the parser's exact slow path from
    state ST_F)."""
    rng = np.random.default_rng(17)
    out = []
    for n in (239, 240, 272, 273, 274, 300, 527, 528, 529, 1100, 1300, 3000, 9000):
        head = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        tail = synth.block(synth.ITB, n, 60000)
        out.append(head + tail)
    return out


def test_fast_path_takes_every_valid_stream(dev, gu):
    """The throughput decoder alone (no fallback to the exact decoder) decodes
    valid streams of every content model and of ITB blocks over the whole C4
    size range bit-exactly -- so parity is the fast path's, not the safety
    net's (a parse error the fast path detects would hand the block over)."""
    blocks = []
    for kib in (4, 12, 64, 100, 128, 160, 192, 256):
        blocks += [synth.block(synth.ITB, 1000 * kib + i, kib * 1024) for i in range(3)]
    for model in range(6):
        blocks += [synth.block(model, 5000 + model * 10 + i, 65536) for i in range(3)]
    blocks += _long_literal_prefix_blocks()
    blocks += [b for b in _adversarial_blocks() if b]
    comps, st = gu.gpu_compress(torch, blocks, dev)
    assert all(s == 0 for s in st)
    outs, st2, fallbacks = gu.gpu_decompress_fast(torch, comps, [len(b) for b in blocks], dev)
    assert all(s == 0 for s in st2)
    bad = [i for i, (o, b) in enumerate(zip(outs, blocks)) if o != b]
    assert not bad, bad[:8]
    assert fallbacks == 0


def test_start_order_is_largest_first(dev):
    """lzo_mi355x_launch_order_by_size (the start order of batches larger than
    one resident round): a permutation of the block indices whose 4 KiB size
    classes never increase, every size above 1 MiB in the first class."""
    lib = lzo.load()
    fn = lib.lzo_mi355x_launch_order_by_size
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(11)
    for n in (1, 1023, 10000):
        keys = rng.integers(0, 3 << 20, n).astype(np.uint32)
        keys[: n // 7] = rng.integers(0, 8192, n // 7)          # (many small ones)
        kd = torch.from_numpy(keys.view(np.int32)).to(dev)
        order = torch.full((n,), -1, dtype=torch.int32, device=dev)
        assert fn(kd.data_ptr(), n, order.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        o = order.cpu().numpy().astype(np.int64)
        assert sorted(o.tolist()) == list(range(n))
        cls = np.minimum(keys[o] >> 12, 255)
        assert (np.diff(cls.astype(np.int64)) <= 0).all()


def test_fast_path_op_sets_are_reused(dev, gu):
    """More blocks than workgroups resident at once: the op-slot sets are
    handed from finished workgroups to new ones (the scratch holds one set per
    resident workgroup, not per block), the blocks start largest first (sizes
    over four 4 KiB classes), every block stays on the fast path, and the
    scratch for config C4's 131,072 blocks stays well under 300 MB."""
    lib = lzo.load()
    resident = int(lib.lzo_mi355x_fast_resident_blocks())
    n = 2 * resident + 123
    blocks = [synth.block(synth.ITB, 70000 + i, 256 + 2048 * (i % 8) + 16 * (i % 64)) for i in range(n)]
    comps, st = gu.gpu_compress(torch, blocks, dev)
    assert all(s == 0 for s in st)
    outs, st2, fallbacks = gu.gpu_decompress_fast(torch, comps, [len(b) for b in blocks], dev)
    assert all(s == 0 for s in st2)
    assert outs == blocks
    assert fallbacks == 0
    assert lzo.decompress_scratch_bytes(131072) < 300e6
    # (+ the fallback list's growth, + the start order once n > resident)
    assert lzo.decompress_scratch_bytes(n) == lzo.decompress_scratch_bytes(resident) + (
        -(-4 * n // 256) - -(-4 * resident // 256)) * 256 + -(-4 * n // 256) * 256


@pytest.mark.parametrize("nsets", [1, 3, 40])
def test_fast_path_op_set_pool_under_contention(dev, gu, nsets):
    """The op-set pool with far fewer sets than blocks (the library sizes it to
    the resident workgroups; here the launcher gets 1, 3 or 40 sets for 600
    blocks): workgroups wait for sets returned by finished ones, in every
    partition, and each block still decodes exactly on the fast path."""
    import ctypes
    lib = lzo.load()
    fn = lib.lzo_mi355x_launch_decompress_fast
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 13 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_void_p]
    lib.lzo_mi355x_fast_ops_bytes_per_block.restype = ctypes.c_size_t
    n = 600
    blocks = [synth.block(synth.ITB, 80000 + i, 4096 + 64 * (i % 97)) for i in range(n)]
    comps, st = gu.gpu_compress(torch, blocks, dev)
    assert all(x == 0 for x in st)
    src = gu.device_batch(torch, comps, dev)
    dst = gu.empty_batch(torch, [len(b) for b in blocks], dev, fill=0x5A)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    ost = torch.full((n,), 99, dtype=torch.int32, device=dev)
    head = torch.zeros(64 + 2048, dtype=torch.int32, device=dev)   # fallback count + pool counters
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    ring = torch.zeros(nsets, dtype=torch.int64, device=dev)
    ops = torch.empty(nsets * lib.lzo_mi355x_fast_ops_bytes_per_block(), dtype=torch.uint8,
                      device=dev)
    p = lambda t: t.data_ptr()
    rc = fn(p(src.arena), p(src.off), p(src.length), p(dst.arena), p(dst.off), p(dst.length),
            p(olen), p(ost), p(head), p(ids), p(head) + 256, p(ring), p(ops), nsets, n, None,
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(head[0].item()) == 0                       # no block left the fast path
    assert ost.cpu().numpy().tolist() == [0] * n
    assert gu.fetch(dst, olen) == blocks


def _mutated_streams(oracle, count=192, seed=23):
    """Valid ITB streams with the damage real storage or wire errors do: a few
    flipped bytes, a truncation, trailing garbage, a zeroed run."""
    rng = np.random.default_rng(seed)
    base = [oracle.compress(synth.block(synth.ITB, 900 + i, 65536)) for i in range(8)]
    out = []
    for i in range(count):
        z = bytearray(base[i % len(base)])
        kind = i % 4
        if kind == 0:
            for _ in range(int(rng.integers(1, 4))):
                z[int(rng.integers(0, len(z)))] ^= int(rng.integers(1, 256))
        elif kind == 1:
            z = z[: int(rng.integers(1, len(z)))]
        elif kind == 2:
            z += rng.integers(0, 256, int(rng.integers(1, 64)), dtype=np.uint8).tobytes()
        else:
            a, k = int(rng.integers(0, len(z) - 16)), int(rng.integers(1, 16))
            z[a: a + k] = bytes(k)
        out.append(bytes(z))
    return out


def test_decompress_mutated_streams_vs_oracle(dev, gu, oracle):
    """Damaged streams through the whole GPU path (fast decoder, refusal,
    exact decoder): LZO_E_* code, produced length and produced bytes equal
    lzo1x_decompress_safe's (the oracle), at capacity n and n/2."""
    streams = _mutated_streams(oracle)
    caps = [65536 if i % 3 else 32768 for i in range(len(streams))]
    outs, st, _ = gu.gpu_decompress(torch, streams, caps, dev)
    bad = []
    for i, (z, c) in enumerate(zip(streams, caps)):
        rc, want = oracle.decompress_safe(z, c)
        if st[i] != rc or outs[i] != want:
            bad.append((i, st[i], rc, len(outs[i]), len(want)))
    assert not bad, bad[:6]


def _large_block(n, seed):
    """ITB-like content with long-distance repeats (the u16 dictionary re-bases
    every 8 KiB past 64 KiB) and an incompressible stretch."""
    rng = np.random.default_rng(seed)
    parts, total = [], 0
    while total < n:
        k = int(rng.integers(0, 3))
        if k == 0:
            b = synth.block(synth.ITB, int(rng.integers(0, 1 << 30)), 65536)
        elif k == 1:
            b = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
        else:
            ref = b"".join(parts)[-200000:] or b"x" * 64
            a = int(rng.integers(0, max(1, len(ref) - 5000)))
            b = ref[a: a + 5000]
        parts.append(b)
        total += len(b)
    return b"".join(parts)[:n]


@pytest.mark.parametrize("n", [(3 << 20) + 5, 16 << 20, (16 << 20) + 1, (32 << 20) + 5])
def test_large_blocks_vs_oracle(dev, gu, oracle, n):
    """Blocks up to the throughput encoder's 16 MiB limit and one byte past it
    (the general encoder), byte-identical to the oracle, and decoded back."""
    blk = _large_block(n, n)
    comps, st = gu.gpu_compress(torch, [blk], dev)
    assert st == [0]
    assert comps[0] == oracle.compress(blk)
    outs, st2, _ = gu.gpu_decompress(torch, comps, [n], dev)
    assert st2 == [0] and outs[0] == blk


def test_host_batch_and_single_call_past_16_mib_vs_oracle(dev, oracle):
    """A block one byte past the throughput encoder's 16 MiB limit through the
    host batch (a chunk of its own, the general encoder's pass launched because
    of it, beside a small block) and through lzo1x_1_compress: byte-identical
    to the oracle."""
    blk = _large_block((16 << 20) + 1, 17)
    small = synth.block(synth.ITB, 18, 65536)
    rc, st, comps = lzo.compress_batch([blk, small])
    assert rc == 0 and st == [0, 0]
    assert comps[0] == oracle.compress(blk) and comps[1] == oracle.compress(small)
    rc, z = lzo.lzo1x_1_compress(blk)
    assert rc == 0 and z == comps[0]


def test_blocks_past_32_mib_vs_oracle(dev, gu, oracle):
    """The general encoder keeps 25-bit dictionary positions relative to a
    base that moves up 16 MiB at a time; blocks of any length stay
    byte-identical to the oracle (the reference handles any length).  The
    block repeats 13 MiB of random bytes three times (every earlier copy is
    past the 0xBFFF match distance, so the reference finds no match there:
    a stale entry must never pass for a live one after a rebase), then has a
    20 MiB zero run (one match moves ip over several rebase steps) and
    ITB-like data."""
    rng = np.random.default_rng(32)
    period = rng.integers(0, 256, (13 << 20) + 7, dtype=np.uint8).tobytes()
    blk = period * 3 + bytes(20 << 20) + synth.block(synth.ITB, 33, 2 << 20)
    assert len(blk) > 60 << 20
    comps, st = gu.gpu_compress(torch, [blk], dev)
    assert st == [0]
    assert comps[0] == oracle.compress(blk)
    outs, st2, _ = gu.gpu_decompress(torch, comps, [len(blk)], dev)
    assert st2 == [0] and outs[0] == blk


def test_decode_full_grammar_streams(dev, gu, oracle):
    """Valid LZO1X streams the LZO1X-1 compressor never writes (M1 after a
    literal run and after trailing literals, long length extensions, M4
    distances above 0x8000, 1-3 byte first runs): bit-exact on the GPU, and
    the throughput decoder takes them all."""
    import lzo_streams
    streams = [lzo_streams.stream(1000 + s, [50, 300, 5000, 40000, 150000][s % 5])
               for s in range(160)]
    comps = [z for z, _ in streams]
    want = [o for _, o in streams]
    outs, st, fallbacks = gu.gpu_decompress_fast(torch, comps, [len(o) for o in want], dev)
    assert st == [0] * len(want)
    assert outs == want
    assert fallbacks == 0
    # the exact decoder on the same streams (capacity one byte short: OUTPUT_OVERRUN)
    outs2, st2, _ = gu.gpu_decompress(torch, comps, [len(o) - 1 for o in want], dev)
    for z, o, s, got in zip(comps, want, st2, outs2):
        rc, ref = oracle.decompress_safe(z, len(o) - 1)
        assert (s, got) == (rc, ref)


def _sweep_blocks(count, seed):
    """Random sizes (0..300 KB) over every content model, with transforms that
    make dense in-window repeats: short periodic stretches, copied runs at
    distances 1..70 (claim conflicts and in-window forwarding), and byte
    noise."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(0, 300000)) if i % 4 else int(rng.integers(0, 2000))
        d = bytearray(synth.block(int(rng.integers(0, 6)), int(rng.integers(0, 1 << 30)), n))
        for _ in range(int(rng.integers(0, 8))):
            if n < 200:
                break
            a = int(rng.integers(0, n - 100))
            L = int(rng.integers(4, min(4000, n - a)))
            k = int(rng.integers(0, 3))
            if k == 0:                                  # periodic stretch
                per = int(rng.integers(1, 70))
                for j in range(a + per, a + L):
                    d[j] = d[j - per]
            elif k == 1:                                # a copied run close behind
                dist = int(rng.integers(1, 71))
                if a >= dist:
                    for j in range(a, a + L):
                        d[j] = d[j - dist]
            else:                                       # noise
                for j in rng.integers(a, a + L, 16):
                    d[int(j)] = int(rng.integers(0, 256))
        out.append(bytes(d))
    return out


def test_encoder_random_sweep_vs_oracle(dev, gu, oracle):
    """600 blocks across every content model and transform, byte-identical to
    the oracle, then decoded back."""
    blocks = _sweep_blocks(600, 77)
    comps, st = gu.gpu_compress(torch, blocks, dev, shift=2)
    assert all(s == 0 for s in st)
    bad = [i for i, (b, c) in enumerate(zip(blocks, comps)) if c != oracle.compress(b)]
    assert not bad, bad[:10]
    outs, st2, _ = gu.gpu_decompress(torch, comps, [len(b) for b in blocks], dev, shift=1)
    assert all(s == 0 for s in st2) and outs == blocks


def test_concurrent_host_threads(dev, oracle):
    """The MDS commit threads, service threads and MDSL GC thread call the
    codec at once: 6 host threads, each with its own HIP stream
    and staging, mixing single calls and batches; every result bit-exact."""
    import threading
    errors = []

    def worker(t):
        try:
            rng = np.random.default_rng(900 + t)
            for it in range(6):
                blocks = [synth.block(int(rng.integers(0, 6)), int(rng.integers(0, 1 << 30)),
                                      int(rng.integers(0, 200000))) for _ in range(int(rng.integers(1, 40)))]
                if it % 2:
                    rc, st, comps = lzo.compress_batch(blocks)
                    assert rc == 0 and all(s == 0 for s in st)
                else:
                    comps = []
                    for b in blocks:
                        rc, z = lzo.lzo1x_1_compress(b)
                        assert rc == 0
                        comps.append(z)
                assert comps == [oracle.compress(b) for b in blocks]
                rc, st, outs = lzo.decompress_batch(comps, [len(b) for b in blocks])
                assert rc == 0 and all(s == 0 for s in st) and list(outs) == blocks
                rc, out = lzo.lzo1x_decompress_safe(comps[0], len(blocks[0]))
                assert (rc, out) == (0, blocks[0])
        except BaseException as e:                 # reported by the main thread
            errors.append((t, repr(e)[:300]))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=110)
    assert not any(th.is_alive() for th in threads)
    assert not errors, errors


def test_host_batch_api_many_mixed_blocks(dev, oracle):
    """The host-resident batch path at scale: 6,000 blocks of mixed sizes
    (0..64 KiB, every content model) through pinned staging, the kernels and
    the pack kernel (only produced bytes come back); a sample checked against
    the oracle byte for byte, every block round-tripped."""
    rng = np.random.default_rng(31)
    sizes = rng.integers(0, 65537, 6000)
    sizes[:50] = 0
    blocks = [synth.block(int(rng.integers(0, 6)), 5000 + i, int(n)) for i, n in enumerate(sizes)]
    rc, st, comps = lzo.compress_batch(blocks)
    assert rc == 0 and all(s == 0 for s in st)
    for i in range(0, len(blocks), 25):
        assert comps[i] == oracle.compress(blocks[i]), i
    rc, st, outs = lzo.decompress_batch(comps, [len(b) for b in blocks])
    assert rc == 0 and all(s == 0 for s in st)
    assert outs == blocks


@pytest.mark.parametrize("kernel", ["gdict_one_wave", "gdict_two_wave", "lds"])
def test_encoder_kernels_vs_oracle(dev, gu, oracle, kernel, monkeypatch):
    """Each throughput encoder kernel (global dictionary with one or two waves
    per block, LDS dictionary) byte-identical to the oracle on the sweep's
    content models, sizes up to 300 KB, more blocks than one grid holds."""
    waves = "enc_waves=2" if kernel == "gdict_two_wave" else "enc_waves=1"
    monkeypatch.setenv("POM_LZO_DEBUG", waves)          # (host_debug.c pom_dbg_str)
    lzo.debug_reload()
    blocks = _sweep_blocks(300, 91)
    src = gu.device_batch(torch, blocks, dev, shift=1)
    dst = gu.empty_batch(torch, [lzo.worst_compress(len(b)) for b in blocks], dev, fill=0xA5)
    olen = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    st = torch.full((len(blocks),), 99, dtype=torch.int32, device=dev)
    if kernel == "lds":
        lzo.compress_dev(src, dst, olen, st, scratch=None)
    else:
        # a grid of 40 workgroups: each dictionary region serves several blocks,
        # taken through the block ticket (scratch sized for the batch, as the
        # ABI requires; its ticket word starts as garbage)
        monkeypatch.setenv("POM_LZO_DEBUG", waves + ",enc_grid=40")
        lzo.debug_reload()
        scr = torch.full((lzo.compress_scratch_bytes(len(blocks)),), 0x5A, dtype=torch.uint8, device=dev)
        lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [0] * len(blocks)
    comps = gu.fetch(dst, olen)
    bad = [i for i, (b, c) in enumerate(zip(blocks, comps)) if c != oracle.compress(b)]
    assert not bad, bad[:10]


def _far_blocks():
    """Blocks larger than the encoder's 64 KiB position window (its u16
    dictionary entries re-base), matches at distances just under and past
    0xBFFF, matches longer than 64 KiB, zero runs, random data and ITB
    records."""
    rng = np.random.default_rng(5)
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    a = rnd(0xBFF0)
    b = rnd(0xC010)
    return [
        _large_block((3 << 20) + 5, 3),
        bytes(1 << 20),
        rnd(1 << 20),
        synth.block(synth.ITB, 7, 536192),
        a + a + a[:5000] + rnd(3000) + a,               # distance 0xBFF0 (inside M4_MAX_OFFSET)
        b + b + rnd(100),                               # distance 0xC010 (past it: literals)
        rnd(70000) + bytes(200000) + rnd(10) + bytes(90000),
        (rnd(37) * 20000)[:700001],
        synth.block(synth.ITB, 8, 65536),
        b"",
        rnd(13),
        rnd(14),
    ]


@pytest.mark.parametrize("which", ["sweep", "far"])
def test_small_batches_on_the_lds_encoder_vs_oracle(dev, gu, oracle, which):
    """Batches without scratch of at most one block per CU (what single calls
    and small host chunks launch: the LDS-dictionary encoder): byte-identical
    to the oracle on the sweep's content models and on blocks with far
    repeats around 0xBFFF, long matches and re-based dictionaries."""
    blocks = _sweep_blocks(200, 93) if which == "sweep" else _far_blocks()
    assert len(blocks) <= torch.cuda.get_device_properties(dev).multi_processor_count
    src = gu.device_batch(torch, blocks, dev, shift=3)
    dst = gu.empty_batch(torch, [lzo.worst_compress(len(b)) for b in blocks], dev, fill=0xA5)
    olen = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    st = torch.full((len(blocks),), 99, dtype=torch.int32, device=dev)
    lzo.compress_dev(src, dst, olen, st, scratch=None)
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [0] * len(blocks)
    comps = gu.fetch(dst, olen)
    bad = [i for i, (b, c) in enumerate(zip(blocks, comps)) if c != oracle.compress(b)]
    assert not bad, bad[:10]


@pytest.mark.gpu
def test_encoder_block_tickets_mixed_sizes(dev, gu):
    """More blocks than the global-dictionary grid, of mixed ITB sizes (C4's
    4-256 KiB): workgroups past their first block draw the next one from the
    ticket counter in the scratch head, whose word starts as garbage, in the
    largest-first start order the launcher sorts into the scratch (the decode
    back likewise, 6000 blocks being more than one resident round).  Every
    block byte-identical to the LDS-dictionary kernel (itself pinned to the
    oracle above), then decoded back."""
    n = 6000                                     # > 4096 resident on a 256-CU MI355X
    sizes = synth.mixed_sizes(n, 77)
    arena, offs, lens = synth.batch(synth.ITB, 0, sizes, align=256, threads=16)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    src = lzo.DeviceBatch(t(arena), t(offs.view(np.int64)), t(lens.view(np.int32)))
    caps = [lzo.worst_compress(int(s)) for s in sizes]
    outs = []
    for scratch in ("tickets", None):
        dst = gu.empty_batch(torch, caps, dev, fill=0xA5)
        olen = torch.zeros(n, dtype=torch.int32, device=dev)
        st = torch.full((n,), 99, dtype=torch.int32, device=dev)
        scr = None
        if scratch:
            scr = torch.full((lzo.compress_scratch_bytes(n),), 0xFF, dtype=torch.uint8, device=dev)
        lzo.compress_dev(src, dst, olen, st, scratch=scr)
        torch.cuda.synchronize()
        assert int((st != 0).sum().item()) == 0
        outs.append((dst, olen))
    (d1, l1), (d2, l2) = outs
    assert torch.equal(l1, l2)
    assert torch.equal(d1.arena, d2.arena)      # (same layout, same 0xA5 fill past each block)
    zsrc = lzo.DeviceBatch(d1.arena, d1.off, l1)
    back = torch.zeros_like(src.arena)
    ob = lzo.DeviceBatch(back, src.off, src.length)
    ol = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.zeros_like(ol)
    scr = torch.zeros(lzo.decompress_scratch_bytes(n), dtype=torch.uint8, device=dev)
    lzo.decompress_dev(zsrc, ob, ol, st, scr)
    torch.cuda.synchronize()
    assert int((st != 0).sum().item()) == 0
    assert torch.equal(back, src.arena)


@pytest.mark.parametrize("kind", ["win"])
def test_window_decoder_every_valid_stream(dev, gu, kind):
    """The windowed decoder (lzo1x_decode_win.hip) alone, without the exact
    decoder behind it: every content model (incompressible blocks with
    literal runs far longer than a 2 KiB piece, all-zero blocks with length
    extensions past a piece), ITB blocks over the C4/C5 size range, the
    adversarial blocks and a 1 MiB block (the 64 KiB LDS ring wraps 16 times)
    decode bit-exactly and none is handed over."""
    blocks = []
    for kib in (4, 12, 64, 100, 256, 524):
        blocks += [synth.block(synth.ITB, 3000 * kib + i, kib * 1024 + 7 * i) for i in range(2)]
    for model in range(6):
        blocks += [synth.block(model, 6000 + model * 10 + i, n)
                   for i, n in enumerate((1, 13, 14, 4096, 65536, 300000))]
    blocks += _long_literal_prefix_blocks()
    blocks += [b for b in _adversarial_blocks() if b]
    blocks.append(synth.block(synth.LZLIKE, 77, 1 << 20))
    comps, st = gu.gpu_compress(torch, blocks, dev)
    assert all(s == 0 for s in st)
    outs, st2, handed = gu.gpu_decompress_win(torch, comps, [len(b) for b in blocks], dev, kind)
    assert handed == []
    assert st2 == [0] * len(blocks)
    bad = [i for i, (o, b) in enumerate(zip(outs, blocks)) if o != b]
    assert not bad, bad[:8]


@pytest.mark.parametrize("kind", ["win"])
def test_window_decoder_full_grammar_streams(dev, gu, kind):
    """LZO1X streams the LZO1X-1 compressor never writes (M1 after literal runs
    and trailing literals, long extensions, first runs of 1-3 bytes) decode
    bit-exactly on the windowed decoder, none handed over."""
    import lzo_streams
    streams = [lzo_streams.stream(2000 + s, [50, 300, 5000, 40000, 150000][s % 5])
               for s in range(80)]
    comps = [z for z, _ in streams]
    want = [o for _, o in streams]
    outs, st, handed = gu.gpu_decompress_win(torch, comps, [len(o) for o in want], dev, kind)
    assert handed == []
    assert st == [0] * len(want)
    assert outs == want


@pytest.mark.parametrize("kind", ["win"])
def test_window_decoder_hands_over_malformed_and_short_room(dev, gu, kind, malformed):
    """Malformed streams, and valid streams whose output does not fit, are
    handed to the exact decoder (status 0x7FFF0001 until it runs) -- never
    reported OK with wrong bytes."""
    comps = list(malformed["streams"][:300])
    caps = list(malformed["caps"][:300])
    want_codes = list(malformed["rc"][:300])
    outs, st, handed = gu.gpu_decompress_win(torch, comps, caps, dev, kind)
    for i, (s, code) in enumerate(zip(st, want_codes)):
        if s == 0:                              # finished: only where the reference says OK
            assert code == 0 and outs[i] == malformed["outs"][i], (i, code)
        else:
            assert s == 0x7FFF0001 and i in handed
    blocks = [synth.block(synth.ITB, 9100 + i, 65536) for i in range(4)]
    comps2, _ = gu.gpu_compress(torch, blocks, dev)
    outs2, st2, handed2 = gu.gpu_decompress_win(torch, comps2, [65535] * 4, dev, kind)
    assert handed2 == [0, 1, 2, 3] and st2 == [0x7FFF0001] * 4


@pytest.mark.parametrize("group", [1, 8])
def test_latency_decoder_valid_streams(dev, gu, group):
    """The latency decoder (lzo1x_decode_lat.hip) alone, one block per
    pipeline and eight side by side: every content model, ITB blocks up to the 536,192-byte maximum, a
    1 MiB block and the full-grammar streams (M1 after runs and trailing
    literals, long extensions, first runs of 1-3 bytes) decode bit-exactly;
    only streams with 64+ zero length-extension bytes are handed over."""
    import lzo_streams
    blocks = [synth.block(synth.ITB, 7100 + i, n)
              for i, n in enumerate((4096, 65536, 100000, 262144, 536192))]
    for model in range(6):
        blocks += [synth.block(model, 7200 + model * 10 + i, n) for i, n in enumerate((1, 14, 65536, 300000))]
    blocks.append(synth.block(synth.LZLIKE, 78, 1 << 20))
    comps, st = gu.gpu_compress(torch, blocks, dev)
    assert all(s == 0 for s in st)
    streams = [lzo_streams.stream(2100 + s, [50, 300, 5000, 40000, 150000][s % 5]) for s in range(20)]
    comps += [z for z, _ in streams]
    want = blocks + [o for _, o in streams]
    outs, st2, handed = gu.gpu_decompress_lat(torch, comps, [len(w) for w in want], dev, group)
    # a node gives up after 64 zero length-extension bytes (runs of ~16 KB and
    # more: the random and zero blocks of 64 KiB and up), so that a zero run
    # costs linear time; those blocks go to the exact decoder, and no others
    long_ext = {i for i, z in enumerate(comps) if bytes(64) in z}
    assert set(handed) <= long_ext, sorted(set(handed) - long_ext)
    assert len(handed) <= 6
    keep = [i for i in range(len(want)) if i not in set(handed)]
    assert [st2[i] for i in keep] == [0] * len(keep)
    bad = [i for i in keep if outs[i] != want[i]]
    assert not bad, bad[:8]


@pytest.mark.parametrize("group", [1, 8])
def test_latency_decoder_hands_over_malformed_and_short_room(dev, gu, malformed, group):
    """Malformed streams, and valid streams whose output does not fit, are
    handed to the exact decoder (status 0x7FFF0001) -- never reported OK with
    wrong bytes."""
    comps = list(malformed["streams"][:200])
    caps = list(malformed["caps"][:200])
    want_codes = list(malformed["rc"][:200])
    outs, st, handed = gu.gpu_decompress_lat(torch, comps, caps, dev, group)
    for i, (s, code) in enumerate(zip(st, want_codes)):
        if s is None:                            # outside the decoder's range: not launched
            continue
        if s == 0:
            assert code == 0 and outs[i] == malformed["outs"][i], (i, code)
        else:
            assert s == 0x7FFF0001 and i in handed
    blocks = [synth.block(synth.ITB, 9200 + i, 65536) for i in range(3)]
    comps2, _ = gu.gpu_compress(torch, blocks, dev)
    outs2, st2, handed2 = gu.gpu_decompress_lat(torch, comps2, [65535] * 3, dev, group)
    assert handed2 == [0, 1, 2] and st2 == [0x7FFF0001] * 3


def test_lone_single_calls_on_the_latency_decoder(dev, oracle):
    """Lone lzo1x_decompress / lzo1x_decompress_safe calls of 2 KB or more of
    compressed input take the latency decoder (host_ctx.c pom_lat_decode): exact
    bytes and lengths from 8 KB to 536,192 B, OUTPUT_OVERRUN for a room one
    byte short and for no room at all, and a malformed stream's code from the
    exact decoder behind it, as the reference (lib/minilzo.c:3703-4190)."""
    for i, n in enumerate((8192, 65536, 200000, 536192)):
        d = synth.block(synth.ITB if i % 2 else synth.TEXT, 5151 + i, n)
        z = oracle.compress(d)
        assert len(z) >= 2048
        rc, back = lzo.lzo1x_decompress(z)
        assert rc == 0 and back == d
        rc, back = lzo.lzo1x_decompress_safe(z, n)
        assert rc == 0 and back == d
        rc, _ = lzo.lzo1x_decompress_safe(z, n - 1)
        assert rc == lzo.LZO_E_OUTPUT_OVERRUN
        rc, _ = lzo.lzo1x_decompress_safe(z, 0)
        assert rc == lzo.LZO_E_OUTPUT_OVERRUN
        cut = z[: len(z) // 2]
        rc, _ = lzo.lzo1x_decompress_safe(cut, n)
        assert rc == oracle.decompress_safe(cut, n)[0]


def test_latency_decoder_zero_runs_stay_linear(dev, oracle):
    """Zero-run input through the single-call path (the latency decoder from
    2 KB of compressed input): 2 MB of zero bytes as a stream, a valid stream
    of 8 MiB of zeros (a length extension of ~33 K zero bytes) and one with a
    4 MiB zero run between two ITB blocks.  Codes, lengths and bytes equal the
    reference's; each call takes well under a second (every node of a zero
    run used to scan the rest of the run: O(z^2))."""
    import time
    cases = [(bytes(2 << 20), 1 << 20)]
    for d in (bytes(8 << 20), synth.block(synth.ITB, 71, 65536) + bytes(4 << 20) + synth.block(synth.ITB, 72, 65536)):
        cases.append((oracle.compress(d), len(d)))
    lzo.lzo1x_decompress_safe(cases[1][0], cases[1][1])     # (warm: staging, code objects)
    # the same call on an ITB stream of the largest output size, no zero run:
    # the scale the zero-run cases are held to (a shared box's host and GPU
    # load move both alike; an O(z^2) scan takes seconds)
    itb8 = synth.block(synth.ITB, 73, 8 << 20)
    zi = oracle.compress(itb8)
    lzo.lzo1x_decompress_safe(zi, len(itb8))
    t0 = time.perf_counter()
    rc, out = lzo.lzo1x_decompress_safe(zi, len(itb8))
    base = time.perf_counter() - t0
    assert rc == 0 and out == itb8
    print(f"ITB 8 MiB reference call: {base * 1e3:.1f} ms")
    for z, cap in cases:
        t0 = time.perf_counter()
        rc, out = lzo.lzo1x_decompress_safe(z, cap)
        dt = time.perf_counter() - t0
        print(f"zero-run case: {len(z)} B in, rc={rc}, {dt * 1e3:.1f} ms")
        want = oracle.decompress_safe(z, cap)
        assert (rc, out) == want
        assert dt < max(1.0, 10 * base), (dt, base)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_small_host_batches_on_the_latency_decoder(dev, oracle, malformed, k):
    """Host batches of up to 8 blocks of 2 KB or more of compressed input
    decode on one latency-decoder pipeline (host_ctx.c pom_lat_decode) with the
    exact decoder behind it: exact bytes, a block one byte short of room
    (OUTPUT_OVERRUN) and a malformed stream's reference code in the same
    batch."""
    blocks = [synth.block(synth.ITB if i % 2 else synth.TEXT, 6161 + i, 20000 + 9000 * i) for i in range(k)]
    comps = [oracle.compress(b) for b in blocks]
    assert all(len(z) >= 2048 for z in comps)
    caps = [len(b) for b in blocks]
    want = [(0, b) for b in blocks]
    if k > 1:
        caps[0] -= 1
        want[0] = oracle.decompress_safe(comps[0], caps[0])
    if k > 2:
        j = next(i for i, z in enumerate(malformed["streams"]) if len(z) >= 2048 and malformed["rc"][i] != 0)
        comps[1], caps[1] = malformed["streams"][j], int(malformed["caps"][j])
        want[1] = oracle.decompress_safe(comps[1], caps[1])
    rc, status, outs = lzo.decompress_batch(comps, caps)
    assert rc == 0
    for i, (s, o) in enumerate(zip(status, outs)):
        assert s == want[i][0], (i, s, want[i][0])
        if s == 0:
            assert o == want[i][1], i


def test_latency_scratch_is_shared_across_threads(dev, oracle):
    """16 threads issuing 8-block host batches (each one latency-decoder
    pipeline, host_ctx.c pom_lat_decode) share ONE latency scratch per device
    (lat_acquire): the device memory they leave allocated stays near one
    scratch plus the threads' staging, where per-thread scratches (round 3)
    would hold 16 of them.  Every batch still decodes exactly."""
    from concurrent.futures import ThreadPoolExecutor
    blocks = [synth.block(synth.ITB, 8181 + i, 262144) for i in range(8)]
    comps = [oracle.compress(b) for b in blocks]
    caps = [len(b) for b in blocks]
    lib = lzo.load()
    lib.lzo_mi355x_decompress_lat_scratch_n.restype = ctypes.c_size_t
    lib.lzo_mi355x_decompress_lat_scratch_n.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint32]
    so = np.zeros(8, np.uint64)
    so[1:] = np.cumsum([(len(z) + 255) // 256 * 256 for z in comps[:-1]])
    zl = np.array([len(z) for z in comps], np.uint32)
    cp = np.array(caps, np.uint32)
    need = lib.lzo_mi355x_decompress_lat_scratch_n(so.ctypes.data, zl.ctypes.data, cp.ctypes.data, 8)
    assert need > 32 << 20                       # (a scratch worth sharing)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()

    def work(i):
        for _ in range(2):
            rc, st, outs = lzo.decompress_batch(comps, caps)
            if rc != 0 or st != [0] * 8 or outs != blocks:
                return False
        return True

    with ThreadPoolExecutor(16) as ex:
        ok = list(ex.map(work, range(16)))
    assert all(ok)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    held = free0 - free1
    staging = 16 * 4 * (int(zl.sum()) + int(cp.sum()) + (1 << 20))   # each thread's chunk staging, generously
    assert held <= 2 * need + staging, (held, need, staging)
    assert held < 16 * need, (held, need)


# ---------------------------------------------------------------------------
# The single calls' and the host batches' paths under the debug keys that
# select them (host_single.c, host_ctx.c pom_lat_decode)
# ---------------------------------------------------------------------------
@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


@pytest.fixture(scope="module")
def single_fx(oracle):
    """ITB blocks of 1, 100, 4,096 and 65,536 bytes with their oracle streams
    (only the last is 2 KiB or more: the latency decoder's), and 300,000 zero
    bytes, whose ~1.2 KB stream decodes past lzo1x_decompress's first guess of
    256 KiB."""
    blocks = [synth.block(synth.ITB, 7300 + i, n) for i, n in enumerate((1, 100, 4096, 65536))]
    comps = [oracle.compress(b) for b in blocks]
    assert [len(z) >= 2048 for z in comps] == [False, False, False, True]
    zeros = bytes(300000)
    zz = oracle.compress(zeros)
    assert len(zz) < 2048 and 16 * len(zz) < (256 << 10) < len(zeros)
    return blocks, comps, zeros, zz


def _decoded_length(z):
    lib = lzo.load()
    need = ctypes.c_ulong(0)
    rc = lib.lzo_mi355x_decoded_length(ctypes.c_char_p(z), len(z), ctypes.byref(need))
    return rc, need.value


@pytest.mark.parametrize("debug", ["", "sc_combine=0", "sc_lat=0", "sc_lat_min=1"])
def test_single_calls_under_debug_settings(dev, debug_env, single_fx, debug):
    """Every minilzo.h single call through the combining queue and without it
    (sc_combine=0), with the latency decoder at its default threshold, off
    (sc_lat=0: the windowed decoder alone) and on for every block
    (sc_lat_min=1): compress equals the oracle; both decoders return the
    block; a room one byte short is LZO_E_OUTPUT_OVERRUN;
    lzo_mi355x_decoded_length returns the block's length; and 300,000 zero
    bytes take the pre-scan and the second round trip and come back exact."""
    blocks, comps, zeros, zz = single_fx
    debug_env(debug)
    for d, z in zip(blocks, comps):
        rc, got = lzo.lzo1x_1_compress(d)
        assert rc == 0 and got == z, len(d)
        rc, back = lzo.lzo1x_decompress(z)
        assert rc == 0 and back == d, len(d)
        rc, back = lzo.lzo1x_decompress_safe(z, len(d))
        assert rc == 0 and back == d, len(d)
        rc, _ = lzo.lzo1x_decompress_safe(z, len(d) - 1)
        assert rc == lzo.LZO_E_OUTPUT_OVERRUN, len(d)
        assert _decoded_length(z) == (0, len(d))
    rc, back = lzo.lzo1x_decompress(zz)
    assert rc == 0 and back == zeros


@pytest.fixture(scope="module")
def lat_limit_fx(oracle):
    """Nine ITB/TEXT blocks whose streams are 2 KiB or more, and one whose
    stream is shorter, with what the oracle decodes them to."""
    blocks = [synth.block(synth.ITB if i % 2 else synth.TEXT, 7400 + i, 24000 + 1000 * i) for i in range(9)]
    small = synth.block(synth.ITB, 7410, 1000)
    comps = [oracle.compress(b) for b in blocks]
    zsmall = oracle.compress(small)
    assert all(len(z) >= 2048 for z in comps) and len(zsmall) < 2048
    return blocks, comps, small, zsmall


@pytest.mark.parametrize("case", ["eight", "nine", "eight_one_short_stream"])
def test_host_batches_around_the_latency_limit(dev, oracle, lat_limit_fx, case):
    """Decode batches at the edge of the latency decoder's range (at most 8
    blocks, each of 2,048 or more compressed bytes): 8 eligible streams (the
    latency pipeline), 9 (the throughput decoders), and 8 of which one is
    under 2,048 compressed bytes (the throughput decoders).  Each gives the
    oracle's codes and bytes."""
    blocks, comps, small, zsmall = lat_limit_fx
    if case == "eight":
        zs, ds = comps[:8], blocks[:8]
    elif case == "nine":
        zs, ds = comps, blocks
    else:
        zs, ds = comps[:5] + [zsmall] + comps[5:7], blocks[:5] + [small] + blocks[5:7]
    caps = [len(d) for d in ds]
    want = [oracle.decompress_safe(z, c) for z, c in zip(zs, caps)]
    assert want == [(0, d) for d in ds]
    rc, status, outs = lzo.decompress_batch(zs, caps)
    assert rc == 0
    assert status == [w[0] for w in want]
    assert outs == [w[1] for w in want]
