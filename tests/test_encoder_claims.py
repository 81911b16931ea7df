"""The encoder's window protocol (one claim post per window from every active
lane, fixed per-lane flags, forwarding rounds in registers) on the smallest
inputs where it can go wrong, through the three throughput encoder kernels,
byte for byte against the oracle.

claim_blocks() builds the inputs; scripts/dbg/enc_claims_sim.c runs the same
protocol on the CPU (write them with dump_framed() for its --framed mode)."""
from __future__ import annotations

import numpy as np
import pytest

from pomegranate_amd import lzo

pytestmark = pytest.mark.gpu

POM_ENC_FWD = 8          # lzo1x_encode_fast.hip: forwardings per window
M2_MAX_OFFSET = 0x800


def _h1(w: np.ndarray) -> np.ndarray:
    """Primary dictionary slot of 4-byte words (rows of a uint8 array), DX3 /
    D_INDEX1 of lib/minilzo.c as lzo1x_emit.h slot_primary computes it."""
    b = w.astype(np.uint32)
    v = ((((b[:, 3] << 6) ^ b[:, 2]) << 5) ^ b[:, 1])
    v = ((v << 5) ^ b[:, 0]) & 0xFFFFFFFF
    return (((v * 33) & 0xFFFFFFFF) >> 5) & 0x3FFF


def _colliders(rng, word: bytes, count: int, same_b3: bool | None = None) -> list:
    """`count` distinct 4-byte words with the primary slot of `word`, their
    first three bytes unlike `word`'s and each other's; same_b3 asks for an
    equal (True) or different (False) fourth byte."""
    target = int(_h1(np.frombuffer(word, np.uint8)[None, :])[0])
    out, seen = [], {word[:3]}
    while len(out) < count:
        cand = rng.integers(0, 256, (1 << 17, 4), dtype=np.uint8)
        for w in cand[_h1(cand) == target]:
            wb = w.tobytes()
            if wb[:3] in seen or (same_b3 is not None and (wb[3] == word[3]) != same_b3):
                continue
            seen.add(wb[:3])
            out.append(wb)
            if len(out) == count:
                break
    return out


def _periodic(rng):
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    prefixes = [0, 9, 17, 30, 41, 52, 60, 63, 64, 70]
    lengths = [40, 64, 65, 130, 257, 600]
    blocks = []
    for k, period in enumerate([1, 2, 3, 4, 5, 7, 8, 13, 16, 31, 32, 33, 63, 64, 65]):
        pat = rnd(period)
        for i, pre in enumerate(prefixes):
            ln = lengths[(i + k) % len(lengths)]
            blocks.append(rnd(pre) + (pat * (ln // period + 1))[:ln] + rnd(16))
    return blocks


def _false_alarms(rng):
    """S matches its earlier copy, so its interior lanes are covered -- they
    still post.  Inside the same 64 positions a literal position has the bytes
    of an interior word of S (its slot holds a collider's position, so the
    three-byte compare fails), or simply is that word again (a short match).
    Several per block, the random filler moving them across the lanes."""
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    blocks = []
    for b in range(40):
        parts = [rnd(int(rng.integers(0, 64)))]
        for u in range(6):
            s = rnd(int(rng.integers(8, 17)))
            i = int(rng.integers(1, len(s) - 4))
            inner = s[i:i + 4]
            if (b + u) % 2:
                # the slot of `inner` ends up holding a collider: a literal
                parts += [s, rnd(3), _colliders(rng, inner, 1)[0], rnd(int(rng.integers(5, 40)))]
            else:
                parts += [s, rnd(int(rng.integers(5, 40)))]
            parts += [s, rnd(int(rng.integers(1, 6))), inner, rnd(int(rng.integers(10, 50)))]
        blocks.append(b"".join(parts))
    return blocks


def _secondary(rng):
    """A and B share the primary slot, fourth bytes differing.  A lies more
    than M2_MAX_OFFSET back, so B fails the primary test and goes to the
    secondary slot; B twice in a window conflicts through h2.  With A again
    in between, the second B's primary slot is written below it: decided
    again, it moves from h2 to h1, which it did not post, and a third B
    reads that slot above it."""
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    blocks = []
    for b in range(48):
        a = rnd(4)
        bw = _colliders(rng, a, 1, same_b3=False)[0]
        far = rnd(M2_MAX_OFFSET + 8 + int(rng.integers(0, 64)))
        g = lambda: rnd(int(rng.integers(1, 9)))
        kind = b % 4
        if kind == 0:
            tail = [bw, g(), bw]
        elif kind == 1:
            tail = [bw, g(), a, g(), bw, g(), bw]
        elif kind == 2:
            tail = [a, g(), bw, g(), bw, g(), a]
        else:
            tail = [bw, g(), bw, g(), a, g(), bw, g(), a, g(), bw]
        blocks.append(rnd(4 + b) + a + far + b"".join(tail) + rnd(20))
    return blocks


def _cap(rng):
    """More than POM_ENC_FWD true conflicts in one window that do not become
    matches (distinct words of one primary slot, back to back: each reads the
    slot the one before writes), and more than POM_ENC_FWD false alarms in one
    window (colliders of the interior words of a matched string).  Every
    prefix length 0..69, so some window holds the whole group."""
    rnd = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    blocks = []
    seed = rnd(4)
    chain = [seed] + _colliders(rng, seed, POM_ENC_FWD + 4)
    s = rnd(14)
    lits = [_colliders(rng, s[i:i + 4], 1)[0] for i in range(1, 11)]
    for pre in range(70):
        blocks.append(rnd(pre) + b"".join(chain) + rnd(30))
        blocks.append(rnd(pre) + s + rnd(40 + pre) + s + b"".join(lits) + rnd(30))
    return blocks


def _ends(rng):
    return [rng.integers(97, 101, n, dtype=np.uint8).tobytes() for n in range(14, 301)]


def claim_blocks():
    rng = np.random.default_rng(20261019)
    out = []
    for name, fn in (("periodic", _periodic), ("false_alarm", _false_alarms), ("secondary", _secondary),
                     ("cap", _cap), ("ends", _ends)):
        out += [(f"{name}[{i}]", b) for i, b in enumerate(fn(rng))]
    assert max(len(b) for _, b in out) <= 4096
    return out


def dump_framed(path):
    """The inputs as [u32 length][bytes], for scripts/dbg/enc_claims_sim.c --framed."""
    with open(path, "wb") as f:
        for _, b in claim_blocks():
            f.write(np.uint32(len(b)).tobytes() + b)


torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(scope="module")
def cases(oracle):
    named = claim_blocks()
    return [n for n, _ in named], [b for _, b in named], [oracle.compress(b) for _, b in named]


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


@pytest.mark.parametrize("kernel", ["gdict_one_wave", "gdict_two_wave", "lds"])
def test_claim_protocol_vs_oracle(dev, oracle, cases, debug_env, kernel):
    import gpu_util as gu
    names, blocks, want = cases
    debug_env("enc_waves=2" if kernel == "gdict_two_wave" else "enc_waves=1")
    src = gu.device_batch(torch, blocks, dev)
    dst = gu.empty_batch(torch, [lzo.worst_compress(len(b)) for b in blocks], dev, fill=0xA5)
    olen = torch.zeros(len(blocks), dtype=torch.int32, device=dev)
    st = torch.full((len(blocks),), 99, dtype=torch.int32, device=dev)
    scr = None
    if kernel != "lds":                                  # (a dirty scratch: dictionaries of garbage)
        scr = torch.full((lzo.compress_scratch_bytes(len(blocks)),), 0x5A, dtype=torch.uint8, device=dev)
    lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == [0] * len(blocks)
    comps = gu.fetch(dst, olen)
    bad = [n for n, c, w in zip(names, comps, want) if c != w]
    assert not bad, f"{len(bad)} of {len(blocks)} differ from the oracle, first {bad[:8]}"
