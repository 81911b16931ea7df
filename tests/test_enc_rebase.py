"""CPU: when the throughput encoder re-bases its u16 dictionary, and to where
(pomegranate_amd/csrc/lzo1x_enc_rebase.h compiled as plain C++,
tests/native/enc_rebase_host.cc), driven as parse_wave drives it: a window
start stepping through blocks of every size up to 65,600 bytes and a sample up
to 600,000.  And the directed inputs of tests/test_gpu_enc_rebase.py
(rebase_blocks()), each checked with the oracle to hit the edge it is for."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from pomegranate_amd import synth

sys.path.insert(0, os.path.join(ROOT, "scripts", "dbg"))
import lzo_ops  # noqa: E402  (the op list of an LZO1X stream)

NATIVE = os.path.join(ROOT, "tests", "native")
LIB = os.path.join(NATIVE, "libenc_rebase_host.so")
CHECK = os.path.join(NATIVE, "enc_rebase_check")
VMAX = 0xFFFF
M4_MAX_OFFSET = 0xBFFF
N_FREE = 65548                 # the longest block that never re-bases: n - 13 <= 0xFFFF
FIXED, RANDOM, CYCLE = 0, 1, 2  # step modes of enc_rebase_sweep_host


class Sweep(ctypes.Structure):
    _fields_ = [("windows", ctypes.c_uint64), ("rebases", ctypes.c_uint64), ("bad_fit", ctypes.c_uint64),
                ("bad_target", ctypes.c_uint64), ("n_first_rebased", ctypes.c_uint32),
                ("min_gap", ctypes.c_uint32), ("last_window_top", ctypes.c_uint32),
                ("last_rebases", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def harness():
    if not (os.path.exists(LIB) and os.path.exists(CHECK)):
        subprocess.run(["make", "-C", NATIVE, "-f", "enc_rebase.mk"], check=True)
    lib = ctypes.CDLL(LIB)
    u32 = ctypes.c_uint32
    lib.enc_rebase_top_host.restype = u32
    lib.enc_rebase_top_host.argtypes = [u32, u32]
    lib.enc_rebase_due_host.restype = ctypes.c_int
    lib.enc_rebase_due_host.argtypes = [u32, u32, u32]
    lib.enc_rebase_target_host.restype = u32
    lib.enc_rebase_target_host.argtypes = [u32]
    lib.enc_rebase_pair_host.restype = u32
    lib.enc_rebase_pair_host.argtypes = [u32, u32]
    lib.enc_rebase_sweep_host.restype = None
    lib.enc_rebase_sweep_host.argtypes = [u32] * 7 + [ctypes.POINTER(Sweep)]
    return lib


def sweep(lib, n_lo, n_hi, n_step, mode, param, jump_at=0, jump_len=0) -> Sweep:
    r = Sweep()
    lib.enc_rebase_sweep_host(n_lo, n_hi, n_step, mode, param, jump_at, jump_len, ctypes.byref(r))
    return r


def test_decision_at_the_edge(harness):
    """The window's highest storable position is min(ip + 63, ip_end - 1); a
    re-base is due exactly when its value, position - base + 1, passes 0xFFFF."""
    lib = harness
    assert lib.enc_rebase_top_host(4, 1000) == 67
    assert lib.enc_rebase_top_host(990, 1000) == 999
    assert lib.enc_rebase_top_host(999, 1000) == 999                 # lane 0 alone
    for ip_end in (65535, 65536, 70000):
        for ip in range(65400, min(ip_end, 65600)):
            for base in (0, 1, 63, 64):
                top = min(ip + 63, ip_end - 1)
                assert bool(lib.enc_rebase_due_host(ip, ip_end, base)) == (top - base + 1 > VMAX), (ip, ip_end, base)
    assert not lib.enc_rebase_due_host(65471, 65535, 0)              # n = 65,548: its last position is 65,534
    assert lib.enc_rebase_due_host(65472, 65536, 0)                  # n = 65,549: 65,535 + 1 does not fit
    assert not lib.enc_rebase_due_host(65471, 65536, 0)
    assert lib.enc_rebase_target_host(65472) == 65472 - 0xC000
    assert lib.enc_rebase_pair_host(0x0005_0003, 3) == 0x0002_0000
    assert lib.enc_rebase_pair_host(0xFFFF_0001, 0x1_0000) == 0


@pytest.mark.parametrize("mode,param", [(CYCLE, 0), (RANDOM, 1), (FIXED, 64), (FIXED, 63), (FIXED, 37)])
def test_every_size_to_65600(harness, mode, param):
    """Every n in 14..65,600: (1) no storable position of any window passes
    0xFFFF after the decision, (2) nb <= ip - 0xC000 and nb >= base, (3) no
    re-base at all up to n = 65,548."""
    r = sweep(harness, 14, 65600, 1, mode, param)
    assert r.windows > 65600 and r.bad_fit == 0 and r.bad_target == 0
    assert r.n_first_rebased == 0 or r.n_first_rebased > N_FREE
    free = sweep(harness, 14, N_FREE, 1, mode, param)
    assert free.rebases == 0 and free.bad_fit == 0


@pytest.mark.parametrize("step", [1, 2, 3, 5, 8, 13, 21, 34, 55, 64])
def test_small_steps_at_the_boundary(harness, step):
    """Fixed steps of 1..64 on the sizes around the first re-base: none up to
    65,548; at 65,549 a walk whose last window reaches ip_end - 1 = 65,535
    re-bases (that position's value would be 0x10000)."""
    lib = harness
    for n in (65535, 65536, 65547, N_FREE):
        r = sweep(lib, n, n, 1, FIXED, step)
        assert (r.rebases, r.bad_fit, r.bad_target) == (0, 0, 0), n
    for n in (65549, 65550, 65600):
        r = sweep(lib, n, n, 1, FIXED, step)
        assert r.bad_fit == 0 and r.bad_target == 0
        assert r.last_window_top <= n - 14
        if r.last_window_top == n - 14:                              # the walk reached ip_end - 1
            assert r.last_rebases >= 1, n
    r = sweep(lib, 65549, 65549, 1, FIXED, 1)                        # step 1 reaches every position
    assert r.last_window_top == 65535 and r.last_rebases == 1


def test_sample_to_600000(harness):
    """Long blocks, every step mode, and one long jump (a match running far
    past its window) of several lengths: the values fit, the targets hold, and
    two re-bases of a block are at least 0xFFFF - 0xC000 - 63 bytes apart."""
    lib = harness
    sizes = [(65601, 600000, 7919), (81920, 81920, 1), (131072, 131072, 1), (200000, 200000, 1),
             (262144, 262144, 1), (600000, 600000, 1)]
    for n_lo, n_hi, n_step in sizes:
        for mode, param in ((CYCLE, 0), (RANDOM, 2), (FIXED, 64), (FIXED, 1 if n_lo == n_hi else 29)):
            r = sweep(lib, n_lo, n_hi, n_step, mode, param)
            assert r.bad_fit == 0 and r.bad_target == 0, (n_lo, mode, param)
            assert r.last_rebases >= 1 and r.n_first_rebased == n_lo
            assert r.min_gap >= VMAX - 0xC000 - 63, (n_lo, mode, param, r.min_gap)
    for jump_at in (4, 30000, 65400, 70000, 150000):
        for jump_len in (65, 300, 0xBFFF, 0xC000, 0xFFFF, 0x10000, 0x10001, 200000, 400000):
            r = sweep(lib, 65601, 600000, 41077, RANDOM, 3, jump_at, jump_len)
            assert r.bad_fit == 0 and r.bad_target == 0, (jump_at, jump_len)
    r = sweep(lib, 600000, 600000, 1, FIXED, 64)                     # 534,452 bytes past the first, 16,320+ apart
    assert 25 <= r.last_rebases <= 33


def test_standalone_checker(harness):
    """The model dictionary under AddressSanitizer and UBSan where they link
    (tests/native/enc_rebase.mk): a stand-alone program."""
    out = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "enc_rebase_check: ok" in out.stdout


# ---------------------------------------------------------------------------
# Directed inputs (tests/test_gpu_enc_rebase.py runs them through the three
# encoder kernels).  Each builder returns (name, block, checks); a check is
# ("match", start, length, distance): the oracle's stream holds a match of
# that distance starting in [start, start + length); or ("literals", start,
# length): every byte of that range is coded as a literal.
# ---------------------------------------------------------------------------
BOUNDARY_SIZES = [65535, 65536, 65547, 65548, 65549, 65550, 65600]
LONG_SIZES = [81920, 131072, 200000]
DISTANCES = [0xBFFE, 0xBFFF, 0xC000, 0xC001, 60000]


def _rnd(rng, k):
    return rng.integers(0, 256, k, dtype=np.uint8)


def _itb(seed, n):
    return np.frombuffer(synth.block(synth.ITB, seed, n), dtype=np.uint8).copy()


def _boundary(rng):
    out = []
    for i, n in enumerate(BOUNDARY_SIZES):
        out.append((f"itb[{n}]", _itb(100 + i, n), []))
        # the last 256 bytes random: every tail position is on the path, and
        # the dictionary puts reach ip_end - 1
        b = _itb(200 + i, n)
        b[n - 256:] = _rnd(rng, 256)
        out.append((f"itb_random_tail[{n}]", b, [("literals", n - 250, 236)]))
        # in the last 200 bytes, a 64-byte chunk first seen exactly 0xC000 back
        # (one byte too far: literals), then one first seen exactly 0xBFFF
        # back (the longest distance there is).  Random bytes up to the first
        # occurrences (some 16 K live entries), then a period of 251 bytes --
        # one long match, so the chunks' entries are still there at the tail
        b = _rnd(rng, n)
        far, near = n - 200, n - 132
        fill = near - M4_MAX_OFFSET + 64
        b[fill: far] = np.resize(_rnd(rng, 251), far - fill)
        b[far: far + 64] = b[far - 0xC000: far - 0xC000 + 64]
        b[near: near + 64] = b[near - M4_MAX_OFFSET: near - M4_MAX_OFFSET + 64]
        out.append((f"edge_tail[{n}]", b, [("literals", far, 60), ("match", near, 60, M4_MAX_OFFSET)]))
    return out


def _reinserted(rng, base, name):
    """1 KiB random chunks, each copied once, DISTANCES[i] further on: the
    copies lie in different stretches of the block, so the first occurrences'
    entries cross zero, one or more re-bases before they are probed."""
    n = len(base)
    b = base.copy()
    stride = (n - DISTANCES[-1] - 1024 - 1000) // len(DISTANCES)
    assert stride >= 1024 + 8
    checks = []
    for i, d in enumerate(DISTANCES):
        a = 1000 + i * stride
        b[a: a + 1024] = _rnd(rng, 1024)
    for i, d in enumerate(DISTANCES):
        a = 1000 + i * stride
        assert a + d + 1024 <= n - 14
        b[a + d: a + d + 1024] = b[a: a + 1024]
        checks.append(("match", a + d, 1020, d) if d <= M4_MAX_OFFSET else ("literals", a + d, 1020))
    return (name, b, checks)


def _long(rng):
    out = []
    for i, n in enumerate(LONG_SIZES):
        out.append(_reinserted(rng, _itb(300 + i, n), f"reinserted_itb[{n}]"))
        out.append(_reinserted(rng, _rnd(rng, n), f"reinserted_random[{n}]"))
    for model, name in ((synth.LZLIKE, "lzlike"), (synth.TEXT, "text"), (synth.ITB, "itb")):
        out.append((f"{name}[200000]", np.frombuffer(synth.block(model, 400, 200000), dtype=np.uint8).copy(), []))
    out.append(("itb[262144]", _itb(401, 262144), []))
    out.append(("itb[536576]", _itb(402, 536576), []))
    return out


def _stale(rng):
    """The first 16 KiB random (16 K dictionary entries that no later probe
    can use once it is 0xBFFF behind), then compressible bytes; past 80 KiB,
    4-byte words of the random head again: their slots hold stale or cleared
    entries, and they must be coded as the oracle codes them -- as literals,
    unless the compressible part happens to offer the word closer by."""
    out = []
    for model, name in ((synth.ITB, "itb"), (synth.TEXT, "text")):
        n = 200000
        b = np.frombuffer(synth.block(model, 500, n), dtype=np.uint8).copy()
        head = _rnd(rng, 16384)
        b[:16384] = head
        at = 81920
        while at < n - 64:
            w = int(rng.integers(0, 16384 - 4))
            b[at: at + 4] = head[w: w + 4]
            at += int(rng.integers(40, 400))
        out.append((f"stale_head_{name}[{n}]", b, []))
    return out


def rebase_blocks():
    rng = np.random.default_rng(20261020)
    out = []
    for fn in (_boundary, _long, _stale):
        out += [(name, b.tobytes(), checks) for name, b, checks in fn(rng)]
    return out


@pytest.fixture(scope="module")
def directed():
    return rebase_blocks()


def test_directed_inputs_hit_their_edges(oracle, directed):
    assert 30 <= len(directed) <= 45
    names = [n for n, _, _ in directed]
    assert len(set(names)) == len(names)
    far_matches = 0
    for name, blk, checks in directed:
        z = oracle.compress(blk)
        ops, produced = lzo_ops.parse(z)
        assert produced == len(blk), name
        lit = np.zeros(len(blk), dtype=bool)
        for op in ops:
            if op[0] == "L":
                lit[op[1]: op[1] + op[2]] = True
        for chk in checks:
            if chk[0] == "literals":
                _, start, length = chk
                assert lit[start: start + length].all(), (name, chk)
            else:
                _, start, length, dist = chk
                hits = [op for op in ops if op[0] == "M" and op[3] == dist and start <= op[1] < start + length]
                assert hits, (name, chk)
                far_matches += dist == M4_MAX_OFFSET
    assert far_matches >= len(BOUNDARY_SIZES) + 2 * len(LONG_SIZES)


def test_directed_inputs_rebase_counts(harness, directed):
    """Which of them re-base at all, by the header: none up to 65,548 bytes,
    the 200,000-byte ones several times even at the widest step."""
    for name, blk, _ in directed:
        n = len(blk)
        r = sweep(harness, n, n, 1, FIXED, 64)
        if n <= N_FREE:
            assert r.last_rebases == 0, name
        if n >= 200000:
            assert r.last_rebases >= 8, name
