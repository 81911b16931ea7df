"""Families of directed LZO1X streams (lzo_directed.assemble) that put match
copies at the edges of the GPU decoders' copy machinery: 16-byte chunks and
the period x phase selector table of the op-set decoder
(lzo1x_decode_fast.hip), its source forwarding inside a 64-op window, its
4 KiB ring / 2 KiB store lag / HBM read-back and 1 KiB source buffer; the
windowed decoder's 4 KiB windows, 64 KiB ring and 1024-entry op table
(lzo1x_decode_win.hip); the latency decoder's origin doubling
(lzo1x_decode_lat.hip).

Every family returns Blocks and asserts what it claims to hold, from the
parsed stream, so a later edit cannot quietly empty it.  Literal bytes are
random and seeded: a wrong phase shows as wrong bytes.  CPU only.
"""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np

import lzo_directed as ld

OK, E_LOOKBEHIND_OVERRUN = 0, -6
LIT_MAX = 15000          # (a literal run of 18 + 62 * 255 bytes or more has 62 zero bytes of extension)


class Block(NamedTuple):
    name: str
    stream: bytes
    output: bytes        # what a decoder writes (up to the failing op when rc != OK)
    cap: int             # the room the tests give it
    rc: int              # the oracle's code at that room
    nops: int


class _Ops:
    """An op list under construction: knows the output offset."""

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.ops: List[tuple] = []
        self.n = 0

    def lit(self, k: int) -> None:
        assert k >= 1
        self.ops.append(("L", self.rng.integers(0, 256, k, dtype=np.uint8).tobytes()))
        self.n += k

    def history(self, k: int) -> None:
        """k fresh bytes for later matches to read, in literal runs short
        enough for a length extension of under 62 zero bytes (a 3-byte match
        between two runs)."""
        while k > LIT_MAX:
            self.lit(LIT_MAX - 3)
            self.match(5, 3)
            k -= LIT_MAX
        self.lit(k)

    def match(self, d: int, length: int, form=None) -> int:
        """-> the index of the op in the list"""
        assert 1 <= d <= self.n, (d, self.n)
        self.ops.append(("M", d, length) if form is None else ("M", d, length, form))
        self.n += length
        return len(self.ops) - 1

    def lit_to(self, residue: int, mod: int, least: int = 1) -> None:
        """Fresh literals, `least` or more, up to the next offset that is
        `residue` mod `mod`."""
        self.lit(least + (residue - self.n - least) % mod)

    def block(self, name: str) -> Block:
        z, out = ld.assemble(self.ops)
        assert len(out) == self.n
        return Block(name, z, out, len(out), OK, len(ld.normalise(self.ops)))


def _matches(z: bytes):
    """(distance, length, output offset, form) of every match of a stream."""
    ops, offs = ld.parse(z)
    return [(op[1], op[2], o, op[3]) for op, o in zip(ops, offs) if op[0] == "M"]


# ---------------------------------------------------------------------------
# P. Period x phase x length x alignment
# ---------------------------------------------------------------------------
P_LENGTHS = [3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 255, 256, 257,
             1023, 1024, 1025, 1040, 1041, 2100]
P_DISTANCES = list(range(1, 34))
P_THIN = [1, 2, 3, 7, 15, 16, 17, 33]          # the latency paths' share


def family_p(distances=P_DISTANCES) -> List[Block]:
    """One block per distance d: every length of P_LENGTHS at every output
    residue mod 16, each match right after d or more fresh literal bytes (the
    pattern it repeats)."""
    out = []
    for d in distances:
        b = _Ops(7100 + d)
        for length in P_LENGTHS:
            for res in range(16):
                b.lit_to(res, 16, least=d)
                b.match(d, length)
        blk = b.block(f"P/d={d}")
        got = {(m[0], m[1], m[2] % 16) for m in _matches(blk.stream)}
        assert got == {(d, n, r) for n in P_LENGTHS for r in range(16)}, blk.name
        assert blk.nops == 2 * 16 * len(P_LENGTHS)
        out.append(blk)
    return out


# ---------------------------------------------------------------------------
# F. A match out of an earlier op of the same window
# ---------------------------------------------------------------------------
F_PERIODS = [1, 2, 3, 5, 15, 16, 17, 31, 40]
F_A_LEN = 200
F_DEPTHS = list(range(1, 9))


def family_f() -> List[Block]:
    """Per period p: op A, a match of period p and length 200 after p + 6
    fresh bytes, and op B zero to two ops later, reading from offset r into A
    with r mod p in {0, 1, p - 1}; B's source span ends one before, at and one
    past a period boundary of A; B once shorter than its distance and once
    periodic itself.  Then forwarding chains: op k copies from inside op
    k - 1 (3..8 bytes each, so a chain lies inside one 1 KiB step), depths
    1..8 with and without trailing literals between, and one block that is a
    single window: a literal and a chain of 63."""
    out = []
    for p in F_PERIODS:
        b = _Ops(7200 + p)
        plan = []                                  # (index of A, index of B, r mod p, end class, periodic)
        case = 0
        for rm in sorted({0, 1 % p, p - 1}):
            for endc in sorted({p - 1, 0, 1 % p}):
                for periodic in (False, True):
                    b.lit(p + 6)
                    ia = b.match(p, F_A_LEN)
                    a0 = b.n - F_A_LEN
                    gap = case % 3                 # ops between A and B
                    case += 1
                    if gap >= 1:
                        b.lit(1 + case % 3)        # A's trailing literals
                    if gap == 2:
                        b.match(b.n - a0 + 3, 4)   # (from the fresh bytes before A)
                    if periodic:                   # the source starts near A's end
                        r = F_A_LEN - 12
                        r -= (r - rm) % p
                        d = b.n - (a0 + r)
                        length = d + 20
                    else:
                        r = 3 * p + rm if p < 16 else p + rm
                        d = b.n - (a0 + r)
                        length = 40
                    length += (endc - (r + length)) % p
                    assert (not periodic and length <= d and r + length <= F_A_LEN) or (periodic and d < length)
                    ib = b.match(d, length)
                    plan.append((ia, ib, rm, endc, periodic))
        blk = b.block(f"F/p={p}")
        ops, offs = ld.parse(blk.stream)
        seen = set()
        for ia, ib, rm, endc, periodic in plan:
            (_, da, na, _), (_, db, nb, _) = ops[ia], ops[ib]
            r = offs[ib] - db - offs[ia]
            assert (da, na) == (p, F_A_LEN) and ib - ia <= 3 and 0 <= r < na
            assert r % p == rm and (r + nb) % p == endc and (db < nb) == periodic
            seen.add((rm, endc, periodic))
        assert len(seen) == len(plan) == 2 * len({0, 1 % p, p - 1}) ** 2
        out.append(blk)

    def chain(b: _Ops, depth: int, trailing: bool):
        """-> the op indices of the chain's matches"""
        b.lit(20)
        prev_o, prev_n, idx = b.n - 8, 8, []       # "op 0": the literal's last 8 bytes
        for k in range(1, depth + 1):
            t = (k % 3) if trailing and k > 1 else 0
            if t:
                b.lit(t)
            skew = k % 2 if prev_n + t - 1 >= 3 else 0
            d = b.n - (prev_o + skew)
            length = min(3 + (5 * k) % 6, d)
            prev_o, prev_n = b.n, length
            idx.append(b.match(d, length))
        return idx

    def check_chain(blk, ops_idx):
        ops, offs = ld.parse(blk.stream)
        depth = ld.chain_depth(ops)
        for chain_idx in ops_idx:
            for k, i in enumerate(chain_idx, 1):
                o, n = offs[i], ops[i][2]
                assert 3 <= n <= 8 and ops[i][1] >= n
                assert depth[o: o + n].max() == k, (blk.name, k)
                if k > 1:                          # its first byte comes out of op k - 1
                    j = chain_idx[k - 2]
                    assert offs[j] <= o - ops[i][1] < offs[j] + ops[j][2]

    b = _Ops(7290)
    chains = [chain(b, depth, trailing) for trailing in (False, True) for depth in F_DEPTHS]
    blk = b.block("F/chains")
    check_chain(blk, chains)
    assert [len(c) for c in chains] == F_DEPTHS * 2
    out.append(blk)

    b = _Ops(7291)
    b.lit(8)
    idx, prev_n = [], 8
    for k in range(1, 64):
        length = 8 - (k * 6) // 64                 # 8 .. 3, never growing: no op overlaps itself
        idx.append(b.match(prev_n, length))        # from the first byte of op k - 1
        prev_n = length
    blk = b.block("F/chain63")
    check_chain(blk, [idx])
    assert blk.nops == 64 and len(idx) == 63 and blk.cap < 1024
    out.append(blk)
    return out


# ---------------------------------------------------------------------------
# D. Distance boundaries
# ---------------------------------------------------------------------------
D_BOUNDS = [1024, 2048, 3072, 4096, 5120, 6144, 8192, 16384, 32768, 0xBFFF]
D_LENGTHS = [3, 16, 33, 300, 1100, 5000]


def family_d() -> List[Block]:
    """One block per boundary B (ring, mirror, store lag, HBM read-back, the
    M2 / M3 / M4 form limits): every distance B - 17 .. B + 17 (up to 0xBFFF)
    at every length of D_LENGTHS, the match starts alternating between
    residue 0 and an odd residue mod 16."""
    out = []
    forms = set()
    for bound in D_BOUNDS:
        dists = [d for d in range(bound - 17, bound + 18) if d <= ld.MAX_DIST]
        b = _Ops(7300 + bound)
        b.history(dists[-1])
        i = 0
        for d in dists:
            for length in D_LENGTHS:
                b.lit_to(0 if i % 2 == 0 else (i % 16) | 1, 16, least=4)
                b.match(d, length)
                i += 1
        blk = b.block(f"D/B={bound}")
        ms = [m for m in _matches(blk.stream) if m[2] >= dists[-1]]      # (not the history's)
        assert {(m[0], m[1]) for m in ms} == {(d, n) for d in dists for n in D_LENGTHS}
        res = [m[2] % 16 for m in ms]
        assert all(r == 0 for r in res[0::2]) and all(r % 2 == 1 for r in res[1::2])
        assert len(set(res)) == 9 and blk.cap <= 1 << 20
        forms |= {(m[3], m[0]) for m in ms}
        out.append(blk)
    # the form limits, from both sides
    assert {("M2", 2048), ("M3", 2049), ("M3", 0x4000), ("M4", 0x4001), ("M4", 0xBFFF)} <= forms
    return out


# ---------------------------------------------------------------------------
# W. Window and ring straddles
# ---------------------------------------------------------------------------
W_BEFORE = [1, 8, 15, 16, 17]
W_DISTANCES = [1, 2, 3, 7, 8, 9, 4095, 4096, 4097, 0xBFFF]
W_LENGTHS = [40, 5000, 9000, 70000]      # inside a window; across one, two, seventeen (and the 64 KiB ring)


def family_w() -> List[Block]:
    """Per distance: every length of W_LENGTHS starting 1, 8, 15, 16 and 17
    bytes before a multiple of 4096 (fresh literals pad up to it).  A distance
    of 4095..4097 puts the source across the boundary before.  The
    70,000-byte matches stand in blocks of their own: their length extension
    is 274 zero bytes, and the latency decoder hands such a stream over."""
    out = []
    for d in W_DISTANCES:
        for lengths in (W_LENGTHS[:3], W_LENGTHS[3:]):
            b = _Ops(7400 + d + lengths[0])
            b.history(max(d, 16))
            for length in lengths:
                for k in W_BEFORE:
                    b.lit_to(4096 - k, 4096, least=4)
                    b.match(d, length)
            blk = b.block(f"W/d={d}" + ("/L=70000" if lengths[0] == 70000 else ""))
            got = {(m[0], m[1], 4096 - m[2] % 4096) for m in _matches(blk.stream) if m[2] >= d}
            assert got == {(d, n, k) for n in lengths for k in W_BEFORE}, blk.name
            assert blk.cap <= 1 << 20 and (ld.extension_zeros(blk.stream) >= 64) == (lengths[0] == 70000)
            out.append(blk)
    assert len(out) == 2 * len(W_DISTANCES) and W_LENGTHS[3] == 70000
    return out


def family_w64() -> List[Block]:
    """The same straddles at the windowed decoder's ring size: one block per
    (distance, bytes before 65536), the lengths taking turns so that each
    meets every distance and every offset; and one block per distance at
    131072, the second wrap, offsets and lengths taking turns."""
    out = []

    def one(name, seed, d, k, edge, length):
        b = _Ops(seed)
        b.history(max(d, 4096))
        # (cheap filler up to the edge: long matches, then 1000 or more fresh bytes)
        while edge - k - b.n > 9000:
            b.match(min(b.n, ld.MAX_DIST - 5), 8000)
            b.lit(2)
        b.lit(edge - k - b.n)
        assert len(b.ops[-1][1]) >= 990
        b.match(d, length)
        blk = b.block(name)
        assert _matches(blk.stream)[-1][:3] == (d, length, edge - k) and blk.cap == edge - k + length
        return blk

    pairs = set()
    for i, d in enumerate(W_DISTANCES):
        for j, k in enumerate(W_BEFORE):
            n = W_LENGTHS[(i + j) % 4]
            out.append(one(f"W64/65536-{k}/d={d}/L={n}", 7500 + 16 * i + j, d, k, 65536, n))
            pairs |= {("d", d, n), ("k", k, n)}
    assert pairs == {("d", d, n) for d in W_DISTANCES for n in W_LENGTHS} | \
        {("k", k, n) for k in W_BEFORE for n in W_LENGTHS}
    for i, d in enumerate(W_DISTANCES):
        k, n = W_BEFORE[i % 5], W_LENGTHS[i % 4]
        out.append(one(f"W64/131072-{k}/d={d}/L={n}", 7700 + i, d, k, 131072, n))
    return out


# ---------------------------------------------------------------------------
# C. Chains
# ---------------------------------------------------------------------------
C_HOPS = [7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32767, 32768, 32769,
          262143, 262144, 262145, 1 << 20]
# the room is the output length, h + 1: the latency decoder's round count R
# (8^R > room) is at its smallest against the chain at h = 8^R - 2
C_HOPS_TIGHT = [8 ** r - 2 for r in range(1, 7)]
C_MATCH_MAX = ld.m3_longest(61)          # 33 + 62 * 255: the extension stays at 61 zero bytes


def family_c() -> List[Block]:
    """One byte, then h bytes copied at distance 1 by consecutive matches of
    at most C_MATCH_MAX bytes: output byte h is h hops from its literal.  A
    longer match would carry 63 or more zero bytes of length extension, and
    the latency decoder hands streams with 64 over.  Deep and shallow chains
    alternate, so every group of 8 holds both."""
    hops = sorted(C_HOPS + C_HOPS_TIGHT)
    half = (len(hops) + 1) // 2
    shallow, deep = hops[:half], hops[half:][::-1]
    order = [h for i in range(half) for h in (shallow[i:i + 1] + deep[i:i + 1])]
    assert sorted(order) == hops
    out = []
    for h in order:
        b = _Ops(7600)
        b.lit(1)
        left = h
        while left:
            n = min(left, C_MATCH_MAX)
            if 0 < left - n < 3:                   # (no match is shorter than 3)
                n -= 3
            b.match(1, n)
            left -= n
        blk = b.block(f"C/h={h}")
        assert blk.cap == h + 1 and blk.output == blk.output[:1] * (h + 1)
        assert bytes(62) not in blk.stream and (h < C_MATCH_MAX or bytes(61) in blk.stream)
        depth = ld.chain_depth(ld.parse(blk.stream)[0])
        assert depth[-1] == h == depth.max() and (np.diff(depth) == 1).all()
        out.append(blk)
    for g in range(0, len(out) - 7, 8):
        caps = [blk.cap for blk in out[g: g + 8]]
        assert max(caps) >= 4096 and max(caps) >= 8 * min(caps), caps   # at least a round apart
    return out


# ---------------------------------------------------------------------------
# N. Op density
# ---------------------------------------------------------------------------
N_REPS = 6000


def family_n() -> List[Block]:
    """The densest streams the grammar has (two ops per 3 input bytes: 1,365
    per 2 KiB piece, more than the windowed decoder's 1024-entry op table per
    4 KiB of output), and the converse for the op-set decoder's 1 KiB source
    buffer: 64-op windows whose literal spans and far sources exceed it."""
    out = []
    for name, n, limit in (("m1c", 2, 1024), ("m2", 3, 2048)):
        b = _Ops(7700 + n)
        b.lit(3)
        for _ in range(N_REPS):
            b.match(int(b.rng.integers(1, min(b.n, limit) + 1)), n, "M1" if n == 2 else "M2")
            b.lit(1)
        blk = b.block(f"N/{name}")
        ops, offs = ld.parse(blk.stream)
        assert len(ops) == 2 * N_REPS + 1 and len(blk.stream) == 1 + 3 + 3 * N_REPS + 3
        assert {op[3] for op in ops if op[0] == "M"} == {"M1" if n == 2 else "M2"}
        per_window = np.bincount(np.asarray(offs) // 4096)
        assert per_window.max() > 1024, per_window
        per_piece = np.bincount((4 + 3 * (np.arange(2 * N_REPS) // 2)) // 2048)
        assert per_piece.max() == 1366             # (683 instructions begin in a full piece)
        out.append(blk)

    def src_bytes(ops):
        """bytes a window's source buffer would hold: literals and far sources"""
        return np.asarray([len(op[1]) if op[0] == "L" else (op[2] if op[1] > 4096 else 0) for op in ops])

    def far(b):
        return int(b.rng.integers(4097, min(b.n, ld.MAX_DIST) + 1))

    for name in ("lit40+m3", "far30", "lit40+far30"):
        b = _Ops(7710 + len(name))
        b.lit(5000)
        for i in range(320):
            if name == "lit40+m3":
                b.match(int(b.rng.integers(3, 2048)), 3)
                b.lit(40)
            elif name == "far30":
                b.match(far(b), 30)
                b.match(far(b), 30)
            else:
                b.match(far(b), 30)
                b.lit(40)
        blk = b.block(f"N/{name}")
        need = src_bytes(ld.parse(blk.stream)[0][1:])
        assert len(need) == 640
        run = np.convolve(need, np.ones(64, dtype=np.int64), "valid")
        assert run.min() > 1024, (name, run.min())  # every 64 consecutive ops
        out.append(blk)
    return out


# ---------------------------------------------------------------------------
# E. Ends
# ---------------------------------------------------------------------------
E_POSITIONS = [1, 2, 3, 4, 15, 16, 17, 2048, 4096, 0xBFFF]


def family_e() -> List[Block]:
    """Blocks that end with a match (shorter than its distance, periodic, and
    a long periodic one) at every output length mod 16; a match whose
    distance is the output offset (its source is byte 0) at E_POSITIONS."""
    out = []
    for kind, d, n, lead in (("plain", 20, 17, 24), ("periodic", 3, 37, 24), ("long", 7, 2100, 3000)):
        for res in range(16):
            b = _Ops(7800 + res)
            b.lit(lead + (res - n - lead) % 16)
            b.match(d, n)
            blk = b.block(f"E/{kind}/n%16={res}")
            ops, _ = ld.parse(blk.stream)
            assert ops[-1][:3] == ("M", d, n) and blk.cap % 16 == res
            out.append(blk)
    assert {(b.name.split("/")[1], b.cap % 16) for b in out} == \
        {(k, r) for k in ("plain", "periodic", "long") for r in range(16)}
    for pos in E_POSITIONS:
        b = _Ops(7900)
        b.history(pos)
        b.match(pos, 20)
        b.lit(2)
        blk = b.block(f"E/byte0/pos={pos}")
        assert _matches(blk.stream)[-1][:3] == (pos, 20, pos)
        out.append(blk)
    return out


def family_e_lookbehind() -> List[Block]:
    """The byte-0 streams of E with the distance one larger: the match reaches
    one byte before the output.  Not valid: the oracle answers
    LOOKBEHIND_OVERRUN with the literals before the match as output.  (Not at
    0xBFFF: the grammar has no distance 0xC000.)"""
    out = []
    for pos in E_POSITIONS:
        if pos + 1 > ld.MAX_DIST:
            continue
        b = _Ops(7900)
        b.lit(pos)
        ops = b.ops + [("M", pos + 1, 20), ("L", b"xy")]
        z, produced = ld.assemble(ops, unchecked=True)
        assert len(produced) == pos
        out.append(Block(f"E/lookbehind/pos={pos}", z, produced, pos + 22, E_LOOKBEHIND_OVERRUN, 3))
    assert len(out) == len(E_POSITIONS) - 1
    return out


# ---------------------------------------------------------------------------
# Z. The latency decoder's zero-run cap
# ---------------------------------------------------------------------------
def family_z() -> List[Block]:
    """One length extension of 63 zero bytes (the largest value they carry)
    and of 64 (the smallest): a literal run of 16,338 / 16,339 bytes, an M3
    match of 16,353 / 16,354, an M4 match of 16,329 / 16,330.  Valid streams;
    the latency decoder alone hands the second of each pair over
    (include/lzo_mi355x.h)."""
    out = []
    for zeros, x in ((63, 255 * 64), (64, 255 * 64 + 1)):
        for kind in ("lit", "m3", "m4"):
            b = _Ops(7950 + zeros)
            if kind == "lit":
                b.lit(7)
                b.match(3, 5)
                b.lit(18 + x)
                b.match(9, 6)
            elif kind == "m3":
                b.lit(40)
                b.match(17, ld.M3_BASE + x, "M3")
            else:
                b.history(0x4100)
                b.match(0x4001 + zeros, ld.M4_BASE + x, "M4")
            blk = b.block(f"Z/{kind}/zeros={zeros}")
            # (the count is the decoder's: a literal run's own instruction byte, 0, is not part of it)
            assert ld.extension_zeros(blk.stream) == zeros and bytes(zeros) in blk.stream
            out.append(blk)
    assert [b.cap for b in out[:3]] == [7 + 5 + 16338 + 6, 40 + 16353, 0x4100 + 16329]
    return out


FAMILIES = {"Z": family_z, "P": family_p, "F": family_f, "D": family_d, "W": family_w, "W64": family_w64,
            "C": family_c, "N": family_n, "E": family_e}


def summary(blocks: List[Block]) -> str:
    return (f"{len(blocks)} blocks, {sum(len(b.output) for b in blocks)} output bytes, "
            f"{sum(len(b.stream) for b in blocks)} stream bytes, {sum(b.nops for b in blocks)} ops")
