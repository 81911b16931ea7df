"""Directed LZO1X streams: assemble(ops) writes the one valid stream of an
explicit op list, so a test can put a match of a chosen distance and length
at a chosen output offset (tests/lzo_families.py).  The grammar is the one
tests/lzo_streams.py states (lib/minilzo.c:3308-3699; SURVEY.md Appendix
A.2); test_directed_streams.py pins the builder against that generator and
against the oracle decoder.

An op is ("L", bytes) -- literal bytes -- or ("M", distance, length[, form])
-- a match; form is "M1" .. "M4", or absent: the form then follows from
(distance, length).  Rules:
  * adjacent literal ops are merged;
  * a literal of 1-3 bytes right after a match is that match's trailing
    literals; a longer one is a literal run (the state after a match without
    trailing literals, A, allows one);
  * the first op is a literal: 1..238 bytes as the first-byte form (17 + k),
    longer as an ordinary run;
  * a match is M2 for length 3..8 at distance <= 2048, else M3 up to distance
    16384 (0x4000 must be M3: as M4 it is the EOF marker), else M4 up to
    0xBFFF;
  * M1 only on request (a 2-byte match has no other form and needs none):
    after a literal run (state B) it copies 3 bytes from distance
    0x801..0xC00, after trailing literals (state C) 2 bytes from distance
    <= 1024.
Whatever the grammar cannot express raises ValueError; nothing is re-shaped.
parse() is the way back (ops and their output offsets), chain_depth() the
number of copies between an output byte and its literal, extension_zeros()
the longest zero run of a length extension (the decoders cap theirs).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

EOF = b"\x11\x00\x00"                # M4 with distance 0x4000
MAX_DIST = 0xBFFF
FIRST_MAX = 238                      # literals of the first-byte form
M3_BASE, M4_BASE = 33, 9             # the longest M3 / M4 match without a length extension


def m3_longest(zeros: int) -> int:
    """The longest M3 match with at most `zeros` zero bytes of extension."""
    return M3_BASE + (zeros + 1) * 255


def _ext(out: bytearray, x: int) -> None:
    """x >= 1 as (x - 1) // 255 zero bytes, then the rest."""
    zeros = (x - 1) // 255
    out.extend(bytes(zeros))
    out.append(x - 255 * zeros)


def normalise(ops: Sequence[tuple]) -> List[tuple]:
    """The op list as a stream holds it: adjacent literals merged, empty
    literals dropped, every match with its form.  Raises as assemble does."""
    merged: List[tuple] = []
    for op in ops:
        if op[0] == "L":
            b = bytes(op[1])
            if not b:
                continue
            if merged and merged[-1][0] == "L":
                merged[-1] = ("L", merged[-1][1] + b)
            else:
                merged.append(("L", b))
        elif op[0] == "M":
            if len(op) not in (3, 4):
                raise ValueError(f"match op {op!r}")
            merged.append(("M", int(op[1]), int(op[2]), op[3] if len(op) == 4 else None))
        else:
            raise ValueError(f"unknown op {op!r}")
    if not merged or merged[0][0] != "L":
        raise ValueError("a stream starts with a literal")
    out: List[tuple] = []
    state = "F"
    for i, op in enumerate(merged):
        if op[0] == "L":
            k = len(op[1])
            # (merged: a literal is the first op or follows a match, so 1-3
            # bytes are first-byte or trailing literals, 4 or more a run in
            # state F or A)
            state = "C" if k < 4 else "B"
            out.append(op)
            continue
        _, d, n, form = op
        if merged[i - 1][0] == "M":
            state = "A"
        out.append(("M", d, n, _form(i, d, n, form, state)))
    return out


def _form(i: int, d: int, n: int, form, state: str) -> str:
    if not 1 <= d <= MAX_DIST:
        raise ValueError(f"op {i}: distance {d}")
    if form is None:
        if n == 2:
            form = "M1"
        elif 3 <= n <= 8 and d <= 2048:
            form = "M2"
        elif d <= 0x4000:
            form = "M3"
        else:
            form = "M4"
    if form == "M1":
        ok = (state == "B" and n == 3 and 0x801 <= d <= 0xC00) or (state == "C" and n == 2 and d <= 1024)
    elif form == "M2":
        ok = 3 <= n <= 8 and d <= 2048
    elif form == "M3":
        ok = n >= 3 and d <= 0x4000
    elif form == "M4":
        ok = n >= 3 and d > 0x4000
    else:
        raise ValueError(f"op {i}: form {form!r}")
    if not ok:
        raise ValueError(f"op {i}: no {form} match of distance {d}, length {n} in state {state}")
    return form


def _copy(out: bytearray, d: int, n: int) -> None:
    if d >= n:
        out += out[len(out) - d: len(out) - d + n]
    else:
        pat = bytes(out[len(out) - d:])
        out += (pat * (n // d + 1))[:n]


def assemble(ops: Sequence[tuple], unchecked: bool = False) -> Tuple[bytes, bytes]:
    """(stream, output) of the op list, the EOF marker at the end.  A match
    that reaches before the output raises -- unless `unchecked`: the stream is
    then written all the same (a decoder must answer LOOKBEHIND_OVERRUN) and
    the output is what stands before that match."""
    norm = normalise(ops)
    z = bytearray()
    out = bytearray()
    broken = False
    for i, op in enumerate(norm):
        nxt = norm[i + 1] if i + 1 < len(norm) else None
        if op[0] == "L":
            b = op[1]
            k = len(b)
            if i == 0:
                if k <= FIRST_MAX:
                    z.append(17 + k)
                else:
                    z.append(0)
                    _ext(z, k - 18)
                z += b
            elif k >= 4:
                if k <= 18:
                    z.append(k - 3)
                else:
                    z.append(0)
                    _ext(z, k - 18)
                z += b
            # (1-3 bytes after a match: written with the match)
            if not broken:
                out += b
            continue
        _, d, n, form = op
        trail = nxt[1] if nxt is not None and nxt[0] == "L" and len(nxt[1]) < 4 else b""
        t_lo = len(trail)
        if form == "M1":
            dd = d - (0x801 if n == 3 else 1)
            z += bytes([((dd & 3) << 2) | t_lo, dd >> 2])
        elif form == "M2":
            dd = d - 1
            z += bytes([((n - 1) << 5) | ((dd & 7) << 2) | t_lo, dd >> 3])
        elif form == "M3":
            if n <= M3_BASE:
                z.append(32 | (n - 2))
            else:
                z.append(32)
                _ext(z, n - M3_BASE)
            v = ((d - 1) << 2) | t_lo
            z += bytes([v & 255, v >> 8])
        else:
            dd = d - 0x4000
            hi = (dd & 0x4000) >> 11
            if n <= M4_BASE:
                z.append(16 | hi | (n - 2))
            else:
                z.append(16 | hi)
                _ext(z, n - M4_BASE)
            v = ((dd & 0x3FFF) << 2) | t_lo
            z += bytes([v & 255, v >> 8])
        z += trail
        if d > len(out) and not broken:
            if not unchecked:
                raise ValueError(f"op {i}: distance {d} at output offset {len(out)}")
            broken = True
        if not broken:
            _copy(out, d, n)
    z += EOF
    return bytes(z), bytes(out)


def parse(z: bytes) -> Tuple[List[tuple], List[int]]:
    """The stream back as normalised ops, and every op's output offset.  For
    streams assemble (or lzo_streams.stream) wrote: anything else raises."""
    ops: List[tuple] = []
    offs: List[int] = []
    o = 0
    p = 0

    def ext(base: int) -> int:
        nonlocal p
        zeros = 0
        while z[p] == 0:
            zeros += 1
            p += 1
        x = 255 * zeros + z[p]
        p += 1
        return base + x

    def lit(k: int) -> None:
        nonlocal p, o
        if p + k > len(z):
            raise ValueError("literals past the end")
        ops.append(("L", bytes(z[p: p + k])))
        offs.append(o)
        p += k
        o += k

    state = "A"
    if z[0] > 17:
        k = z[0] - 17
        p = 1
        lit(k)
        state = "C" if k < 4 else "B"
    while True:
        t = z[p]
        p += 1
        if t < 16 and state == "A":
            lit(t + 3 if t else ext(18))
            state = "B"
            continue
        if t < 16:
            form = "M1"
            if state == "B":
                n, d = 3, 0x801 + (t >> 2) + (z[p] << 2)
            else:
                n, d = 2, 1 + (t >> 2) + (z[p] << 2)
            p += 1
            t_lo = t & 3
        elif t >= 64:
            form = "M2"
            n = (t >> 5) + 1
            d = 1 + ((t >> 2) & 7) + (z[p] << 3)
            p += 1
            t_lo = t & 3
        elif t >= 32:
            form = "M3"
            n = (t & 31) + 2 if t & 31 else ext(M3_BASE)
            v = z[p] | z[p + 1] << 8
            p += 2
            d = 1 + (v >> 2)
            t_lo = v & 3
        else:
            form = "M4"
            n = (t & 7) + 2 if t & 7 else ext(M4_BASE)
            v = z[p] | z[p + 1] << 8
            p += 2
            d = 0x4000 + ((t & 8) << 11) + (v >> 2)
            t_lo = v & 3
            if d == 0x4000:
                if n != 3 or t_lo or p != len(z):
                    raise ValueError("EOF marker not at the end")
                return ops, offs
        ops.append(("M", d, n, form))
        offs.append(o)
        o += n
        if t_lo:
            lit(t_lo)
            state = "C"
        else:
            state = "A"


def output_length(ops: Sequence[tuple]) -> int:
    return sum(len(op[1]) if op[0] == "L" else op[2] for op in ops)


def chain_depth(ops: Sequence[tuple]) -> np.ndarray:
    """Hops per output byte until a literal: 0 for a literal byte, else one
    more than the byte the match copies it from."""
    depth = np.zeros(output_length(ops), dtype=np.int64)
    o = 0
    for op in ops:
        if op[0] == "L":
            o += len(op[1])
            continue
        d, n = op[1], op[2]
        if d > o:
            raise ValueError(f"distance {d} at output offset {o}")
        if d >= n:
            depth[o: o + n] = depth[o - d: o - d + n] + 1
        else:
            j = np.arange(n)
            depth[o: o + n] = depth[o - d: o][j % d] + 1 + j // d
        o += n
    return depth


def extension_zeros(z: bytes) -> int:
    """The most zero bytes in one length extension of the stream (the
    decoders cap their zero runs: lzo1x_grammar.h)."""
    most = 0
    for op in parse(z)[0]:
        if op[0] == "L":
            x = len(op[1]) - 18
        elif op[3] in ("M3", "M4"):
            x = op[2] - (M3_BASE if op[3] == "M3" else M4_BASE)
        else:
            continue
        if x >= 1:
            most = max(most, (x - 1) // 255)
    return most
