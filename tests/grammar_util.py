"""Loader of tests/native/libgrammar_host.so (pomegranate_amd/csrc/
lzo1x_grammar.h on the CPU) for test_grammar.py and
test_directed_streams.py: the modes, and one guarded decode call."""
from __future__ import annotations

import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
LIB = os.path.join(NATIVE, "libgrammar_host.so")
CHECK = os.path.join(NATIVE, "grammar_check")

DONE, REFUSED, CAPACITY, LOOKBEHIND = 0, 1, 2, 3
GENERAL = 4
# zero bytes of one length extension from which a policy refuses (lzo1x_grammar.h)
POLICIES = {"fast": (0, None), "win_spec": (1, 65), "win_true": (2, 1 << 24), "lat": (3, 64)}
MODES = [(f"{name}{'-general' if g else ''}", pol | g, limit)
         for name, (pol, limit) in POLICIES.items() for g in (0, GENERAL)]

GUARD = 64


def load():
    if not (os.path.exists(LIB) and os.path.exists(CHECK)):
        subprocess.run(["make", "-C", NATIVE], check=True)
    lib = ctypes.CDLL(LIB)
    lib.grammar_decode.restype = ctypes.c_int
    lib.grammar_decode.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                   ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
    return lib


def decode(lib, z: bytes, cap: int, mode: int):
    """(status, bytes written); the GUARD bytes past the room must stay."""
    src = ctypes.create_string_buffer(z, max(len(z), 1))
    out = ctypes.create_string_buffer(b"\xA5" * (cap + GUARD), cap + GUARD)
    n = ctypes.c_uint32(0)
    rc = lib.grammar_decode(src, len(z), out, cap, mode, ctypes.byref(n))
    assert n.value <= cap and out.raw[cap:] == b"\xA5" * GUARD, "wrote past the room"
    return rc, out.raw[: n.value]
