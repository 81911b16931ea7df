"""CPU: column reads by offset and size (include/pom_column.h
pom_col_read_batch, pom_col_slice_dev) without a GPU -- the shared decision
and copy plan (pomegranate_amd/csrc/col_slice.h, compiled as plain C++)
against a Python restatement of api/api.c:6447-6460 and a byte slice, the
length bound of the staging against directed streams, the stand-alone checker,
the exports, and the refusal without a GPU."""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess

import pytest

import lzo_directed as ld
from conftest import ROOT
from grammar_util import DONE, MODES, decode, load as load_grammar
from pomegranate_amd import column, lzo

NATIVE = os.path.join(ROOT, "tests", "native")
LIB = os.path.join(NATIVE, "libcol_slice_host.so")
CHECK = os.path.join(NATIVE, "col_slice_check")
EINVAL = -22
U64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def harness():
    if not (os.path.exists(LIB) and os.path.exists(CHECK)):
        subprocess.run(["make", "-C", NATIVE, "-f", "col_slice.mk"], check=True)
    lib = ctypes.CDLL(LIB)
    u64 = ctypes.c_uint64
    lib.col_slice_decide_host.restype = ctypes.c_int32
    lib.col_slice_decide_host.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int32, u64, u64, u64, u64,
                                          ctypes.POINTER(u64)]
    lib.col_slice_want_ok_host.restype = ctypes.c_int
    lib.col_slice_want_ok_host.argtypes = [u64, u64]
    lib.col_slice_copy_host.restype = ctypes.c_int
    lib.col_slice_copy_host.argtypes = [ctypes.c_void_p, u64, u64, u64, ctypes.c_uint32, ctypes.c_void_p, u64]
    return lib


def decide(lib, ncol, col, hdr_ok, status, produced, want, offset, size):
    n = ctypes.c_uint64(77)
    e = lib.col_slice_decide_host(col < ncol, hdr_ok, status, produced, want, offset, size, ctypes.byref(n))
    return e, n.value


def reference_read(ncol, col, hdr_ok, status, produced, want, offset, size):
    """What a read returns: the decode's checks (api/api.c:6427-6446, a length
    mismatch being an error here), then :6447-6460 -- an offset past the end is
    -EINVAL, else the region [offset, min(offset + size, olen)) in Python's
    unbounded integers."""
    if col >= ncol:
        return EINVAL, 0
    if not hdr_ok:
        return lzo.LZO_E_ERROR, 0
    if status != 0:
        return status, 0
    if produced != want:
        return lzo.LZO_E_ERROR, 0
    if offset > want:
        return EINVAL, 0
    return 0, min(offset + size, want) - offset


def test_decision_rules(harness):
    W = 5000
    cases = [(3, 1, 1, 0, W, W, W, 10),              # offset == W: a valid empty read
             (3, 1, 1, 0, W, W, W + 1, 10),          # offset == W + 1
             (3, 1, 1, 0, W, W, 0, U64),             # size = 2**64 - 1
             (3, 1, 1, 0, W, W, 4999, U64), (3, 1, 1, 0, W, W, W, U64), (3, 1, 1, 0, W, W, U64, U64),
             (3, 1, 1, 0, W, W, 100, 0),             # size = 0
             (3, 3, 1, 0, W, W, 0, 10), (3, 2 ** 32 - 1, 1, 0, W, W, 0, 10),   # col out of range
             (3, 0, 0, 0, 0, 0, 0, 10),              # no header
             (3, 0, 1, -4, 17, W, 0, 10), (3, 0, 1, -8, W, W, 0, 10),          # the decoder's code
             (3, 0, 1, 0, W - 1, W, 0, 10), (3, 0, 1, 0, W + 1, W, 0, 10),     # another length than recorded
             (3, 0, 1, 0, W, W, 100, 200), (3, 0, 1, 0, W, W, 4900, 200), (3, 0, 1, 0, 0, 0, 0, 1)]
    for c in cases:
        assert decide(harness, *c) == reference_read(*c), c
    assert decide(harness, *cases[0]) == (0, 0) and decide(harness, *cases[1]) == (EINVAL, 0)
    assert decide(harness, *cases[2]) == (0, W) and decide(harness, *cases[3]) == (0, 1)
    # the order: the column index before the header, the header before the code,
    # the code before the length, the length before the offset
    assert decide(harness, 3, 3, 0, -4, 1, 2, 9, 1)[0] == EINVAL
    assert decide(harness, 3, 0, 0, -4, 1, 2, 9, 1)[0] == lzo.LZO_E_ERROR
    assert decide(harness, 3, 0, 1, -4, 1, 2, 9, 1)[0] == -4
    assert decide(harness, 3, 0, 1, 0, 1, 2, 9, 1)[0] == lzo.LZO_E_ERROR
    assert decide(harness, 3, 0, 1, 0, 2, 2, 9, 1)[0] == EINVAL


def test_decision_rules_swept(harness):
    for want in (0, 1, 4096, 0xFFFFFFF0):
        for offset in (0, 1, max(want - 1, 0), want, want + 1, U64):
            for size in (0, 1, want, want + 1, U64 - 1, U64):
                c = (1, 0, 1, 0, want, want, offset, size)
                assert decide(harness, *c) == reference_read(*c), c


def test_copy_plan_equals_a_byte_slice(harness):
    """The kernel's address arithmetic, every tile and lane, over checked
    memory: the bytes of col[offset: offset + n], no load outside the column's
    dwords, every destination byte stored once."""
    col = bytes((i * 131 + 7) % 251 for i in range(3 * 4096 + 100))
    for col_res, offset, n, dst_res in [(0, 0, len(col), 0), (3, 17, 4097, 9), (15, 1, 31, 15), (8, 4095, 8193, 1),
                                        (5, len(col), 0, 2), (1, len(col) - 1, 1, 0)]:
        src = ctypes.create_string_buffer(col, len(col))
        dst = ctypes.create_string_buffer(b"\xA5" * (n + 1), n + 1)
        rc = harness.col_slice_copy_host(src, 0x40000 + col_res, len(col), offset, n, dst, 0x80000 + dst_res)
        assert rc == 0, (col_res, offset, n, dst_res, rc)
        assert dst.raw == col[offset: offset + n] + b"\xA5", (col_res, offset, n, dst_res)


def longest_ratio_stream(zeros: int):
    """One literal byte, then the densest match there is: an M3 token, `zeros`
    zero bytes of extension, the final length byte 255 and two offset bytes --
    288 + 255 * zeros bytes out of zeros + 4 in."""
    return ld.assemble([("L", b"q"), ("M", 1, ld.m3_longest(zeros))])


@pytest.mark.parametrize("zeros", [0, 1, 40])
def test_length_bound_against_the_grammar(harness, oracle, zeros):
    """W <= 255 * (zip_len - 8) holds for the densest stream the grammar can
    express, with less than 8 input bytes' worth to spare; one more than the
    bound is refused."""
    z, out = longest_ratio_stream(zeros)
    assert len(z) == 2 + (zeros + 4) + 3 and len(out) == 1 + 288 + 255 * zeros
    assert ld.extension_zeros(z) == zeros
    assert oracle.decompress_safe(z, len(out)) == (0, out)
    grammar = load_grammar()
    for _, mode, limit in MODES:
        if limit is None:
            assert decode(grammar, z, len(out), mode) == (DONE, out)
    ok = harness.col_slice_want_ok_host
    assert ok(len(out), len(z)) == 1
    assert ok(len(out), len(z) - 8) == 0             # the bound is within 8 input bytes of this stream
    # the match alone, without the literal before it and the end marker behind
    assert 288 + 255 * zeros <= 255 * (zeros + 4)
    assert ok(255 * len(z), len(z)) == 1 and ok(255 * len(z) + 1, len(z)) == 0
    # the header of such a column, one byte above the bound: refused
    hdr = struct.pack("<Q", 255 * len(z) + 1)
    assert ok(struct.unpack("<Q", hdr)[0], len(hdr + z) - 8) == 0


def test_length_bound_edges(harness):
    ok = harness.col_slice_want_ok_host
    assert ok(0, 0) == 1 and ok(1, 0) == 0 and ok(255, 1) == 1 and ok(256, 1) == 0
    assert ok(0xFFFFFFF0, U64) == 1 and ok(0xFFFFFFF1, U64) == 0 and ok(U64, U64) == 0
    assert ok(0xFFFFFFF0, 0xFFFFFFF0 // 255) == 0 and ok(0xFFFFFFF0, 0xFFFFFFF0 // 255 + 1) == 1


def test_checker_exits_0(harness):
    """tests/native/col_slice_check: the sweep of source offsets, destination
    alignments and lengths against a byte loop, under ASan and UBSan where
    they link (a stand-alone program)."""
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "col_slice_check: ok" in r.stdout


def test_new_exports_present():
    lib = ctypes.CDLL(lzo.LIB_PATH)
    for name in ("pom_col_read_batch", "pom_col_slice_dev"):
        assert name in lzo.EXPORTS and hasattr(lib, name), name
    assert ctypes.sizeof(column.Req) == 24


def _gpu_present():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_gpu_present(), reason="checks the no-GPU refusal")
def test_read_batch_refuses_without_gpu():
    z = struct.pack("<Q", 1) + b"\x12q\x11\x00\x00"
    with pytest.raises(RuntimeError, match="pom_col_read_batch: -1"):
        column.read_batch([z], [(0, 0, 1)])
    with pytest.raises(RuntimeError):
        column.read_batch([z], [])
