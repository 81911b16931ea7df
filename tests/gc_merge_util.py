"""The GC range merge's test model, range families and CPU harness (shared by
test_gc_merge.py and test_gpu_gc_merge.py).

model() restates what the reference's range tree computes (lib/brtree.c
brt_add walked by brt_loop_on_ranges, folded by gc_data_stat_cb,
mdsl/gc.c:746-753), checked against the reference's own answers recorded in
tests/golden/brt_ranges.json:
  sort the ranges by low; a range starts a new extent if and only if its low
  is strictly greater than the largest high seen so far; an extent is [first
  low, largest high); the extents come out ascending.
plus the rule of include/pom_gc.h for what the reference leaves undefined: a
range with high <= low is dropped and counted.  It does not look at the
product's gc_merge.h."""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import NamedTuple

import numpy as np

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
HOST_LIB = os.path.join(NATIVE, "libgc_merge_host.so")
CHECK = os.path.join(NATIVE, "gc_merge_check")
EINVAL, E_NOSPACE = -22, -4098
U64 = np.uint64


class Merged(NamedTuple):
    out: np.ndarray         # uint64 [nout, 2]
    valid: int              # mod 2^64
    max: int
    nout: int
    nin: int
    nwrapped: int

    @property
    def stat(self):
        return (self.valid, self.max, self.nout, self.nin, self.nwrapped)


def as_ranges(rows) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(rows, dtype=U64).reshape(-1, 2))


def model(ranges) -> Merged:
    r = as_ranges(ranges)
    n = len(r)
    keep = r[:, 1] > r[:, 0]
    k = r[keep]
    k = k[np.argsort(k[:, 0], kind="stable")]
    if len(k) == 0:
        return Merged(np.zeros((0, 2), dtype=U64), 0, 0, 0, n, n)
    runmax = np.maximum.accumulate(k[:, 1])
    head = np.ones(len(k), dtype=bool)
    head[1:] = k[1:, 0] > runmax[:-1]
    last = np.ones(len(k), dtype=bool)
    last[:-1] = head[1:]
    out = np.stack([k[head, 0], runmax[last]], axis=1)
    valid = int((out[:, 1] - out[:, 0]).sum(dtype=U64))
    return Merged(out, valid, int(out[-1, 1]), len(out), n, n - len(k))


def build_native(out_dir=None, inc_dir=None):
    """The harnesses of tests/native/gc_merge.mk, the compiler's words on failure."""
    cmd = ["make", "-C", NATIVE, "-f", "gc_merge.mk"]
    if out_dir:
        cmd += [f"OUT={out_dir}/", f"GC_MERGE_INC=-I{inc_dir}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


class Host:
    """libgc_merge_host.so: gc_merge.h composed on the CPU, and the host fold."""

    def __init__(self, path=HOST_LIB):
        if path == HOST_LIB and not os.path.exists(path):
            build_native()
        lib = self.lib = ctypes.CDLL(path)
        lib.gc_merge_const.restype = ctypes.c_uint32
        lib.gc_merge_const.argtypes = [ctypes.c_int]
        lib.gc_merge_host.restype = ctypes.c_int
        lib.gc_merge_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p]
        lib.pom_gc_fold.restype = ctypes.c_int
        lib.pom_gc_fold.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                    ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        self.sort_tile, self.scan_tile, self.agg_threads, self.max_n = (int(lib.gc_merge_const(i)) for i in range(4))

    def merge(self, ranges, out_cap=None):
        """(rc, out[min(nout, cap)], stat tuple, the whole out buffer with one guard row)."""
        r = as_ranges(ranges)
        n = len(r)
        before = r.copy()
        cap = n if out_cap is None else out_cap
        out = np.full((cap + 1, 2), 0xA5A5A5A5A5A5A5A5, dtype=U64)
        st = np.full(5, 7, dtype=U64)
        rc = self.lib.gc_merge_host(r.ctypes.data if n else None, n, out.ctypes.data, cap, st.ctypes.data)
        assert (r == before).all(), "the input was modified"
        fit = min(int(st[2]), cap)
        assert (out[fit:] == U64(0xA5A5A5A5A5A5A5A5)).all(), "written past min(nout, out_cap)"
        return rc, out[:fit], tuple(int(x) for x in st)

    def fold(self, maps, seed=None, merged_cap=None):
        """(rc, merged[min(nout, cap)], stat tuple) of pom_gc_fold."""
        maps = [as_ranges(m) for m in maps]
        seed = as_ranges([] if seed is None else seed)
        ptrs = (ctypes.c_void_p * max(len(maps), 1))(*[m.ctypes.data for m in maps])
        cnts = (ctypes.c_size_t * max(len(maps), 1))(*[len(m) for m in maps])
        cap = sum(len(m) for m in maps) + len(seed) if merged_cap is None else merged_cap
        merged = np.full((cap + 1, 2), 0xA5A5A5A5A5A5A5A5, dtype=U64)
        st = np.full(5, 7, dtype=U64)
        rc = self.lib.pom_gc_fold(ptrs, cnts, len(maps), seed.ctypes.data if len(seed) else None, len(seed),
                                  merged.ctypes.data, cap, st.ctypes.data)
        fit = min(int(st[2]), cap)
        assert (merged[fit:] == U64(0xA5A5A5A5A5A5A5A5)).all(), "written past min(nout, merged_cap)"
        return rc, merged[:fit], tuple(int(x) for x in st)


def sizes(host: Host):
    """0, 1, 2, 63, 64, 65 and T - 1, T, T + 1, 2T + 1 for the sort's and the scan's tile."""
    s = [0, 1, 2, 63, 64, 65]
    for t in (host.scan_tile, host.sort_tile):
        s += [t - 1, t, t + 1, 2 * t + 1]
    return sorted(set(s))


# --------------------------------------------------------------------------
# Range families: name -> function of (n, rng) -> uint64 [n, 2]
# --------------------------------------------------------------------------
def _one_byte(byte):
    def make(n, rng):
        base = U64(0x1111111111111111) & ~(U64(0xFF) << U64(8 * byte))
        low = base | (rng.integers(0, 256, n, dtype=U64) << U64(8 * byte))
        return np.stack([low, low + U64(1) + rng.integers(0, 4, n, dtype=U64)], axis=1)
    return make


def _all_equal(n, rng):
    return np.stack([np.full(n, 1000, dtype=U64), U64(1001) + rng.integers(0, 256, n, dtype=U64)], axis=1)


def _descending(n, rng):
    low = U64(6) * np.arange(n, dtype=U64)[::-1]
    return np.stack([low, low + U64(1) + rng.integers(0, 9, n, dtype=U64)], axis=1)


def _touching_chain(n, rng):
    low = U64(10) * rng.permutation(n).astype(U64)
    return np.stack([low, low + U64(10)], axis=1)


def _gap_of_one_chain(n, rng):
    low = U64(10) * rng.permutation(n).astype(U64)
    return np.stack([low, low + U64(9)], axis=1)


def _wrapped_mixed(n, rng):
    low = rng.integers(0, 1 << 62, n, dtype=U64) >> rng.integers(0, 60, n, dtype=U64)
    high = low + rng.integers(1, 1 << 16, n, dtype=U64)
    pick = rng.integers(0, 7, n)
    high[pick == 0] = low[pick == 0]                                        # high == low
    high[pick == 1] = low[pick == 1] - rng.integers(0, 256, int((pick == 1).sum()), dtype=U64)   # wraps below
    return np.stack([low, high], axis=1)


def _sparse(n, rng):
    low = rng.integers(0, 1 << 40, n, dtype=U64)
    return np.stack([low, low + rng.integers(1, 1 << 20, n, dtype=U64)], axis=1)


FAMILIES = {f"byte{b}": _one_byte(b) for b in range(8)}
FAMILIES.update(all_equal=_all_equal, descending=_descending, touching_chain=_touching_chain,
                gap_of_one_chain=_gap_of_one_chain, wrapped_mixed=_wrapped_mixed, sparse=_sparse)


def family(name, n, seed=0):
    return as_ranges(FAMILIES[name](n, np.random.default_rng([seed, n, sorted(FAMILIES).index(name)])))


def tile_edge_extents(tile, tiles=3):
    """Extents of exactly `tile` touching ranges with a gap between: in sorted
    order every extent's head is a tile's first element and its last element a
    tile's last."""
    i = np.arange(tiles * tile, dtype=U64)
    low = U64(4) * i + (i // U64(tile)) * U64(100)
    return np.stack([low, low + U64(4)], axis=1)


def wide_over_tiles(tile, wide_last, seed=3):
    """[0, 2^40) and three tiles of small ranges inside it: the running maximum
    crosses the tiles, 1 extent.  The wide range is first in sorted order; in
    the input it comes first or last."""
    rng = np.random.default_rng(seed)
    low = rng.integers(1, (1 << 40) - (1 << 21), 3 * tile, dtype=U64)
    small = np.stack([low, low + rng.integers(1, 1 << 20, 3 * tile, dtype=U64)], axis=1)
    wide = np.array([[0, 1 << 40]], dtype=U64)
    return as_ranges(np.concatenate([small, wide] if wide_last else [wide, small]))
