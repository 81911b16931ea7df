"""CPU: the grouped encoder's index arithmetic and selection rule
(pomegranate_amd/csrc/lzo1x_enc_group.h compiled as plain C++,
tests/native/enc_group_host.cc): for every grid 0..70 and the shapes 4+1, 8+1
and 8+2, every region has exactly one owner, no owner lies past the grid, the
workgroup count is the ceiling, only the last workgroup has idle waves, and
every parse slot has exactly one emit wave."""
from __future__ import annotations

import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
LIB = os.path.join(NATIVE, "libenc_group_host.so")
CHECK = os.path.join(NATIVE, "enc_group_check")
SHAPES = [(4, 1), (8, 1), (8, 2)]


class Walk(ctypes.Structure):
    _fields_ = [(name, ctypes.c_uint32) for name in
                ("workgroups", "owned", "multi", "past", "idle", "idle_outside_last", "slots_served",
                 "slots_unserved")]


@pytest.fixture(scope="module")
def harness():
    if not (os.path.exists(LIB) and os.path.exists(CHECK)):
        subprocess.run(["make", "-C", NATIVE, "-f", "enc_group.mk"], check=True)
    lib = ctypes.CDLL(LIB)
    u32 = ctypes.c_uint32
    lib.enc_group_workgroups_host.restype = u32
    lib.enc_group_workgroups_host.argtypes = [u32, u32]
    lib.enc_group_region_host.restype = u32
    lib.enc_group_region_host.argtypes = [u32, u32, u32]
    lib.enc_group_idle_host.restype = ctypes.c_int
    lib.enc_group_idle_host.argtypes = [u32, u32, u32, u32]
    lib.enc_group_use_host.restype = ctypes.c_int
    lib.enc_group_use_host.argtypes = [u32, u32, u32]
    lib.enc_group_walk_host.restype = ctypes.c_int
    lib.enc_group_walk_host.argtypes = [u32, u32, u32, ctypes.POINTER(Walk)]
    return lib


@pytest.mark.parametrize("group,emitters", SHAPES)
def test_every_grid_to_70(harness, group, emitters):
    for grid in range(71):
        r = Walk()
        assert harness.enc_group_walk_host(grid, group, emitters, ctypes.byref(r)) == 0
        ceil_wg = -(-grid // group)
        assert r.workgroups == ceil_wg, grid
        assert (r.owned, r.multi, r.past) == (grid, 0, 0), grid
        assert (r.idle, r.idle_outside_last) == (ceil_wg * group - grid, 0), grid
        assert (r.slots_served, r.slots_unserved) == (group, 0)


@pytest.mark.parametrize("group,emitters", SHAPES)
def test_owner_of_every_region(harness, group, emitters):
    """Region r belongs to wave r % group of workgroup r // group, and to no other."""
    for grid in (0, 1, group - 1, group, group + 1, 70):
        owners = {}
        for wg in range(harness.enc_group_workgroups_host(grid, group)):
            for w in range(group):
                if not harness.enc_group_idle_host(wg, w, group, grid):
                    owners.setdefault(harness.enc_group_region_host(wg, w, group), []).append((wg, w))
        assert owners == {r: [(r // group, r % group)] for r in range(grid)}


def test_selection_rule(harness):
    """Grouped only with a whole group and a workgroup for every CU."""
    use = harness.enc_group_use_host
    for group in (4, 8):
        for cus in (1, 2, 64, 256, 304):
            edge = group * (cus - 1) + 1             # the smallest grid of `cus` workgroups
            for regions in range(0, group * cus + 2 * group):
                want = regions >= group and regions >= edge
                assert bool(use(regions, group, cus)) == want, (regions, group, cus)
    assert not use(1, 4, 256) and not use(1020, 4, 256) and use(1021, 4, 256) and use(4096, 4, 256)


def test_standalone_checker(harness):
    """The same walk under AddressSanitizer and UBSan where they link
    (tests/native/enc_group.mk): a stand-alone program."""
    out = subprocess.run([CHECK], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "enc_group_check: ok" in out.stdout
