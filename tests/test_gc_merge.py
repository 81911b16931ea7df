"""CPU: the GC range merge (pomegranate_amd/csrc/gc_merge.h, gc_fold.c) against
the model of gc_merge_util.py, itself checked against the reference's range
tree (tests/golden/brt_ranges.json).  gc_merge.h runs here as plain C++
(tests/native/libgc_merge_host.so, gc_merge_check); the kernels that compile
the same header run in test_gpu_gc_merge.py.  Two deliberately wrong headers
show that these tests bite."""
from __future__ import annotations

import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gc_merge_util import (CHECK, EINVAL, E_NOSPACE, FAMILIES, U64, Host, as_ranges, build_native, family, model,
                           sizes, tile_edge_extents, wide_over_tiles)

GOLDEN = os.path.join(ROOT, "tests", "golden", "brt_ranges.json")
CSRC = os.path.join(ROOT, "pomegranate_amd", "csrc")


@pytest.fixture(scope="module")
def host():
    build_native()
    return Host()


def check(host, ranges, caps=("nout",)):
    """The host composition equals the model, for each out_cap."""
    want = model(ranges)
    for cap in caps:
        cap = {"nout": want.nout, "nout-1": max(want.nout - 1, 0), "zero": 0}[cap]
        rc, out, stat = host.merge(ranges, cap)
        assert rc == 0
        assert stat == want.stat
        assert (out == want.out[:cap]).all()
    return want


# ---------------------------------------------------------------------------
# The model against the reference
# ---------------------------------------------------------------------------
def test_golden_covers_the_kinds():
    cases = json.load(open(GOLDEN))["cases"]
    assert len(cases) >= 190 and os.path.getsize(GOLDEN) < 100_000
    assert {c["kind"] for c in cases} >= {"touching", "gap_of_one", "nested", "identical", "one_covers_all",
                                          "descending", "equal_low", "dense", "sparse"}
    for c in cases:
        r = as_ranges(c["in"])
        assert (r[:, 1] > r[:, 0]).all()                # no wrapped range: the reference is undefined there


def test_model_equals_reference_tree():
    for c in json.load(open(GOLDEN))["cases"]:
        got = model(c["in"])
        assert got.out.tolist() == as_ranges(c["out"]).tolist(), c["kind"]
        assert (got.valid, got.max, got.nwrapped) == (c["valid"], c["max"], 0)


def test_host_equals_reference_tree(host):
    for c in json.load(open(GOLDEN))["cases"]:
        rc, out, stat = host.merge(c["in"])
        assert rc == 0 and out.tolist() == as_ranges(c["out"]).tolist()
        assert stat[:3] == (c["valid"], c["max"], len(c["out"]) // 2)


# ---------------------------------------------------------------------------
# gc_merge.h on the CPU
# ---------------------------------------------------------------------------
def test_constants(host):
    assert host.sort_tile >= 256 and host.scan_tile >= 256 and host.agg_threads >= 64 and host.max_n == 1 << 30


@pytest.mark.parametrize("byte", range(8))
def test_keys_differ_in_one_byte(host, byte):
    """Only pass `byte` of the radix sort has anything to order (bytes 7: bits
    at and above 2^56)."""
    for n in sizes(host):
        want = check(host, family(f"byte{byte}", n))
        assert byte == 0 or n < 64 or want.nout > 1        # (byte 0: the neighbours touch)


@pytest.mark.parametrize("name", ["all_equal", "descending", "sparse"])
def test_families_every_size(host, name):
    for n in sizes(host):
        check(host, family(name, n))


def test_touching_chain_collapses(host):
    for n in sizes(host):
        want = check(host, family("touching_chain", n))
        assert want.nout == min(n, 1)


def test_gap_of_one_chain_stays(host):
    for n in sizes(host):
        want = check(host, family("gap_of_one_chain", n))
        assert want.nout == n


@pytest.mark.parametrize("which", ["scan", "sort"])
def test_heads_and_lasts_at_tile_edges(host, which):
    """Every extent's head is a tile's first element, its last element a tile's last."""
    tile = host.scan_tile if which == "scan" else host.sort_tile
    r = tile_edge_extents(tile)
    assert check(host, r).nout == 3
    assert check(host, r[::-1]).nout == 3
    assert check(host, r[1:]).nout == 3                 # and one off


@pytest.mark.parametrize("wide_last", [False, True])
def test_running_maximum_crosses_tiles(host, wide_last):
    for tile in (host.scan_tile, host.sort_tile):
        want = check(host, wide_over_tiles(tile, wide_last))
        assert want.nout == 1 and want.valid == 1 << 40


def test_wrapped_ranges_are_dropped(host):
    for n in sizes(host):
        want = check(host, family("wrapped_mixed", n))
        assert n < 64 or 0 < want.nwrapped < n
    only = as_ranges([[5, 5], [9, 3], [2**64 - 1, 0]])
    assert check(host, only).stat == (0, 0, 0, 3, 3)
    top = as_ranges([[2**64 - 2, 2**64 - 1], [7, 7]])   # the largest key a kept range can have
    assert check(host, top).out.tolist() == [[2**64 - 2, 2**64 - 1]]


@pytest.mark.parametrize("cap", ["zero", "nout-1", "nout"])
def test_out_cap(host, cap):
    for name in ("sparse", "wrapped_mixed", "gap_of_one_chain"):
        check(host, family(name, 2 * host.scan_tile + 1), caps=(cap,))


def test_carry_loop_of_the_aggregates(host):
    """More tile aggregates than the aggregates' pass is wide."""
    n = host.agg_threads * host.scan_tile + 3 * host.scan_tile + 5
    check(host, family("sparse", n))


def test_refuses_more_than_the_bound(host):
    assert host.lib.gc_merge_host(None, host.max_n + 1, None, 0, None) == -1


def test_gc_merge_check_program():
    """gc_merge.h and the fold against the checker's own naive merge, under
    AddressSanitizer and UBSan where they link."""
    build_native()
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    m = re.search(r"gc_merge_check: (\d+) checks ok", r.stdout)
    assert m and int(m.group(1)) > 1000


# ---------------------------------------------------------------------------
# The host fold (gc_fold.c)
# ---------------------------------------------------------------------------
def chunk_maps(ranges, cuts):
    parts = np.split(as_ranges(ranges), cuts)
    return [model(p).out for p in parts]


def test_fold_no_seed(host):
    r = family("sparse", 3000)
    want = model(r)
    for cuts in ([], [1000], [10, 11, 2500], [0, 3000]):
        maps = chunk_maps(r, cuts)
        for order in (maps, maps[::-1]):
            rc, merged, stat = host.fold(order)
            assert rc == 0 and (merged == want.out).all()
            assert stat == (want.valid, want.max, want.nout, 0, 0)
    rc, merged, stat = host.fold([])
    assert (rc, len(merged), stat) == (0, 0, (0, 0, 0, 0, 0))


def test_fold_seed_bridges_two_chunk_extents(host):
    a, b = as_ranges([[0, 10], [100, 110]]), as_ranges([[20, 30], [200, 210]])
    rc, merged, stat = host.fold([a, b], seed=[[10, 20]])
    assert rc == 0 and merged.tolist() == [[0, 30], [100, 110], [200, 210]]
    assert stat == (50, 210, 3, 0, 0)
    rc, merged, stat = host.fold([a, b], seed=[[11, 20]])   # a gap of one does not bridge
    assert merged.tolist() == [[0, 10], [11, 30], [100, 110], [200, 210]]
    r = family("sparse", 500)
    seed = model(family("sparse", 80, seed=9)).out
    want = model(np.concatenate([r, seed]))
    rc, merged, stat = host.fold(chunk_maps(r, [100, 300]), seed=seed)
    assert rc == 0 and (merged == want.out).all() and stat[:3] == want.stat[:3]


def test_fold_bad_seed(host):
    m = [as_ranges([[0, 10]])]
    assert host.fold(m, seed=[[50, 60], [20, 30]])[0] == EINVAL         # unsorted
    assert host.fold(m, seed=[[20, 30], [30, 40]])[0] == EINVAL         # touching
    assert host.fold(m, seed=[[20, 30], [25, 40]])[0] == EINVAL         # overlapping
    assert host.fold(m, seed=[[20, 20]])[0] == EINVAL                   # empty extent
    assert host.fold(m, seed=[[20, 30], [31, 40]])[0] == 0


def test_fold_capacity(host):
    maps = chunk_maps(family("gap_of_one_chain", 100), [50])
    rc, merged, stat = host.fold(maps, merged_cap=99)
    assert rc == E_NOSPACE and len(merged) == 99 and stat[:3] == model(family("gap_of_one_chain", 100)).stat[:3]
    assert host.fold(maps, merged_cap=100)[0] == 0
    assert host.fold(maps, merged_cap=0)[0] == E_NOSPACE


# ---------------------------------------------------------------------------
# That the tests bite: two deliberately wrong headers
# ---------------------------------------------------------------------------
WRONG = {
    # heads by >= instead of >: touching ranges no longer merge
    "heads_ge": ("(i == 0 || key > runmax_before)", "(i == 0 || key >= runmax_before)"),
    # equal digits ranked in reverse inside a round: the scatter is not stable
    "unstable": ("return base + equal_before;", "return base + (equal_in_round - 1u - equal_before);"),
}


@pytest.mark.parametrize("which", sorted(WRONG))
def test_wrong_header_fails(which, tmp_path):
    """The checker and the directed cases fail against the wrong rule (how many
    of this file's tests fail is in DESIGN 3.18)."""
    old, new = WRONG[which]
    text = open(os.path.join(CSRC, "gc_merge.h")).read()
    assert text.count(old) == 1
    (tmp_path / "gc_merge.h").write_text(text.replace(old, new))
    build_native(out_dir=str(tmp_path), inc_dir=str(tmp_path))
    r = subprocess.run([str(tmp_path / "gc_merge_check"), "quick"], capture_output=True, text=True)
    assert r.returncode != 0 and "FAILED" in r.stderr
    wrong = Host(str(tmp_path / "libgc_merge_host.so"))
    bad = 0
    for name in sorted(FAMILIES):
        for n in (65, wrong.scan_tile + 1):
            ranges = family(name, n)
            try:
                rc, out, stat = wrong.merge(ranges)
            except AssertionError:
                bad += 1
                continue
            want = model(ranges)
            bad += not (rc == 0 and stat == want.stat and (out == want.out).all())
    assert bad >= 3, bad
