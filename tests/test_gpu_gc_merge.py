"""GPU: the GC range merge (include/pom_gc.h) against the model of
gc_merge_util.py -- pom_gc_merge_dev on guarded arenas with in, out, stat and
scratch at shifted 8-byte residues, pom_gc_scan_dev and pom_gc_merge_dev
chained on one stream, and pom_gc_stat_batch through the host chunk pipeline
against pom_gc_scan_batch and the model."""
from __future__ import annotations

import numpy as np
import pytest

from gc_merge_util import E_NOSPACE, FAMILIES, U64, Host, as_ranges, family, model, sizes, tile_edge_extents, \
    wide_over_tiles
from gc_scan_util import expect_batch, lzo_record, make_record
from gpu_util import assert_guards, guarded_batch
from pomegranate_amd import gc, itb, lzo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H = itb.ITBH_SIZE
FILL = 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


@pytest.fixture(autouse=True)
def _needs_gpu(dev):
    """The host batches pick the device themselves; without one they skip too."""


@pytest.fixture(scope="module")
def host():
    return Host()


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


def payload_of(rec) -> bytes:
    return bytes(rec[H: itb.header_fields(rec)[0]])


# ---------------------------------------------------------------------------
# pom_gc_merge_dev on guarded arenas
# ---------------------------------------------------------------------------
def merge_dev_once(dev, ranges, cap="nout", shifts=(8, 8, 8, 0), want=None):
    """One call with in, scratch, out and stat at shifts[0 .. 3] mod 16 inside
    arenas of guard bytes; in and every byte outside scratch, stat and
    out[0, min(nout, cap)) are checked afterwards; the result is compared with
    the model."""
    r = as_ranges(ranges)
    n = len(r)
    want = model(r) if want is None else want
    cap = {"nout": want.nout, "nout-1": max(want.nout - 1, 0), "zero": 0, "n": n}[cap]
    nscr = gc.merge_scratch_bytes(n)
    src = guarded_batch(torch, [r.tobytes()], dev, [shifts[0]], fill=0xEE)
    dst = guarded_batch(torch, [nscr, 16 * cap, 40], dev, list(shifts[1:]), fill=FILL)
    before = src.arena.cpu().numpy().copy()

    def view(batch, i, dtype):
        o, k = int(batch.host_off[i]), int(batch.host_len[i])
        t = batch.arena[o: o + k].view(dtype)
        return t if dtype == torch.uint8 or k == 40 else t.view(k // 16, 2)
    gc.merge_dev(view(src, 0, torch.int64), n, view(dst, 0, torch.uint8), view(dst, 1, torch.int64),
                 view(dst, 2, torch.int64), out_cap=cap)
    torch.cuda.synchronize()
    assert (src.arena.cpu().numpy() == before).all(), "in, or its neighbourhood, was modified"
    fit = min(want.nout, cap)
    arena = assert_guards(dst, [nscr, 16 * fit, 40], FILL)
    o_out, o_stat = int(dst.host_off[1]), int(dst.host_off[2])
    stat = tuple(int(x) for x in arena[o_stat: o_stat + 40].view(U64))
    assert stat == want.stat
    out = arena[o_out: o_out + 16 * fit].view(U64).reshape(-1, 2)
    assert (out == want.out[:fit]).all()
    return want


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_dev_families_every_size(dev, host, name):
    """Keys that differ in one byte only (one family per byte), all equal,
    descending, chains that collapse or stay, wrapped ranges mixed in: at 0, 1,
    2, 63, 64, 65 and around both tiles."""
    for k, n in enumerate(sizes(host)):
        merge_dev_once(dev, family(name, n), shifts=[(0, 8, 8, 0), (8, 8, 0, 8), (8, 0, 8, 8)][k % 3])


@pytest.mark.parametrize("which", ["scan", "sort"])
def test_dev_heads_and_lasts_at_tile_edges(dev, host, which):
    r = tile_edge_extents(host.scan_tile if which == "scan" else host.sort_tile)
    assert merge_dev_once(dev, r).nout == 3
    assert merge_dev_once(dev, r[::-1]).nout == 3
    assert merge_dev_once(dev, r[1:]).nout == 3


@pytest.mark.parametrize("wide_last", [False, True])
def test_dev_running_maximum_crosses_tiles(dev, host, wide_last):
    for tile in (host.scan_tile, host.sort_tile):
        want = merge_dev_once(dev, wide_over_tiles(tile, wide_last))
        assert want.nout == 1 and want.valid == 1 << 40


@pytest.mark.parametrize("cap", ["zero", "nout-1", "nout", "n"])
def test_dev_out_cap(dev, host, cap):
    """Nothing is written at or past out_cap, nor past nout; stat is complete anyway."""
    for name in ("sparse", "wrapped_mixed", "gap_of_one_chain"):
        merge_dev_once(dev, family(name, 2 * host.scan_tile + 1), cap=cap)


def test_dev_only_wrapped_and_the_largest_key(dev):
    assert merge_dev_once(dev, [[5, 5], [9, 3], [2**64 - 1, 0]]).stat == (0, 0, 0, 3, 3)
    assert merge_dev_once(dev, [[2**64 - 2, 2**64 - 1], [7, 7]]).nout == 1


def test_dev_carry_loop_of_the_aggregates(dev, host):
    """More tile aggregates than the aggregates' workgroup is wide: its carry
    loop runs twice."""
    n = host.agg_threads * host.scan_tile + 3 * host.scan_tile + 5
    want = merge_dev_once(dev, family("sparse", n))
    assert want.nout > 1000


def test_dev_refusals(dev):
    """Too little scratch, and scratch off the 8-byte grid: -1, nothing launched."""
    r = torch.zeros((100, 2), dtype=torch.int64, device=dev)
    out = torch.zeros((100, 2), dtype=torch.int64, device=dev)
    stat = torch.full((5,), 7, dtype=torch.int64, device=dev)
    scratch = torch.zeros(gc.merge_scratch_bytes(100) + 8, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError):
        gc.merge_dev(r, 100, scratch[: gc.merge_scratch_bytes(100) - 1], out, stat)
    with pytest.raises(RuntimeError):
        gc.merge_dev(r, 100, scratch[4:], out, stat)
    with pytest.raises(ValueError):
        gc.merge_scratch_bytes((1 << 30) + 1)
    assert gc._lib().pom_gc_merge_scratch((1 << 30) + 1) == 0
    assert gc._lib().pom_gc_merge_dev(None, (1 << 30) + 1, None, 1 << 40, None, 0, None, None) == -1
    torch.cuda.synchronize()
    assert (stat.cpu().numpy() == 7).all()


# ---------------------------------------------------------------------------
# pom_gc_scan_dev and pom_gc_merge_dev chained on one stream
# ---------------------------------------------------------------------------
def log_columns(rng, n_ites, at, wraps=False):
    """Columns as an append log writes them: each ITE's offset is where the one
    before ended (high = offset + len + 1, so neighbours touch), with an
    empty column (no range) or a gap now and then.  Returns ({nr: six
    columns}, the log's end)."""
    cols = {}
    for nr in range(n_ites):
        pick = int(rng.integers(0, 12))
        ln = 0 if pick == 0 else int(rng.integers(1, 5000))
        off = at
        if wraps and pick == 1:
            off, ln = 2**64 - 5, 10                     # offset + len + 1 wraps: a dropped range
        elif ln:
            at += ln + 1 + (int(rng.integers(1, 100)) if pick == 2 else 0)
        cols[nr] = [(ln, off)] * 6
    return cols, at


@pytest.fixture(scope="module")
def log_records(oracle):
    """40 records of one append log, 20 ... 76 ITEs each, in shuffled order,
    stored and LZO mixed; some ranges wrap."""
    rng = np.random.default_rng(77)
    recs, at = [], 4096
    for i in range(40):
        n_ites = 20 + 7 * (i % 9)
        cols, at = log_columns(rng, n_ites, at, wraps=True)
        recs.append(make_record(1200 + i, n_ites, 8, range(0, n_ites, 2 if i % 5 == 0 else 1), columns=cols))
    order = rng.permutation(40)
    recs = [recs[i] for i in order]
    stored = [r if i % 4 == 1 else lzo_record(oracle, r) for i, r in enumerate(recs)]
    return recs, stored


def test_scan_and_merge_chained(dev, log_records):
    recs = log_records[0][:16]
    payloads = [payload_of(r) for r in recs]
    src = guarded_batch(torch, payloads, dev, list(range(16)), fill=0xEE)
    column = 2
    _, _, first, ranges = expect_batch(payloads, [8] * 16, column)
    total = int(first[16])
    want = model(ranges)
    assert total > 300 and 1 < want.nout < total // 2 and want.nwrapped > 0
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device=dev)
    live, nranges, err = i32(16), i32(16), i32(16)
    dfirst = torch.zeros(17, dtype=torch.int64, device=dev)
    dranges = torch.zeros((total, 2), dtype=torch.int64, device=dev)
    adepth = torch.full((16,), 8, dtype=torch.uint8, device=dev)
    scratch = torch.zeros(gc.merge_scratch_bytes(total), dtype=torch.uint8, device=dev)
    out = torch.zeros((total, 2), dtype=torch.int64, device=dev)
    stat = torch.zeros(5, dtype=torch.int64, device=dev)
    gc.scan_dev(src, adepth, column, live, nranges, dfirst, dranges, err)
    gc.merge_dev(dranges, total, scratch, out, stat)            # no wait in between: stream order
    torch.cuda.synchronize()
    assert (dranges.cpu().numpy().view(U64) == ranges).all()
    assert tuple(int(x) for x in stat.cpu().numpy().view(U64)) == want.stat
    assert (out.cpu().numpy().view(U64)[: want.nout] == want.out).all()


# ---------------------------------------------------------------------------
# pom_gc_stat_batch
# ---------------------------------------------------------------------------
def check_stat_batch(stored, payloads, column, seed=None, want_err=None, **kw):
    """Per ITB equal to pom_gc_scan_batch and the oracle walk; merged and stat
    equal to the model over the walk's ranges (and the seed)."""
    res = gc.stat_batch(stored, column, seed=seed, **kw)
    scan = gc.scan_batch(stored, column)
    for got, ref in ((res.live, scan.live), (res.err, scan.err), (res.len_ok, scan.len_ok),
                     (res.entries_ok, scan.entries_ok)):
        assert (got == ref).all()
    errs, lives, first, ranges = expect_batch(payloads, [8] * len(stored), column)
    for b in range(len(stored)):
        e = want_err[b] if errs[b] is None else errs[b]
        assert (int(res.err[b]), int(res.live[b])) == (e, lives[b]), b
    assert (scan.ranges == ranges).all()
    mine = model(ranges)
    want = mine if seed is None else model(np.concatenate([ranges, as_ranges(seed)]))
    assert res.stat == (want.valid, want.max, want.nout, mine.nin, mine.nwrapped)
    cap = kw.get("merged_cap")
    fit = want.nout if cap is None else min(cap, want.nout)
    assert res.rc == (E_NOSPACE if fit < want.nout else 0)
    assert res.merged.shape[0] == fit and (res.merged == want.out[:fit]).all()
    return res, want


def test_stat_batch_40_records(log_records, debug_env):
    recs, stored = log_records
    payloads = [payload_of(r) for r in recs]
    res, want = check_stat_batch(stored, payloads, 2)
    assert res.len_ok.all() and res.entries_ok.all()
    assert 1 < want.nout < want.nin // 2 and want.nwrapped > 0
    # several chunks (about 1.5 MB of records under a 1 MiB budget, a quarter of it for the first)
    debug_env("chunk_mb=1")
    res1, _ = check_stat_batch(stored, payloads, 2)
    assert res1.merged.tobytes() == res.merged.tobytes() and res1.stat == res.stat
    for column in (0, 5):
        check_stat_batch(stored, payloads, column)


def test_stat_batch_seed(log_records, debug_env):
    recs, stored = log_records
    payloads = [payload_of(r) for r in recs]
    _, base = check_stat_batch(stored, payloads, 2)
    assert base.nout >= 2
    # one extent bridging the first two of the batch, one far beyond, one below
    seed = [[1, 9], [int(base.out[0, 1]), int(base.out[1, 0])], [1 << 50, (1 << 50) + 5]]
    res, want = check_stat_batch(stored, payloads, 2, seed=seed)
    assert want.nout == base.nout + 1
    debug_env("chunk_mb=1")
    res1, _ = check_stat_batch(stored, payloads, 2, seed=seed)
    assert res1.merged.tobytes() == res.merged.tobytes()
    with pytest.raises(ValueError):
        gc.stat_batch(stored, 2, seed=[[50, 60], [20, 30]])
    with pytest.raises(ValueError):
        gc.stat_batch(stored, 2, seed=[[20, 30], [30, 40]])
    with pytest.raises(ValueError):
        gc.stat_batch(stored, 6)


def test_stat_batch_bad_record(log_records, oracle):
    """A record without a whole header and one whose LZO stream is cut short:
    their ranges are absent, their neighbours' are there."""
    import struct
    recs, stored = log_records[0], list(log_records[1])
    payloads = [payload_of(r) for r in recs]
    stored[7] = stored[7][:200]
    payloads[7] = None
    b = next(i for i in range(10, 40) if i % 4 != 1)            # an LZO record
    ln, zlen, _ = itb.header_fields(stored[b])
    cut = bytearray(stored[b][: ln - 9])
    struct.pack_into("<I", cut, itb.LEN_OFF, ln - 9)
    stored[b] = cut
    rc, _ = oracle.decompress_safe(bytes(cut[H:]), zlen - H)
    assert rc != 0
    payloads[b] = None
    res, want = check_stat_batch(stored, payloads, 2, want_err={7: -22, b: rc})
    whole = model(expect_batch([payload_of(r) for r in recs], [8] * 40, 2)[3])
    assert want.nin < whole.nin and want.valid < whole.valid


def test_stat_batch_capacity(log_records):
    recs, stored = log_records
    payloads = [payload_of(r) for r in recs]
    nout = model(expect_batch(payloads, [8] * 40, 2)[3]).nout
    res, _ = check_stat_batch(stored, payloads, 2, merged_cap=nout - 1)
    assert res.rc == E_NOSPACE and res.stat.nout == nout
    res, _ = check_stat_batch(stored, payloads, 2, merged_cap=nout)
    assert res.rc == 0
    check_stat_batch(stored, payloads, 2, merged_cap=0)


def test_stat_batch_nothing_to_merge():
    """No record reaches the GPU: the seed alone is folded."""
    res = gc.stat_batch([bytes(200)], 0, seed=[[5, 9]])
    assert res.rc == 0 and res.err.tolist() == [-22] and res.merged.tolist() == [[5, 9]]
    assert res.stat == (4, 9, 1, 0, 0)
    res = gc.stat_batch([], 0)
    assert res.rc == 0 and res.stat == (0, 0, 0, 0, 0)
