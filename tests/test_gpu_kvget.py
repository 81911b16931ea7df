"""GPU: the key/value point get (include/pom_kvget.h) against the Python
restatement of mds/itb.c:1095-1116, :1769-1814 and mds/cbht.c:929-977 in
kvget_util.py -- pom_kvget_dev on guarded arenas, pom_kvget_batch through the
host chunk pipeline.  err, nr, depth, len, lease, first[] and every record byte
are compared."""
from __future__ import annotations

import ctypes
import struct

import numpy as np
import pytest

import kvget_util as U
from gpu_util import guarded_batch
from pomegranate_amd import itb, kvget, lzo

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


@pytest.fixture
def debug_env(monkeypatch):
    def set_(value):
        monkeypatch.setenv("POM_LZO_DEBUG", value)      # (host_debug.c pom_dbg_str)
        lzo.debug_reload()
    yield set_
    monkeypatch.delenv("POM_LZO_DEBUG", raising=False)
    lzo.debug_reload()


@pytest.fixture(scope="module")
def families():
    """Every case family once, with the oracle's answer worked out:
    name -> (records, adepths, req, keys, want)."""
    fams = {}
    for name, fam in U.FAMILIES.items():
        recs, adepths, req, keys = fam()
        if name == "mixed":
            req = np.ascontiguousarray(req[np.random.default_rng(5).permutation(len(req))])
        fams[name] = (recs, adepths, req, keys, U.Want([U.payload_of(r) for r in recs], adepths, req, keys))
    return fams


# ---------------------------------------------------------------------------
# pom_kvget_dev on guarded arenas
# ---------------------------------------------------------------------------
class Outputs:
    """The six result arrays and out carved out of ONE arena of FILL bytes with
    guard bytes around each, so a stray store shows; out starts at residue
    `oshift` mod 16 and has exactly out_cap bytes."""

    def __init__(self, dev, nreq, oshift, out_cap):
        self.sizes = [("err", 4 * nreq), ("nr", 4 * nreq), ("depth", 4 * nreq), ("len", 4 * nreq),
                      ("lease", 8 * nreq), ("first", 8 * (nreq + 1)), ("out", out_cap)]
        self.at, pos = {}, 4096
        for name, nbytes in self.sizes:
            if name == "out":
                pos += oshift
            self.at[name] = (pos, nbytes)
            pos = (pos + nbytes + 4096 + 255) // 256 * 256
        self.arena = torch.full((pos,), FILL, dtype=torch.uint8, device=dev)
        assert self.arena.data_ptr() % 256 == 0 and self.at["out"][0] % 16 == oshift

    def view(self, name, dtype=torch.uint8):
        o, nbytes = self.at[name]
        return self.arena[o: o + nbytes].view(dtype)

    def results(self, nreq):
        """(err, nr, depth, len, lease, first, out bytes) on the host, after
        checking that nothing outside the six arrays and out[0, min(first[nreq],
        out_cap)) changed."""
        host = self.arena.cpu().numpy()
        cut = lambda name: host[self.at[name][0]: self.at[name][0] + self.at[name][1]]
        first = cut("first").view(np.uint64).copy()
        used = min(int(first[nreq]), self.at["out"][1])
        changed = host != FILL
        for name, nbytes in self.sizes:
            o = self.at[name][0]
            changed[o: o + (used if name == "out" else nbytes)] = False
        bad = np.flatnonzero(changed)
        assert len(bad) == 0, f"{len(bad)} bytes changed outside the outputs, first at arena byte {int(bad[0])} " \
                              f"(out is at {self.at['out'][0]}, {used} bytes used)"
        return (cut("err").view(np.int32), cut("nr").view(np.uint32), cut("depth").view(np.uint32),
                cut("len").view(np.uint32), cut("lease").view(np.uint64), first, cut("out")[:used].tobytes())


def get_dev_once(dev, recs, adepths, req, keys, shifts=None, kshift=0, oshift=0, status=None, continuation=None,
                 out_cap=None):
    payloads = [U.payload_of(r) for r in recs]
    shifts = [0] * len(recs) if shifts is None else shifts
    src = guarded_batch(torch, payloads, dev, shifts, fill=0xEE,
                        neighbours=None if continuation is None else "continuation", continuation=continuation)
    blob = guarded_batch(torch, [bytes(keys)], dev, [kshift], fill=0xEE)
    nreq = len(req)
    dreq = torch.from_numpy(np.ascontiguousarray(req).view(np.uint8).copy()).to(dev)
    adepth = torch.tensor(adepths, dtype=torch.uint8, device=dev)
    st = None if status is None else torch.tensor(status, dtype=torch.int32, device=dev)
    cap = U.REC_MAX * nreq if out_cap is None else out_cap
    out = Outputs(dev, nreq, oshift, cap)
    kvget.kvget_dev(src, adepth, dreq, nreq, blob.arena[int(blob.host_off[0]):], len(keys),
                    out.view("err", torch.int32), out.view("nr", torch.int32), out.view("depth", torch.int32),
                    out.view("len", torch.int32), out.view("lease", torch.int64), out.view("first", torch.int64),
                    out.view("out") if cap else None, cap, status=st)
    torch.cuda.synchronize()
    return out.results(nreq)


def both_copy_forms(debug_env, run, want, out_cap=None):
    """The granule emit and the per-lane byte copy (debug key kvget_copy=1):
    the oracle's bytes from both."""
    debug_env("kvget_copy=0")
    a = run()
    U.same(a, want, out_cap)
    debug_env("kvget_copy=1")
    b = run()
    U.same(b, want, out_cap)
    assert a[6] == b[6]


@pytest.mark.parametrize("family", ["values", "corners", "mixed"])
def test_dev_families(dev, families, debug_env, family):
    """v.len 0 ... 321 with and without every column; the matching corners and
    the chains of 8 and of 1,024 hops; the mixed batch with its runs of misses:
    payloads at residues of their own, the output aligned and at odd
    addresses, in both copy forms -- the same bytes."""
    recs, adepths, req, keys, want = families[family]
    shifts = [(3 * b + 1) % 16 for b in range(len(recs))]
    both_copy_forms(debug_env, lambda: get_dev_once(dev, recs, adepths, req, keys, shifts, 5, 0), want)
    both_copy_forms(debug_env, lambda: get_dev_once(dev, recs, adepths, req, keys, None, 0, 7), want)
    assert (want.err == 0).sum() > 30
    if family == "corners":
        assert want.depth.max() == 1024


def test_dev_handmade_tables(dev, families, debug_env):
    """Nothing past a UNIQUE slot that misses; OVERFLOW followed like CONFLICT;
    conflict 2048 ends as a miss; a self-loop and a 2-cycle return
    POM_LK_E_LOOP at depth 2048; an entry whose ITE ends past the payload, and
    entry 32,767, are POM_GC_E_TRUNCATED for that request only -- with the cut
    ITE's missing byte right behind the payload."""
    recs, adepths, req, keys, want = families["handmade"]
    whole = U.payload_of(recs[0])
    both_copy_forms(debug_env, lambda: get_dev_once(dev, recs, adepths, req, keys, [0, 9], 2, 0,
                                                    continuation=[b"", whole[-1:]]), want)
    U.same(get_dev_once(dev, recs, adepths, req, keys, [5, 0], 0, 3, continuation=[b"", whole[-1:]]), want)
    # (in the record one byte short the 2-cycle runs into the cut ITE 7 first)
    assert (want.err == U.E_LOOP).sum() == 4 and (want.depth[want.err == U.E_LOOP] == 2048).all()
    assert (want.err == U.E_TRUNCATED).sum() == 9 and (want.err == 0).sum() == 13


@pytest.mark.parametrize("shift", range(8))
def test_dev_string_keys_and_alignment(dev, families, shift):
    """sklen 0, 1, 7, 8, 9, 16, 17, 255, 256, 320 and 321 at every blob offset
    residue, the blob and the payload themselves at residue `shift`; the
    refusals (stray flag and kvflag bits, keys outside the blob)."""
    recs, adepths, req, keys, want = families["strkeys"]
    U.same(get_dev_once(dev, recs, adepths, req, keys, [shift], shift, (5 * shift) % 16), want)
    assert (want.err == U.EINVAL).sum() == 22 and (want.err == 0).sum() == 84


@pytest.mark.parametrize("nreq", [1, 2, 63, 64, 65, 129, 257])
def test_dev_buffer_contract(dev, families, debug_env, nreq):
    """Whole and partial waves: the poison around the six arrays and out
    stays, and out at residues 0, 8 and 1 holds identical bytes in both copy
    forms."""
    recs, adepths, req, keys, want = families["mixed"]
    pick = np.arange(nreq) * 3 % len(req)
    sub = want.pick(pick)
    assert (sub.err != 0).any() or nreq < 3
    outs = []
    for copy in (0, 1):
        debug_env(f"kvget_copy={copy}")
        outs += [get_dev_once(dev, recs, adepths, req[pick], keys, None, 0, oshift) for oshift in (0, 8, 1)]
    for got in outs:
        U.same(got, sub)
    assert all(got[6] == outs[0][6] for got in outs)


def test_dev_out_cap_cuts(dev, families, debug_env):
    """out is exactly out_cap bytes inside the poisoned arena: a cap inside a
    header, inside a value, inside a column, at a record's end and at 0 (no
    emit launch, out NULL)."""
    recs, adepths, req, keys, want = families["values"]
    r = 8 * 6 + 2                                       # v.len 28 with column 1: 72 bytes
    f = int(want.first[r])
    assert want.len[r] == 72
    for cap in (0, f + 7, f + 25, f + 48 + 5, f + 72, int(want.first[-1]) - 1):
        for oshift in (0, 5):
            both_copy_forms(debug_env, lambda: get_dev_once(dev, recs, adepths, req, keys, [2], 0, oshift, out_cap=cap),
                            want, cap)


def test_dev_rule_order_status_and_itb_range(dev):
    recs, adepths, status, req, keys = U.rule_order_case()
    want = U.Want([U.payload_of(r) for r in recs], adepths, req, keys, status)
    U.same(get_dev_once(dev, recs, adepths, req, keys, [1, 2, 3, 4, 5], 1, 0, status=status), want)
    assert want.err.tolist() == [0, U.EINVAL, -6, -6, -5, -5, U.E_TRUNCATED, U.E_TRUNCATED] + [U.EINVAL] * 6


def test_dev_many_requests_grid_stride(dev, families):
    """600,000 requests over the mixed batch: more waves than the capped grid
    holds (2,048 workgroups of 4), so the grid stride and the multi-tile prefix
    run."""
    recs, adepths, req, keys, want = families["mixed"]
    n = 600_000
    pick = np.arange(n) % len(req)
    total = int(want.len.astype(np.uint64)[pick].sum())
    got = get_dev_once(dev, recs, adepths, req[pick], keys, None, 3, 0, out_cap=total)
    for g, w, what in zip(got[:5], (want.err, want.nr, want.depth, want.len, want.lease),
                          ("err", "nr", "depth", "len", "lease")):
        assert (np.asarray(g) == w[pick]).all(), what
    first = np.zeros(n + 1, np.uint64)
    first[1:] = np.cumsum(want.len.astype(np.uint64)[pick])
    assert (got[5] == first).all()
    reps, rest = divmod(n, len(req))
    assert got[6] == want.data * reps + want.pick(np.arange(rest)).data


# ---------------------------------------------------------------------------
# pom_kvget_batch against the oracle
# ---------------------------------------------------------------------------
def stored_mix(oracle, recs):
    """COMPR_LZO and COMPR_NONE alternately."""
    return [r if b % 3 == 1 else U.lzo_record(oracle, r) for b, r in enumerate(recs)]


def same_batch(res, want, out_cap=None):
    U.same((res.err, res.nr, res.depth, res.len, res.lease, res.first, b"" if res.out is None else res.out.tobytes()),
           want, out_cap)


def test_batch_mixed(oracle, families):
    """24 records, adepth 1 ... 10, LZO and stored, and one record no request
    names (a stream that cannot be decoded: it is never uploaded)."""
    recs, adepths, req, keys, want = families["mixed"]
    stored = stored_mix(oracle, recs)
    unnamed = U.lzo_record(oracle, recs[4])
    unnamed[H + 5: H + 40] = bytes(35)
    res = kvget.kvget_batch(stored + [unnamed], req, keys)
    assert res.rc == 0
    same_batch(res, want)
    r = int(np.flatnonzero(want.err == 0)[0])
    assert res.record(r) == want.recs[r]


@pytest.mark.parametrize("family", ["values", "strkeys", "corners", "handmade"])
def test_batch_families(oracle, families, family):
    recs, adepths, req, keys, want = families[family]
    same_batch(kvget.kvget_batch([U.lzo_record(oracle, r) for r in recs], req, keys), want)
    same_batch(kvget.kvget_batch(recs, req, keys), want)


def test_batch_errors_stay_local(oracle, families):
    """A malformed stream gives its requests the decoder's code, a bad adepth
    and itb >= n give -EINVAL; the other ITBs' requests are unaffected."""
    recs, adepths, req, keys, want = families["mixed"]
    stored = stored_mix(oracle, recs)
    ln, zlen, _ = itb.header_fields(stored[2])
    cut = bytearray(stored[2][: ln - 9])
    struct.pack_into("<I", cut, itb.LEN_OFF, ln - 9)
    rc, _ = oracle.decompress_safe(bytes(cut[H:]), zlen - H)
    assert rc != 0
    stored[2] = cut
    stored[5] = bytearray(stored[5])
    stored[5][3] = 11                                   # adepth
    stored[6] = bytearray(stored[6])
    stored[6][3] = 0
    req = req.copy()
    far = np.flatnonzero(req["itb"] == 10)
    req["itb"][far[:3]] = [len(stored), len(stored) + 5, 0xFFFFFFFF]
    err = want.err.copy()
    for b, code in ((2, rc), (5, U.EINVAL), (6, U.EINVAL)):
        err[req["itb"] == b] = code
    err[far[:3]] = U.EINVAL
    lost = err != want.err
    assert lost.sum() > 30
    w = want.pick(np.arange(len(req)))
    w.err = err
    for a in (w.nr, w.depth, w.len, w.lease):
        a[lost] = 0
    w.recs = [b"" if lost[r] else rec for r, rec in enumerate(w.recs)]
    w.first[1:] = np.cumsum(w.len.astype(np.uint64))
    w.data = b"".join(w.recs)
    same_batch(kvget.kvget_batch(stored, req, keys), w)


def test_batch_itbid_check_and_just_split(oracle):
    """itbid_check: a key whose bits above 10 do not select h.itbid is -ESPLIT
    with depth 0 and no walk; a miss on a JUST_SPLIT record is -ESPLIT."""
    ka = [0x400 * 5 + nr for nr in range(8)]
    a = U.make_table(8600, 8, 3, ka)
    a[U.L.ITBH_DEPTH] = 3
    struct.pack_into("<Q", a, U.L.ITBH_ITBID, 5)
    kb = U.L.spread_hashes(78, 8)
    b = U.make_table(8601, 8, 3, kb)
    b[U.L.ITBH_FLAG] = U.ITB_JUST_SPLIT
    rows = [(k, 0, U.GET, U.KV_NORMAL, 0, 0) for k in ka] + [(k, 1, U.GET, U.KV_NORMAL, 0, 0) for k in kb]
    rows += [(kb[3] ^ (1 << 40), 1, U.GET, U.KV_NORMAL, 0, 0), (ka[2] ^ (1 << 40), 0, U.GET, U.KV_NORMAL, 0, 0),
             (ka[1] ^ 0x400, 0, U.GET, U.KV_NORMAL, 0, 0)]                  # itbid 4
    req = U.rows_to_req(rows)
    want = U.Want([U.payload_of(a), U.payload_of(b)], [3, 3], req, b"")
    assert want.err[-3:].tolist() == [U.ENOENT] * 3
    want.err[16] = U.ESPLIT
    stored = [U.lzo_record(oracle, a), b]
    same_batch(kvget.kvget_batch(stored, req), want)
    # with the check on: the last request does not walk (the one before it still has itbid 5)
    want.err[-1], want.depth[-1] = U.ESPLIT, 0
    same_batch(kvget.kvget_batch(stored, req, itbid_check=True), want)
    # ... and an ITB all of whose requests fail the check is not decoded at all
    damaged = bytearray(stored[0])
    damaged[H + 5: H + 40] = bytes(35)
    res = kvget.kvget_batch([damaged, b], req[-1:], itbid_check=True)
    assert (res.err.tolist(), res.depth.tolist(), res.len.tolist(), int(res.first[1])) == ([U.ESPLIT], [0], [0], 0)


def test_batch_nospace_then_sized_and_lengths_only(oracle, families):
    """POM_GC_E_NOSPACE with first[] and the per-request arrays complete and
    only out[0, out_cap) written; a second call sized by first[nreq]; out ==
    NULL returns the lengths alone."""
    recs, adepths, req, keys, want = families["values"]
    stored = [U.lzo_record(oracle, r) for r in recs]
    total = int(want.first[-1])
    for cap in (0, 1, int(want.first[50]) + 25, total - 1):
        res = kvget.kvget_batch(stored, req, keys, out_cap=cap)
        assert res.rc == U.E_NOSPACE
        same_batch(res, want, cap)
    res = kvget.kvget_batch(stored, req, keys, out_cap=int(res.first[-1]))
    assert res.rc == 0
    same_batch(res, want)
    res = kvget.kvget_batch(stored, req, keys, lengths_only=True)
    assert res.rc == 0 and res.out is None
    same_batch(res, want, 0)
    # the raw call: the poison behind out_cap stays
    n, nreq, cap = len(stored), len(req), int(want.first[50]) + 25
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    out = np.full(total + 64, 7, dtype=np.uint8)
    first = np.zeros(nreq + 1, np.uint64)
    err = np.zeros(nreq, np.int32)
    nr, depth, ln = (np.zeros(nreq, np.uint32) for _ in range(3))
    lease = np.zeros(nreq, np.uint64)
    rc = kvget._lib().pom_kvget_batch(ptrs, lens, n, 0, req.ctypes.data, nreq, None, 0, out.ctypes.data, cap,
                                      first.ctypes.data, err.ctypes.data, nr.ctypes.data, depth.ctypes.data,
                                      ln.ctypes.data, lease.ctypes.data)
    assert rc == U.E_NOSPACE and out[:cap].tobytes() == want.data[:cap] and (out[cap:] == 7).all()


@pytest.fixture(scope="module")
def chunky(oracle):
    """60 records of about 50 KB, every fourth stored uncompressed, with
    shuffled requests to all of them: several chunks under chunk_mb=1.
    (stored, req, keys, want)."""
    recs, rows, blob = [], [], U.Blob()
    rng = np.random.default_rng(12)
    for b in range(60):
        n_ites = 60 + 7 * (b % 9)
        keys_of = U.L.spread_hashes(950 + b, n_ites)
        kv = {nr: dict(flags=U.KV_STR, klen=5 + nr % 9, vlen=int(rng.integers(9, 120))) for nr in range(1, n_ites, 3)}
        rec = U.make_table(8700 + b, n_ites, 8, keys_of, kv)
        recs.append(rec)
        for nr in range(b % 4, n_ites, 4):
            _, _, key, klen, value = U.kv_fields(rec, nr)
            if nr in kv:
                rows.append((key, b, U.GET, U.KV_STR, blob.put(value[:klen]), klen))
            else:
                rows.append((key, b, U.GET | U.F_COLUMN, U.KV_NORMAL | nr % 6, 0, 0))
        rows.append((keys_of[b % n_ites] ^ (1 << 33), b, U.GET, U.KV_NORMAL, 0, 0))
    req = U.rows_to_req(rows)
    req = np.ascontiguousarray(req[np.random.default_rng(11).permutation(len(req))])
    keys = bytes(blob.bytes)
    want = U.Want([U.payload_of(r) for r in recs], [8] * 60, req, keys)
    return [r if b % 4 == 1 else U.lzo_record(oracle, r) for b, r in enumerate(recs)], req, keys, want


def test_batch_spans_chunks(chunky, debug_env, monkeypatch):
    """chunk_mb=1: about 50 KB a record, so 60 records take several chunks, on
    one GPU and on every visible one; the chunks reorder the blocks (smallest
    first, LZO before stored) and the records still come packed in request
    order."""
    stored, req, keys, want = chunky
    debug_env("chunk_mb=1")
    same_batch(kvget.kvget_batch(stored, req, keys), want)
    monkeypatch.setenv("POM_LZO_DEVICES", "0")
    same_batch(kvget.kvget_batch(stored, req, keys), want)


def test_batch_failed_chunk(chunky, debug_env):
    """fail_chunk=1: the device's second chunk delivery fails as a failed GPU
    stream would.  The call returns LZO_E_ERROR; a request either reads
    LZO_E_ERROR with no record or has the unfailed run's result, and both
    kinds occur; the same call succeeds in full afterwards."""
    stored, req, keys, want = chunky
    debug_env("chunk_mb=1,fail_chunk=1")
    with pytest.raises(RuntimeError, match=str(lzo.LZO_E_ERROR)):
        kvget.kvget_batch(stored, req, keys)
    n, nreq = len(stored), len(req)
    bufs = [np.frombuffer(r, dtype=np.uint8) for r in stored]
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    blob = np.frombuffer(keys, dtype=np.uint8)
    total = int(want.first[-1])
    out = np.full(total + 16, 7, dtype=np.uint8)
    first = np.zeros(nreq + 1, np.uint64)
    err = np.full(nreq, 7, np.int32)
    nr, depth, ln = (np.full(nreq, 7, np.uint32) for _ in range(3))
    lease = np.full(nreq, 7, np.uint64)
    rc = kvget._lib().pom_kvget_batch(ptrs, lens, n, 0, req.ctypes.data, nreq, blob.ctypes.data, len(keys),
                                      out.ctypes.data, total, first.ctypes.data, err.ctypes.data, nr.ctypes.data,
                                      depth.ctypes.data, ln.ctypes.data, lease.ctypes.data)
    assert rc == lzo.LZO_E_ERROR
    lost = err == lzo.LZO_E_ERROR
    assert 0 < lost.sum() < nreq and not ln[lost].any() and not lease[lost].any() and not nr[lost].any()
    kept = np.flatnonzero(~lost)
    w = want.pick(kept)
    assert (err[kept] == w.err).all() and (ln[kept] == w.len).all() and (lease[kept] == w.lease).all()
    assert (first[1:] == np.cumsum(ln.astype(np.uint64))).all()
    assert out[: int(first[-1])].tobytes() == w.data and (out[int(first[-1]):] == 7).all()
    debug_env("chunk_mb=1")
    same_batch(kvget.kvget_batch(stored, req, keys), want)
