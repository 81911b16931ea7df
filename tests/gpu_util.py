"""Helpers for GPU tests: pack host blocks into device batches and run the
device-resident C-ABI (lzo_mi355x_compress_dev / _decompress_dev)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from pomegranate_amd import lzo


def _offsets(sizes, align=16):
    sizes = np.asarray(sizes, dtype=np.uint64)
    padded = (sizes + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    off = np.zeros(len(sizes), dtype=np.uint64)
    if len(sizes) > 1:
        off[1:] = np.cumsum(padded[:-1])
    total = int(padded.sum()) if len(sizes) else 0
    return off, total


def device_batch(torch, blocks: Sequence[bytes], dev, shift: int = 0):
    """Pack blocks (each 16-B aligned + shift) into one HBM arena."""
    sizes = [len(b) for b in blocks]
    off, total = _offsets([s + shift for s in sizes])
    off = off + np.uint64(shift)
    host = np.zeros(max(total + shift, 1), dtype=np.uint8)
    for b, o in zip(blocks, off):
        host[int(o): int(o) + len(b)] = np.frombuffer(b, dtype=np.uint8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return lzo.DeviceBatch(t(host), t(off.view(np.int64)),
                           t(np.asarray(sizes, np.uint32).view(np.int32)))


def empty_batch(torch, caps: Sequence[int], dev, fill: int = 0):
    off, total = _offsets(caps)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    arena = torch.full((max(total, 1),), fill, dtype=torch.uint8, device=dev)
    return lzo.DeviceBatch(arena, t(off.view(np.int64)),
                           t(np.asarray(caps, np.uint32).view(np.int32)))


def gpu_compress(torch, blocks: Sequence[bytes], dev, shift: int = 0, scratch: bool = False):
    """Device-batch compress.  Without scratch: the LDS-dictionary encoder;
    with scratch: the global-dictionary one-wave encoder the bench times
    (lzo1x_encode_gdict1_kernel)."""
    src = device_batch(torch, blocks, dev, shift)
    dst = empty_batch(torch, [lzo.worst_compress(len(b)) for b in blocks], dev, fill=0xA5)
    n = len(blocks)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    scr = torch.zeros(lzo.compress_scratch_bytes(n), dtype=torch.uint8, device=dev) if scratch else None
    lzo.compress_dev(src, dst, olen, st, scratch=scr)
    torch.cuda.synchronize()
    return fetch(dst, olen), st.cpu().numpy().tolist()


def gpu_decompress(torch, comps: Sequence[bytes], caps: Sequence[int], dev, shift: int = 0):
    src = device_batch(torch, comps, dev, shift)
    dst = empty_batch(torch, caps, dev, fill=0x5A)
    n = len(comps)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    nscr = lzo.decompress_scratch_bytes(n)
    scratch = torch.empty(max(nscr, 1), dtype=torch.uint8, device=dev) if nscr else None
    lzo.decompress_dev(src, dst, olen, st, scratch)
    torch.cuda.synchronize()
    outs = fetch(dst, olen, cap=caps)
    return outs, st.cpu().numpy().tolist(), dst


def gpu_decompress_fast(torch, comps: Sequence[bytes], caps: Sequence[int], dev):
    """gpu_decompress plus the number of blocks the throughput decoder handed
    to the exact decoder (the fallback list count at the head of scratch)."""
    src = device_batch(torch, comps, dev)
    dst = empty_batch(torch, caps, dev, fill=0x5A)
    n = len(comps)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    scratch = torch.zeros(lzo.decompress_scratch_bytes(n), dtype=torch.uint8, device=dev)
    lzo.decompress_dev(src, dst, olen, st, scratch)
    torch.cuda.synchronize()
    fallbacks = int(scratch[:4].view(torch.int32).item())
    return fetch(dst, olen, cap=caps), st.cpu().numpy().tolist(), fallbacks


def fetch(batch, olen, cap=None) -> List[bytes]:
    host = batch.arena.cpu().numpy()
    off = batch.off.cpu().numpy()
    ol = olen.cpu().numpy().astype(np.int64)
    res = []
    for i in range(len(off)):
        n = int(ol[i]) if cap is None else min(int(ol[i]), int(cap[i]))
        res.append(host[int(off[i]): int(off[i]) + n].tobytes())
    return res


def gpu_decompress_win(torch, comps: Sequence[bytes], caps: Sequence[int], dev, kind: str = "win",
                       src=None, dst=None):
    """The windowed decoder alone (lzo_mi355x_launch_decompress_win), without
    the exact decoder behind it.  Returns the outputs, statuses and the ids of
    the blocks it handed over (fallback list).  src / dst: the caller's own
    batches of comps / caps (guarded_batch) in place of the packed ones; the
    raw out_len of every block is left in dst.out_len."""
    import ctypes
    lib = lzo.load()
    fn = getattr(lib, f"lzo_mi355x_launch_decompress_{kind}")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 10 + [ctypes.c_uint32, ctypes.c_void_p]
    src = device_batch(torch, comps, dev) if src is None else src
    dst = empty_batch(torch, caps, dev, fill=0x5A) if dst is None else dst
    n = len(comps)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    head = torch.zeros(64, dtype=torch.int32, device=dev)
    ids = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    p = lambda x: x.data_ptr()
    rc = fn(p(src.arena), p(src.off), p(src.length), p(dst.arena), p(dst.off), p(dst.length),
            p(olen), p(st), p(head), p(ids), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    nfb = int(head[0].item())
    dst.out_len = olen.cpu().numpy().view(np.uint32).tolist()
    return fetch(dst, olen, cap=caps), st.cpu().numpy().tolist(), sorted(ids[:nfb].cpu().numpy().tolist())


def gpu_decompress_lat(torch, comps: Sequence[bytes], caps: Sequence[int], dev, group: int = 1,
                       src=None, dst=None):
    """The latency decoder (lzo1x_decode_lat.hip) alone, without the exact
    decoder behind it: one block per pipeline (group 1,
    lzo_mi355x_launch_decompress_lat) or up to `group` blocks side by side in
    one pipeline (lzo_mi355x_launch_decompress_lat_n).  Returns the outputs,
    statuses and the ids of the blocks it handed over; blocks outside its range
    (the launcher returns -1) are reported with status None.  src / dst: the
    caller's own batches of comps / caps (guarded_batch); the raw out_len of
    every block is left in dst.out_len."""
    import ctypes
    lib = lzo.load()
    one = lib.lzo_mi355x_launch_decompress_lat
    one.restype = ctypes.c_int
    one.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                    ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    many = lib.lzo_mi355x_launch_decompress_lat_n
    many.restype = ctypes.c_int
    many.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4 + \
        [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    sz = lib.lzo_mi355x_decompress_lat_scratch
    sz.restype = ctypes.c_size_t
    sz.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    szn = lib.lzo_mi355x_decompress_lat_scratch_n
    szn.restype = ctypes.c_size_t
    szn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    src = device_batch(torch, comps, dev) if src is None else src
    dst = empty_batch(torch, caps, dev, fill=0x5A) if dst is None else dst
    n = len(comps)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    head = torch.zeros(64, dtype=torch.int32, device=dev)
    ids = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    p = lambda x: x.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    soff = src.off.cpu().numpy().astype(np.uint64)
    doff = dst.off.cpu().numpy().astype(np.uint64)
    launched = [False] * n
    for g0 in range(0, n, group):
        g1 = min(n, g0 + group)
        if group == 1:
            z, cap = comps[g0], int(caps[g0])
            need = int(sz(len(z), cap)) if len(z) else 0
            scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            rc = one(p(src.arena) + int(soff[g0]), len(z), p(dst.arena) + int(doff[g0]), cap,
                     p(olen), p(st), p(head), p(ids), g0, p(scratch), need, s)
        else:
            so = np.ascontiguousarray(soff[g0:g1] - soff[g0])
            do = np.ascontiguousarray(doff[g0:g1] - doff[g0])
            zz = np.array([len(c) for c in comps[g0:g1]], dtype=np.uint32)
            cc = np.array([int(c) for c in caps[g0:g1]], dtype=np.uint32)
            need = int(szn(so.ctypes.data, zz.ctypes.data, cc.ctypes.data, g1 - g0))
            scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            rc = many(p(src.arena) + int(soff[g0]), so.ctypes.data, zz.ctypes.data,
                      p(dst.arena) + int(doff[g0]), do.ctypes.data, cc.ctypes.data, g1 - g0,
                      p(olen), p(st), p(head), p(ids), g0, p(scratch), need, s)
        torch.cuda.synchronize()
        for i in range(g0, g1):
            launched[i] = rc == 0
    nfb = int(head[0].item())
    sts = [x if ok else None for x, ok in zip(st.cpu().numpy().tolist(), launched)]
    dst.out_len = olen.cpu().numpy().view(np.uint32).tolist()
    return fetch(dst, olen, cap=caps), sts, sorted(ids[:nfb].cpu().numpy().tolist())


# ---------------------------------------------------------------------------
# Guarded batches: blocks at chosen residues mod 16 inside one allocation, with
# guard bytes around each, to see what a kernel touches outside its block.
# ---------------------------------------------------------------------------
GUARD_ENDS = 4096        # guard bytes before the first block and after the last


def guarded_batch(torch, blocks_or_caps, dev, shifts, fill, gap=64, neighbours=None,
                  continuation=None, ends=GUARD_ENDS):
    """A DeviceBatch in ONE allocation: block i at off[i] with off[i] % 16 ==
    shifts[i], at least `gap` guard bytes between consecutive blocks and `ends`
    (at least GUARD_ENDS) before the first and after the last, so that a stray
    access stays in memory the test owns (and shows, instead of faulting).

    blocks_or_caps: bytes objects (a source batch: the blocks' contents) or
    ints (a destination batch: capacities; the whole arena holds `fill`).
    neighbours (source batches) decides what the guard bytes hold: None
    (`fill`), "zero", "ff", "random" (seeded), or "continuation": the bytes
    right behind block i are continuation[i] (the guard grows to hold them),
    the rest `fill`.  The batch also carries host_off / host_len (numpy)."""
    n = len(blocks_or_caps)
    is_src = n > 0 and isinstance(blocks_or_caps[0], (bytes, bytearray))
    sizes = [len(b) if is_src else int(b) for b in blocks_or_caps]
    assert len(shifts) == n and all(0 <= s < 16 for s in shifts)
    assert neighbours in (None, "zero", "ff", "random", "continuation")
    assert (neighbours == "continuation") == (continuation is not None)
    assert ends >= GUARD_ENDS
    off = np.zeros(n, dtype=np.int64)
    pos = ends
    for i in range(n):
        o = (pos - shifts[i] + 15) // 16 * 16 + shifts[i]
        off[i] = o
        tail = len(continuation[i]) if continuation is not None else 0
        pos = o + sizes[i] + max(gap, tail)
    total = pos + ends
    if neighbours == "random":
        host = np.random.default_rng(0x6A5D).integers(0, 256, total, dtype=np.uint8)
    else:
        host = np.full(total, {"zero": 0, "ff": 0xFF}.get(neighbours, fill), dtype=np.uint8)
    if is_src:
        for i, b in enumerate(blocks_or_caps):
            o = int(off[i])
            host[o: o + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
            if continuation is not None:
                c = continuation[i]
                host[o + len(b): o + len(b) + len(c)] = np.frombuffer(bytes(c), dtype=np.uint8)
    assert (off % 16 == np.asarray(shifts, dtype=np.int64)).all()
    assert n == 0 or off[0] >= ends
    assert (off[1:] - (off[:-1] + np.asarray(sizes[:-1], dtype=np.int64)) >= gap).all()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    arena = t(host)
    assert arena.data_ptr() % 256 == 0           # offset alignment is address alignment
    batch = lzo.DeviceBatch(arena, t(off), t(np.asarray(sizes, np.uint32).view(np.int32)))
    batch.host_off = off
    batch.host_len = np.asarray(sizes, dtype=np.int64)
    return batch


def assert_guards(batch, written, fill):
    """Every byte of the batch's arena outside the union of [off[i], off[i] +
    written[i]) still equals `fill`.  written[i]: min(out_len, cap) of a
    finished block, cap of a block a speculative decoder handed over (it may
    have written anything inside its room, nothing outside).  Returns the
    arena (numpy) for the caller's own look at the blocks."""
    arena = batch.arena.cpu().numpy()
    off = batch.host_off
    cap = batch.host_len
    w = np.asarray(written, dtype=np.int64)
    assert len(w) == len(off) and (w >= 0).all() and (w <= cap).all()
    changed = arena != fill                      # one pass over the arena
    for o, k in zip(off.tolist(), w.tolist()):
        changed[o: o + k] = False
    bad = np.flatnonzero(changed)
    if len(bad):
        at = int(bad[0])
        i = int(np.searchsorted(off, at, side="right")) - 1
        msgs = []
        if i >= 0:
            msgs.append(f"{at - int(off[i] + w[i])} bytes past the end of block {i}'s {int(w[i])} written "
                        f"bytes (cap {int(cap[i])}, off % 16 = {int(off[i]) % 16})")
        if i + 1 < len(off):
            msgs.append(f"{int(off[i + 1]) - at} bytes before the start of block {i + 1}")
        raise AssertionError(f"{len(bad)} guard bytes changed, first at arena byte {at} "
                             f"(0x{int(arena[at]):02X}): " + "; ".join(msgs))
    return arena


def gpu_decompress_dev(torch, src, dst, dev, scratch: bool):
    """lzo_mi355x_decompress_dev on the caller's batches: without scratch every
    block takes the exact decoder, with it the throughput decoder the library
    (or its `decoder` debug key) picks, then the exact one.  Returns out_len,
    status (lists) and the fallback count at scratch byte 0 (None without)."""
    n = src.nblocks
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    scr = torch.zeros(lzo.decompress_scratch_bytes(n), dtype=torch.uint8, device=dev) if scratch else None
    lzo.decompress_dev(src, dst, olen, st, scr)
    torch.cuda.synchronize()
    fb = int(scr[:4].view(torch.int32).item()) if scratch else None
    return (olen.cpu().numpy().view(np.uint32).tolist(), st.cpu().numpy().tolist(), fb)


def gpu_decompress_fast_alone(torch, src, dst, dev):
    """The op-set throughput decoder alone (lzo_mi355x_launch_decompress_fast),
    without the exact decoder behind it, its pool sized as the library sizes
    it (one set per resident workgroup; larger batches start largest first).
    Returns out_len, status and the sorted ids of the blocks it handed over."""
    import ctypes
    lib = lzo.load()
    fn = lib.lzo_mi355x_launch_decompress_fast
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 13 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                            ctypes.c_void_p]
    lib.lzo_mi355x_fast_ops_bytes_per_block.restype = ctypes.c_size_t
    lib.lzo_mi355x_fast_resident_blocks.restype = ctypes.c_uint32
    n = src.nblocks
    resident = int(lib.lzo_mi355x_fast_resident_blocks())
    nsets = min(n, resident)
    olen = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.full((n,), 99, dtype=torch.int32, device=dev)
    head = torch.zeros(64 + 2048, dtype=torch.int32, device=dev)   # fallback count + pool counters
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    ring = torch.zeros(nsets, dtype=torch.int64, device=dev)
    ops = torch.empty(nsets * lib.lzo_mi355x_fast_ops_bytes_per_block(), dtype=torch.uint8, device=dev)
    order = torch.zeros(n, dtype=torch.int32, device=dev) if n > resident else None
    p = lambda t: t.data_ptr()
    rc = fn(p(src.arena), p(src.off), p(src.length), p(dst.arena), p(dst.off), p(dst.length),
            p(olen), p(st), p(head), p(ids), p(head) + 256, p(ring), p(ops), nsets, n,
            p(order) if order is not None else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    nfb = int(head[0].item())
    return (olen.cpu().numpy().view(np.uint32).tolist(), st.cpu().numpy().tolist(),
            sorted(ids[:nfb].cpu().numpy().tolist()))


# ---------------------------------------------------------------------------
# The decoder paths on guarded batches (test_gpu_buffers.py, test_gpu_directed.py)
# ---------------------------------------------------------------------------
HANDED = 0x7FFF0001          # status of a block a throughput decoder handed over
FILL = 0x5A                  # destination guard byte (decoders)
FILL_ENC = 0xA5              # destination guard byte (encoders)
OK, E_INPUT_OVERRUN, E_OUTPUT_OVERRUN = 0, -4, -5
E_EOF_NOT_FOUND, E_INPUT_NOT_CONSUMED = -7, -8

PATHS = ["exact", "win+exact", "fast+exact", "win", "fast", "lat1", "lat8"]


def run_path(torch, path, dev, debug_env, comps, caps, src, dst):
    """One launch of `path` on the caller's batches -> out_len, status, the
    sorted ids a stand-alone throughput decoder handed over (None for the
    paths with the exact decoder behind them) and the fallback count at
    scratch byte 0 (None without scratch).  debug_env(value): sets
    POM_LZO_DEBUG and has the library re-read it."""
    if path in ("exact", "win+exact", "fast+exact"):
        if path != "exact":
            debug_env("decoder=" + path.split("+")[0])
        olen, st, fb = gpu_decompress_dev(torch, src, dst, dev, scratch=path != "exact")
        return olen, st, None, fb
    if path == "win":
        _, st, handed = gpu_decompress_win(torch, comps, caps, dev, src=src, dst=dst)
        return dst.out_len, st, handed, None
    if path == "fast":
        olen, st, handed = gpu_decompress_fast_alone(torch, src, dst, dev)
        return olen, st, handed, None
    _, st, handed = gpu_decompress_lat(torch, comps, caps, dev, group=int(path[3:]), src=src, dst=dst)
    return dst.out_len, st, handed, None


def check_decoded(names, want, caps, olen, st, handed, dst):
    """The oracle rule and the guard rule.  With the exact decoder behind
    (handed is None): status, out_len and bytes equal the oracle's.  A
    stand-alone throughput decoder reports OK only where the oracle does, then
    with its bytes; anything else is handed over (status HANDED, the id in
    the list; None: a block the latency decoder's launcher does not take).
    Guards: a finished block wrote min(out_len, cap) bytes, a handed-over one
    at most its room."""
    alone = handed is not None
    n = len(want)
    written = [int(caps[i]) if alone and st[i] != OK else min(int(olen[i]), int(caps[i]))
               for i in range(n)]
    problems = []
    try:
        arena = assert_guards(dst, written, FILL)
    except AssertionError as e:
        problems.append(str(e))
        arena = dst.arena.cpu().numpy()
    off = dst.host_off
    hset = set(handed or [])
    bad = []
    for i, (rc, ref) in enumerate(want):
        got = arena[int(off[i]): int(off[i]) + written[i]].tobytes()
        if not alone or st[i] == OK:
            good = (st[i], int(olen[i]), got) == (rc, len(ref), ref)
        else:
            good = st[i] is None or (st[i] == HANDED and i in hset)
        if not good:
            bad.append((names[i], st[i], rc, int(olen[i]), len(ref)))
    if bad:
        problems.append(f"{len(bad)} of {n} blocks wrong (name, status, oracle's, out_len, oracle's): {bad[:6]}")
    if alone and sorted(hset) != [i for i in range(n) if st[i] == HANDED]:
        problems.append("the fallback list is not the blocks with status HANDED")
    print(f"{n} blocks: {sum(s == OK for s in st)} OK, {sum(s == HANDED for s in st)} handed over, "
          f"{sum(s is None for s in st)} not launched, {sum(rc == OK for rc, _ in want)} OK by the oracle")
    assert not problems, "\n".join(problems)
