"""Diagnostic: phase breakdown of the throughput encoder's parse wave
(s_memtime stamps build).  Usage: python scripts/diag_encode.py [--blocks N] [--model itb]"""
import argparse, ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pomegranate_amd import lzo, synth

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=4096)
ap.add_argument("--model", default="itb")
ap.add_argument("--bytes", type=int, default=65536)
ap.add_argument("--lib", default=None)
ap.add_argument("--nostamps", action="store_true")
a = ap.parse_args()
if a.lib:
    lzo.LIB_PATH = a.lib
dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
lib = lzo.load()
model = {v: k for k, v in synth.MODEL_NAMES.items()}[a.model]
arena, offs, lens = synth.batch(model, 0, [a.bytes] * a.blocks, align=256, threads=16)
t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
nb = a.blocks
src = lzo.DeviceBatch(t(arena), t(offs.view(np.int64)), t(lens.view(np.int32)))
caps = np.array([lzo.worst_compress(int(n)) for n in lens], dtype=np.uint64)
zo = np.zeros(nb, dtype=np.uint64); zo[1:] = np.cumsum((caps[:-1] + 255) // 256 * 256)
za = torch.zeros(int(zo[-1] + caps[-1]) + 256, dtype=torch.uint8, device=dev)
zb = lzo.DeviceBatch(za, t(zo.view(np.int64)), t(caps.astype(np.uint32).view(np.int32)))
zl = torch.zeros(nb, dtype=torch.int32, device=dev); zs = torch.zeros_like(zl)
SLOTS = 24                                 # (kEncStampSlots)
stamps = torch.zeros(nb * SLOTS, dtype=torch.int64, device=dev)
fn = getattr(lib, "lzo_mi355x_debug_compress_fast_stamps", None)
if fn is not None:
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
gfn = getattr(lib, "lzo_mi355x_debug_compress_gdict_stamps", None)
if gfn is not None:
    gfn.restype = ctypes.c_int
    gfn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_void_p]
g1fn = getattr(lib, "lzo_mi355x_debug_compress_gdict1_stamps", None)
if g1fn is not None:
    g1fn.restype = ctypes.c_int
    g1fn.argtypes = gfn.argtypes
grfn = getattr(lib, "lzo_mi355x_debug_compress_group_stamps", None)   # (the bench's grouped kernel)
if grfn is not None:
    grfn.restype = ctypes.c_int
    grfn.argtypes = gfn.argtypes
p = lambda x: x.data_ptr()
sh = torch.cuda.current_stream().cuda_stream
scr = torch.empty(max(lzo.compress_scratch_bytes(nb), 1), dtype=torch.uint8, device=dev)
ref_out = None
gstamps = torch.zeros(nb * SLOTS, dtype=torch.int64, device=dev)
g1stamps = torch.zeros(nb * SLOTS, dtype=torch.int64, device=dev)
grstamps = torch.zeros(nb * SLOTS, dtype=torch.int64, device=dev)
STAMPED = ("stamps", "gstamps", "g1stamps", "grstamps")
for mode in ("lds", "gdict", "stamps", "gstamps", "g1stamps", "grstamps"):
    if mode in STAMPED and (fn is None or gfn is None or g1fn is None or a.nostamps):
        continue
    if mode == "grstamps" and grfn is None:
        continue
    ts = []
    for _ in range(1 if mode in STAMPED else 5):
        za.zero_()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        if mode == "stamps":
            fn(p(src.arena), p(src.off), p(src.length), p(za), p(zb.off), p(zb.length), p(zl), p(zs), nb, p(stamps), sh)
        elif mode == "gstamps":
            gfn(p(src.arena), p(src.off), p(src.length), p(za), p(zb.off), p(zb.length), p(zl), p(zs), nb,
                p(scr), scr.numel(), p(gstamps), sh)
        elif mode == "grstamps":               # (the bench's grouped kernel)
            grfn(p(src.arena), p(src.off), p(src.length), p(za), p(zb.off), p(zb.length), p(zl), p(zs), nb,
                 p(scr), scr.numel(), p(grstamps), sh)
        elif mode == "g1stamps":               # (the one-wave kernel)
            g1fn(p(src.arena), p(src.off), p(src.length), p(za), p(zb.off), p(zb.length), p(zl), p(zs), nb,
                 p(scr), scr.numel(), p(g1stamps), sh)
        else:
            lzo.compress_dev(src, zb, zl, zs, scratch=scr if mode == "gdict" else None)
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    same = ""
    if mode not in STAMPED:
        got = (za.clone(), zl.clone())
        if ref_out is None:
            ref_out = got
        else:
            same = f", identical to lds {torch.equal(got[0], ref_out[0]) and torch.equal(got[1], ref_out[1])}"
    print(f"{mode}: {float(np.median(ts)):.3f} ms (min {min(ts):.3f}), status ok {bool((zs == 0).all())}{same}")
if fn is None or a.nostamps:
    sys.exit(0)
phases = ["setup", "probe", "cand", "path", "claim", "tok", "dict", "pushwait"]
counts = ["windows", "extend", "tokens", "pathit", "extit", "end_cross", "end_cap", "fwd"]
# (slots 16..19: the forwarding rounds' cycles -- "claim" is the claim reads up
# to the first conflict mask --, false alarms, and the HW_ID and XCC_ID registers;
# slots 20, 21: the dictionary re-bases' cycles and their count -- 0 per block
# up to 65,548 bytes)
FWDR, FALSE, HWID, XCC, REBASE, NREBASE, T0, T1 = 16, 17, 18, 19, 20, 21, 22, 23
runs = [("lds", stamps), ("gdict", gstamps), ("gdict1f", g1stamps)]
if grfn is not None:
    runs.append(("group", grstamps))
for name, t_ in runs:
    st = t_.view(nb, SLOTS).double().cpu().numpy()
    cyc = {n: int(st[:, i].mean()) for i, n in enumerate(phases)}
    cyc["fwdrounds"] = int(st[:, FWDR].mean())
    cyc["rebase"] = int(st[:, REBASE].mean())
    total = sum(cyc.values())
    print(name, "parse cycles/block (mean):", cyc, "total", total)
    print(name, "share of the chain (%):", {n: round(100.0 * v / max(total, 1), 1) for n, v in cyc.items()})
    cnt = {n: round(float(st[:, len(phases) + i].mean()), 1) for i, n in enumerate(counts)}
    cnt["false_alarm"] = round(float(st[:, FALSE].mean()), 1)
    cnt["rebase"] = round(float(st[:, NREBASE].mean()), 2)
    print(name, "counts/block (mean):", cnt)
# Where and when the one-wave and grouped kernels' blocks ran: HW_ID has the
# SIMD in bits 5:4, cu_id in bits 11:8, sh_id in bit 12 and se_id in bits
# 15:13; XCC_ID has the XCD in bits 3:0.  T0 / T1: s_memtime (100 MHz) at the
# block's start and after its tail token -- blocks that start late ran in a
# second round, after others of their CU had ended.
for name, t_ in runs[2:]:
    raw = t_.view(nb, SLOTS).cpu().numpy()
    hw, xcc = raw[:, HWID], raw[:, XCC] & 0xF
    cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 0xF)
    per_cu = np.bincount(np.unique(cu, return_inverse=True)[1])
    print(f"{name} blocks per CU: {len(per_cu)} CUs used, histogram (blocks: CUs)",
          {int(k): int(v) for k, v in zip(*np.unique(per_cu, return_counts=True))})
    print(f"{name} blocks per XCD:", {int(k): int(v) for k, v in zip(*np.unique(xcc, return_counts=True))})
    simd = (hw >> 4) & 3
    per_simd = np.bincount((np.unique(cu, return_inverse=True)[1] << 2) | simd)
    print(f"{name} blocks per SIMD of a CU, histogram (blocks: SIMDs)",
          {int(k): int(v) for k, v in zip(*np.unique(per_simd, return_counts=True))})
    t0 = (raw[:, T0] - raw[:, T0].min()) / 100.0          # us
    dur = (raw[:, T1] - raw[:, T0]) / 100.0
    print(f"{name} block start after the first (us): deciles",
          [round(float(x), 1) for x in np.percentile(t0, range(0, 101, 10))])
    print(f"{name} block duration (us): deciles", [round(float(x), 1) for x in np.percentile(dur, range(0, 101, 10))])
