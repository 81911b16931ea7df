#!/usr/bin/env python3
"""LZO1X block codec benchmark on MI355X (BASELINE.json metric).

The metric is "LZO1X compress+decompress GiB/s (device-resident)".  Default
workload (BASELINE.json configs[2], C3): 4096 x 64 KiB synthetic ITB blocks
per GPU in HBM before the timed region starts.  A "step" is one LZO1X-1
compression of the whole batch followed by one decompression of what it just
produced; value = uncompressed bytes of every rank / max-over-ranks wall time
of the steps, in GiB/s (so value = n / (t_compress + t_decompress)).

A plain run (`bench.py --gpus 1 --steps N --warmup W`) does what that figure
needs and no more: it generates the batch, warms up, times the N steps, checks
the last step's round trip on the device and prints the line, with the HBM
roofline of each kernel from the HIP events of the timed steps (`roofline` is
the decoder, whose roofline fraction the north star targets;
`compress_roofline` the encoder, the larger share of a step).
`--dump-outputs DIR` also writes what the last timed step returned
(dump_outputs below).

`--full` adds, each in a run of its own after the timed steps: the decode-only
rate of the same batch (configs[1], C2), a measured device-to-device copy
beside the rooflines, the two-stream pipelined legs, C4, C5 and the single
calls (`other_configs`), and the reference's own lib/minilzo.c (oracle/_ref,
compiled from the reference sources) on the host cores: a bounded sample of
the same ITB blocks, whose compressed bytes are also compared with the GPU's
(C3 byte identity), and configs[0] (C1: random 64 KiB blocks, compress ->
decompress round trip on the CPU).

Other workloads (--workload; each reports all it measures, with or without
--full):
  c2  decompress-only steps (configs[1])
  c4  mixed 4-256 KiB ITB blocks, decompress GiB/s; --c4-blocks per GPU
      (default 131072 = 1 M / 8: the 8-GPU run is exactly configs[3])
  c5  end-to-end ITB write/read through the MDSL append-file loopback with
      the host-resident batch API (pinned staging, hipMemcpyAsync in and out)
  single  per-call latency of the minilzo.h drop-in (lzo1x_1_compress,
      lzo1x_decompress) at ITB sizes, next to lib/minilzo.c on the host

Multi-GPU (python -m torch.distributed.run ... bench.py --gpus N): global
block i goes to rank i mod N (weak scaling: per-GPU work fixed); the only
collective is the RCCL completion barrier (error sum, elapsed max).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
GIB = float(1 << 30)
METRIC = "LZO1X compress+decompress GiB/s (device-resident), 4-256 KiB ITB block batches"


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--workload", choices=("c3", "c2", "c4", "c5", "single"), default="c3")
    p.add_argument("--blocks", type=int, default=4096, help="C2: blocks per GPU")
    p.add_argument("--block-bytes", type=int, default=65536)
    p.add_argument("--c4-blocks", type=int, default=131072, help="C4: blocks per GPU")
    p.add_argument("--c5-records", type=int, default=1024, help="C5: ITB records")
    p.add_argument("--model", default="itb")
    p.add_argument("--compress-steps", type=int, default=3)
    p.add_argument("--cpu-seconds", type=float, default=10.0)
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--no-others", action="store_true",
                   help="C3 with --full: skip the C4 and C5 measurements reported beside the headline")
    p.add_argument("--full", action="store_true",
                   help="C3: also measure what is reported beside the headline (decode-only and "
                        "pipelined legs, measured copy bandwidth, CPU baselines, C4, C5, single calls)")
    p.add_argument("--dump-outputs", metavar="DIR",
                   help="c2/c3/c4: write what the last timed step returned as DIR/<name>.npy")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and args.workload in ("c5", "single"):
        p.error("--dump-outputs covers the device-resident workloads (c2, c3, c4)")
    return args


# ---------------------------------------------------------------------------
# CPU baseline: the reference's lib/minilzo.c on the host cores
# ---------------------------------------------------------------------------
def host_cores():
    """Host cores this process may run on: its CPU affinity set, capped by
    OMP_NUM_THREADS when that is set (the GPU box sets it to the box's share
    of a shared machine, 16 per GPU, and os.cpu_count() counts the whole
    machine)."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    cap = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return max(1, min(n, cap) if cap > 0 else n)


def affinity_cpus():
    """Every CPU of this process's affinity set (the CPU baseline's headline
    thread count)."""
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        return os.cpu_count() or 1


def host_cpu_info():
    """What `cores` was taken from: the affinity set, the OMP_NUM_THREADS cap
    and the machine's logical CPUs (a GPU box is a share of a larger machine)."""
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = None
    return {"affinity_cpus": aff, "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
            "machine_logical_cpus": os.cpu_count()}


def _ref_lib():
    """lib/minilzo.c compiled from the reference sources (oracle/_ref), or None."""
    path = os.path.join(ROOT, "oracle", "_ref", "libminilzo_ref.so")
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    for f in (lib.lzo1x_decompress, lib.lzo1x_1_compress):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_ulong, ctypes.c_void_p,
                      ctypes.POINTER(ctypes.c_ulong), ctypes.c_void_p]
    getattr(lib, "__lzo_init_v2")(0x2040, 2, 4, 8, 4, 8, 8, 8, 8, 48)
    return lib


def _cpu_bench(plain, comps, threads, seconds, wrk="reuse"):
    """oracle/cpu_bench (native pthreads, no Python in the loop) on the sample:
    lib/minilzo.c from oracle/_ref, else the oracle port.  Returns its JSON.
    This process keeps to one CPU of its set while the harness runs, and the
    harness's threads avoid that CPU (POM_CPU_AVOID) while they are fewer than
    the set."""
    import struct
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "oracle", "cpu_bench")
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libminilzo_ref.so")
    lib = ref_path if os.path.exists(ref_path) else os.path.join(ROOT, "oracle", "liboracle.so")
    if not os.path.exists(exe):
        return None
    d = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = os.path.join(d, f"pom_cpu_sample_{os.getpid()}.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(plain)))
        for p_, z_ in zip(plain, comps):
            f.write(struct.pack("<II", len(p_), len(z_)))
            f.write(p_)
            f.write(z_)
    try:
        full = os.sched_getaffinity(0)
    except (AttributeError, OSError):
        full = None
    env = dict(os.environ)
    if full and len(full) > 1:
        mine = max(full)
        env["POM_CPU_AVOID"] = str(mine)
        os.sched_setaffinity(0, {mine})
    try:
        r = subprocess.run([exe, lib, path, str(threads), str(seconds), "1", wrk], capture_output=True,
                           text=True, timeout=seconds + 120, env=env,
                           preexec_fn=(lambda: os.sched_setaffinity(0, full)) if full else None)
    finally:
        if full:
            os.sched_setaffinity(0, full)
        os.unlink(path)
    if r.returncode != 0:
        raise RuntimeError(f"cpu_bench failed ({r.returncode}): {r.stderr.strip()[:200]}")
    return json.loads(r.stdout)


def _leg(j, roundtrip=True):
    c, d = j["compress_Bps"] / GIB, j["decompress_Bps"] / GIB
    rt = 1.0 / (1.0 / c + 1.0 / d) if roundtrip else d
    return {"value": round(rt, 4), "compress_value": round(c, 4), "decompress_value": round(d, 4),
            "threads": j["threads"], "seconds": round(j["decompress_s"] + j["compress_s"], 1),
            "per_thread_compress_GiBps": [round(x / GIB, 3) for x in j["per_thread_compress_Bps"]],
            "per_thread_decompress_GiBps": [round(x / GIB, 3) for x in j["per_thread_decompress_Bps"]]}


def cpu_c1(synth, seconds):
    """configs[0] (C1): lib/minilzo.c compress -> decompress round trip of
    random 64 KiB blocks (xorshift64, seed 42 + b) on the box's share of host
    cores, through the native harness (oracle/cpu_bench)."""
    lib = _ref_lib()
    if lib is None:
        return None
    threads = host_cores()
    plain = [synth.block(synth.RANDOM, 42 + b, 65536) for b in range(64)]
    comps = []
    wrk = ctypes.create_string_buffer(131072)
    z = ctypes.create_string_buffer(65536 + 65536 // 16 + 128)
    for p_ in plain:
        zl = ctypes.c_ulong(0)
        ctypes.memset(wrk, 0, 131072)
        lib.lzo1x_1_compress(p_, len(p_), z, ctypes.byref(zl), wrk)
        comps.append(z.raw[: zl.value])
    j = _cpu_bench(plain, comps, threads, seconds)
    if j is None:                                   # oracle/cpu_bench not built
        return None
    leg = _leg(j)
    return {"roundtrip_value": leg["value"], "unit": "GiB/s", "cores": threads,
            "compress_value": leg["compress_value"], "decompress_value": leg["decompress_value"],
            "kind": j["kind"],
            "sample": f"configs[0]: 64 random 64 KiB blocks (seed 42+b), lib/minilzo.c (oracle/_ref) "
                      f"on {threads} pinned threads of oracle/cpu_bench for {seconds:.0f} s "
                      f"(decompress 60 %, then compress 40 %)"}


def cpu_baseline(plain, comps, seconds, roundtrip=True):
    """The reference's lib/minilzo.c (oracle/_ref; the oracle port if absent)
    timed by oracle/cpu_bench -- native threads pinned one per CPU, per-thread
    wrkmem and buffers, no Python in the loop -- on the same blocks the GPU
    coded (their compressed bytes are the GPU's: the harness checks the
    reference reproduces each one, C3 byte identity).  `value` and `cores` are
    the box's CPU share (OMP_NUM_THREADS, 16 on the GPU box), a fixed, stated
    core count; one core and the whole affinity set are beside it."""
    share = host_cores()
    counts = [share]
    for c in (1, affinity_cpus()):
        if c not in counts:
            counts.append(c)
    runs = {}
    for c in counts:
        runs[c] = _cpu_bench(plain, comps, c, seconds if c == share else seconds / 2)
    if runs[share] is None:
        return None
    by = {str(c): _leg(j, roundtrip) for c, j in runs.items()}
    top, one = by[str(share)], by["1"]
    j = runs[share]
    # One core in the two other regimes, so the one-core figure can be set
    # against the single-call one (lib/minilzo.c on one 64 KiB block, the
    # wrkmem zeroed per call): the same cycled sample with the wrkmem zeroed
    # before every call, and one block repeated (cache-resident) likewise.
    one_zero = _cpu_bench(plain, comps, 1, seconds / 2, wrk="zero")
    one_res = _cpu_bench(plain[:1], comps[:1], 1, seconds / 2, wrk="zero")
    regimes = {
        "cycled_reused_wrkmem": {"compress_value": one["compress_value"],
                                 "decompress_value": one["decompress_value"],
                                 "working_set_bytes": runs[1]["per_thread_working_set_bytes"]},
        "cycled_zeroed_wrkmem": {"compress_value": _leg(one_zero)["compress_value"],
                                 "decompress_value": _leg(one_zero)["decompress_value"],
                                 "working_set_bytes": one_zero["per_thread_working_set_bytes"]},
        "resident_zeroed_wrkmem": {"compress_value": _leg(one_res)["compress_value"],
                                   "decompress_value": _leg(one_res)["decompress_value"],
                                   "working_set_bytes": one_res["per_thread_working_set_bytes"]},
        "note": (f"one_core (and value) cycle the whole sample, {runs[1]['per_thread_working_set_bytes'] / 1e6:.1f} MB "
                 "per thread, beyond one core's caches, and reuse each thread's wrkmem without clearing "
                 "it, as mds/itb.c:2913 does; the single-call figure (other_configs.single, 'ref') repeats "
                 "one cache-resident block with the wrkmem zeroed per call: the resident_zeroed_wrkmem "
                 f"regime, {_leg(one_res)['compress_value']:.2f} against {one['compress_value']:.2f} GiB/s "
                 "compress here; cycled_zeroed_wrkmem separates the two effects")}
    return {"value": top["value"], "unit": "GiB/s", "cores": share,
            "affinity_cpus": affinity_cpus(), "host": host_cpu_info(),
            "kind": j["kind"], "compress_value": top["compress_value"],
            "decompress_value": top["decompress_value"],
            "scaling_vs_one_core": {"compress": round(top["compress_value"] / one["compress_value"], 2),
                                    "decompress": round(top["decompress_value"] / one["decompress_value"], 2)},
            "by_threads": by, "one_core": one, "one_core_regimes": regimes,
            "byte_identical_blocks": f"{j['byte_identical']}/{j['blocks']}",
            "harness": "oracle/cpu_bench.c (pthreads, pinned, wrkmem reused per thread as mds/itb.c:2913)",
            "sample": f"{len(plain)} of the same {len(plain[0])}-byte ITB blocks, round-robin over "
                      f"{share} pinned threads (the box's OMP_NUM_THREADS share) for {seconds:.0f} s "
                      f"(decompress 60 %, then compress 40 %); 1 thread and the {affinity_cpus()}-CPU "
                      f"affinity set for {seconds / 2:.0f} s each (by_threads); "
                      + ("lib/minilzo.c built from the reference sources (oracle/_ref)"
                         if j["kind"] == "reference" else "oracle/lzo1x_oracle.c port")}


KERNEL_SOURCES = {"decode": "pomegranate_amd/csrc/lzo1x_decode_fast.hip",
                  "encode": "pomegranate_amd/csrc/lzo1x_encode_fast.hip"}


def source_sha16(kind):
    """SHA-256 (16 hex digits) of the kernel's source file: the build a
    profile summary was measured on."""
    import hashlib
    with open(os.path.join(ROOT, KERNEL_SOURCES[kind]), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def load_traffic(kind, block_bytes, nblocks):
    """HBM bytes per launch of the decode / encode kernel from a committed
    rocprofv3 PMC summary (profiles/*_{kind}_pmc.json, scripts/profile_pmc.py)
    measured on THIS kernel source (its source_sha16 must match), else None."""
    import glob
    sha = source_sha16(kind)
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"*{kind}_pmc.json"))):
        try:
            with open(path) as f:
                j = json.load(f)
        except Exception:
            continue
        if (j.get("block_bytes") == block_bytes and j.get("nblocks") == nblocks and
                j.get("source_sha16") == sha):
            best = j
    return best


# ---------------------------------------------------------------------------
# Device-resident workloads (C2, C3, C4)
# ---------------------------------------------------------------------------
class Resident:
    """Synthetic blocks in HBM, their GPU-compressed images, and output space."""

    def __init__(self, torch, lzo, synth, dev, model, sizes, seeds, chunk=4096):
        self.torch, self.lzo, self.dev = torch, lzo, dev
        sizes = np.asarray(sizes, dtype=np.uint64)
        nb = len(sizes)
        pad = (sizes + np.uint64(255)) // np.uint64(256) * np.uint64(256)
        offs = np.zeros(nb, dtype=np.uint64)
        offs[1:] = np.cumsum(pad[:-1])
        total = int(pad.sum())
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        arena = torch.empty(total, dtype=torch.uint8, device=dev)
        for c0 in range(0, nb, chunk):             # generated on the host a chunk at a time
            c1 = min(nb, c0 + chunk)
            a, _, _ = synth.batch(model, 0, sizes[c0:c1], seeds=seeds[c0:c1], align=256,
                                  threads=16)
            base = int(offs[c0])
            arena[base: base + a.size].copy_(torch.from_numpy(a))
        self.n_bytes = float(sizes.astype(np.float64).sum())
        self.sizes = sizes
        self.src = lzo.DeviceBatch(arena, t(offs.view(np.int64)), t(sizes.astype(np.uint32).view(np.int32)))
        caps = np.array([lzo.worst_compress(int(n)) for n in sizes], dtype=np.uint64)
        zoffs = np.zeros(nb, dtype=np.uint64)
        zoffs[1:] = np.cumsum((caps[:-1] + np.uint64(255)) // np.uint64(256) * np.uint64(256))
        self.zoffs = zoffs
        zarena = torch.empty(int(zoffs[-1] + caps[-1]) + 256, dtype=torch.uint8, device=dev)
        self.zdst = lzo.DeviceBatch(zarena, t(zoffs.view(np.int64)),
                                    t(caps.astype(np.uint32).view(np.int32)))
        self.zlen = torch.zeros(nb, dtype=torch.int32, device=dev)
        self.zst = torch.zeros(nb, dtype=torch.int32, device=dev)
        self.out = torch.zeros_like(arena)
        self.odst = lzo.DeviceBatch(self.out, self.src.off, self.src.length)
        self.olen = torch.zeros(nb, dtype=torch.int32, device=dev)
        self.ost = torch.zeros(nb, dtype=torch.int32, device=dev)
        nscr = lzo.decompress_scratch_bytes(nb)
        self.scratch = torch.empty(max(nscr, 1), dtype=torch.uint8, device=dev)
        self.cscratch = torch.empty(max(lzo.compress_scratch_bytes(nb), 1), dtype=torch.uint8,
                                    device=dev)
        self.compress()
        torch.cuda.synchronize()
        self.zsrc = lzo.DeviceBatch(zarena, self.zdst.off, self.zlen)
        self.decompress()
        torch.cuda.synchronize()
        self.z_bytes = float(self.zlen.double().sum().item())
        self.fallback_blocks = int(self.scratch[:4].view(torch.int32).item())

    def compress(self):
        self.lzo.compress_dev(self.src, self.zdst, self.zlen, self.zst, scratch=self.cscratch)

    def decompress(self):
        self.lzo.decompress_dev(self.zsrc, self.odst, self.olen, self.ost, self.scratch)

    def pipelined(self, steps, warmup=2):
        """Wall time of `steps` decodes of the batch issued back to back on two
        streams, each with its own output, lengths, status and scratch (so a
        batch's start overlaps the previous batch's last blocks), and whether
        both outputs are exact."""
        torch = self.torch
        if not hasattr(self, "_pipe"):
            out2 = torch.zeros_like(self.out)
            self._pipe = [(self.odst, self.olen, self.ost, self.scratch, torch.cuda.Stream()),
                          (self.lzo.DeviceBatch(out2, self.src.off, self.src.length),
                           torch.zeros_like(self.olen), torch.zeros_like(self.ost),
                           torch.empty_like(self.scratch), torch.cuda.Stream())]

        def step(i):
            d, ol, st, scr, s = self._pipe[i & 1]
            self.lzo.decompress_dev(self.zsrc, d, ol, st, scr, stream=s)
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ok = all(torch.equal(d.arena, self.src.arena) and bool((st == 0).all())
                 for d, _, st, _, _ in self._pipe)
        return wall, ok

    def roundtrip_pipelined(self, steps, warmup=2):
        """Wall time of `steps` C3 round trips (compress, then decompress what it
        produced) issued back to back on two streams, each stream with its own
        compressed image, output and scratch: one round trip's decode overlaps
        the next one's encode.  Every round trip keeps its data dependence; the
        outputs of both streams are checked."""
        torch, lzo = self.torch, self.lzo
        if not hasattr(self, "_rt"):
            sets = []
            for i in range(2):
                if i == 0:
                    zd, zl, zs, od, ol, os_, scr, cscr = (self.zdst, self.zlen, self.zst, self.odst,
                                                           self.olen, self.ost, self.scratch,
                                                           self.cscratch)
                else:
                    za = torch.empty_like(self.zdst.arena)
                    zd = lzo.DeviceBatch(za, self.zdst.off, self.zdst.length)
                    zl, zs = torch.zeros_like(self.zlen), torch.zeros_like(self.zst)
                    od = lzo.DeviceBatch(torch.zeros_like(self.out), self.src.off, self.src.length)
                    ol, os_ = torch.zeros_like(self.olen), torch.zeros_like(self.ost)
                    scr, cscr = torch.empty_like(self.scratch), torch.empty_like(self.cscratch)
                zsrc = lzo.DeviceBatch(zd.arena, zd.off, zl)
                sets.append((zd, zl, zs, zsrc, od, ol, os_, scr, cscr, torch.cuda.Stream()))
            self._rt = sets

        def step(i):
            zd, zl, zs, zsrc, od, ol, os_, scr, cscr, s = self._rt[i & 1]
            lzo.compress_dev(self.src, zd, zl, zs, stream=s, scratch=cscr)
            lzo.decompress_dev(zsrc, od, ol, os_, scr, stream=s)
        torch.cuda.synchronize()
        for i in range(warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        ok = all(torch.equal(od.arena, self.src.arena) and bool((os_ == 0).all()) and bool((zs == 0).all())
                 for _, _, zs, _, od, _, os_, _, _, _ in self._rt)
        return wall, ok

    def errors(self):
        torch = self.torch
        e = int((self.zst != 0).sum().item()) + int((self.ost != 0).sum().item())
        e += int((self.olen != self.src.length).sum().item())
        return e + (0 if torch.equal(self.out, self.src.arena) else 1)

    def sample(self, k):
        """(plain, compressed) bytes of the first k blocks, for the CPU leg."""
        zl = self.zlen[:k].cpu().numpy()
        plain, comps = [], []
        for b in range(k):
            o, n = int(self.src.off[b].item()), int(self.sizes[b])
            plain.append(self.src.arena[o: o + n].cpu().numpy().tobytes())
            z0 = int(self.zoffs[b])
            comps.append(self.zdst.arena[z0: z0 + int(zl[b])].cpu().numpy().tobytes())
        return plain, comps


def dist_on(dist) -> bool:
    """A process group exists (torchrun ranks; the RCCL test at world size 1)."""
    return dist.is_available() and dist.is_initialized()


def timed(torch, dist, world, stream, phases, steps, warmup):
    """Wall time of `steps` steps (each: the phases in order), bracketed by a
    barrier and a synchronize on both sides, and the average HIP-event time of
    each phase on the stream its kernels run on."""
    for _ in range(warmup):
        for f in phases:
            f()
    if dist_on(dist):
        dist.barrier()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(len(phases) + 1)]
           for _ in range(steps)]
    t0 = time.perf_counter()
    for k in range(steps):
        evs[k][0].record(stream)
        for i, f in enumerate(phases):
            f()
            evs[k][i + 1].record(stream)
    torch.cuda.synchronize()
    if dist_on(dist):
        dist.barrier()
    wall = time.perf_counter() - t0
    per = [sum(evs[k][i].elapsed_time(evs[k][i + 1]) for k in range(steps)) / 1e3 / max(steps, 1)
           for i in range(len(phases))]
    return wall, per


def copy_gbps(torch, dev, nbytes=1 << 30, reps=10):
    """Measured HBM bandwidth of a plain device-to-device copy (read + write
    bytes per second), SURVEY.md §8(d): reported next to the 8 TB/s peak."""
    a = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / 1e3 / reps
    del a, b
    return 2 * nbytes / t / 1e9


def roofline(kind, nbytes, kernel_s, block_bytes, nblocks, note):
    """HBM roofline of one kernel: algorithmic bytes (compressed + uncompressed,
    SURVEY.md §8(d)) per launch over the launch's average duration."""
    achieved = nbytes / kernel_s / 1e9
    rec = load_traffic(kind, block_bytes, nblocks)
    return {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBPS, 4),
            "traffic": rec.get("hbm_bytes_per_launch") if rec else None,
            "traffic_source": rec.get("profile") if rec else None,
            "kernel_ms": round(kernel_s * 1e3, 4), "algorithmic_bytes_per_launch": int(nbytes),
            "kernel": note}


DUMP_SEED = 20241                       # the block and byte sample of --dump-outputs
DUMP_ARRAY_BYTES = 16 << 20             # per sampled array; three of them plus the per-block ones < 64 MB


def dump_outputs(R, directory, compressed):
    """What a caller of the timed step receives, as float .npy files (the
    inputs are seeded, so two builds can be compared array for array):
      decompressed_length, decompress_status    every block (float64)
      decompressed_blocks   a fixed seeded sample of whole blocks, one row each,
                            zero beyond the block's length (float32)
      decompressed_bytes    a fixed seeded sample of byte positions of the
                            whole output arena (float32)
    and where the step compresses (C3) the same for the compressed side:
      compressed_length, compress_status, compressed_blocks (the same sampled
      blocks; each row is the block's stream, zero beyond its length).
    The block sample is as many blocks as fit DUMP_ARRAY_BYTES at the widest
    block's compressed capacity."""
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(DUMP_SEED)
    nb = len(R.sizes)
    caps = R.zdst.length.cpu().numpy().astype(np.int64)
    k = max(1, min(nb, DUMP_ARRAY_BYTES // (4 * int(caps.max()))))
    idx = np.sort(rng.choice(nb, size=k, replace=False))
    pos = np.sort(rng.integers(0, R.out.numel(), size=min(R.out.numel(), DUMP_ARRAY_BYTES // 4)))

    def save(name, a, dtype):
        np.save(os.path.join(directory, name + ".npy"), np.asarray(a).astype(dtype))

    def rows(arena, off, length, width):
        a = np.zeros((k, width), dtype=np.float32)
        for j, b in enumerate(idx):
            o, n = int(off[b]), int(length[b])
            a[j, :n] = arena[o: o + n].cpu().numpy()
        return a

    off = R.src.off.cpu().numpy()
    olen = R.olen.cpu().numpy()
    save("decompressed_length", olen, np.float64)
    save("decompress_status", R.ost.cpu().numpy(), np.float64)
    save("decompressed_blocks", rows(R.out, off, olen, int(R.sizes.max())), np.float32)
    save("decompressed_bytes", R.out[R.torch.from_numpy(pos).to(R.dev)].cpu().numpy(), np.float32)
    if compressed:
        zlen = R.zlen.cpu().numpy()
        save("compressed_length", zlen, np.float64)
        save("compress_status", R.zst.cpu().numpy(), np.float64)
        save("compressed_blocks", rows(R.zdst.arena, R.zoffs, zlen, int(caps.max())), np.float32)


def run_resident(args, torch, dist, lzo, synth, shard, dev, world, rank, backend):
    model = {v: k for k, v in synth.MODEL_NAMES.items()}[args.model]
    if args.workload in ("c2", "c3"):
        nglobal = args.blocks * world
        mine = shard.round_robin(nglobal, rank, world)         # global ids i = rank mod G
        sizes = [args.block_bytes] * len(mine)
        if args.workload == "c3":
            workload = (f"configs[2]: {args.blocks} x {args.block_bytes // 1024} KiB {args.model} "
                        "blocks per GPU, LZO1X-1 compress + decompress round trip, "
                        "device-resident, byte identity vs lib/minilzo.c checked")
        else:
            workload = (f"configs[1]: {args.blocks} x {args.block_bytes // 1024} KiB {args.model} "
                        "blocks per GPU, LZO1X decompress-only, device-resident")
    else:
        nglobal = args.c4_blocks * world
        mine = shard.round_robin(nglobal, rank, world)
        sizes = synth.mixed_sizes(nglobal, 4242)[mine]
        workload = (f"configs[3]: {nglobal} mixed 4-256 KiB {args.model} blocks "
                    f"round-robin over {world} GPU(s), LZO1X decompress-only, device-resident")
    R = Resident(torch, lzo, synth, dev, model, sizes, np.asarray(mine, dtype=np.uint64))
    stream = torch.cuda.current_stream()
    errors = R.errors()
    n_bytes, z_bytes = R.n_bytes, R.z_bytes
    bb = args.block_bytes if args.workload != "c4" else None
    # what is measured beside the headline, in runs of their own: always for
    # c2 / c4 (they are asked for by name), for C3 only with --full
    full = args.workload != "c3" or args.full
    dump = args.dump_outputs if rank == 0 else None      # (rank 0's share)
    # headline: C3 steps (compress, then decompress what it produced), or
    # decompress-only steps for c2 / c4
    if args.workload == "c3":
        wall, (t_c, t_d) = timed(torch, dist, world, stream, [R.compress, R.decompress],
                                 args.steps, args.warmup)
        errors += R.errors()                               # the last step's round trip
        if dump:
            dump_outputs(R, dump, compressed=True)
        if full:
            dec_wall, _ = timed(torch, dist, world, stream, [R.decompress], args.steps, 1)
    else:
        wall, (t_d,) = timed(torch, dist, world, stream, [R.decompress], args.steps, args.warmup)
        if dump:
            dump_outputs(R, dump, compressed=False)
        dec_wall = wall
        comp_wall, (t_c,) = timed(torch, dist, world, stream, [R.compress], args.compress_steps, 1)
        errors += int((R.ost != 0).sum().item()) + int((R.zst != 0).sum().item())
    if dist_on(dist):
        errors, wall = shard.completion_barrier(dist, dev, errors, wall)
        if full:
            _, dec_wall = shard.completion_barrier(dist, dev, 0, dec_wall)
        if args.workload != "c3":
            _, comp_wall = shard.completion_barrier(dist, dev, 0, comp_wall)
        tot = torch.tensor([n_bytes, z_bytes], dtype=torch.float64,
                           device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tot)
        n_all, z_all = float(tot[0].item()), float(tot[1].item())
    else:
        n_all, z_all = n_bytes, z_bytes
    value = n_all * args.steps / wall / GIB
    nb = len(mine)
    if args.workload == "c3":
        metric = METRIC
    else:
        metric = "LZO1X decompress GiB/s (device-resident), " + (
            "4096 x 64 KiB ITB blocks" if args.workload == "c2" else "mixed 4-256 KiB ITB blocks")
    result = {
        "metric": metric,
        "value": round(value, 3),
        "unit": "GiB/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(wall / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic ITB payload images (SURVEY.md Appendix B generator, libpom_synth)",
        "config": {"workload": workload, "blocks_per_gpu": nb,
                   "block_bytes": args.block_bytes if args.workload != "c4" else "4-256 KiB",
                   "compression_ratio": round(z_all / n_all, 4),
                   "parallelism": f"round-robin blocks over {world} GPU(s)"},
        # the decoder's roofline (the north star's target); the encoder's next to it
        "roofline": roofline("decode", z_bytes + n_bytes, t_d, bb, nb,
                             "lzo1x_decode_fast_kernel (+ the exact pass over its refusals)"),
        "compress_roofline": roofline("encode", z_bytes + n_bytes, t_c, bb, nb,
                                      "lzo1x_encode_gdict1_kernel" if "enc_waves=2" not in os.environ.get("POM_LZO_DEBUG", "")
                                      else "lzo1x_encode_gdict_kernel"),
        "step_ms": {"compress": round(t_c * 1e3, 4), "decompress": round(t_d * 1e3, 4)},
        "compress_kernel_gibps": round(n_bytes / t_c / GIB, 3),      # this GPU, HIP events
        "errors": errors,
        "fallback_blocks": R.fallback_blocks,
    }
    # whole-job HBM fraction over every GPU of the run:
    # algorithmic bytes of all ranks over the max-over-ranks time, against
    # G x 8 TB/s -- both kernels of the round trip, and (below) decode alone
    agg = {"gpus": world, "peak_GBps_per_gpu": HBM_PEAK_GBPS}
    result["aggregate_hbm"] = agg
    if args.workload == "c3":
        agg["roundtrip_frac"] = round(2 * (z_all + n_all) * args.steps / wall / 1e9 / (world * HBM_PEAK_GBPS), 4)
    if not full:
        return result, errors
    result["decompress_gibps"] = round(n_all * args.steps / dec_wall / GIB, 3)
    agg["decode_frac"] = round((z_all + n_all) * args.steps / dec_wall / 1e9 / (world * HBM_PEAK_GBPS), 4)
    if args.workload != "c3":
        # the metric's own quantity on this workload: compress + decompress of
        # every byte, whole job (each leg's max-over-ranks wall time per pass)
        t_rt = comp_wall / args.compress_steps + dec_wall / args.steps
        result["roundtrip_gibps"] = round(n_all / t_rt / GIB, 3)
        result["compress_gibps"] = round(n_all * args.compress_steps / comp_wall / GIB, 3)
        agg["roundtrip_frac"] = round(2 * (z_all + n_all) / t_rt / 1e9 / (world * HBM_PEAK_GBPS), 4)
    copy = copy_gbps(torch, dev)
    for key in ("roofline", "compress_roofline"):
        result[key]["copy_GBps_measured"] = round(copy, 1)
        result[key]["frac_of_copy"] = round(result[key]["achieved"] / copy, 4)
    if world == 1 and args.workload in ("c2", "c3"):
        # Successive decode batches on two streams (each launch's 4096 blocks
        # fill the chip in one round, so its first pieces and last blocks
        # leave SIMDs idle; the next launch recovers them).  Reported beside
        # the decode-only rate.
        p_wall, p_ok = R.pipelined(args.steps)
        result["decompress_pipelined_gibps"] = round(n_all * args.steps / p_wall / GIB, 3)
        result["decompress_pipelined_exact"] = p_ok
        errors += 0 if p_ok else 1
        if args.workload == "c3":
            # round trips on two streams: one's decode beside the next one's
            # encode (reported beside `value`, which runs them one at a time)
            r_wall, r_ok = R.roundtrip_pipelined(args.steps)
            result["roundtrip_pipelined_gibps"] = round(n_all * args.steps / r_wall / GIB, 3)
            result["roundtrip_pipelined_exact"] = r_ok
            errors += 0 if r_ok else 1
        result["errors"] = errors
    if rank == 0 and world == 1 and not args.no_cpu and args.workload in ("c2", "c3"):
        plain, comps = R.sample(min(len(mine), 512))
        result["cpu_baseline"] = cpu_baseline(plain, comps, args.cpu_seconds,
                                              roundtrip=args.workload == "c3")
        c1 = cpu_c1(synth, args.cpu_seconds / 2)
        if c1:
            result["cpu_baseline"]["c1"] = c1
    return result, errors


# ---------------------------------------------------------------------------
# C5: end-to-end ITB write/read with pinned host<->device copies
# ---------------------------------------------------------------------------
def _c5_xnet(args, recs, originals, tmps, rbufs, path, itb, xnet, plain_bytes):
    """C5 through the xnet wire format: MDS write-back
    REQs (compress + frame), MDSL parse + append; MDSL read + XNET_RPY_DATA_ITB
    replies, MDS parse + receive (copy into whole ITBs + in-place decode)."""
    n = len(recs)
    dests = [(0x200 + i % 8, i) for i in range(n)]
    reqs = [(0x11, i, 0x1000 + i) for i in range(n)]
    wire = bytearray(sum(itb.header_fields(r)[0] + xnet.TX_SIZE for r in recs))
    bufs = [bytearray(itb.ITB_FULL) for _ in recs]
    best = None
    for _ in range(max(1, args.steps // 5)):
        t0 = time.perf_counter()
        rc, wl, err = xnet.wb_batch(recs, tmps, dests, 0x11, 1, 3, wire)
        frames, used = xnet.parse(wire, wl, magic=3)
        af = itb.AppendFile(path)
        locs = af.append_batch([memoryview(wire)[f.offset: f.offset + f.tx.len] for f in frames])
        af.close()
        t1 = time.perf_counter()
        fd = os.open(path, os.O_RDONLY)
        stored = itb.read_batch(fd, locs, rbufs)
        os.close(fd)
        ta = time.perf_counter()
        rc2, wl2 = xnet.reply_batch(stored, reqs, 0x200, 3, wire)
        tb = time.perf_counter()
        frames2, _ = xnet.parse(wire, wl2, magic=3)
        tc = time.perf_counter()
        rerr = xnet.recv_batch(wire, frames2, bufs)
        t2 = time.perf_counter()
        stages = {"read_ms": round(1e3 * (ta - t1), 2), "reply_ms": round(1e3 * (tb - ta), 2),
                  "parse_ms": round(1e3 * (tc - tb), 2), "recv_ms": round(1e3 * (t2 - tc), 2)}
        errors = (rc != 0) + (rc2 != 0) + (used != wl) + sum(1 for e in err if e) + \
            sum(1 for e in rerr if e) + (len(frames2) != n)
        for b, o in zip(bufs, originals):
            h = bytearray(b[: itb.ITBH_SIZE])
            h[itb.ZLEN_OFF: itb.ZLEN_OFF + 4] = o[itb.ZLEN_OFF: itb.ZLEN_OFF + 4]
            errors += bytes(h) + bytes(b[itb.ITBH_SIZE: len(o)]) != o
        cur = (t1 - t0, t2 - t1, errors, wl, stages)
        if best is None or cur[0] + cur[1] < best[0] + best[1]:
            best = cur
    w, r, errors, wl, stages = best
    return {"write_gibps": round(plain_bytes / w / GIB, 3), "read_gibps": round(plain_bytes / r / GIB, 3),
            "wire_bytes": int(wl), "messages": n, "errors": errors, "read_stages": stages}


def run_c5(args, rank):
    import tempfile

    from pomegranate_amd import itb, xnet
    rng = np.random.default_rng(5)
    ites = rng.integers(1, 1025, args.c5_records)
    recs = [itb.make_record(100000 + i, int(k)) for i, k in enumerate(ites)]
    plain_bytes = float(sum(itb.header_fields(r)[0] - itb.ITBH_SIZE for r in recs))
    originals = [bytes(r[: itb.header_fields(r)[0]]) for r in recs]
    tmps = [bytearray(itb.ITB_FULL) for _ in recs]
    rbufs = [bytearray(itb.ITB_FULL) for _ in recs]             # read buffers (whole ITBs), reused
    # warm-up: one untimed pass over the whole batch, so the library's pinned and
    # device staging for full-size chunks exists before the timed passes
    wwhich, _ = itb.compress_batch(recs, tmps)
    itb.decompress_batch([bytearray(t) for t, w in zip(tmps, wwhich) if w])
    d = "/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir()
    path = os.path.join(d, f"pom_c5_{os.getpid()}_{rank}.itb")
    res = {}
    try:
        best = None
        for _ in range(max(1, args.steps // 5)):
            # the codec alone (H2D + kernels + D2H), then the write path: each
            # chunk's records appended while the GPU compresses the next chunks
            # (pom_itb_lzo_compress_append_batch), and the same as two calls
            tc0 = time.perf_counter()
            which, err = itb.compress_batch(recs, tmps)
            tc1 = time.perf_counter()
            af = itb.AppendFile(path + ".serial")
            outs = [t if w else r for r, t, w in zip(recs, tmps, which)]
            af.append_batch(outs, [itb.header_fields(o)[0] for o in outs])
            af.close()
            tc2 = time.perf_counter()
            os.unlink(path + ".serial")
            t0 = time.perf_counter()
            af = itb.AppendFile(path)
            which, err, locs = itb.compress_append_batch(recs, tmps, af)
            af.close()
            t2 = time.perf_counter()
            t1 = t0 + (tc1 - tc0)
            # read: the records, then the LZO ones decoded in place -- as two
            # calls (pom_itb_read_batch, pom_itb_lzo_decompress_batch), and
            # fused: each chunk's payloads read just before the decode batch
            # stages it (pom_itb_read_lzo_decompress_batch, the read_gibps)
            fd = os.open(path, os.O_RDONLY)
            tr0 = time.perf_counter()
            back = itb.read_batch(fd, locs, rbufs)            # pom_itb_read_batch
            t3 = time.perf_counter()
            comp_idx = [i for i, b in enumerate(back) if itb.header_fields(b)[2] == itb.COMPR_LZO]
            derr, ok = itb.decompress_batch([back[i] for i in comp_idx])
            t4 = time.perf_counter()
            for rb in rbufs:                                  # (the fused call reads into clean buffers)
                rb[: itb.ITBH_SIZE] = bytes(itb.ITBH_SIZE)
            tf0 = time.perf_counter()
            back, rerr, derr2, ok2 = itb.read_decompress_batch(fd, locs, rbufs)
            tf1 = time.perf_counter()
            os.close(fd)
            errors = sum(1 for e in err if e) + sum(1 for e in derr if e) + ok.count(0)
            errors += sum(1 for e in rerr if e) + sum(1 for e in derr2 if e) + ok2.count(0)
            # the record as written, except h.zlen: itb_lzo_decompress leaves the
            # uncompressed length there (mds/itb.c:2949-2980)
            for b, o in zip(back, originals):
                h = bytearray(b[: itb.ITBH_SIZE])
                h[itb.ZLEN_OFF: itb.ZLEN_OFF + 4] = o[itb.ZLEN_OFF: itb.ZLEN_OFF + 4]
                errors += bytes(h) + bytes(b[itb.ITBH_SIZE: len(o)]) != o
            cur = (t1 - t0, t2 - t0, t4 - t3, tf1 - tf0, errors, len(comp_idx),
                   os.path.getsize(path), tc2 - tc0, t4 - tr0)
            if best is None or cur[1] + cur[3] < best[1] + best[3]:
                best = cur
        c, w, dcd, r, errors, ncomp, fbytes, wser, rser = best
        xres = _c5_xnet(args, recs, originals, tmps, rbufs, path, itb, xnet, plain_bytes)
        res = {"records": len(recs), "uncompressed_bytes": int(plain_bytes),
               "file_bytes": fbytes, "compressed_records": ncomp,
               "write_gibps": round(plain_bytes / w / GIB, 3),
               "write_serial_gibps": round(plain_bytes / wser / GIB, 3),
               "read_gibps": round(plain_bytes / r / GIB, 3),
               "read_serial_gibps": round(plain_bytes / rser / GIB, 3),
               "compress_pcie_gibps": round(plain_bytes / c / GIB, 3),
               "decompress_pcie_gibps": round(plain_bytes / dcd / GIB, 3),
               "errors": errors + xres["errors"], "xnet": xres}
    finally:
        if os.path.exists(path):
            os.unlink(path)
    result = {
        "metric": "LZO1X end-to-end ITB write/read GiB/s (host-resident, pinned copies)",
        "value": res["read_gibps"], "unit": "GiB/s", "n_gpus": 1, "steps": max(1, args.steps // 5),
        "warmup": 1, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u8", "data": "synthetic ITB records (real h.len distribution 12,416-536,192 B)",
        "config": {"workload": "configs[4]: mdsl/storage.c ITB append-file write/read loopback "
                               "(/dev/shm) with the GPU LZO drop-in, pinned host<->device copies "
                               "included", "records": len(recs)},
        "e2e": res,
    }
    return result, res["errors"]


# ---------------------------------------------------------------------------
# Single calls: the minilzo.h drop-in one block at a time
# ---------------------------------------------------------------------------
def run_single(args, lzo, synth):
    """Per-call latency of lzo1x_1_compress / lzo1x_decompress (the unchanged
    callers mds/itb.c:2923, :2964, mdsl/gc.c:770, api/api.c:6523/:6438) at the
    smallest ITB, a 64 KiB block and the largest ITB payload, next to the
    reference's lib/minilzo.c on one host core."""
    lib = lzo.load()
    ref = _ref_lib()
    ulong = ctypes.c_ulong
    out = {}
    for n in (12416, 65536, 536192):
        d = synth.block(synth.ITB, 777 + n, n)
        src = ctypes.create_string_buffer(d, n)
        z = ctypes.create_string_buffer(n + n // 16 + 128)
        back = ctypes.create_string_buffer(n + 64)
        wrk = ctypes.create_string_buffer(131072)
        zl, ol = ulong(0), ulong(0)
        row = {}
        for name, L in (("gpu", lib), ("ref", ref)):
            if L is None:
                continue
            reps = max(3, args.steps)
            if name == "ref":
                ctypes.memset(wrk, 0, 131072)
            L.lzo1x_1_compress(src, n, z, ctypes.byref(zl), wrk)      # warm-up
            L.lzo1x_decompress(z, zl.value, back, ctypes.byref(ol), None)
            t0 = time.perf_counter()
            for _ in range(reps):
                if name == "ref":
                    ctypes.memset(wrk, 0, 131072)               # zero-filled wrkmem, as defined
                L.lzo1x_1_compress(src, n, z, ctypes.byref(zl), wrk)
            t1 = time.perf_counter()
            for _ in range(reps):
                rc = L.lzo1x_decompress(z, zl.value, back, ctypes.byref(ol), None)
            t2 = time.perf_counter()
            ok = rc == 0 and ol.value == n and back.raw[:n] == d
            row[name] = {"compress_us": round((t1 - t0) / reps * 1e6, 1),
                         "decompress_us": round((t2 - t1) / reps * 1e6, 1),
                         "zlen": int(zl.value), "exact": ok}
        out[str(n)] = row
    v = out["65536"]["gpu"]["decompress_us"]
    errors = sum(0 if r.get("exact", True) else 1 for row in out.values() for r in row.values())
    # concurrent callers (the MDS commit / service threads): 64 KiB calls from
    # 8 threads at once, combined by the library into shared launches
    from concurrent.futures import ThreadPoolExecutor
    n = 65536
    d = synth.block(synth.ITB, 777 + n, n)
    nthr, per = 8, max(3, args.steps)
    bufs = [(ctypes.create_string_buffer(d, n), ctypes.create_string_buffer(n + n // 16 + 128),
             ctypes.create_string_buffer(n + 64)) for _ in range(nthr)]

    def one(t, what):
        src, z, back = bufs[t]
        zl, ol = ulong(0), ulong(0)
        ok = True
        lib.lzo1x_1_compress(src, n, z, ctypes.byref(zl), None)
        for _ in range(per):
            if what == "compress":
                ok &= lib.lzo1x_1_compress(src, n, z, ctypes.byref(zl), None) == 0
            else:
                ok &= lib.lzo1x_decompress(z, zl.value, back, ctypes.byref(ol), None) == 0 and \
                    back.raw[:n] == d
        return ok

    z0, zl0 = ctypes.create_string_buffer(n + n // 16 + 128), ulong(0)
    lib.lzo1x_1_compress(bufs[0][0], n, z0, ctypes.byref(zl0), None)
    conc = {"threads": nthr, "calls_per_thread": per, "block_bytes": n}
    for what in ("compress", "decompress"):
        with ThreadPoolExecutor(nthr) as ex:            # (untimed: staging grows to its groups)
            list(ex.map(lambda t: one(t, what), range(nthr)))
        with ThreadPoolExecutor(nthr) as ex:
            t0 = time.perf_counter()
            oks = list(ex.map(lambda t: one(t, what), range(nthr)))
            dt = time.perf_counter() - t0
        errors += oks.count(False)
        conc[f"{what}_calls_per_s"] = round(nthr * per / dt, 1)
        conc[f"{what}_serial_calls_per_s"] = round(1e6 / out["65536"]["gpu"][f"{what}_us"], 1)
        # a lone call right after the group: the library's leader waits up to
        # ~50 us for company when the last group had some
        src, z, back = bufs[0]
        zl, ol = ulong(0), ulong(0)
        t0 = time.perf_counter()
        if what == "compress":
            errors += lib.lzo1x_1_compress(src, n, z, ctypes.byref(zl), None) != 0
        else:
            errors += lib.lzo1x_decompress(z0, zl0.value, back, ctypes.byref(ol), None) != 0
        conc[f"{what}_lone_after_group_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    result = {
        "metric": "LZO1X single-call latency, lzo1x_decompress of one 64 KiB ITB block (us)",
        "value": v, "unit": "us", "n_gpus": 1, "steps": max(3, args.steps), "warmup": 1,
        "higher_is_better": False, "scaling": "none", "vs_baseline": None, "dtype": "u8",
        "data": "synthetic ITB payload images", "config": {
            "workload": "minilzo.h single calls (host buffers in, host buffers out: one H2D copy, "
                        "kernels writing into mapped pinned staging, one stream sync per call; "
                        "calls from several threads combined into shared launches) "
                        "vs lib/minilzo.c on one core"},
        "calls": out, "concurrent": conc}
    return result, errors


def run_others(args, torch, dist, lzo, synth, shard, dev, world, rank, backend):
    """C5 (configs[4]: the append-file loop, N = 1 only) and C4 (configs[3]:
    131,072 mixed 4-256 KiB blocks per GPU, global block i on rank i mod G, so
    8 ranks hold the 1 M blocks; decode and compress kernels, whole-job rates)
    measured in the same run as the C3 headline, so the driver's record holds
    them too (its 1/2/4/8-GPU runs give the C4 curve).  Each is reported
    beside the headline, never as its value."""
    import copy
    import gc
    out = {}
    gc.collect()
    torch.cuda.empty_cache()
    a = copy.copy(args)
    # 4 timed passes (best of), not 2: the read is host- and PCIe-bound, and
    # the best of two spread 22.0-24.9 GiB/s over one session's runs on the
    # same tree
    a.workload, a.steps, a.warmup = "c5", 20, 1
    try:
        if world == 1:
            r, e = run_c5(a, rank)
            out["c5"] = dict(r["e2e"], metric=r["metric"], workload=r["config"]["workload"], errors=e)
            out["c5"].pop("xnet", None)
    except Exception as exc:
        out["c5"] = {"error": repr(exc), "errors": 1}
    gc.collect()
    torch.cuda.empty_cache()
    a = copy.copy(args)
    a.workload, a.steps, a.warmup, a.compress_steps, a.no_cpu = "c4", 3, 1, 1, True
    a.dump_outputs = None                          # (the dump is the headline's)
    try:
        r, e = run_resident(a, torch, dist, lzo, synth, shard, dev, world, rank, backend)
        out["c4"] = {"workload": r["config"]["workload"], "n_gpus": world,
                     "blocks_per_gpu": r["config"]["blocks_per_gpu"],
                     "decompress_gibps": r["value"],             # all ranks' blocks / max rank time
                     "compress_gibps": r["compress_gibps"],
                     # compress + decompress of the 4-256 KiB blocks: the metric's
                     # own wording (BASELINE.json), beside C3's `value`
                     "roundtrip_gibps": r["roundtrip_gibps"],
                     "aggregate_hbm": r["aggregate_hbm"],
                     "compress_kernel_gibps_rank0": r["compress_kernel_gibps"],
                     "step_ms_rank0": r["step_ms"], "compression_ratio": r["config"]["compression_ratio"],
                     "decode_roofline_frac_rank0": r["roofline"]["frac"], "errors": e}
    except Exception as exc:                       # (reported, never hides the headline)
        out["c4"] = {"error": repr(exc), "errors": 1}
    if world == 1:
        # the minilzo.h single calls of the unchanged callers (µs per call)
        a = copy.copy(args)
        a.workload, a.steps = "single", 20
        try:
            r, e = run_single(a, lzo, synth)
            out["single"] = {"metric": r["metric"], "calls": r["calls"], "concurrent": r["concurrent"],
                             "errors": e}
        except Exception as exc:
            out["single"] = {"error": repr(exc), "errors": 1}
    return out


def launch_ranks(n):
    """`bench.py --gpus N` (N > 1) started without a launcher: start N rank
    processes through torch.distributed.run on 127.0.0.1 -- one per GPU, the
    driver's own command -- and return their exit code.  Runs before anything
    imports torch or touches a GPU (the ranks are children, not an exec)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)]
    cmd += sys.argv[1:]
    print(f"bench: --gpus {n} without a launcher: starting {n} ranks", file=sys.stderr, flush=True)
    return subprocess.run(cmd).returncode


def rank_plan(args):
    """(world, rank, local rank) from the launcher's environment.  A request
    for N GPUs is never measured on a different number of ranks: a WORLD_SIZE
    that disagrees with --gpus is an error."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"bench: WORLD_SIZE={world} but --gpus={args.gpus}; "
                         "the run must have one rank per requested GPU")
    return world, rank, local


def main():
    args = parse()
    if args.gpus < 1:
        raise SystemExit("bench: --gpus must be at least 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))
    world, rank, local = rank_plan(args)
    if os.environ.get("POM_BENCH_PLAN_ONLY"):
        # (tests: the rank layout a run would use, without touching a GPU)
        print(json.dumps({"plan": True, "n_gpus": world, "rank": rank, "local_rank": local}),
              flush=True)
        return
    import torch
    import torch.distributed as dist

    from pomegranate_amd import lzo, shard, synth

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the LZO1X path has no CPU fallback)")
    # One process per GPU.  POM_DIST_BACKEND=gloo rehearses N ranks on fewer GPUs.
    backend = os.environ.get("POM_DIST_BACKEND", "nccl")
    if backend == "nccl" and world > torch.cuda.device_count():
        raise SystemExit(f"bench: {world} ranks over RCCL need {world} GPUs, "
                         f"{torch.cuda.device_count()} visible")
    dev = torch.device(f"cuda:{local % torch.cuda.device_count()}")
    torch.cuda.set_device(dev)
    # One rank per GPU: the library's host batches stay on this rank's GPU
    # (its own split over every visible GPU is for single-process callers).
    if world > 1:
        os.environ.setdefault("POM_LZO_DEVICES", str(dev.index))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    lzo.load()
    if args.workload == "c5":
        result, errors = run_c5(args, rank)
    elif args.workload == "single":
        result, errors = run_single(args, lzo, synth)
    else:
        result, errors = run_resident(args, torch, dist, lzo, synth, shard, dev, world, rank,
                                      backend)
        if args.workload == "c3" and args.full and not args.no_others:
            result["other_configs"] = run_others(args, torch, dist, lzo, synth, shard, dev, world,
                                                 rank, backend)
            errors += sum(o.get("errors", 1) for o in result["other_configs"].values())
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()
    if errors:
        raise SystemExit(f"bench: {errors} blocks failed the round trip")


if __name__ == "__main__":
    main()
