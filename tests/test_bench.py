"""The bench's plain run: only the headline's work, the number of timed steps
--steps asks for, and --dump-outputs writing what the last timed step returned."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pomegranate_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = float(1 << 30)
# what only --full measures (runs of their own beside the timed steps)
FULL_ONLY = ("decompress_gibps", "decompress_pipelined_gibps", "roundtrip_pipelined_gibps",
             "cpu_baseline", "other_configs")


def _bench(args, timeout=240):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_refuses_zero_steps_and_a_dump_of_host_workloads():
    assert _bench(["--gpus", "1", "--steps", "0"]).returncode != 0
    assert _bench(["--gpus", "1", "--workload", "c5", "--dump-outputs", "x"]).returncode != 0


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, oracle):
    """40 blocks of 20,000 bytes (every block fits the dump's sample, so row b
    is block b): the line holds the headline and ms_per_step for the 3 timed
    steps and nothing that takes a run of its own; the dumped arrays are float,
    under 64 MB, the compressed rows are the oracle's streams and the
    decompressed rows the inputs."""
    nb, n, steps = 40, 20000, 3
    out = tmp_path / "dump"
    r = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--blocks", str(nb),
                "--block-bytes", str(n), "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["errors"] == 0 and line["ms_per_step"] > 0
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    # value and ms_per_step are the same wall time (both rounded on the line)
    assert line["value"] == pytest.approx(nb * n / (line["ms_per_step"] / 1e3) / GIB, rel=1e-3, abs=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    assert "copy_GBps_measured" not in line["roofline"]

    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrays) == {"compressed_length", "compress_status", "compressed_blocks",
                           "decompressed_length", "decompress_status", "decompressed_blocks",
                           "decompressed_bytes"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64e6
    plain = [synth.block(synth.ITB, b, n) for b in range(nb)]
    comps = [oracle.compress(p) for p in plain]
    assert (arrays["compress_status"] == 0).all() and (arrays["decompress_status"] == 0).all()
    assert arrays["compressed_length"].tolist() == [len(z) for z in comps]
    assert arrays["decompressed_length"].tolist() == [n] * nb
    for b in range(nb):
        zrow = arrays["compressed_blocks"][b]
        assert bytes(zrow[: len(comps[b])].astype(np.uint8)) == comps[b] and not zrow[len(comps[b]):].any()
        assert bytes(arrays["decompressed_blocks"][b].astype(np.uint8)) == plain[b]
