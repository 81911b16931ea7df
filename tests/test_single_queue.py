"""The single calls' combining queue (pomegranate_amd/csrc/single_queue.c) and
the debug keys (host_debug.c) on the CPU: tests/native/single_check, built once
with AddressSanitizer and UBSan and once with ThreadSanitizer, checks the
selection of a group without threads (one kind out of a mixed list, the tail
fix-up, the 64-call and 256 MiB caps), runs 8 threads of 300 calls each through
two queues with a recording callback (every call once, with its own result;
groups of one kind, at most 64, one at a time per queue; every thread returns),
and reads POM_LZO_DEBUG through pom_dbg_str and pom_dbg_int."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


@pytest.mark.parametrize("build", ["asan", "tsan"])
def test_single_check_program(build):
    check = os.path.join(NATIVE, "single_check_" + build)
    if not os.path.exists(check):
        subprocess.run(["make", "-C", NATIVE], check=True)
    r = subprocess.run([check], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "single_check: ok" in r.stdout and not r.stderr, r.stdout + r.stderr
