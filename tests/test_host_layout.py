"""The staging layouts of the host batches
(pomegranate_amd/csrc/host_layout.c) on the CPU: tests/native/layout_check,
built with AddressSanitizer and UBSan, lays out every operation's chunk over
every combination of block count, LZO prefix, sizes, request counts, name
lengths and kvlist options, and checks alignment, disjointness, the totals, the
H2D span and the result D2H spans."""
from __future__ import annotations

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CHECK = os.path.join(NATIVE, "layout_check")


def test_layout_check_program():
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", NATIVE], check=True)
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"layout_check: (\d+) layouts ok", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
