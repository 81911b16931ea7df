"""The host arithmetic of the request operations
(pomegranate_amd/csrc/host_requests.c) on the CPU: tests/native/req_check,
built with AddressSanitizer and UBSan, runs the selection and grouping of
lookups and key/value gets over handmade ITB headers against a naive model,
the JUST_SPLIT pass, and the staging and scatter of a chunk whose block order
is not the caller's, refused names and keys included."""
from __future__ import annotations

import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CHECK = os.path.join(NATIVE, "req_check")


def test_req_check_program():
    if not os.path.exists(CHECK):
        subprocess.run(["make", "-C", NATIVE], check=True)
    r = subprocess.run([CHECK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"req_check: (\d+) checks ok", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
