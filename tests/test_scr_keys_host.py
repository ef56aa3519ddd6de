"""Host only: the key tracker of the screened Dp = 256 sweep (csrc/vq_scr_keys.h: register tag in the value's low mantissa
bits, three lowest keys, the sub-tiles of the two lowest, decode), the same code the kernel runs, compiled into a host program
with the address and undefined-behaviour sanitizers and set against a sort (tests/cabi/scr_keys.cpp)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vector-quantization-by-ml_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tracker_against_a_sort_under_sanitizers(tmp_path):
    exe = tmp_path / "scr_keys"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(ROOT, "tests", "cabi", "scr_keys.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "scr keys ok" in r.stdout, r.stdout + r.stderr
