"""CPU: csrc/vq_search_plan.h, the launch plans of the search, compiled alone into tests/cabi/search_plan.cpp and swept over
devices of 32 .. 304 compute units (every plan sound by its own arithmetic, the documented 256-CU plans pinned); once more
under the address and undefined-behaviour sanitizers where g++ links them (the products at M = 2^31 - 1)."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vector-quantization-by-ml_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cabi", "search_plan.cpp")
GXX = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build_and_run(exe, extra=()):
    r = subprocess.run(GXX + list(extra) + [SRC, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "search plan ok" in r.stdout, r.stdout + r.stderr


def test_search_plans_are_sound_on_every_device(tmp_path):
    _build_and_run(tmp_path / "search_plan")


def test_search_plans_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SANITIZE, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    _build_and_run(tmp_path / "search_plan_san", SANITIZE)
