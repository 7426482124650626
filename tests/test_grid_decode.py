"""The strip-words raster's launch descriptor on the host (csrc/ggs_internal.h):
grid_div_make's multiply-shift constants, strip_launch_grid / strip_launch_block
(the grid decode every strip wave runs) and strip_table_entry (the dispatch table
whose entries are decoded strips) are plain host functions; tests/c/
grid_decode_check.cpp is a stand-alone program around them, built here with the
host compiler (as test_capi.py builds its C host).  It checks

  * quotient and remainder against / and % for every divisor 1 .. 4096: every
    dividend up to 2^20, 2^31 - 1, multiples of the divisor +- 1, and a constant
    built for a launch-sized bound at every dividend up to that bound;
  * (candidate, dispatch group) of every block against the prologue that divides,
    restated in the program: the test canvases' tile counts, B = 1 .. 1032, one
    chunk, full chunks with a ragged last one, and the single-round range in which
    the middle third of the grid runs reversed;
  * every table entry of the test canvases against (tx0, ty0, wv) of the raster's
    formulas.

No GPU, and no entry point of libggs: the program includes the header alone."""
from __future__ import annotations

import os
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "genetic-gaussian-splats_amd", "csrc")


def test_descriptor_constants_decode_and_table(tmp_path):
    exe = os.path.join(tmp_path, "grid_decode_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-pthread", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", CSRC,
                    os.path.join(os.path.dirname(__file__), "c", "grid_decode_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 4096 * (1 << 20)

