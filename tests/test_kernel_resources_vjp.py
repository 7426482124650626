"""Register budget of the render-VJP kernels (csrc/ggs_grad.hip), read from the
library's own code objects with the reader tests/test_kernel_resources_grad.py uses
(CPU only): no scratch, no spills, wave64, and the figures DESIGN.md §8e records.
vjp_finish_kernel has one instance per row layout (its template argument)."""
from __future__ import annotations

import importlib.util
import os

import pytest

from conftest import REPO

STRIP = "vjp_strip_kernel"
FINISH = {"renderer": "vjp_finish_kernelILi0E", "axes": "vjp_finish_kernelILi1E"}


@pytest.fixture(scope="module")
def res():
    import ggs
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.kernel_resources(ggs.LIB_PATH)


def _one(res, name):
    hits = {n: r for n, r in res.items() if name in n}
    assert len(hits) == 1, sorted(res)
    return next(iter(hits.values()))


@pytest.mark.parametrize("name", [STRIP, *FINISH.values()])
def test_no_scratch_and_no_spills(res, name):
    r = _one(res, name)
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["wavefront_size"] == 64, r


def test_strip_kernel_is_the_recorded_size(res):
    r = _one(res, STRIP)
    assert r["vgpr_count"] == STRIP_VGPRS and r["waves_per_simd"] == 3, r
    assert r["group_segment_fixed_size"] == 0, r          # no LDS: nothing is shared between lanes but shuffles


@pytest.mark.parametrize("layout", sorted(FINISH))
def test_finish_kernel_is_the_recorded_size(res, layout):
    r = _one(res, FINISH[layout])
    assert r["vgpr_count"] == FINISH_VGPRS[layout] and r["waves_per_simd"] == 8, r


def test_there_are_exactly_the_three_vjp_kernels(res):
    assert len([n for n in res if "vjp_" in n]) == 3, sorted(res)


STRIP_VGPRS = 144
FINISH_VGPRS = {"renderer": 54, "axes": 54}
