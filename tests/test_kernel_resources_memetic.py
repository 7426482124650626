"""Register budget of the kernels the memetic island GA adds (csrc/ggs_grad.hip),
read from the library's own code objects with the reader
tests/test_kernel_resources.py uses (CPU only): no scratch, no spills, and the
figures DESIGN.md §8d records."""
from __future__ import annotations

import importlib.util
import os

import pytest

from conftest import REPO

SET_STRIP_VGPRS = 144


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


@pytest.mark.parametrize("name", ["grad_set_strip_kernel", "polish_stage_kernel", "polish_install_kernel"])
def test_no_scratch_and_no_spills(res, name):
    r = _one(res, name)
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["wavefront_size"] == 64, r


def test_set_strip_kernel_is_the_recorded_size(res):
    r = _one(res, "grad_set_strip_kernel")
    assert r["vgpr_count"] == SET_STRIP_VGPRS and r["waves_per_simd"] == 3, r
    assert r["group_segment_fixed_size"] == 0, r          # no LDS, as the single-target kernel


def test_the_single_target_kernel_is_still_alone_under_its_name(res):
    # tests/test_kernel_resources_grad.py pins it through this substring
    assert len([n for n in res if "grad_strip_kernel" in n]) == 1, sorted(res)

