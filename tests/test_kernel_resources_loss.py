"""Register and LDS budget of the image-loss kernels (csrc/ggs_loss.hip), read from the
library's own code objects with the reader tests/test_kernel_resources_grad.py uses (CPU
only): no scratch, no spills, wave64, and the figures DESIGN.md §8f records.
image_loss_kernel has one instance with a cotangent and one without (its template
argument); at least two of either fit a CU's 160 KiB of LDS."""
from __future__ import annotations

import importlib.util
import os

import pytest

from conftest import REPO

TILE = {"cot": "image_loss_kernelILb1E", "loss": "image_loss_kernelILb0E"}
FINALIZE = "image_loss_finalize_kernel"
VGPRS = {"cot": 198, "loss": 182, FINALIZE: 22}
LDS = {"cot": 62520, "loss": 24504, FINALIZE: 1536}
WAVES = {"cot": 2, "loss": 2, FINALIZE: 8}              # a workgroup is one wave per SIMD: two workgroups a CU
CU_LDS = 160 * 1024


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


@pytest.mark.parametrize("name", [*TILE.values(), FINALIZE])
def test_no_scratch_and_no_spills(res, name):
    r = _one(res, name)
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["wavefront_size"] == 64, r


@pytest.mark.parametrize("which", sorted(TILE))
def test_tile_kernel_is_the_recorded_size(res, which):
    r = _one(res, TILE[which])
    assert r["vgpr_count"] == VGPRS[which] and r["waves_per_simd"] == WAVES[which], r
    assert r["group_segment_fixed_size"] == LDS[which], r
    assert r["max_flat_workgroup_size"] == 256, r
    assert 2 * r["group_segment_fixed_size"] <= CU_LDS            # two workgroups per CU


def test_finalize_kernel_is_the_recorded_size(res):
    r = _one(res, FINALIZE)
    assert r["vgpr_count"] == VGPRS[FINALIZE] and r["waves_per_simd"] == WAVES[FINALIZE], r
    assert r["group_segment_fixed_size"] == LDS[FINALIZE], r


def test_there_are_exactly_the_three_loss_kernels(res):
    names = [n for n in res if "image_loss" in n]
    assert len(names) == 3, sorted(res)
    # the substrings the other resource tests count kernels by
    assert not [n for n in names if "vjp_" in n or "grad_strip_kernel" in n]
