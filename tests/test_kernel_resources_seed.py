"""Register and LDS budget of the placement kernels (csrc/ggs_seed.hip), read from the
library's own code objects with the reader tests/test_kernel_resources_loss.py uses (CPU
only): no scratch, no spills, wave64, and the figures DESIGN.md §8h records."""
from __future__ import annotations

import importlib.util
import os

import pytest

from conftest import REPO

KERNELS = ("seed_cell_kernel", "seed_rank_kernel", "seed_apply_kernel")
VGPRS = {"seed_cell_kernel": 30, "seed_rank_kernel": 42, "seed_apply_kernel": 38}
SGPRS = {"seed_cell_kernel": 36, "seed_rank_kernel": 22, "seed_apply_kernel": 32}
LDS = {"seed_cell_kernel": 0, "seed_rank_kernel": 2048, "seed_apply_kernel": 0}   # a tile of 256 64-bit keys
# the substrings the other resource tests count kernels by
OTHERS = ("raster", "vjp_", "grad_strip_kernel", "image_loss", "density_", "chain_strips_kernel", "bounds_cull_kernel")


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


@pytest.mark.parametrize("name", KERNELS)
def test_no_scratch_no_spills_and_the_recorded_size(res, name):
    r = _one(res, name)
    assert r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["wavefront_size"] == 64 and r["max_flat_workgroup_size"] == 256, r
    print(name, "vgprs", r["vgpr_count"], "sgprs", r["sgpr_count"], "lds", r["group_segment_fixed_size"],
          "waves/simd", r["waves_per_simd"])
    assert r["vgpr_count"] == VGPRS[name] and r["sgpr_count"] == SGPRS[name], r
    assert r["group_segment_fixed_size"] == LDS[name] and r.get("agpr_count", 0) == 0, r
    assert r["waves_per_simd"] == 8, r


def test_there_are_exactly_the_three_seed_kernels(res):
    names = [n for n in res if "seed_" in n]
    assert len(names) == 3 and all(any(k in n for k in KERNELS) for n in names), sorted(res)
    assert not [n for n in names if any(o in n for o in OTHERS)]
