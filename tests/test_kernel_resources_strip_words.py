"""Register budget of bounds_cull_kernel, the twin of raster_kernel<MODE, false,
false> that culls from the bounds (launches without strip words): the same body,
so the same limits as tests/test_kernel_resources.py holds the raster_kernel
instances to.  Read from the library's own code objects (CPU only)."""
from __future__ import annotations

import importlib.util
import os

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def res():
    import ggs
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", os.path.join(REPO, "tools", "kernel_resources.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.kernel_resources(ggs.LIB_PATH)


def test_bounds_cull_twins_fit_three_waves_without_scratch_or_spills(res):
    twins = {n: r for n, r in res.items() if "bounds_cull_kernel" in n}
    assert len(twins) == 2, sorted(res)      # image and fitness
    for n, r in twins.items():
        assert r["vgpr_count"] <= 168, (n, r)
        assert r["waves_per_simd"] == 3, (n, r)
        assert r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["wavefront_size"] == 64, (n, r)
