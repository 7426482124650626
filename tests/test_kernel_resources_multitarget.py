"""Register budget of every raster entry point in libggs.so, the plan-set ones
(raster_multi_kernel) included: the body they share with raster_kernel is sized
for 3 waves per SIMD (<= 168 VGPRs, csrc/ggs_kernels.hip OCC), so an entry point
that adds arguments must not push it to 2 waves, into scratch or into spills.
Read from the library's own code objects (tools/kernel_resources.py; CPU only)."""
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


def test_every_raster_entry_point_fits_three_waves_without_scratch_or_spills(res):
    raster = {n: r for n, r in res.items() if "raster" in n}
    multi = [n for n in raster if "raster_multi_kernel" in n]
    # fitness against a plan set: with / without the saturation cut-off, with / without the folded finalize
    assert len(multi) == 4, sorted(raster)
    assert len(raster) == 10, sorted(raster)
    for n, r in raster.items():
        assert r["vgpr_count"] <= 168, (n, r)
        assert r["waves_per_simd"] == 3, (n, r)
        assert r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["wavefront_size"] == 64, (n, r)
