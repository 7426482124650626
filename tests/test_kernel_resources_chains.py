"""Register budget of the SA chain groups' fitness raster (chain_strips_kernel, the
entry points over raster_body that read each candidate's plan from the compact
candidate list): like every other entry point of that body they must keep 3
waves per SIMD without scratch or spills.  Read from the library's own code
objects (tools/kernel_resources.py; CPU only)."""
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


def test_the_two_chain_entry_points_fit_three_waves_without_scratch_or_spills(res):
    chain = {n: r for n, r in res.items() if "chain_strips_kernel" in n}
    # with / without the saturation cut-off, both unfused
    assert len(chain) == 2, sorted(res)
    for n, r in chain.items():
        assert r["vgpr_count"] <= 168, (n, r)
        assert r["waves_per_simd"] == 3, (n, r)
        assert r["private_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["wavefront_size"] == 64, (n, r)
