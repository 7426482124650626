"""finalize with one candidate per 64-thread workgroup (csrc/ggs_kernels.hip
finalize_kernel, b = blockIdx.x).

Batches of 1, 3, 4 and 5 candidates (below, at and past the four candidates the
256-thread workgroup used to hold), weighted and boost fitness, at 64x128 (one
tile: 4 strip partials per candidate, most lanes of the wave sum nothing) and at
512^2 (128 strip partials, two per lane): candidate b's scalar in the batch has
the bits of the same candidate evaluated alone, the batch invariance the project
asserts for the raster.  One plan-set launch, B = 6 with group = 3, against the
two ``TargetPlan`` calls it stands for (finalize picks plan b // group's weight
block).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ggs
import ggs_oracle as O
from ggs import hip

pytestmark = pytest.mark.gpu
N = 24
MODES = {"weighted": False, "boost": True}


@functools.lru_cache(maxsize=None)
def _problem(H, W):
    """Five candidates, target, mask, and per mode each candidate's fitness alone."""
    rng = np.random.default_rng(H + W)
    pop = O.synthetic_population(5, N, H, W, seed=H)
    tgt = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    mask = rng.uniform(0.4, 1.0, (H, W)).astype(np.float32)
    alone = {m: np.concatenate([ggs.fitness(pop[b:b + 1], tgt, H, W, 3.0, weight_mask=mask, boost_only=boost)
                                for b in range(5)]) for m, boost in MODES.items()}
    for a in (pop, tgt, mask, *alone.values()):
        a.setflags(write=False)
    return pop, tgt, mask, alone


@pytest.mark.parametrize("B", [1, 3, 4, 5])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("H,W", [(64, 128), (512, 512)])
def test_batch_scalar_has_the_bits_of_the_candidate_alone(H, W, mode, B):
    pop, tgt, mask, alone = _problem(H, W)
    assert np.isfinite(alone[mode]).all() and len(set(alone[mode].tolist())) == 5
    got = ggs.fitness(pop[:B], tgt, H, W, 3.0, weight_mask=mask, boost_only=MODES[mode])
    np.testing.assert_array_equal(got, alone[mode][:B])


def test_plan_set_group_of_three_equals_the_single_plans():
    H, W, K, group = 64, 128, 2, 3
    rng = np.random.default_rng(9)
    pop = O.synthetic_population(K * group, N, H, W, seed=6)
    targets = rng.uniform(0, 1, (K, H, W, 3)).astype(np.float32)
    masks = rng.uniform(0.4, 1.0, (K, H, W)).astype(np.float32)
    st = hip.Stream()
    g = hip.DeviceArray.from_host(pop)
    for mode in (ggs.GGS_FIT_WEIGHTED, ggs.GGS_FIT_BOOST):
        want = []
        for k in range(K):
            t, m = hip.DeviceArray.from_host(targets[k]), hip.DeviceArray.from_host(masks[k])
            gk, o = hip.DeviceArray.from_host(pop[k * group:(k + 1) * group]), hip.DeviceArray((group,))
            plan = ggs.TargetPlan(0, st.handle, t.ptr, m.ptr, mode, 1.0, H, W)
            try:
                plan.fitness_device(st.handle, gk.ptr, group, N, 9, 3.0, o.ptr)
                st.synchronize()
                want.append(o.to_host().copy())
            finally:
                plan.close()
        t, m, o = hip.DeviceArray.from_host(targets), hip.DeviceArray.from_host(masks), hip.DeviceArray((K * group,))
        ps = ggs.TargetPlanSet(0, st.handle, t.ptr, m.ptr, mode, 1.0, H, W, K)
        try:
            ps.fitness_device(st.handle, g.ptr, K * group, N, 9, group, 3.0, o.ptr)
            st.synchronize()
            got = o.to_host().copy()
        finally:
            ps.close()
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, np.concatenate(want))
