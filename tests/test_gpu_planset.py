"""Plan sets (ggs.TargetPlanSet, ggs_planset_* / raster_multi_kernel) on an MI355X.

One grouped launch over B = K * group candidates, candidate b against plan
b // group, must give every candidate the bits K separate ``TargetPlan`` calls
over the same slices give it: the library's fitness of a candidate does not
depend on the batch it rides in.  Every comparison is exact.

The shapes are the smallest that reach each grid / kernel path of the raster:

* 40x40, N 33, K 3, group 5: a partial tile, the instance without the saturation
  check, the separate finalize; group is no multiple of 8, so the candidate
  rotation over the XCDs crosses group borders;
* 128x512, N 16, K 2, group 3: 4 * tiles = 32, the smallest canvas on which the
  finalize folds into the raster (GGS_FITNESS_FOLD=1 folds the fitness API's);
* 40x40, N 600, K 2, group 4: N > 512, the saturation-checking instances;
* 24x24, N 4096, K 4, group 34: B = 136 > raster_chunk(4096) = 128, the chunked grid.
"""
from __future__ import annotations

import numpy as np
import pytest

import ggs
from ggs import ga, hip
from ggs.mask import compute_importance_mask

pytestmark = pytest.mark.gpu
MIN_S, MAX_S = 3.0, 0.1
MODES = {"none": ggs.GGS_FIT_NONE, "weighted": ggs.GGS_FIT_WEIGHTED, "boost": ggs.GGS_FIT_BOOST}
_inputs = {}


def _problem(H, W, N, K, group):
    """K targets / masks from distinct seeds and K * group genomes (built once per shape)."""
    key = (H, W, N, K, group)
    if key not in _inputs:
        targets = np.stack([np.random.default_rng(1000 * H + W + 17 * k).uniform(0, 1, (H, W, 3))
                            for k in range(K)]).astype(np.float32)
        masks = np.stack([compute_importance_mask(t, H, W, smooth=3, strength=0.7) for t in targets])
        masks = np.ascontiguousarray(masks, np.float32)
        pop = ga.new_population(K * group, N, H, W, MIN_S, MAX_S, np.random.default_rng(H + N + K))
        _inputs[key] = (targets, masks, np.ascontiguousarray(pop, np.float32))
    return _inputs[key]


def _separate(st, targets, masks, pop, mode, slices, plans_of):
    """Fitness of pop[slices[i]] against the single plan plans_of[i], one TargetPlan call each."""
    H, W = targets.shape[1:3]
    out = []
    for sl, k in zip(slices, plans_of):
        t = hip.DeviceArray.from_host(targets[k])
        m = hip.DeviceArray.from_host(masks[k]) if mode != ggs.GGS_FIT_NONE else None
        g = hip.DeviceArray.from_host(pop[sl])
        o = hip.DeviceArray((len(pop[sl]),))
        plan = ggs.TargetPlan(0, st.handle, t.ptr, m.ptr if m is not None else 0, mode, 1.0, H, W)
        try:
            plan.fitness_device(st.handle, g.ptr, len(pop[sl]), pop.shape[1], 9, 3.0, o.ptr)
            st.synchronize()
            out.append(o.to_host().copy())
        finally:
            plan.close()
    return out


def _grouped(st, targets, masks, pop, mode, group, K=None):
    H, W = targets.shape[1:3]
    K = len(targets) if K is None else K
    t = hip.DeviceArray.from_host(targets)
    m = hip.DeviceArray.from_host(masks) if mode != ggs.GGS_FIT_NONE else None
    g = hip.DeviceArray.from_host(pop)
    o = hip.DeviceArray((len(pop),))
    ps = ggs.TargetPlanSet(0, st.handle, t.ptr, m.ptr if m is not None else 0, mode, 1.0, H, W, K)
    try:
        ps.fitness_device(st.handle, g.ptr, len(pop), pop.shape[1], 9, group, 3.0, o.ptr)
        st.synchronize()
        return o.to_host().copy()
    finally:
        ps.close()


def _check(H, W, N, K, group, mode):
    targets, masks, pop = _problem(H, W, N, K, group)
    st = hip.Stream()
    slices = [slice(k * group, (k + 1) * group) for k in range(K)]
    want = _separate(st, targets, masks, pop, mode, slices, range(K))
    # the plans tell the targets apart: group 1's genomes against plan 0 score differently
    (cross,) = _separate(st, targets, masks, pop, mode, [slices[1]], [0])
    assert not np.array_equal(cross, want[1]), "plans 0 and 1 give the same fitness: the test sees no index"
    got = _grouped(st, targets, masks, pop, mode, group)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, np.concatenate(want))


@pytest.mark.parametrize("mode", list(MODES))
def test_partial_tile_separate_finalize_all_modes(mode):
    _check(40, 40, 33, 3, 5, MODES[mode])


@pytest.mark.parametrize("fold", [False, True], ids=["finalize_launch", "folded_finalize"])
def test_smallest_canvas_with_the_folded_finalize(fold, monkeypatch):
    monkeypatch.delenv("GGS_FITNESS_FOLD", raising=False)
    if fold:
        monkeypatch.setenv("GGS_FITNESS_FOLD", "1")
        ggs.profile_reset()
        ggs.profile_enable(True)
    try:
        _check(128, 512, 16, 2, 3, ggs.GGS_FIT_WEIGHTED)
        if fold:      # the folded path really ran: no finalize launch at all
            assert ggs.profile_read("finalize")[1] == 0
            assert ggs.profile_read("raster")[1] >= 4
    finally:
        if fold:
            ggs.profile_enable(False)


@pytest.mark.parametrize("fold", [False, True], ids=["finalize_launch", "folded_finalize"])
def test_folded_finalize_boost_mode_reads_each_plans_weight_sum(fold, monkeypatch):
    """Boost and weighted modes divide by the plan's own Sum w: the folded finalize
    and the finalize launch both have to pick plan b // group's weight block."""
    monkeypatch.delenv("GGS_FITNESS_FOLD", raising=False)
    if fold:
        monkeypatch.setenv("GGS_FITNESS_FOLD", "1")
    _check(128, 512, 16, 2, 3, ggs.GGS_FIT_BOOST)


def test_saturation_instances():
    _check(40, 40, 600, 2, 4, ggs.GGS_FIT_WEIGHTED)


def test_chunked_grid():
    _check(24, 24, 4096, 4, 34, ggs.GGS_FIT_WEIGHTED)


def test_one_plan_is_a_target_plan():
    H, W, N, K, group = 40, 40, 33, 3, 5
    targets, masks, pop = _problem(H, W, N, K, group)
    st = hip.Stream()
    (want,) = _separate(st, targets, masks, pop, ggs.GGS_FIT_WEIGHTED, [slice(None)], [0])
    got = _grouped(st, targets[:1], masks[:1], pop, ggs.GGS_FIT_WEIGHTED, len(pop))
    np.testing.assert_array_equal(got, want)


def test_fewer_groups_than_plans_use_the_first_plans():
    H, W, N, K, group = 40, 40, 33, 3, 5
    targets, masks, pop = _problem(H, W, N, K, group)
    st = hip.Stream()
    sub = pop[:2 * group]
    want = _separate(st, targets, masks, sub, ggs.GGS_FIT_WEIGHTED,
                     [slice(0, group), slice(group, 2 * group)], [0, 1])
    got = _grouped(st, targets, masks, sub, ggs.GGS_FIT_WEIGHTED, group)      # K = 3 plans, 2 groups
    np.testing.assert_array_equal(got, np.concatenate(want))
    # an empty batch is valid and touches nothing
    t = hip.DeviceArray.from_host(targets)
    m = hip.DeviceArray.from_host(masks)
    o = hip.DeviceArray((1,))
    ps = ggs.TargetPlanSet(0, st.handle, t.ptr, m.ptr, ggs.GGS_FIT_WEIGHTED, 1.0, H, W, K)
    try:
        ps.fitness_device(st.handle, 0, 0, N, 9, group, 3.0, o.ptr)
        st.synchronize()
    finally:
        ps.close()


def test_more_groups_than_plans_is_an_input_error():
    H, W, N, K, group = 40, 40, 33, 3, 5
    targets, masks, pop = _problem(H, W, N, K, group)
    st = hip.Stream()
    t = hip.DeviceArray.from_host(targets)
    m = hip.DeviceArray.from_host(masks)
    g = hip.DeviceArray.from_host(pop)
    o = hip.DeviceArray((len(pop),))
    ps = ggs.TargetPlanSet(0, st.handle, t.ptr, m.ptr, ggs.GGS_FIT_WEIGHTED, 1.0, H, W, 2)   # 2 plans only
    try:
        with pytest.raises(ggs.GGSInputError, match="plans"):
            ps.fitness_device(st.handle, g.ptr, len(pop), N, 9, group, 3.0, o.ptr)           # 3 groups
        with pytest.raises(ggs.GGSInputError, match="multiple"):
            ps.fitness_device(st.handle, g.ptr, len(pop), N, 9, 4, 3.0, o.ptr)
        with pytest.raises(ggs.GGSInputError, match="group"):
            ps.fitness_device(st.handle, g.ptr, len(pop), N, 9, 0, 3.0, o.ptr)
    finally:
        ps.close()
