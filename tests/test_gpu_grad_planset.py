"""The gradient with a target per candidate (ggs_fitness_grad_targets,
ggs_fitness_grad_device_planset / grad_set_strip_kernel) on an MI355X.

Candidate b of one grouped call, differentiated against image b // group, must
carry the bytes ``api.fitness_grad`` gives it against that image alone, fitness
and gradient.  The K images differ, so a wrong image index cannot pass.

* 40 x 48 (2 x 3 strips of 16 x 32, the lower strip row partial), N = 70 (crosses the
  64-splat chunk), K = 3, group = 2, B = 6, every mode, strides C = 9 and 12;
* B = 4: fewer groups than plans, the first two plans;
* 256 x 256, N = 512, K = 2, group = 8, B = 16: one candidate's partials are
  128 strips x 512 x 48 B = 3 MiB, the 40 MiB budget holds 13, so the second chunk
  begins inside the second group.
"""
from __future__ import annotations

import numpy as np
import pytest

import ggs
from ggs import api, ga, hip

pytestmark = pytest.mark.gpu
MIN_S, MAX_S = 3.0, 0.1
MODES = {"none": ggs.GGS_FIT_NONE, "weighted": ggs.GGS_FIT_WEIGHTED, "boost": ggs.GGS_FIT_BOOST}
_inputs, _solo = {}, {}


def _problem(H, W, N, K, B, C):
    key = (H, W, N, K, B, C)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * H + W + N)
        targets = rng.uniform(0, 1, (K, H, W, 3)).astype(np.float32)
        masks = rng.uniform(0.1, 1.0, (K, H, W)).astype(np.float32)
        pop = np.zeros((B, N, C), np.float32)
        pop[..., :9] = ga.new_population(B, N, H, W, MIN_S, MAX_S, np.random.default_rng(H + N + K))
        pop[..., 9:] = rng.uniform(-1, 1, (B, N, C - 9))          # columns past 9 are not read
        _inputs[key] = (targets, masks, pop)
    return _inputs[key]


def _kw(mode, mask):
    return dict(weight_mask=None if mode == "none" else mask, boost_only=mode == "boost", boost_beta=0.75)


def _per_image(key, mode, group):
    """(fit [B], grad [B,N,9]) by one single-target call per image (computed once, shared)."""
    if (key, mode, group) not in _solo:
        targets, masks, pop = _problem(*key)
        H, W = key[0], key[1]
        fits, grads = [], []
        for k in range(len(pop) // group):
            f, g = api.fitness_grad(pop[k * group:(k + 1) * group], targets[k], H, W, 3.0, **_kw(mode, masks[k]))
            fits.append(f)
            grads.append(g)
        _solo[key, mode, group] = (np.concatenate(fits), np.concatenate(grads))
    return _solo[key, mode, group]


def _device_form(key, mode, group):
    targets, masks, pop = _problem(*key)
    H, W, N, K, B, C = key
    st = hip.Stream()
    t = hip.DeviceArray.from_host(targets)
    m = hip.DeviceArray.from_host(masks) if mode != "none" else None
    g = hip.DeviceArray.from_host(pop)
    o, d = hip.DeviceArray((B,)), hip.DeviceArray((B, N, 9))
    mp = m.ptr if m is not None else 0
    ps = ggs.TargetPlanSet(0, st.handle, t.ptr, mp, MODES[mode], 0.75, H, W, K)
    try:
        ps.fitness_grad(st.handle, g.ptr, B, N, C, group, t.ptr, mp, 3.0, o.ptr, d.ptr)
        st.synchronize()
        return o.to_host().copy(), d.to_host().copy()
    finally:
        ps.close()


@pytest.mark.parametrize("C", [9, 12])
@pytest.mark.parametrize("mode", list(MODES))
def test_a_candidate_has_the_bytes_of_the_call_against_its_image_alone(mode, C):
    key = (40, 48, 70, 3, 6, C)
    targets, masks, pop = _problem(*key)
    want_f, want_g = _per_image(key, mode, 2)
    # the images tell each other apart: group 1's genomes against image 0 differ
    cross_f, cross_g = api.fitness_grad(pop[2:4], targets[0], 40, 48, 3.0, **_kw(mode, masks[0]))
    assert not np.array_equal(cross_f, want_f[2:4]) and not np.array_equal(cross_g, want_g[2:4])
    fit, grad = api.fitness_grad(pop, targets, 40, 48, 3.0, group=2, **_kw(mode, masks))
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    assert fit.tobytes() == want_f.tobytes()
    assert grad.tobytes() == want_g.tobytes()
    dfit, dgrad = _device_form(key, mode, 2)
    assert dfit.tobytes() == want_f.tobytes()
    assert dgrad.tobytes() == want_g.tobytes()
    # reruns
    fit2, grad2 = api.fitness_grad(pop, targets, 40, 48, 3.0, group=2, **_kw(mode, masks))
    assert fit2.tobytes() == fit.tobytes() and grad2.tobytes() == grad.tobytes()


def test_fewer_groups_than_plans_use_the_first_plans():
    key = (40, 48, 70, 3, 6, 9)
    targets, masks, pop = _problem(*key)
    want_f, want_g = _per_image(key, "weighted", 2)
    fit, grad = api.fitness_grad(pop[:4], targets, 40, 48, 3.0, group=2, **_kw("weighted", masks))
    assert fit.tobytes() == want_f[:4].tobytes() and grad.tobytes() == want_g[:4].tobytes()


def test_a_chunk_boundary_inside_a_group():
    key = (256, 256, 512, 2, 16, 9)
    targets, masks, pop = _problem(*key)
    want_f, want_g = _per_image(key, "weighted", 8)
    fit, grad = api.fitness_grad(pop, targets, 256, 256, 3.0, group=8, **_kw("weighted", masks))
    assert fit.tobytes() == want_f.tobytes()
    for b in range(16):
        assert grad[b].tobytes() == want_g[b].tobytes(), b


def test_a_live_set_refuses_what_would_read_past_its_images():
    """GGS_EINVAL before any launch: more groups than plans, B no multiple of group, a
    masked mode without the masks.  The outputs keep their bytes."""
    key = (40, 48, 70, 3, 6, 9)
    targets, masks, pop = _problem(*key)
    H, W, N, K, B, C = key
    st = hip.Stream()
    t, m, g = (hip.DeviceArray.from_host(a) for a in (targets, masks, pop))
    o, d = hip.DeviceArray.from_host(np.full((B,), 7, np.float32)), hip.DeviceArray.from_host(
        np.full((B, N, 9), 7, np.float32))
    ps = ggs.TargetPlanSet(0, st.handle, t.ptr, m.ptr, MODES["weighted"], 0.75, H, W, K)
    try:
        for nb, group, mp, word in ((6, 1, m.ptr, "holds"), (4, 1, m.ptr, "holds"), (5, 2, m.ptr, "multiple"),
                                    (6, 0, m.ptr, "group="), (6, 2, 0, "mask")):
            with pytest.raises(ggs.GGSInputError, match=word):
                ps.fitness_grad(st.handle, g.ptr, nb, N, C, group, t.ptr, mp, 3.0, o.ptr, d.ptr)
        with pytest.raises(ggs.GGSInputError, match="null"):
            ps.fitness_grad(st.handle, g.ptr, B, N, C, 2, 0, m.ptr, 3.0, o.ptr, d.ptr)
        st.synchronize()
        assert (o.to_host() == 7).all() and (d.to_host() == 7).all()
        # and the set still works
        ps.fitness_grad(st.handle, g.ptr, B, N, C, 2, t.ptr, m.ptr, 3.0, o.ptr, d.ptr)
        st.synchronize()
        assert o.to_host().tobytes() == _per_image(key, "weighted", 2)[0].tobytes()
    finally:
        ps.close()
