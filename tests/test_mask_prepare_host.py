"""Target preparation and importance mask for K images: what holds without a GPU.

* ggs_targets_prepare / ggs_targets_prepare_device / ggs_quantiles are declared,
  exported and bound, and reject bad arguments (GGS_EINVAL, with a message) before
  any device is initialised — on a host without a GPU a well-formed call gets as
  far as GGS_ENODEV, a malformed one never does;
* the host ggs.mask against the reference's own outputs: the edge-case fixtures
  (tests/golden/mask_edges.npz, make_golden_mask_edges.py) and the committed 512^2
  mask (headline_512.npz), at the bars tests/test_mask.py applies (2e-5 / 5e-6);
* ``prepare_targets(backend="host")`` is the per-image functions bit for bit, and
  grouping by input shape keeps the input order.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ggs
from conftest import load_golden
from ggs import _lib
from ggs import mask as gm

KW = dict(edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3, gamma=0.7, floor=0.15, smooth=3)
EDGE_CASES = ["t33x47", "t9x13", "u8_100x70", "max400", "stack0", "stack1", "stack2"]
NEW = ("ggs_targets_prepare", "ggs_targets_prepare_device", "ggs_quantiles")


def _fp(a):
    return a.ctypes.data_as(_lib._f32p)


# ---- the C boundary ------------------------------------------------------------------
def test_new_entry_points_are_declared_exported_and_bound():
    from test_capi import declared_functions
    names = declared_functions()
    for n in NEW:
        assert n in names and n in _lib.SIGNATURES and hasattr(ggs.lib, n)
    assert sorted(_lib.SIGNATURES) == names
    # typedef struct ggs_mask_params: 1 + 4 int32, 5 floats, 1 int32
    assert C.sizeof(_lib.MaskParams) == 44
    assert [f[0] for f in _lib.MaskParams._fields_] == ["n_scales", "edge_scales", "w_edge", "w_var", "gamma",
                                                       "floor", "strength", "smooth"]


def _call(K=1, H0=8, W0=8, H=8, W=8, params="default", null=(), device_form=False, **over):
    img = np.zeros((max(K, 1), H0, W0, 3), np.float32)
    tgt = np.zeros((max(K, 1), max(H, 1), max(W, 1), 3), np.float32)
    msk = np.zeros((max(K, 1), max(H, 1), max(W, 1)), np.float32)
    prm = None
    if params == "default":
        prm = gm.mask_params(strength=0.7, **KW)
        for k, v in over.items():
            if k == "edge_scales":
                prm.n_scales = len(v)
                for i, s in enumerate(v):
                    prm.edge_scales[i] = s
            else:
                setattr(prm, k, v)
    a = {"images": _fp(img), "targets": _fp(tgt), "masks": _fp(msk) if prm is not None else None}
    for n in null:
        a[n] = None
    if over.get("want_masks_without_params"):
        a["masks"] = _fp(msk)
    if device_form:
        cast = {k: (C.cast(v, C.c_void_p) if v is not None else None) for k, v in a.items()}
        rc = ggs.lib.ggs_targets_prepare_device(0, None, cast["images"], K, H0, W0, H, W, prm, cast["targets"],
                                                cast["masks"])
    else:
        rc = ggs.lib.ggs_targets_prepare(a["images"], K, H0, W0, H, W, prm, a["targets"], a["masks"], 0)
    return rc, ggs.lib.ggs_last_error().decode()


BAD = [
    (dict(K=0), "K=0"),
    (dict(K=-3), "K=-3"),
    (dict(null=("images",)), "null"),
    (dict(null=("targets",)), "null"),
    (dict(null=("masks",)), "null masks"),
    (dict(params=None, want_masks_without_params=True), "targets only"),
    (dict(n_scales=0), "n_scales=0"),
    (dict(n_scales=5), "n_scales=5"),
    (dict(edge_scales=(1, 0, 4)), "edge scale 0"),
    (dict(edge_scales=(1, 2, 16)), "edge scale 16"),          # 8 / 16 < 1
    (dict(H=40, W=6, H0=40, W0=6, edge_scales=(1, 8)), "edge scale 8"),   # W / s < 1 only
    (dict(smooth=2), "smooth=2"),
    (dict(smooth=4), "smooth=4"),
    (dict(H=3, W=40), "min(H, W) = 3"),
    (dict(H=40, W=2), "min(H, W) = 2"),
    (dict(H0=0), "must be >= 1"),
]


@pytest.mark.parametrize("device_form", [False, True])
@pytest.mark.parametrize("kw,msg", BAD)
def test_bad_arguments_are_einval_before_any_device(kw, msg, device_form):
    rc, err = _call(device_form=device_form, **kw)
    assert rc == _lib.GGS_EINVAL, (rc, err)
    assert msg in err, err


def test_targets_only_is_well_formed_and_reaches_the_device_layer():
    """params == NULL with masks == NULL is valid: without a GPU the call gets past the
    argument checks to GGS_ENODEV (with one it runs); smooth = 0 and odd windows too."""
    have_gpu = ggs.lib.ggs_init(0) > 0
    want = (_lib.GGS_OK,) if have_gpu else (_lib.GGS_ENODEV,)
    for kw in (dict(params=None), dict(smooth=0), dict(smooth=5), dict(edge_scales=(2,)), dict(H=4, W=4, H0=9, W0=5,
                                                                                            edge_scales=(1, 4))):
        rc, err = _call(**kw)
        assert rc in want, (kw, rc, err)


def test_quantiles_rejects_bad_arguments():
    x = np.zeros(4, np.float32)
    out = np.zeros(8, np.float32)
    f64 = C.POINTER(C.c_double)

    def call(xp, n, q, nq, op):
        qa = np.asarray(q, np.float64)
        return ggs.lib.ggs_quantiles(xp, n, qa.ctypes.data_as(f64) if q is not None else None, nq, op)

    assert call(None, 4, [0.5], 1, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 4, None, 1, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 4, [0.5], 1, None) == _lib.GGS_EINVAL
    assert call(_fp(x), 0, [0.5], 1, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 2**31, [0.5], 1, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 4, [0.5], 0, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 4, [0.5] * 9, 9, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 4, [1.5], 1, _fp(out)) == _lib.GGS_EINVAL
    assert call(_fp(x), 4, [float("nan")], 1, _fp(out)) == _lib.GGS_EINVAL
    assert b"outside" in ggs.lib.ggs_last_error()


# ---- the host restatement against the reference --------------------------------------
@pytest.mark.parametrize("case", EDGE_CASES)
def test_host_mask_matches_reference_edge_cases(case):
    d = load_golden("mask_edges.npz")
    H, W = (int(v) for v in d[f"{case}__HW"])
    t = gm.prepare_target(d[f"{case}__image"], H, W)
    np.testing.assert_allclose(t, d[f"{case}__target"], atol=5e-6, rtol=0)
    m = gm.compute_importance_mask(t, H, W, strength=float(d[f"{case}__strength"]), **KW)
    np.testing.assert_allclose(m, d[f"{case}__mask"], atol=2e-5, rtol=0)


def test_edge_fixture_exercises_the_double_rescale():
    d = load_golden("mask_edges.npz")
    assert d["max400__image"].max() == 400.0
    assert d["max400__target"].max() > 1.5            # still above the rule after one /255


def test_host_mask_matches_reference_512():
    """The committed 512^2 mask: target u8 / 255, the arguments of make_golden_512.py."""
    d = load_golden("headline_512.npz")
    target = d["target_u8"].astype(np.float32) / np.float32(255.0)
    m = gm.compute_importance_mask(target, 512, 512, strength=0.7, **KW)
    np.testing.assert_allclose(m, d["mask"], atol=2e-5, rtol=0)


# ---- prepare_targets on the host -------------------------------------------------------
def _mixed_images():
    rng = np.random.default_rng(77)
    shapes = [(30, 22), (26, 26), (30, 22), (20, 31), (26, 26), (30, 22)]
    return [rng.uniform(0, 255 if i % 2 else 1, (h, w, 3)).astype(np.float32) for i, (h, w) in enumerate(shapes)]


def test_prepare_targets_host_is_the_per_image_functions():
    imgs = _mixed_images()
    H, W = 24, 20
    t, m = gm.prepare_targets(imgs, H, W, strength=0.7, backend="host")
    assert t.shape == (6, H, W, 3) and m.shape == (6, H, W) and t.dtype == m.dtype == np.float32
    for k, im in enumerate(imgs):
        tk = gm.prepare_target(im, H, W)
        np.testing.assert_array_equal(t[k], tk)
        np.testing.assert_array_equal(m[k], gm.compute_importance_mask(tk, H, W, strength=0.7, **KW))
    # a 4-D array is a list of its images
    stack = np.stack([imgs[0], imgs[2], imgs[5]])
    t4, m4 = gm.prepare_targets(stack, H, W, strength=0.7, backend="host")
    np.testing.assert_array_equal(t4, t[[0, 2, 5]])
    np.testing.assert_array_equal(m4, m[[0, 2, 5]])
    with pytest.raises(ValueError):
        gm.prepare_targets(imgs, H, W, strength=0.7, backend="torch")
    with pytest.raises(ValueError):
        gm.prepare_targets([], H, W, strength=0.7, backend="host")


def test_grouping_by_shape_preserves_order(monkeypatch):
    imgs = _mixed_images()
    assert gm.group_by_shape(imgs) == [((30, 22), [0, 2, 5]), ((26, 26), [1, 4]), ((20, 31), [3])]
    # the device backend makes one library call per shape and puts the results back in
    # input order: a stand-in for the call marks each output with its image's first value
    calls = []

    def fake(images, K, H0, W0, H, W, prm, targets, masks, device):
        calls.append((K, H0, W0))
        src = np.ctypeslib.as_array(images, (K, H0, W0, 3))
        np.ctypeslib.as_array(targets, (K, H, W, 3))[:] = src[:, :1, :1, :1]
        np.ctypeslib.as_array(masks, (K, H, W))[:] = src[:, :1, :1, 0] + 1.0
        return 0

    monkeypatch.setattr(_lib.lib, "ggs_targets_prepare", fake, raising=True)
    t, m = gm.prepare_targets(imgs, 8, 8, strength=0.7, backend="device", device=0)
    assert calls == [(3, 30, 22), (2, 26, 26), (1, 20, 31)]
    for k, im in enumerate(imgs):
        assert np.all(t[k] == im[0, 0, 0]) and np.all(m[k] == im[0, 0, 0] + np.float32(1.0)), k


def test_genetic_approx_many_rejects_an_unknown_prep():
    from ggs import ga
    with pytest.raises(ValueError, match="prep"):
        ga.genetic_approx_many([np.zeros((8, 8, 3), np.float32)], 8, 8, "cuda", 4, 4, 1, 2, 1, 0.5, 0.1, {}, {},
                               "cosine", 3.0, 0.1, 3.0, 0.7, False, prep="gpu")
