"""Target preparation and importance mask on the device (csrc/ggs_mask.hip) on an
MI355X: ggs_quantiles, ggs_targets_prepare and ggs_targets_prepare_device.

1. ``ggs_quantiles`` against ``np.sort`` / ``np.quantile``: where q (n - 1) is an
   integer the result IS that order statistic (bitwise; -0 counts as +0), otherwise
   it is within 1 float32 ulp of float32(np.quantile(float64(x), q)).
2. Device targets and masks against the reference's own outputs (mask.npz, the
   fitness.npz masks, headline_512.npz, mask_edges.npz) at the bars
   tests/test_mask.py applies to the host path: masks 2e-5, targets 5e-6.
3. Determinism and layout: a K = 3 call is three K = 1 calls, two runs agree, and
   the device form on a caller's stream is the host-pointer form — all bit for bit.
4. Degenerate images (constant; a two-level checker): finite, within
   [1 - strength + strength floor, 1] and batch-invariant.  No parity claim: the
   reference's _norm01 divides by 1e-12 there.
5. ``genetic_approx_many(prep="device")`` is a DeviceGAIslands run on what
   ``prepare_targets(backend="device")`` returns.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ggs
from conftest import load_golden
from ggs import _lib, ga, hip
from ggs import mask as gm
from ggs.ga_device import run_device_ga_islands

pytestmark = pytest.mark.gpu
KW = dict(edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3, gamma=0.7, floor=0.15, smooth=3)
MASK_ATOL, TARGET_ATOL = 2e-5, 5e-6


def _dev(images, H, W, strength=0.7, **kw):
    return gm.prepare_targets(images, H, W, strength=strength, backend="device", device=0, **{**KW, **kw})


# ---- 1. quantiles ----------------------------------------------------------------------
QS = [0.02, 0.98]


def _inputs(n):
    rng = np.random.default_rng(n)
    mixed = rng.normal(0, 3, n).astype(np.float32)                     # negatives and positives
    ties = rng.integers(-2, 3, n).astype(np.float32)                   # heavy ties around zero ...
    ties[ties == 0] = np.where(rng.uniform(size=int((ties == 0).sum())) < 0.5, -0.0, 0.0)   # ... of both signs
    small = (rng.uniform(0, 1, n) ** 8).astype(np.float32)             # many exponents, tiny values
    return {"mixed": mixed, "ties": ties, "all_equal": np.full(n, -1.25, np.float32), "small": small,
            "zeros": np.where(np.arange(n) % 2 == 0, -0.0, 0.0).astype(np.float32)}


@pytest.mark.parametrize("n", [1, 2, 51, 2501, 100003])
def test_quantiles_are_numpys(n):
    for name, x in _inputs(n).items():
        got = gm.quantiles(x, QS)
        assert got.dtype == np.float32 and got.shape == (2,)
        srt = np.sort(x)
        for q, g in zip(QS, got):
            idx = q * (n - 1)
            if n in (51, 2501):
                assert float(idx).is_integer(), (n, q, idx)
            if float(idx).is_integer():
                want = srt[int(idx)]
                assert (g + np.float32(0)).view(np.uint32) == (want + np.float32(0)).view(np.uint32), \
                    (name, n, q, g, want)
            else:
                want = np.float32(np.quantile(x.astype(np.float64), q))
                assert abs(float(g) - float(want)) <= float(np.spacing(np.abs(want))), (name, n, q, g, want)


def test_quantiles_more_points_share_one_select():
    x = np.random.default_rng(3).normal(0, 1, 4099).astype(np.float32)
    qs = [0.0, 0.02, 0.25, 0.5, 0.75, 0.98, 1.0]
    got = gm.quantiles(x, qs)
    want = np.quantile(x.astype(np.float64), qs).astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), (got, want)
    assert got[0] == x.min() and got[-1] == x.max()


# ---- 2. the reference's fixtures -------------------------------------------------------
def test_mask_npz():
    d = load_golden("mask.npz")
    for strength in (1.0, 0.7):
        t, m = _dev(d["target"][None], 96, 80, strength)
        np.testing.assert_array_equal(t[0], d["target"])               # same size, range [0, 1]: the identity
        err = float(np.abs(m[0] - d[f"mask_s{strength}"]).max())
        print(f"mask.npz 96x80 strength {strength}: max|device - reference| = {err:.3e}")
        assert err <= MASK_ATOL
    t, m = _dev(d["target_u8"][None], 64, 48, 0.7)
    et = float(np.abs(t[0] - d["target_prep_64x48"]).max())
    em = float(np.abs(m[0] - d["mask_resized_64x48"]).max())
    print(f"mask.npz 100x70 -> 64x48: target {et:.3e}, mask {em:.3e}")
    assert et <= TARGET_ATOL and em <= MASK_ATOL
    t, _ = _dev(d["target_u8"][None], 150, 90, 0.7)
    et = float(np.abs(t[0] - d["target_prep_150x90"]).max())
    print(f"mask.npz 100x70 -> 150x90: target {et:.3e}")
    assert et <= TARGET_ATOL


@pytest.mark.parametrize("case", ["f64", "f128", "f40x56"])
def test_fitness_fixture_masks(case):
    d = load_golden("fitness.npz")
    H, W = (int(v) for v in d[f"{case}__HW"])
    _, m = _dev(d[f"{case}__target"][None], H, W, 0.7)
    err = float(np.abs(m[0] - d[f"{case}__mask"]).max())
    print(f"fitness.npz {case}: max|device - reference| = {err:.3e}")
    assert err <= MASK_ATOL


def test_headline_512_mask():
    d = load_golden("headline_512.npz")
    t, m = _dev(d["target_u8"][None], 512, 512, 0.7)                   # uint8 in: the /255 happens on the device
    np.testing.assert_array_equal(t[0], d["target_u8"].astype(np.float32) / np.float32(255.0))
    err = float(np.abs(m[0] - d["mask"]).max())
    print(f"headline_512: max|device - reference| = {err:.3e}")
    assert err <= MASK_ATOL


def test_mask_edges_npz():
    d = load_golden("mask_edges.npz")
    for case in ("t33x47", "t9x13", "u8_100x70", "max400"):
        H, W = (int(v) for v in d[f"{case}__HW"])
        t, m = _dev(d[f"{case}__image"][None], H, W, float(d[f"{case}__strength"]))
        et = float(np.abs(t[0] - d[f"{case}__target"]).max())
        em = float(np.abs(m[0] - d[f"{case}__mask"]).max())
        print(f"mask_edges.npz {case}: target {et:.3e}, mask {em:.3e}")
        assert et <= TARGET_ATOL and em <= MASK_ATOL, case
    stack = np.stack([d[f"stack{i}__image"] for i in range(3)])
    t, m = _dev(stack, 48, 40, 0.7)
    for i in range(3):
        et = float(np.abs(t[i] - d[f"stack{i}__target"]).max())
        em = float(np.abs(m[i] - d[f"stack{i}__mask"]).max())
        print(f"mask_edges.npz stack{i}: target {et:.3e}, mask {em:.3e}")
        assert et <= TARGET_ATOL and em <= MASK_ATOL, i


# ---- 3. determinism and layout -----------------------------------------------------------
def _three_images():
    rng = np.random.default_rng(12)
    imgs = [rng.uniform(0, hi, (70, 53, 3)).astype(np.float32) for hi in (1.0, 255.0, 400.0)]
    return np.stack(imgs)


def test_batch_is_its_images_and_runs_repeat():
    imgs = _three_images()
    H, W = 45, 38                               # more than one workgroup per image, no multiple of anything
    t, m = _dev(imgs, H, W)
    t2, m2 = _dev(imgs, H, W)
    np.testing.assert_array_equal(t, t2)
    np.testing.assert_array_equal(m, m2)
    for k in range(3):
        tk, mk = _dev(imgs[k:k + 1], H, W)
        np.testing.assert_array_equal(tk[0], t[k], err_msg=f"target {k}")
        np.testing.assert_array_equal(mk[0], m[k], err_msg=f"mask {k}")
    assert np.abs(m[0] - m[1]).max() > 1e-3     # the images differ


def test_device_form_on_a_stream_is_the_host_form():
    imgs = _three_images()
    K, H0, W0 = imgs.shape[:3]
    H, W = 45, 38
    t, m = _dev(imgs, H, W)
    hip.set_device(0)
    st = hip.Stream()
    d_img = hip.DeviceArray.from_host(imgs)
    d_t = hip.DeviceArray((K, H, W, 3))
    d_m = hip.DeviceArray((K, H, W))
    prm = gm.mask_params(strength=0.7, **KW)
    try:
        _lib.check(ggs.lib.ggs_targets_prepare_device(0, C.c_void_p(st.handle), C.c_void_p(d_img.ptr), K, H0, W0,
                                                      H, W, prm, C.c_void_p(d_t.ptr), C.c_void_p(d_m.ptr)),
                   "ggs_targets_prepare_device")
        np.testing.assert_array_equal(d_t.to_host(st), t)
        np.testing.assert_array_equal(d_m.to_host(st), m)
        # targets only
        d_t2 = hip.DeviceArray((K, H, W, 3))
        _lib.check(ggs.lib.ggs_targets_prepare_device(0, C.c_void_p(st.handle), C.c_void_p(d_img.ptr), K, H0, W0,
                                                      H, W, None, C.c_void_p(d_t2.ptr), None),
                   "ggs_targets_prepare_device")
        np.testing.assert_array_equal(d_t2.to_host(st), t)
        d_t2.free()
    finally:
        st.synchronize()
        for a in (d_img, d_t, d_m):
            a.free()
        st.close()


def test_other_parameters_follow_the_host():
    """No smoothing, one scale, gamma 1, strength 1: the paths the defaults skip, against
    the host restatement (same arithmetic, so the bar of the fixtures holds)."""
    img = np.random.default_rng(21).uniform(0, 1, (1, 37, 29, 3)).astype(np.float32)
    for kw in (dict(smooth=0), dict(edge_scales=(4,), smooth=5), dict(gamma=1.0, edge_scales=(2, 1)),
               dict(floor=0.0, w_edge=0.2, w_var=0.8)):
        t, m = _dev(img, 37, 29, 1.0, **kw)
        want = gm.compute_importance_mask(gm.prepare_target(img[0], 37, 29), 37, 29, strength=1.0, **{**KW, **kw})
        err = float(np.abs(m[0] - want).max())
        print(f"{kw}: max|device - host| = {err:.3e}")
        assert err <= MASK_ATOL, kw


# ---- 4. degenerate images -------------------------------------------------------------------
def test_degenerate_images_are_finite_bounded_and_batch_invariant():
    H, W, strength, floor = 32, 40, 0.7, 0.15
    const = np.full((H, W, 3), 0.5, np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.where(((yy // 4 + xx // 4) % 2)[..., None] == 0, 0.25, 0.75).astype(np.float32) * np.ones(3, np.float32)
    noise = np.random.default_rng(4).uniform(0, 1, (H, W, 3)).astype(np.float32)
    batch = np.stack([const, checker, noise])
    t, m = _dev(batch, H, W, strength)
    np.testing.assert_array_equal(t, batch)
    assert np.isfinite(m).all()
    lo = 1.0 - strength + strength * floor
    assert m.min() >= lo - 1e-6 and m.max() <= 1.0 + 1e-6, (m.min(), m.max())     # float32 rounding of the bounds
    for k in range(3):
        _, mk = _dev(batch[k:k + 1], H, W, strength)
        np.testing.assert_array_equal(mk[0], m[k], err_msg=f"image {k}")
    _, mr = _dev(batch[::-1], H, W, strength)
    np.testing.assert_array_equal(mr[::-1], m)


# ---- 5. end to end -------------------------------------------------------------------------
def test_genetic_approx_many_with_device_prep():
    H = W = 32
    K, seed = 2, 5
    images = [np.random.default_rng(90 + k).uniform(0, 255, (41 + k, 37, 3)).astype(np.float32) for k in range(K)]
    cfg = dict(mut_sigma_max={"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0},
               mut_sigma_min={"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0},
               schedule="cosine")
    kw = dict(tour_k=3, elite_k=2, cxpb=0.3, mutpb=0.1, min_scale_splats=3.0, max_scale_splats=0.1, k_sigma=3.0,
              boost_only=False, **cfg)
    many = ga.genetic_approx_many(images, H, W, "cuda:0", pop_size=8, n_splats=16, generations=5, mask_strength=0.7,
                                  seed=seed, progress=False, return_state=True, prep="device", **kw)
    t, m = gm.prepare_targets(images, H, W, strength=0.7, backend="device", device=0, **KW)
    seeds = [seed + k for k in range(K)]
    pops = np.stack([ga.new_population(8, 16, H, W, 3.0, 0.1, np.random.default_rng(s)) for s in seeds])
    st = run_device_ga_islands(t, m, pops, seeds, 5, migrate_every=0, n_migrants=0, chunk=50, device=0, **kw)
    for k in range(K):
        np.testing.assert_array_equal(many[k][0], st["best"][k])
        assert many[k][1] == float(st["best_fit"][k])
        np.testing.assert_array_equal(many[k][2]["population"], st["population"][k])
        np.testing.assert_array_equal(many[k][2]["fitness"], st["fitness"][k])
