"""tests/_loss_ref.py, the image loss's reference, pinned on the CPU (no device):

* its SSIM map against a direct, non-separable numpy double loop over an explicitly
  zero-padded image at 5 x 7 (smaller than the window on both axes);
* its autograd cotangent against the analytic three-map formula the kernel uses
  (``_loss_ref.analytic_cot``) at 5 x 7, 11 x 11, 33 x 47 and 70 x 100, and against
  central differences;
* x == y gives loss exactly 0; weights (0, 1, 0) are ``oracle.fitness_many`` in mode none.

Bars: both sides of the first two comparisons are float64 evaluations of the same
real-valued expression with O(100) operations per value and derivative maps of size
<= 2 / C2 ~ 2200 that cancel to O(1), so 2200 * 100 * 2^-53 ~ 2.5e-11 bounds the
relative difference; 1e-10 is the bar.  Central differences with step h = 1e-6 carry
O(h^2) truncation times the third derivative (~1 / C2^2 at worst) and 2^-53 / h
rounding: 1e-6 relative to max|cot| is the bar.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _loss_ref as ref
import ggs_oracle as oracle

SIZES = [(5, 7), (11, 11), (33, 47), (70, 100)]
WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.8, 0.0, 0.2)]


def _images(H, W, seed, flat=False):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    y = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    if flat:                                   # a constant half where x == y
        y[:, : W // 2] = 1.0
        x[:, : W // 2] = 1.0
    return x, y


def _direct_ssim(x, y):
    """m [H,W,3] by the definition: 121 taps per pixel over a zero-padded copy."""
    H, W, _ = x.shape
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    g /= g.sum()
    w2 = g[:, None] * g[None, :]
    R = ref.RADIUS
    xp = np.zeros((H + 2 * R, W + 2 * R, 3))
    yp = np.zeros_like(xp)
    xp[R:R + H, R:R + W] = x
    yp[R:R + H, R:R + W] = y
    m = np.empty((H, W, 3))
    for i in range(H):
        for j in range(W):
            for c in range(3):
                a, b = xp[i:i + 11, j:j + 11, c], yp[i:i + 11, j:j + 11, c]
                mux, muy = (w2 * a).sum(), (w2 * b).sum()
                sxx = (w2 * a * a).sum() - mux * mux
                syy = (w2 * b * b).sum() - muy * muy
                sxy = (w2 * a * b).sum() - mux * muy
                m[i, j, c] = ((2 * mux * muy + ref.C1) * (2 * sxy + ref.C2)) / \
                             ((mux * mux + muy * muy + ref.C1) * (sxx + syy + ref.C2))
    return m


def test_taps_are_the_normalised_gaussian():
    g = ref.taps().numpy()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15
    assert np.allclose(g / g[5], np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5), rtol=1e-15)


@pytest.mark.parametrize("flat", [False, True])
def test_ssim_map_against_the_direct_double_loop(flat):
    x, y = _images(5, 7, 1, flat)
    got = ref.ssim_map(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(y.astype(np.float64)))
    want = _direct_ssim(x.astype(np.float64), y.astype(np.float64))
    err = np.abs(got.permute(1, 2, 0).numpy() - want).max()
    print(f"5x7 flat={flat}: max |ssim_map - direct| {err:.2e}")
    assert err <= 1e-10


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flat", [False, True])
def test_autograd_cotangent_is_the_three_map_formula(size, flat):
    H, W = size
    x, y = _images(H, W, 10 + H, flat)
    for w in WEIGHTS:
        loss, cot = ref.image_loss(x[None], y, w)
        want = ref.analytic_cot(x, y, w)
        rel = np.abs(cot[0] - want).max() / np.abs(want).max()
        print(f"{H}x{W} flat={flat} w={w}: max |autograd - analytic| / max|cot| {rel:.2e}")
        assert rel <= 1e-10, (w, rel)


def test_cotangent_against_central_differences():
    H, W = 5, 7
    x, y = _images(H, W, 3)
    w = (0.3, 0.5, 0.2)
    _, cot = ref.image_loss(x[None], y, w)
    xt, yt = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(y.astype(np.float64))
    assert np.abs(x.astype(np.float64) - y).min() > 1e-5       # no |d| kink inside a step
    h = 1e-6
    fd = np.empty((H, W, 3))
    for idx in np.ndindex(H, W, 3):
        e = torch.zeros_like(xt)
        e[idx] = h
        fd[idx] = (float(ref.loss_tensor(xt + e, yt, w)) - float(ref.loss_tensor(xt - e, yt, w))) / (2 * h)
    rel = np.abs(cot[0] - fd).max() / np.abs(fd).max()
    print(f"central differences: {rel:.2e}")
    assert rel <= 1e-6


@pytest.mark.parametrize("size", SIZES[:3], ids=lambda s: f"{s[0]}x{s[1]}")
def test_equal_images_have_zero_loss(size):
    H, W = size
    x, _ = _images(H, W, 5, flat=True)
    for w in WEIGHTS:
        loss, cot = ref.image_loss(x[None], x, w)
        assert loss[0] == 0.0, (w, loss)
    m = ref.ssim_map(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(x.astype(np.float64)))
    assert (m == 1.0).all()


def test_mse_weights_are_the_unweighted_fitness():
    # fitness_many squares float32 differences: each term carries <= 2 |d| 2^-25 + d^2 2^-23,
    # i.e. ~6e-8 (mean|d| / mse + 2) ~ 3e-7 of the mean at these images; 1e-6 is the bar
    H, W, N, B = 33, 47, 12, 3
    pop = oracle.synthetic_population(B, N, H, W, seed=8)
    tgt = np.random.default_rng(9).uniform(0, 1, (H, W, 3)).astype(np.float32)
    img = oracle.render(oracle.genome_to_renderer_batched(pop), H, W, k_sigma=3.0)
    loss, _ = ref.image_loss(img, tgt, (0.0, 1.0, 0.0))
    want = oracle.fitness_many(list(pop), tgt, H, W, 3.0)
    rel = np.abs(loss - want).max() / np.abs(want).max()
    print(f"mse vs fitness_many: {rel:.2e}")
    assert rel <= 1e-6


def test_group_and_single_target_addressing():
    H, W = 11, 16
    rng = np.random.default_rng(12)
    img = rng.uniform(0, 1, (4, H, W, 3)).astype(np.float32)
    tg = rng.uniform(0, 1, (2, H, W, 3)).astype(np.float32)
    loss, cot = ref.image_loss(img, tg, (0.8, 0.0, 0.2), group=2)
    for b in range(4):
        l1, c1 = ref.image_loss(img[b:b + 1], tg[b // 2], (0.8, 0.0, 0.2))
        assert l1[0] == loss[b] and np.array_equal(c1[0], cot[b])
