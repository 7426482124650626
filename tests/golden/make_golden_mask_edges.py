"""Edge-case fixtures of the target preparation and importance mask, made by
running the REFERENCE itself -> tests/golden/mask_edges.npz.

Build container only (refuses without /root/reference), same method as
make_golden.py: the reference's modules/mask.py is imported read-only and
``compute_importance_mask`` called by name with the arguments of
algorithm.py:42-49; the target preparation is algorithm.py:33-39 spelled with the
same torch calls make_golden.py uses for mask.npz (float32, /255 when max > 1.5,
F.interpolate bilinear align_corners=False when the size differs).

Cases (name: input -> work size, strength):
  t33x47     textured default_rng image, odd sizes, no resize
  t9x13      smaller than the 9x9 variance window; scale 4 leaves a 2x3 grid
  u8_100x70  0..255-range float image resized 100x70 -> 40x56
  stack0..2  the three images of a stack at 48x40 (the tests stack them)
  max400     raw maximum 400: /255 in the preparation leaves a maximum > 1.5, so
             the mask divides by 255 once more (mask.py:42) - the double rescale

Per case the npz holds <name>__image, <name>__HW, <name>__strength and the
reference's <name>__target and <name>__mask.

Before a case is written the host restatement (ggs/mask.py) must be within 2e-5
(mask) and 5e-6 (target) of the reference.  A case that misses is
ill-conditioned (qh - ql of a _norm01 is tiny, so the division amplifies ulps):
replace its image (another seed) and note it below; the bar does not move.
Replaced so far: none.

    python tests/golden/make_golden_mask_edges.py
"""
from __future__ import annotations

import os
import sys

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

if not os.path.isdir(os.path.join(REF, "modules")):
    raise SystemExit("make_golden_mask_edges.py: /root/reference is not present; fixtures are "
                     "generated in the build container only")

sys.dont_write_bytecode = True
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import modules.mask as M  # noqa: E402  (reference)

KW = dict(edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3, gamma=0.7, floor=0.15, smooth=3)


def textured(seed: int, h: int, w: int, hi: float = 1.0) -> np.ndarray:
    """Noise over a few smooth waves and a step, so edges and variance both vary."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.25 * np.sin(xx / 3.1 + rng.uniform(0, 6)) * np.cos(yy / 4.3 + rng.uniform(0, 6))
    base = base + 0.15 * (xx > w * rng.uniform(0.3, 0.7))
    img = base[..., None] * rng.uniform(0.6, 1.0, 3) + rng.uniform(-0.2, 0.2, (h, w, 3))
    img = np.clip(img, 0.0, 1.0)
    img.flat[rng.integers(img.size)] = 1.0            # the maximum is exactly `hi`
    return (img * hi).astype(np.float32)


def ref_prepare(img: np.ndarray, H: int, W: int) -> torch.Tensor:
    """algorithm.py:33-39."""
    t = torch.from_numpy(img).to(torch.float32)
    if t.max() > 1.5:
        t = t / 255.0
    if t.shape[0] != H or t.shape[1] != W:
        t = torch.nn.functional.interpolate(t.permute(2, 0, 1).unsqueeze(0), size=(H, W), mode="bilinear",
                                            align_corners=False)[0].permute(1, 2, 0)
    return t.contiguous()


def main() -> None:
    sys.path.insert(0, os.path.join(REPO, "genetic-gaussian-splats_amd"))
    from ggs.mask import compute_importance_mask, prepare_target   # the host restatement (the check)

    cases = [("t33x47", textured(33, 33, 47), 33, 47, 0.7),
             ("t9x13", textured(9, 9, 13), 9, 13, 1.0),
             ("u8_100x70", textured(100, 100, 70, hi=255.0), 40, 56, 0.7),
             ("max400", textured(400, 40, 36, hi=400.0), 40, 36, 0.7)]
    cases += [(f"stack{i}", textured(480 + i, 48, 40), 48, 40, 0.7) for i in range(3)]
    out = {}
    for name, img, H, W, strength in cases:
        t = ref_prepare(img, H, W)
        mask = M.compute_importance_mask(t, H, W, strength=strength, **KW).numpy()
        tgt = t.numpy()
        host_t = prepare_target(img, H, W)
        host_m = compute_importance_mask(host_t, H, W, strength=strength, **KW)
        et, em = float(np.abs(host_t - tgt).max()), float(np.abs(host_m - mask).max())
        print(f"{name}: raw max {img.max():.4g}, prepared max {tgt.max():.4g}, "
              f"host target err {et:.2e}, host mask err {em:.2e}")
        if not (et <= 5e-6 and em <= 2e-5):
            raise SystemExit(f"{name}: ill-conditioned (host restatement misses the bar); replace the image")
        out[f"{name}__image"] = img
        out[f"{name}__HW"] = np.array([H, W], np.int32)
        out[f"{name}__strength"] = np.array(strength, np.float64)
        out[f"{name}__target"] = tgt
        out[f"{name}__mask"] = mask
    assert out["max400__image"].max() > 1.5 * 255 and out["max400__target"].max() > 1.5
    np.savez_compressed(os.path.join(HERE, "mask_edges.npz"), **out)
    print("done")


if __name__ == "__main__":
    main()
