"""Problems for the image-loss tests (TEST INFRASTRUCTURE): shapes, batchings, weights
and the three kinds of input, each built once per process and read-only.

Shapes are height x width.  The kernel's output tile is 16 x 16 with an 11-tap window:
5 x 7 is smaller than the window on both axes, 11 x 16 is one window by one tile,
33 x 47 spans three tiles per axis and is a multiple of none, 70 x 130 has interior
tiles whose whole halo lies inside the image.

Inputs (images [B,H,W,3] against targets [K,H,W,3]):
* ``uniform``: seeded uniform images and targets;
* ``flat``: the target has a constant (white) left half and a constant band, the image
  equals it there and is noise elsewhere (the case a float32 SSIM graph loses);
* ``render``: the images come from ``render_fn`` (the device's or the oracle's render) of
  seeded genomes, against seeded targets.
"""
from __future__ import annotations

import functools

import numpy as np

import ggs_oracle as oracle

SHAPES = [(5, 7), (11, 16), (33, 47), (70, 130)]
# B, K, group.  B = 3 against K = 2 with group 1 wants three images of two: the group rule
# (B / group <= K) refuses it, REFUSED is tested as a refusal; K = 3 for B = 2 is its valid twin
BATCHINGS = [(3, 3, 1), (4, 2, 2), (2, 3, 1)]
REFUSED = (3, 2, 1)
WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.8, 0.0, 0.2)]
INPUTS = ("uniform", "flat", "render")
N_SPLATS = 12


def shape_id(s) -> str:
    return f"{s[0]}x{s[1]}"


@functools.lru_cache(maxsize=None)
def targets(H: int, W: int, kind: str) -> np.ndarray:
    """[3,H,W,3] float32 (a batching takes the first K)."""
    rng = np.random.default_rng(100 * H + W)
    t = rng.uniform(0, 1, (3, H, W, 3)).astype(np.float32)
    if kind == "flat":
        t[:, :, : W // 2] = 1.0
        t[:, H // 3: H // 3 + max(H // 4, 1)] = 0.25
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def genomes(H: int, W: int) -> np.ndarray:
    G = oracle.synthetic_population(4, N_SPLATS, H, W, seed=7 + H)
    G.setflags(write=False)
    return G


def images(H: int, W: int, kind: str, B: int, group: int, render_fn=None) -> np.ndarray:
    """[B,H,W,3] float32 for a batching (the flat image copies its own target's flat parts)."""
    if kind == "render":
        return np.ascontiguousarray(render_fn(np.ascontiguousarray(genomes(H, W)[:B]), H, W))
    x = np.random.default_rng(200 * H + W).uniform(0, 1, (B, H, W, 3)).astype(np.float32)
    if kind == "flat":
        t = targets(H, W, kind)
        for b in range(B):
            x[b, :, : W // 2] = t[b // group, :, : W // 2]
            band = slice(H // 3, H // 3 + max(H // 4, 1))
            x[b, band] = t[b // group, band]
    return x
