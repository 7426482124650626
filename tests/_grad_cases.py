"""Problems for the fitness-gradient tests (TEST INFRASTRUCTURE): genomes from
``oracle.synthetic_population`` with planted rows, a target, a mask, and the
float64 reference of each case computed once per process (tests/_grad_ref.py).

Sizes are width x height.  Planted rows, all in candidate 0 (``PLANTED``):

* ``opaque``: alpha 255 and the centre exactly on a pixel, in the middle of the
  depth order — f = 1 there, the backward's exact walk;
* ``clipped``: x < 0 and red above 255 — zero gradient in those two columns;
* ``tiny``: scales small enough that the half-extent is floored to 1;
* ``corner``: a small splat in the last strip, away from everything near it.
"""
from __future__ import annotations

import functools

import numpy as np

import _grad_ref
import ggs_oracle as oracle

K_SIGMA = 3.0
BETA = 0.7
# (W, H, N): one partial tile with odd sizes; exactly one forward tile and two cull
# chunks; several ragged strips both ways; more splats than the saturation threshold
SHAPES = {"48x40": (48, 40, 24), "64x128": (64, 128, 96), "130x70": (130, 70, 40), "n600": (56, 40, 600)}
MODES = ("none", "weighted", "boost")
PLANTED = {"opaque": None, "clipped": 1, "tiny": 2, "corner": 3}    # opaque: N // 2


def planted_index(name: str, N: int) -> int:
    return N // 2 if name == "opaque" else PLANTED[name]


def _on_pixel(n: int, frac: float) -> np.float32:
    """A float32 x in [0, 1] with float32(x * (n - 1)) an integer near frac * (n - 1)."""
    m = np.float32(n - 1)
    for px in range(int(frac * (n - 1)), n):
        x = np.float32(px) / m
        if np.float32(x * m) == np.float32(px):
            return x
    raise AssertionError("no exact pixel centre")


@functools.lru_cache(maxsize=None)
def problem(shape: str):
    """(G [3,N,9] float32, target [H,W,3], mask [H,W]) of a shape."""
    W, H, N = SHAPES[shape]
    G = oracle.synthetic_population(3, N, H, W, seed=1000 + N)
    g = G[0]
    i = planted_index("opaque", N)
    g[i, 0], g[i, 1], g[i, 8] = _on_pixel(W, 0.4), _on_pixel(H, 0.45), 255.0
    i = planted_index("clipped", N)
    g[i, 0], g[i, 5] = -0.05, 300.0
    i = planted_index("tiny", N)
    g[i, 2], g[i, 3] = np.log(0.2), np.log(0.25)
    i = planted_index("corner", N)
    g[i, 0], g[i, 1], g[i, 2], g[i, 3] = 0.985, 0.98, np.log(1.1), np.log(0.9)
    rng = np.random.default_rng(77 + N)
    target = oracle.render(oracle.genome_to_renderer_batched(
        oracle.synthetic_population(1, max(8, N // 3), H, W, seed=5 + N)), H, W, k_sigma=K_SIGMA)[0]
    target = np.clip(target + rng.normal(0, 0.05, target.shape), 0, 1).astype(np.float32)
    mask = rng.uniform(0.0, 1.2, (H, W)).astype(np.float32)
    G.setflags(write=False)
    target.setflags(write=False)
    mask.setflags(write=False)
    return G, target, mask


def mode_kwargs(mode: str, mask):
    """keyword arguments of api.fitness / api.fitness_grad / _grad_ref for a mode."""
    if mode == "none":
        return dict(weight_mask=None, boost_only=False, boost_beta=1.0)
    return dict(weight_mask=mask, boost_only=mode == "boost", boost_beta=BETA if mode == "boost" else 1.0)


@functools.lru_cache(maxsize=None)
def reference(shape: str, mode: str):
    """(loss [3], grad [3,N,9]) float64 of tests/_grad_ref.py, read-only."""
    W, H, N = SHAPES[shape]
    G, target, mask = problem(shape)
    L, g = _grad_ref.loss_and_grad(G, target, H, W, K_SIGMA, **mode_kwargs(mode, mask))
    L.setflags(write=False)
    g.setflags(write=False)
    return L, g
