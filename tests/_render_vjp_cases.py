"""Problems for the render-VJP tests (TEST INFRASTRUCTURE): the shapes, genomes,
targets and masks of tests/_grad_cases.py, the rows of each layout, the cotangents
and the float64 reference of tests/_render_vjp_ref.py.

Rows: ``"axes"`` rows are the problem's genomes; ``"renderer"`` rows are their
encoding with the ``clipped`` row's red set to 300 afterwards (encode clips colours,
so the planted value has to be put back).  The ``opaque`` row keeps alpha 255 and
its centre on a pixel through the encoding; the ``clipped`` row keeps x < 0.
"""
from __future__ import annotations

import numpy as np
import torch

import _grad_cases as cases
import _grad_ref
import _render_vjp_ref as ref
import ggs_oracle as oracle

WHITE, COLOUR, BLACK = (1.0, 1.0, 1.0), (0.2, 0.5, 0.9), (0.0, 0.0, 0.0)
# shape, layout, genome stride, background: every shape with both layouts, every
# stride and every background with both layouts
CASES = [("48x40", "axes", 9, WHITE), ("48x40", "renderer", 12, COLOUR),
         ("64x128", "axes", 12, COLOUR), ("64x128", "renderer", 9, BLACK),
         ("130x70", "axes", 9, BLACK), ("130x70", "renderer", 9, WHITE), ("130x70", "axes", 12, COLOUR),
         ("n600", "axes", 9, COLOUR), ("n600", "renderer", 12, WHITE)]


def case_id(case) -> str:
    shape, layout, C, bg = case
    return f"{shape}-{layout}-C{C}-bg{'-'.join(f'{v:g}' for v in bg)}"


def rows(shape: str, layout: str, encode=oracle.genome_to_renderer_batched) -> np.ndarray:
    """The [3,N,9] float32 rows of a layout; ``encode``: axes-angle [B,N,9] -> renderer rows."""
    G = cases.problem(shape)[0]
    if layout == "axes":
        return np.array(G)
    R = np.array(encode(G), np.float32)
    R[0, cases.planted_index("clipped", R.shape[1]), 5] = 300.0
    return R


def widen(G, C):
    if C == 9:
        return np.ascontiguousarray(G)
    out = np.full(G.shape[:2] + (C,), 123.0, np.float32)        # the extra columns are never read
    out[..., :9] = G
    return out


def normal_cotangent(shape: str) -> np.ndarray:
    W, H, N = cases.SHAPES[shape]
    return np.random.default_rng(4242 + N).standard_normal((3, H, W, 3)).astype(np.float32)


def fitness_cotangent(img, target, mask, mode: str) -> np.ndarray:
    """V = 2 omega (img - t) / D in float64 on the host, cast to float32: d fitness / d img
    of a mode (fitness.py:7-31) at the images ``img`` [B,H,W,3]."""
    H, W = target.shape[:2]
    omega, D = _grad_ref._weights(H, W, **cases.mode_kwargs(mode, mask), dt=torch.float64)
    om = omega.numpy()[None, :, :, None]
    return (2.0 * om * (np.asarray(img, np.float64) - np.asarray(target, np.float64)[None]) / D).astype(np.float32)


def reference(shape: str, layout: str, bg, cots, dtype=torch.float64):
    """(image [3,H,W,3], [grad [3,N,9] per cotangent]) of tests/_render_vjp_ref.py."""
    W, H, N = cases.SHAPES[shape]
    return ref.render_vjp(rows(shape, layout), list(cots), H, W, cases.K_SIGMA, layout, bg, dtype)
