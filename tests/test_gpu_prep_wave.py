"""prep with one wave per workgroup (csrc/ggs_kernels.hip prep_kernel, 64 threads,
grid ceil(S / 64)) at splat counts around the wave size.

S = B * N of 1, 63, 64, 65, 130 and 257 at 64x128: a lone lane, a partial wave, a
full one, one lane into the second workgroup, two lanes into the third, one lane
into the fifth; B x N of 65 x 1 has one splat per candidate.  All of prep's output
modes run: ``ggs.encode`` (enc9), ``ggs.preprocess`` (f9 + i4), ``ggs.render``
(records + cull bounds from renderer rows) and ``ggs.fitness`` (the same from
axes-angle rows, encode fused).

The last splat of every population with more than one splat (the lane at the end
of S) is degenerate: zero scale and alpha 0, built on the thin-splat generator of
tests/test_degenerate_splats.py, so the Cholesky factors sit at their 1e-6 clamps (encode.py:18,
render.py:20: sxx = syy = 1e12) and log2(alpha) is -inf.

Bars: encode and the 13 preprocess outputs bit-equal to the oracle (as
tests/test_gpu_parity.py asks at its sizes), images <= 1e-4 abs, fitness rel <= 1e-5.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ggs
import ggs_oracle as O
import test_degenerate_splats as D

pytestmark = pytest.mark.gpu
H, W = 64, 128
IMG_TOL, FIT_RTOL = 1e-4, 1e-5
SHAPES = [(1, 1), (3, 21), (2, 32), (65, 1), (2, 65), (1, 257)]     # S = 1, 63, 64, 65, 130, 257


def _degenerate_axes(rng):
    """One axes-angle row: a thin rotated splat of the degenerate-splat generators
    shrunk to zero scale (exp(-103) underflows to 0 in float32) with alpha 0."""
    row = D._to_axes(D._thin(rng, 1))[0]
    row[2] = row[3] = -103.0
    row[8] = 0.0
    return row


@functools.lru_cache(maxsize=None)
def _case(B, N):
    rng = np.random.default_rng(100 * B + N)
    pop = O.synthetic_population(B, N, H, W, seed=B + N)
    if B * N > 1:
        pop[-1, -1] = _degenerate_axes(rng)
    tgt = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    mask = rng.uniform(0.4, 1.0, (H, W)).astype(np.float32)
    with np.errstate(all="ignore"):
        enc = O.genome_to_renderer_batched(pop)
        ref = dict(enc=enc, prep=O.preprocess(enc.reshape(-1, 9), H, W, 3.0), img=O.render(enc, H, W),
                   fit={m: O.fitness_many(list(pop), tgt, H, W, 3.0, **kw) for m, kw in _modes(mask).items()})
    for a in (pop, tgt, mask, ref["enc"], ref["img"]):
        a.setflags(write=False)
    return pop, tgt, mask, ref


def _modes(mask):
    return {"none": {}, "weighted": {"weight_mask": mask}, "boost": {"weight_mask": mask, "boost_only": True}}


def test_shapes_cover_the_wave_edges():
    assert [b * n for b, n in SHAPES] == [1, 63, 64, 65, 130, 257]


@pytest.mark.parametrize("B,N", SHAPES)
def test_encode_and_preprocess_bit_equal_to_the_oracle(B, N):
    pop, _, _, ref = _case(B, N)
    enc = ggs.encode(pop)
    np.testing.assert_array_equal(enc, ref["enc"])
    got = ggs.preprocess(enc.reshape(-1, 9), H, W, 3.0)
    assert len(O.BOUND_KEYS + O.FLOAT_KEYS) == 13
    for k in O.BOUND_KEYS + O.FLOAT_KEYS:
        assert got[k].shape == (B * N,)
        np.testing.assert_array_equal(got[k], ref["prep"][k], err_msg=k)
    if B * N > 1:                                   # the degenerate lane is what it claims to be
        assert ref["prep"]["a"][-1] == 0.0 and ref["prep"]["syy"][-1] >= 1e11


@pytest.mark.parametrize("B,N", SHAPES)
def test_render_and_fitness_within_the_bars(B, N):
    pop, tgt, mask, ref = _case(B, N)
    img = ggs.render(ref["enc"], H, W)
    assert np.isfinite(img).all()
    err = float(np.abs(img - ref["img"]).max())
    print(f"S={B * N}: image max abs err {err:.3e}")
    assert err <= IMG_TOL
    for m, kw in _modes(mask).items():
        got = ggs.fitness(pop, tgt, H, W, 3.0, **kw)
        assert np.isfinite(ref["fit"][m]).all()
        rel = float(np.max(np.abs(got - ref["fit"][m]) / np.abs(ref["fit"][m])))
        print(f"S={B * N} {m}: fitness max rel err {rel:.3e}")
        np.testing.assert_allclose(got, ref["fit"][m], rtol=FIT_RTOL, err_msg=m)
