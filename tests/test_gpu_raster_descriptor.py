"""The strip-words raster's grid decode from the host-built launch descriptor
(csrc/ggs_internal.h StripLaunch: multiply-shift constants for the grid's divisions,
a dispatch table whose entries are decoded strips) against the same call with
GGS_STRIP_WORDS=0, which runs bounds_cull_kernel: that twin keeps the prologue
that divides on the device, so it is an independent decode of (candidate, strip)
from the block index.  The fitness vectors of all three modes and the rendered
images must be equal bit for bit.

Canvases: one tile; a ragged last tile in both directions (two of them); the
bench's 512 x 512.  B = 20 at 512 x 512 is 2,560 strip waves, inside the
single-round range 2 x SIMDs .. 3 x SIMDs where the middle third of the grid runs
reversed.  B = 1032 at N = 512 is more than one candidate chunk."""
from __future__ import annotations

import numpy as np
import pytest

import ggs
import strip_words_cases as S

pytestmark = pytest.mark.gpu

CANVASES = [(64, 128), (70, 130), (200, 136), (512, 512)]
NS = [64, 256, 512]


def _both(monkeypatch, fn):
    monkeypatch.delenv("GGS_STRIP_WORDS", raising=False)
    new = fn()
    monkeypatch.setenv("GGS_STRIP_WORDS", "0")
    old = fn()
    monkeypatch.delenv("GGS_STRIP_WORDS", raising=False)
    return new, old


def _planes(H, W, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (H, W, 3)).astype(np.float32), rng.uniform(0.4, 1.0, (H, W)).astype(np.float32)


def _modes(mask):
    return [dict(weight_mask=mask), dict(), dict(weight_mask=mask, boost_only=True, boost_beta=0.7)]


def _compare(monkeypatch, pop, H, W, tgt, mask, render=True):
    for kw in _modes(mask):
        new, old = _both(monkeypatch, lambda: ggs.fitness(pop, tgt, H, W, S.K_SIGMA, **kw))
        assert np.isfinite(new).all() and (new > 0).all()
        assert np.array_equal(new, old), (len(pop), sorted(kw), np.flatnonzero(new != old)[:8])
    if render:
        enc = ggs.encode(pop)
        new, old = _both(monkeypatch, lambda: ggs.render(enc, H, W, k_sigma=S.K_SIGMA))
        assert np.array_equal(new, old), (len(pop), np.argwhere(new != old)[:4])
        assert new.min() < 1.0          # something was drawn on the white background


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("H,W", CANVASES)
def test_descriptor_decode_equals_the_dividing_prologue(H, W, N, monkeypatch):
    tgt, mask = _planes(H, W, 5)
    nine = S.batch(H, W, N)
    for B, pick in S.SUBSETS.items():        # B = 1, 3, 9
        _compare(monkeypatch, np.ascontiguousarray(nine[pick]), H, W, tgt, mask)


def test_single_round_grid_with_the_reversed_middle_third(monkeypatch):
    """512 x 512, B = 20: 2,560 strip waves, between 2 x 1,024 and 3 x 1,024 SIMDs."""
    H = W = 512
    tgt, mask = _planes(H, W, 6)
    nine = S.batch(H, W, 256)
    _compare(monkeypatch, np.ascontiguousarray(nine[np.arange(20) % 9]), H, W, tgt, mask)


def test_chunked_grid_with_a_ragged_last_chunk(monkeypatch):
    """B = 1032 > raster_chunk(512) = 1024: a full chunk and one of 8 candidates, each
    with its own divisor; the one-tile canvas keeps it short."""
    H, W, N, B = 64, 128, 512, 1032
    tgt, mask = _planes(H, W, 7)
    nine = S.batch(H, W, N)
    pop = np.ascontiguousarray(nine[np.arange(B) % 9])
    new, old = _both(monkeypatch, lambda: ggs.fitness(pop, tgt, H, W, S.K_SIGMA, weight_mask=mask))
    assert np.array_equal(new, old), np.flatnonzero(new != old)[:8]
    small = ggs.fitness(nine, tgt, H, W, S.K_SIGMA, weight_mask=mask)
    assert np.array_equal(new, small[np.arange(B) % 9])
