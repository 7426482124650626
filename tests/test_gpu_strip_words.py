"""Strip words on the GPU: prep's row words and chunk masks, compacted by the
raster, against the raster's own cull from the bounds (GGS_STRIP_WORDS=0).  The
strip lists are the same word for word, so every output is compared with
np.array_equal: the fitness vectors of all three fitness modes (prep_kernel<true>)
and the rendered images (prep_kernel<false>).  Shapes and genomes: see
strip_words_cases.py; N = 100 and N = 576 take the cull from the bounds either
way and must still agree."""
from __future__ import annotations

import numpy as np
import pytest

import ggs
import strip_words_cases as S

pytestmark = pytest.mark.gpu


def _both(monkeypatch, fn):
    monkeypatch.delenv("GGS_STRIP_WORDS", raising=False)
    new = fn()
    monkeypatch.setenv("GGS_STRIP_WORDS", "0")
    old = fn()
    monkeypatch.delenv("GGS_STRIP_WORDS", raising=False)
    return new, old


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(3)
    return {(H, W): (rng.uniform(0, 1, (H, W, 3)).astype(np.float32),
                     rng.uniform(0.4, 1.0, (H, W)).astype(np.float32)) for H, W in S.SIZES}


@pytest.mark.parametrize("N", S.NS + S.NS_FALLBACK)
@pytest.mark.parametrize("H,W", S.SIZES)
def test_strip_words_equal_the_cull_from_the_bounds(H, W, N, planes, monkeypatch):
    tgt, mask = planes[H, W]
    all9 = S.batch(H, W, N)
    for B, pick in S.SUBSETS.items():
        pop = np.ascontiguousarray(all9[pick])
        modes = [dict(weight_mask=mask)]
        if B == 9:
            modes += [dict(), dict(weight_mask=mask, boost_only=True, boost_beta=0.7)]
        for kw in modes:
            new, old = _both(monkeypatch, lambda: ggs.fitness(pop, tgt, H, W, S.K_SIGMA, **kw))
            assert np.isfinite(new).all() and (new > 0).all()
            assert np.array_equal(new, old), (B, sorted(kw), new, old)
        enc = ggs.encode(pop)
        new, old = _both(monkeypatch, lambda: ggs.render(enc, H, W, k_sigma=S.K_SIGMA))
        assert np.array_equal(new, old), (B, np.argwhere(new != old)[:4])
        assert new.min() < 1.0          # something was drawn on the white background


def test_strip_words_in_a_chunked_grid(monkeypatch):
    """B > raster_chunk(N): the grid runs in candidate chunks (40 MiB of records and
    bounds: 1024 candidates at N = 512); 1032 = one full chunk and a ragged one of 8,
    whose candidates index the words and masks by their batch position."""
    H, W, N, B = 33, 47, 512, 1032
    nine = S.batch(H, W, N)
    pop = np.ascontiguousarray(nine[np.arange(B) % 9])
    rng = np.random.default_rng(4)
    tgt = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    mask = rng.uniform(0.4, 1.0, (H, W)).astype(np.float32)
    new, old = _both(monkeypatch, lambda: ggs.fitness(pop, tgt, H, W, S.K_SIGMA, weight_mask=mask))
    assert np.array_equal(new, old)
    small = ggs.fitness(nine, tgt, H, W, S.K_SIGMA, weight_mask=mask)
    assert np.array_equal(new, small[np.arange(B) % 9])
