"""The strip-words layout without a GPU: a numpy restatement of what prep writes
(row words and the three kinds of chunk masks, from the oracle's bit-exact
bounds) compacted per strip the way the raster does it must give, word for word,
the list a brute-force cull from the bounds gives with visit_word.  Pins the bit
order (chunk c, bit L = splat N - 1 - 64 c - L, the prefix over higher splat
indices) and the semantics of the column-hit, column-clip and row-hit masks."""
from __future__ import annotations

import numpy as np
import pytest

import strip_words_cases as S


@pytest.mark.parametrize("N", S.NS)
@pytest.mark.parametrize("H,W", S.SIZES)
def test_compacted_masks_and_words_equal_the_brute_force_cull(H, W, N):
    nTY, nTX = S.n_tiles(H, W)
    nCS = 4 * nTX
    lens = {}
    for b, cand in enumerate(S.batch(H, W, N)):
        bnd = S.bounds(cand, H, W)
        words, masks = S.layout(bnd, H, W)
        assert len(masks) == 2 * nCS + nTY and all(len(m) == N // 64 for m in masks)
        for ty in range(nTY):
            for cs in range(nCS):
                want = S.brute_list(bnd, H, W, ty, cs)
                assert S.compact(words, masks, N, nCS, ty, cs) == want, (b, ty, cs)
                lens[b, ty, cs] = len(want)
                if cs * S.STRIP >= W:        # strips past W: zero masks, empty lists
                    assert not any(masks[cs]) and not any(masks[nCS + cs]) and not want
    # the special candidates are what they claim to be
    assert all(lens[5, ty, cs] == 0 for ty in range(nTY) for cs in range(1, nCS))
    assert lens[6, 0, 1] == N
    assert any(lens[5, ty, 0] for ty in range(nTY))


@pytest.mark.parametrize("H,W", S.SIZES)
def test_edge_and_corner_candidates_end_on_the_boundaries(H, W):
    x0, x1, y0, y1 = S.bounds(S.edge_candidate(512, H, W), H, W)
    for a in (x0, x1):
        assert {0, 15} <= set((a % 16).tolist())
    if H > S.TILE_H:
        for a in (y0, y1):
            assert {0, 127} <= set((a % 128).tolist())
    else:
        assert 0 in y0 and H - 1 in y1
    x0, x1, y0, y1 = S.bounds(S.corner_candidate(64, H, W), H, W)
    boxes = set(zip(x0.tolist(), x1.tolist(), y0.tolist(), y1.tolist()))
    assert boxes == {(0, 1, 0, 1), (W - 2, W - 1, 0, 1), (0, 1, H - 2, H - 1), (W - 2, W - 1, H - 2, H - 1)}


def test_row_word_fields():
    """A word's fields against hand-worked boxes of the row tile at ty0 = 128."""
    y0 = np.array([0, 128, 129, 200, 255, 130], np.int64)
    y1 = np.array([300, 255, 140, 254, 255, 135], np.int64)
    w = S.row_words(y0, y1, 128)
    assert (w >> 6 & 0xFFFFF).tolist() == list(range(6))            # record index (offset / 64)
    assert (w & 31).tolist() == [16, 16, 1, 15, 16, 0]              # kB: last row pair, 16 past the tile
    assert (w >> 5 & 1).tolist() == [1, 1, 0, 0, 0, 0]              # starts at or above the tile
    assert (w >> S.VW_KA & 15).tolist() == [0, 0, 0, 9, 15, 0]      # kA: first row pair
    assert (w >> S.VW_CLIP).tolist() == [0] * 6
