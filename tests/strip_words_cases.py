"""Shapes, genomes and a numpy restatement for the strip-words tests
(test_strip_words_layout.py on the CPU, test_gpu_strip_words.py on the GPU).

Strip words (csrc/ggs_kernels.hip, prep_strip_words): prep makes the raster's
integer cull tests once per candidate instead of once per strip wave.  Per
candidate of N splats (N % 64 == 0, N <= 512), TILE 64 x 128, 16-column strips:

  words [nTY][N]      visit_row_word(i, y0, y1, ty0): i << 6 | kB | above << 5 | kA << 26
  masks [R][N / 64]   64-bit cull-chunk masks, R = 2 nCS + nTY, nCS = 4 ceil(W / 64):
                      rows [0, nCS) column hit, [nCS, 2 nCS) column clip, then row hit.
                      Chunk c, bit L is splat N - 1 - 64 c - L (the cull's lane order).
"""
from __future__ import annotations

import numpy as np

import ggs_oracle as O

TILE_W, TILE_H, STRIP = 64, 128, 16
VW_ABOVE, VW_KA, VW_CLIP = 32, 26, 31

# image sizes (H, W): one tile; strips past W and a clipped tile; two row tiles with the
# last one partial and strips past W in the third tile column; two full row tiles
SIZES = [(64, 128), (33, 47), (200, 136), (128, 256)]
# one chunk; one full step; an odd chunk count; the bench's; the offset field's limit
NS = [64, 128, 192, 256, 512]
NS_FALLBACK = [100, 576]     # N % 64 != 0; N > 512: the cull from the bounds
K_SIGMA = 3.0


def n_tiles(H, W):
    return (H + TILE_H - 1) // TILE_H, (W + TILE_W - 1) // TILE_W


# ---- genomes ---------------------------------------------------------------------------
def _rows(boxes, H, W, seed):
    """Axes-angle genome rows whose integer AABBs are exactly `boxes` [n][4] =
    (x0, x1, y0, y1): theta = 0, half sizes a quarter pixel inside the box (the
    renderer's half size is at least one pixel, so a box spans >= 3 pixels unless
    the image border clips it)."""
    b = np.asarray(boxes, np.float64)
    rng = np.random.default_rng(seed)
    g = np.zeros((len(b), 9), np.float64)
    for (lo, hi), col, ext in (((0, 1), 0, W), ((2, 3), 1, H)):
        c = 0.5 * (b[:, lo] + b[:, hi])
        h = np.maximum(0.5 * (b[:, hi] - b[:, lo]) - 0.25, 1.0)
        # a box the border clips: centre on the border, half size reaching the far side
        at0, at1 = b[:, lo] <= 0, b[:, hi] >= ext - 1
        short = (b[:, hi] - b[:, lo]) < 3
        c = np.where(short & at0, 0.0, np.where(short & at1, ext - 1.0, c))
        h = np.where(short, 0.5, h)          # (the renderer raises it to exactly one pixel)
        g[:, col] = c / max(ext - 1, 1)
        g[:, 2 + col] = np.log(h / K_SIGMA)
    g[:, 5:8] = rng.uniform(0.0, 255.0, (len(b), 3))
    g[:, 8] = rng.uniform(120.0, 255.0, len(b))
    return g.astype(np.float32)


def _spans(ext, period):
    """(lo, hi) pairs in [0, ext) whose ends lie on the period's boundaries."""
    marks = sorted({m for p in range(0, ext + period, period) for m in (p - 1, p, p + period - 1)
                    if 0 <= m < ext} | {0, ext - 1})
    out = [(lo, hi) for lo in marks for hi in marks if hi - lo >= 3]
    # ends next to a boundary from the inside, and short spans that end on one
    out += [(m, m + 3) for m in marks if m + 3 < ext] + [(m - 3, m) for m in marks if m - 3 >= 0]
    return out or [(0, ext - 1)]


def edge_candidate(N, H, W, seed=0):
    """AABBs that end exactly on strip (x mod 16 in {0, 15}) and tile (y mod 128 in
    {0, 127}) boundaries, every x span with every y span in turn."""
    xs, ys = _spans(W, STRIP), _spans(H, TILE_H)
    boxes = [(*xs[j % len(xs)], *ys[(j // len(xs) + j) % len(ys)]) for j in range(N)]
    return _rows(boxes, H, W, seed)


def corner_candidate(N, H, W, seed=0):
    """The smallest boxes (half size one pixel) at the four image corners, in turn."""
    c = [(0, 1, 0, 1), (W - 2, W - 1, 0, 1), (0, 1, H - 2, H - 1), (W - 2, W - 1, H - 2, H - 1)]
    return _rows([c[j % 4] for j in range(N)], H, W, seed)


def nohit_candidate(N, H, W, seed=0):
    """No splat reaches the columns from 16 on: strips 1.. of every tile row stay empty."""
    rng = np.random.default_rng(seed)
    y0 = rng.integers(0, max(H - 4, 1), N)
    boxes = [(0, 12, int(a), int(min(a + 3 + j % 40, H - 1))) for j, a in enumerate(y0)]
    return _rows(boxes, H, W, seed)


def allhit_candidate(N, H, W, seed=0):
    """Every splat covers columns 16..31 of the first tile row (its strip 1 lists all N)."""
    rng = np.random.default_rng(seed)
    x0 = rng.integers(0, 17, N)
    x1 = rng.integers(31, W, N) if W > 32 else np.full(N, W - 1)
    boxes = [(int(a), int(max(b, a + 3)), 0, int(min(3 + j % 60, H - 1))) for j, (a, b) in enumerate(zip(x0, x1))]
    return _rows(boxes, H, W, seed)


def batch(H, W, N, seed=0):
    """Nine candidates [9][N][9]: the population distributions (0-2, 7, 8), the edge
    set (3), the corners (4), an empty-strip (5) and an all-hit (6) candidate."""
    pop = O.synthetic_population(5, N, H, W, seed=seed + 17 * N + H)
    return np.stack([pop[0], pop[1], pop[2], edge_candidate(N, H, W, seed), corner_candidate(N, H, W, seed),
                     nohit_candidate(N, H, W, seed), allhit_candidate(N, H, W, seed), pop[3], pop[4]])


SUBSETS = {1: [3], 3: [3, 6, 0], 9: list(range(9))}    # B -> candidates of batch()


def bounds(cand, H, W):
    """The oracle's bit-exact integer AABBs of one candidate's splats: x0, x1, y0, y1 [N]."""
    p = O.preprocess(O.genome_to_renderer_batched(cand[None])[0], H, W, K_SIGMA)
    return tuple(p[k].astype(np.int64) for k in ("x0", "x1", "y0", "y1"))


# ---- the layout, restated -----------------------------------------------------------------
def _u32(x):
    return np.asarray(x, np.int64) & 0xFFFFFFFF


def row_words(y0, y1, ty0):
    """visit_row_word for every splat i against the row tile starting at ty0 (uint32 bits)."""
    i = np.arange(len(y0), dtype=np.int64)
    dy0, dy1 = y0 - ty0, y1 - ty0
    kA = np.maximum(dy0, 0) >> 3
    kB = np.where(dy1 >= TILE_H - 1, TILE_H // 8, _u32(dy1) >> 3)
    above = np.where(dy0 <= 0, VW_ABOVE, 0)
    return _u32((i << 6) | kB | above | (kA << VW_KA))


def _chunk_masks(flags):
    """Per-splat booleans [N] -> python ints [N / 64]: chunk c, bit L = splat N - 1 - 64 c - L."""
    N = len(flags)
    rev = np.asarray(flags, bool)[::-1]
    return [sum(1 << L for L in range(64) if rev[64 * c + L]) for c in range(N // 64)]


def layout(bnd, H, W):
    """words [nTY][N] and masks [R][N / 64] of one candidate from its bounds."""
    x0, x1, y0, y1 = bnd
    nTY, nTX = n_tiles(H, W)
    nCS = 4 * nTX
    words = [row_words(y0, y1, ty * TILE_H) for ty in range(nTY)]
    hit, clip, rows = [], [], []
    for cs in range(nCS):
        sx0 = cs * STRIP
        inside = sx0 < W                     # strips that start at or past W: zero masks
        hit.append(_chunk_masks(inside & (x1 >= sx0) & (x0 <= sx0 + 15)))
        clip.append(_chunk_masks(inside & (np.maximum(x0 - sx0, sx0 + 15 - x1) > 0)))
    for ty in range(nTY):
        ty0 = ty * TILE_H
        ty1 = min(ty0 + TILE_H, H) - 1
        rows.append(_chunk_masks((y1 >= ty0) & (y0 <= ty1)))
    return words, hit + clip + rows


def compact(words, masks, N, nCS, ty, cs):
    """The raster's strip-words cull: the list of strip (ty, cs) from words and masks."""
    out = []
    for c in range(N // 64):
        h = masks[cs][c] & masks[2 * nCS + ty][c]
        k = masks[nCS + cs][c]
        for L in range(64):                  # the prefix runs over the lower lanes
            if (h >> L) & 1:
                out.append(int(words[ty][N - 1 - 64 * c - L]) | (((k >> L) & 1) << VW_CLIP))
    return out


def brute_list(bnd, H, W, ty, cs):
    """The cull from the bounds: visit_word of every hit, descending splat index."""
    x0, x1, y0, y1 = (a.tolist() for a in bnd)
    ty0, sx0 = ty * TILE_H, cs * STRIP
    ty1 = min(ty0 + TILE_H, H) - 1
    out = []
    for i in range(len(x0) - 1, -1, -1):
        if not (y1[i] >= ty0 and y0[i] <= ty1 and x1[i] >= sx0 and x0[i] <= sx0 + 15):
            continue
        dy0, dy1 = y0[i] - ty0, y1[i] - ty0
        kA = max(dy0, 0) >> 3
        kB = TILE_H // 8 if dy1 >= TILE_H - 1 else dy1 >> 3
        w = (i << 6) | kB | (VW_ABOVE if dy0 <= 0 else 0) | (kA << VW_KA)
        if max(x0[i] - sx0, sx0 + 15 - x1[i]) > 0:
            w |= 1 << VW_CLIP
        out.append(w)
    return out
