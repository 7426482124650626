"""Inputs shared by the seeding tests (tests/test_seed_host.py on the CPU,
tests/test_gpu_seed_sites.py and tests/test_gpu_seed_genomes.py on the device)."""
from __future__ import annotations

import numpy as np

from ggs.seed import SeedRound

# (B, H, W, cell) of the stage-export parity: partial cells on both axes; one partial cell
# with W - 1 = 0; a whole wave per cell; 32 cells per wave; more than one wave per cell row
SITE_SHAPES = [(3, 33, 47, 8), (1, 5, 1, 4), (2, 64, 64, 64), (2, 16, 16, 2), (2, 70, 100, 16)]


def flat_blocks(K: int, H: int, W: int, s: int, seed: int, channels: int = 3) -> np.ndarray:
    """[K,H,W,channels] of flat s x s blocks with values k / 8, k in 1..8 (exact in
    float32, as are their sums), different per image: cells inside one block tie exactly."""
    rng = np.random.default_rng(seed)
    by, bx = -(-H // s), -(-W // s)
    blocks = (rng.integers(1, 9, (K, by, bx, channels)) / 8.0).astype(np.float32)
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, s, axis=1), s, axis=2)[:, :H, :W])


def flat_targets(K: int, H: int, W: int, seed: int) -> np.ndarray:
    """``flat_blocks`` with a block size of 2 to 9 pixels drawn from the seed."""
    return flat_blocks(K, H, W, int(np.random.default_rng(seed).integers(2, 10)), seed + 1)


def noisy_image(B: int, H: int, W: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(0, 1, (B, H, W, 3)).astype(np.float32)


def weights(K: int, H: int, W: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(0.25, 1.0, (K, H, W)).astype(np.float32)


def genomes(B: int, N: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).normal(0, 1, (B, N, 9)).astype(np.float32)


# ---- the quality condition ------------------------------------------------------------
Q_H, Q_W, Q_N, Q_P, Q_K_SIGMA = 48, 64, 24, 16, 3.0
Q_ROUNDS = [SeedRound(16, 8, float(np.float32(np.log(5.0))), 255.0),
            SeedRound(8, 16, float(np.float32(np.log(3.0))), 255.0)]


def rectangles_target() -> np.ndarray:
    """A few flat rectangles on the white background, [1,H,W,3]."""
    t = np.ones((Q_H, Q_W, 3), np.float32)
    t[4:20, 6:30] = (0.75, 0.125, 0.125)
    t[26:44, 10:26] = (0.125, 0.5, 0.75)
    t[8:40, 40:58] = (0.25, 0.625, 0.25)
    return t[None]


def rectangles_mask() -> np.ndarray:
    """The importance mask of the quality case, [1,H,W]: 1 inside the frame's middle, 0.5 outside."""
    m = np.full((Q_H, Q_W), 0.5, np.float32)
    m[6:42, 8:56] = 1.0
    return m[None]
