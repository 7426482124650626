"""The device DE's in-kernel random draws, restated in numpy integer arithmetic
(test infrastructure, CPU only; a helper module like ``_philox.py``, on whose
``block`` / ``u01`` it is built).

Written from the counter layout DESIGN.md documents, not from the kernels.
Stream ``S_DE = 9``: target row ``i`` of generation ``gen`` draws from the blocks

    counter = (gen, i, what, 9)      key = (seed & 0xFFFFFFFF, seed >> 32)

    what            words x, y, z, w feed
    0               r1 = x mod (P-1), r2 = y mod (P-2), r3 = z mod (P-3) (then
                    de-collided), jrand = w mod 9N (per gene) or w mod N (per splat)
    1               f_u = u01(x); y, z, w unused
    2 + 3s + k      crossover uniforms of splat s, genes 4k .. 4k+3 (k = 2: x only,
                    gene 8); the per-splat crossover uses only word x of k = 0

No word feeds two draws (``layout`` lists every consumer).
"""
from __future__ import annotations

from typing import Dict, Iterator

import numpy as np

import _philox as X
from ggs.de import crossover_id, de_decollide

S_DE = 9


def draws(seed: int, gen: int, P: int, N: int, per_splat: bool) -> Dict[str, np.ndarray]:
    """One generation's draws in ``ggs.de.de_trials``' layout."""
    i = np.arange(P, dtype=np.uint64)
    x, y, z, w = (v.astype(np.uint64) for v in X.block(seed, gen, i, 0, S_DE))
    raw = np.stack([x % np.uint64(P - 1), y % np.uint64(P - 2), z % np.uint64(P - 3)], axis=1)
    r = np.array([de_decollide(k, raw[k]) for k in range(P)], np.int32)
    jrand = (w % np.uint64(N if per_splat else 9 * N)).astype(np.int32)
    f_u = X.u01(X.block(seed, gen, i, 1, S_DE)[0])
    s = np.arange(N, dtype=np.uint64)[None, :]
    cr_u = np.zeros((P, N, 9), np.float32)
    if per_splat:
        cr_u[:, :, 0] = X.u01(X.block(seed, gen, i[:, None], np.uint64(2) + np.uint64(3) * s, S_DE)[0])
    else:
        for k in range(3):
            words = X.block(seed, gen, i[:, None], np.uint64(2 + k) + np.uint64(3) * s, S_DE)
            for j in range(4 if k < 2 else 1):
                cr_u[:, :, 4 * k + j] = X.u01(words[j])
    return {"r": r, "jrand": jrand, "f_u": f_u, "cr_u": cr_u}


class PhiloxDeDraws:
    """A ``ggs.de`` draw source (``generation(gen, P, N)``) over the device's
    Philox stream keyed by ``seed``: the host loop on it follows the device run."""

    def __init__(self, seed: int, crossover="gene"):
        self.seed, self.per_splat = int(seed) & (2**64 - 1), crossover_id(crossover) == 1

    def generation(self, gen: int, P: int, N: int) -> Dict[str, np.ndarray]:
        return draws(self.seed, gen, P, N, self.per_splat)


def layout(P: int, N: int, per_splat: bool) -> Iterator[tuple]:
    """Every word one generation consumes: (draw, (stream, who, what, word)), one
    entry per consumer.  Plain loops over the table in the docstring."""
    for i in range(P):
        for w, name in enumerate(("r1", "r2", "r3", "jrand")):
            yield (name, i), (S_DE, i, 0, w)
        yield ("f_u", i), (S_DE, i, 1, 0)
        for s in range(N):
            if per_splat:
                yield ("cr_u", i, s, 0), (S_DE, i, 2 + 3 * s, 0)
                continue
            for c in range(9):
                yield ("cr_u", i, s, c), (S_DE, i, 2 + 3 * s + c // 4, c % 4)
