"""The device GA / SA's in-kernel random draws, restated in numpy integer
arithmetic (test infrastructure, CPU only; a helper module like ``_fakes.py``).

Written from the counter layout DESIGN.md documents ("Philox counter layout"),
not from the kernels: every draw is one or two 32-bit words of a Philox4x32-10
block (Salmon et al., SC'11) with

    counter = (gen, who, what, stream)      key = (seed & 0xFFFFFFFF, seed >> 32)

``gen`` is the generation (SA: the iteration).  ``who`` / ``what`` per stream:

    stream      who             what    words x, y, z, w feed
    1 MASK      offspring og    2s      u_xy[s,0], u_xy[s,1], u_ab[s,0], u_ab[s,1]
    1 MASK      offspring og    2s+1    u_t[s], u_rgb[s], u_a[s], -
    2 NORM_A    offspring og    s       (x, y) -> n_xy[s,0], n_xy[s,1]; (z, w) -> n_ab[s,0], n_ab[s,1]
    3 NORM_B    offspring og    s       (x, y) -> n_t[s], n_rgba[s,0]; (z, w) -> n_rgba[s,1], n_rgba[s,2]
    4 NORM_C    offspring og    s       (x, y) -> n_rgba[s,3], (second output unused); z, w: -
    5 IND       offspring og    0..3    x -> k_color, k_xy, k_ab (mod 2N), k_t (mod N)
    5 IND       offspring og    4, 5    x -> swap_i (mod N-1); x -> swap_u
    6 TOUR      slot q          j       x -> tour_idx[q, j]
    7 CX        pair            0       x -> cx[pair] (u01 < cxpb)
    7 CX        pair            s+1     x -> cx_u[pair, s]
    8 ACCEPT    (counter (it, try, 0, 8))   x, y -> the SA acceptance uniform (53 bits)

og = first + local offspring (SA: the try); pairs and slots count from the
launch's offspring 0.  Words to draws: u01 = (x >> 8) 2^-24; tournament index
min(int(f32(u01) f32(P)), P - 1); a pair of words (a, b) gives the Box-Muller
pair r cos(2 pi u2), r sin(2 pi u2) with u1 = ((a >> 8) + 1) 2^-24, u2 = (b >> 8)
2^-24, r = sqrt(-2 ln u1) — here in float64.

Two words are shared on purpose (``SHARED``): the crossover mask uniform of
(pair, s) by the pair's two children, and, for odd P, tournament slot
(2 pair + 1) mod P = 0 of the last pair, which is also the first pair's first slot.
"""
from __future__ import annotations

from typing import Dict, Iterator, List, Tuple

import numpy as np

S_MASK, S_NORM_A, S_NORM_B, S_NORM_C, S_IND, S_TOUR, S_CX, S_ACCEPT = 1, 2, 3, 4, 5, 6, 7, 8
_M = np.uint64(0xFFFFFFFF)
_MUL0, _MUL1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_S32 = np.uint64(32)

SHARED = ("cx_u[pair, s] is consumed by both children of the pair",
          "odd P: the last pair's second tournament slot (2 pair + 1) mod P is slot 0")


def philox4x32(c0, c1, c2, c3, k0: int, k1: int, rounds: int = 10):
    """Philox4x32 on arrays of counters (broadcast together) and one key:
    the four output words as uint32 arrays."""
    c = [np.asarray(v, np.uint64) & _M for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(rounds):
        p0, p1 = _MUL0 * c[0], _MUL1 * c[2]                       # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _M, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _M]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(v.astype(np.uint32) for v in c)


def block(seed: int, gen, who, what, stream):
    """Words x, y, z, w of the block (gen, who, what, stream) under ``seed``."""
    seed = int(seed) & (2**64 - 1)
    return philox4x32(gen, who, what, stream, seed & 0xFFFFFFFF, seed >> 32)


def u01(x) -> np.ndarray:
    """[0, 1) from the top 24 bits, exact in float32."""
    return ((np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0).astype(np.float32)


def accept_uniform(seed: int, it: int, k: int) -> float:
    x, y, _, _ = block(seed, it, k, 0, S_ACCEPT)
    return float(((int(x) >> 5) * 67108864.0 + (int(y) >> 6)) / 9007199254740992.0)


def box_muller(a, b) -> Tuple[np.ndarray, np.ndarray]:
    """float64 Box-Muller pair of the words (a, b): u1 in (0, 1], u2 in revolutions."""
    u1 = ((np.asarray(a, np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (np.asarray(b, np.uint32) >> np.uint32(8)).astype(np.float64) / 16777216.0
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


# the five Box-Muller pairs of a splat: (stream, first word, second word) and the
# two draws they feed, as (field, column) (None: the output is not used)
NORMAL_PAIRS = [
    (S_NORM_A, 0, 1, ("n_xy", 0), ("n_xy", 1)),
    (S_NORM_A, 2, 3, ("n_ab", 0), ("n_ab", 1)),
    (S_NORM_B, 0, 1, ("n_t", 0), ("n_rgba", 0)),
    (S_NORM_B, 2, 3, ("n_rgba", 1), ("n_rgba", 2)),
    (S_NORM_C, 0, 1, ("n_rgba", 3), None),
]


def draws(seed: int, gen: int, n_off: int, P: int, N: int, tour_k: int, cxpb: float,
          first: int = 0) -> Dict[str, np.ndarray]:
    """The exported dict (``ggs.ga_device.philox_draws``) from the layout above;
    the normals in float64."""
    n, np2 = n_off, (n_off + 1) // 2
    og = (first + np.arange(n, dtype=np.uint64))[:, None]
    s = np.arange(N, dtype=np.uint64)[None, :]
    out: Dict[str, np.ndarray] = {}
    m0 = block(seed, gen, og, 2 * s, S_MASK)
    m1 = block(seed, gen, og, 2 * s + np.uint64(1), S_MASK)
    out["u_xy"] = np.stack([u01(m0[0]), u01(m0[1])], -1)
    out["u_ab"] = np.stack([u01(m0[2]), u01(m0[3])], -1)
    out["u_t"], out["u_rgb"], out["u_a"] = (u01(m1[i])[..., None] for i in range(3))
    out["n_xy"], out["n_ab"] = np.empty((n, N, 2)), np.empty((n, N, 2))
    out["n_t"], out["n_rgba"] = np.empty((n, N, 1)), np.empty((n, N, 4))
    words = {st: block(seed, gen, og, s, st) for st in (S_NORM_A, S_NORM_B, S_NORM_C)}
    for st, ia, ib, first_out, second_out in NORMAL_PAIRS:
        for dst, val in zip((first_out, second_out), box_muller(words[st][ia], words[st][ib])):
            if dst is not None:
                out[dst[0]][..., dst[1]] = val
    ind = [block(seed, gen, og[:, 0], what, S_IND)[0] for what in range(6)]
    for name, w, mod in (("k_color", 0, 2 * N), ("k_xy", 1, 2 * N), ("k_ab", 2, 2 * N), ("k_t", 3, N)):
        out[name] = (ind[w].astype(np.uint64) % np.uint64(mod)).astype(np.int32)
    out["swap_i"] = ((ind[4].astype(np.uint64) % np.uint64(N - 1)).astype(np.int32) if N >= 2
                     else np.zeros(n, np.int32))
    out["swap_pick"] = np.full(n, -1, np.int32)
    out["swap_u"] = u01(ind[5]).astype(np.float64)
    q = np.arange(P, dtype=np.uint64)[:, None]
    j = np.arange(tour_k, dtype=np.uint64)[None, :]
    ut = u01(block(seed, gen, q, j, S_TOUR)[0])
    out["tour_idx"] = np.minimum((ut * np.float32(P)).astype(np.int32), P - 1).astype(np.int32)   # float32 multiply
    out["perm"] = np.arange(P, dtype=np.int32)
    pair = np.arange(np2, dtype=np.uint64)
    out["cx"] = (u01(block(seed, gen, pair, 0, S_CX)[0]) < np.float32(cxpb)).astype(np.int32)
    out["cx_u"] = u01(block(seed, gen, pair[:, None], s + np.uint64(1), S_CX)[0])
    return out


def layout(n_off: int, P: int, N: int, tour_k: int, first: int = 0) -> Iterator[tuple]:
    """Every word one generation consumes: (draw, (stream, who, what, word)), the
    draw named (field, index...) — one entry per consumer, so a shared word shows
    up once per draw it feeds.  Plain loops over the table in the docstring."""
    for o in range(n_off):
        og = first + o
        for s in range(N):
            for w, (f, c) in enumerate((("u_xy", 0), ("u_xy", 1), ("u_ab", 0), ("u_ab", 1))):
                yield (f, o, s, c), (S_MASK, og, 2 * s, w)
            for w, f in enumerate(("u_t", "u_rgb", "u_a")):
                yield (f, o, s, 0), (S_MASK, og, 2 * s + 1, w)
            for st, ia, ib, d1, d2 in NORMAL_PAIRS:
                for dst in (d1, d2):
                    if dst is not None:       # both words feed each output of the pair
                        yield (dst[0], o, s, dst[1]), (st, og, s, ia)
                        yield (dst[0], o, s, dst[1]), (st, og, s, ib)
        for what, f in enumerate(("k_color", "k_xy", "k_ab", "k_t", "swap_i", "swap_u")):
            if f == "swap_i" and N < 2:
                continue                      # no swap with one splat: the word is not drawn
            yield (f, o), (S_IND, og, what, 0)
    for pair in range((n_off + 1) // 2):
        yield ("cx", pair), (S_CX, pair, 0, 0)
        for child in (2 * pair, 2 * pair + 1):
            if child < n_off:
                for s in range(N):
                    yield ("cx_u", pair, s, "child", child), (S_CX, pair, s + 1, 0)
        for h, q in enumerate((2 * pair, (2 * pair + 1) % P)):   # the pair's two tournaments
            for j in range(tour_k):
                yield ("tour", "pair", pair, "parent", h, j), (S_TOUR, q, j, 0)


def word_users(entries) -> Dict[tuple, List[tuple]]:
    """word -> the distinct draws it feeds (the two outputs of a Box-Muller pair
    count as one consumer: they share both words by construction)."""
    users: Dict[tuple, List[tuple]] = {}
    for draw, word in entries:
        key = draw
        if draw[0].startswith("n_"):
            key = ("normal_pair",) + tuple(_pair_of(draw))
        lst = users.setdefault(word, [])
        if key not in lst:
            lst.append(key)
    return users


def _pair_of(draw) -> tuple:
    f, o, s, c = draw
    for i, (_, _, _, d1, d2) in enumerate(NORMAL_PAIRS):
        if (f, c) in (d1, d2):
            return (o, s, i)
    raise KeyError(draw)


class ExportedDraws:
    """A ``ggs.ga`` draw source (``tournament``, ``shuffle``, ``uniform``,
    ``generation``) over per-generation exported dicts, so that the numpy GA
    (``ga.genetic_approx(..., draws=ExportedDraws(dicts))``) consumes exactly the
    draws of a Philox run: ``shuffle`` is the identity, ``uniform`` returns values
    whose ``< cxpb`` is the exported ``cx`` (for any 0 < cxpb <= 1), ``generation``
    the crossover masks of the crossing pairs only and the mutation fields in the
    host shapes."""

    def __init__(self, generations):
        self.dicts = list(generations)
        self.g = -1

    def tournament(self, P, k):
        self.g += 1
        t = np.asarray(self.dicts[self.g]["tour_idx"]).reshape(P, k)
        return t

    def shuffle(self, P):
        perm = np.asarray(self.dicts[self.g]["perm"])
        assert np.array_equal(perm, np.arange(P)), "Philox mode does not shuffle"
        return np.arange(P)

    def uniform(self, n):
        cx = np.asarray(self.dicts[self.g]["cx"]).reshape(n)
        return np.where(cx != 0, 0.0, 1.0)

    def generation(self, cx, n_off, N, mutpb):
        from ggs.ga_device import MUTATION_KEYS
        d = self.dicts[self.g]
        host = {"u_xy": (n_off, N, 2), "u_ab": (n_off, N, 2), "u_t": (n_off, N, 1), "u_rgb": (n_off, N, 1),
                "u_a": (n_off, N, 1), "n_xy": (n_off, N, 2), "n_ab": (n_off, N, 2), "n_t": (n_off, N, 1),
                "n_rgba": (n_off, N, 4)}
        mut = {k: np.asarray(d[k]).reshape(host.get(k, (n_off,))) for k in MUTATION_KEYS}
        cxu = np.asarray(d["cx_u"], np.float32).reshape(len(cx), N)[np.asarray(cx, bool)].reshape(-1, N, 1)
        return cxu, mut
