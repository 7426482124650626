"""Batched genetic algorithm around the MI355X evaluator.

Restates the reference's GA layer over whole populations instead of one
individual at a time:

* ``new_population``          population.py:20-46   (numpy RNG)
* ``tournament`` / ``crossover`` / ``mutate_batch``
                              genetic.py:8-21, 32-91 (every candidate of a
                              generation in one set of numpy array ops)
* ``build_mut_sigma`` / ``wrap_angle`` / ``clamp_genome``   utils.py:10-45
* ``genetic_approx``          algorithm.py:17-195    (same signature; one
                              libggs fitness launch per generation)

Randomness comes from a *draw source*.  ``NumpyDraws`` (default) samples the
same distributions as the reference's torch / Python RNG calls, in batches.
The operators consume the draws with exactly the reference's arithmetic
(float32, same operation order), so given the reference's own draws they
reproduce its results bit for bit — tests/test_ga.py replays draws recorded
from the reference (tests/golden/make_golden_ga.py) to prove it.

Two deliberate differences, both in what is evaluated, not in any result: the
reference re-evaluates the elites every generation (algorithm.py:134-137); the
evaluator is deterministic (same genome → same bits, tests/test_gpu_parity.py),
so their fitness is carried over instead of recomputed.  And it evaluates all
P offspring (algorithm.py:123-126) although only offspring[:P - elite_k] survive
(:140-141) and nothing reads the others' fitness; they are bred (their draws keep
the trajectory) but not evaluated, so an ``evaluate`` hook sees P - elite_k rows
per generation.  The returned values are identical.
"""
from __future__ import annotations

import csv
import math
import os
import random
import statistics
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

_f32 = np.float32
PI32 = _f32(np.pi)
TWO_PI32 = _f32(2 * np.pi)


# ---------------------------------------------------------------------------
# utils.py:10-45
# ---------------------------------------------------------------------------
def wrap_angle(theta: np.ndarray) -> np.ndarray:
    """utils.py:10-11: (θ + π) mod 2π − π in float32 (Python-style modulo)."""
    return np.remainder(theta + PI32, TWO_PI32) - PI32


def anneal_factor(gen: int, total: int, kind: str) -> float:
    """utils.py:14-27."""
    g = max(0, min(gen, total))
    p = g / max(1, total)
    if kind == "cosine":
        raw = 0.5 * (1.0 + math.cos(math.pi * p))
    elif kind == "linear":
        raw = 1.0 - p
    elif kind == "exp":
        decay = 0.2 ** (1.0 / max(1, total))
        raw = decay ** g
    else:
        raw = 1.0 - p
    return max(0.0, raw)


def build_mut_sigma(gen: int, total_gens: int, kind: str, mut_sigma_max: Dict[str, float],
                    mut_sigma_min: Dict[str, float]) -> Dict[str, float]:
    """utils.py:30-32."""
    f = anneal_factor(gen, total_gens, kind)
    return {k: mut_sigma_min[k] + f * (mut_sigma_max[k] - mut_sigma_min[k]) for k in mut_sigma_max}


def scale_log_bounds(H: int, W: int, min_scale_splats: float,
                     max_scale_splats: float) -> Tuple[np.float32, np.float32]:
    """utils.py:38-39: log of the float32 scale bounds."""
    max_side = float(max(H, W))
    return (np.log(_f32(min_scale_splats)).astype(np.float32),
            np.log(_f32(max_scale_splats * max_side)).astype(np.float32))


def clamp_genome(G: np.ndarray, H: int, W: int, min_scale_splats: float,
                 max_scale_splats: float) -> np.ndarray:
    """utils.py:35-45 on [..., N, 9] in place."""
    lo, hi = scale_log_bounds(H, W, min_scale_splats, max_scale_splats)
    G[..., 0:2] = np.clip(G[..., 0:2], _f32(0.0), _f32(1.0))
    G[..., 2] = np.clip(G[..., 2], lo, hi)
    G[..., 3] = np.clip(G[..., 3], lo, hi)
    G[..., 4] = wrap_angle(G[..., 4])
    G[..., 5:9] = np.clip(G[..., 5:9], _f32(0.0), _f32(255.0))
    return G


# ---------------------------------------------------------------------------
# draw sources
# ---------------------------------------------------------------------------
def resolve_seed(seed: Optional[int] = None) -> int:
    """An explicit seed, or — when None — one drawn from Python's global ``random``
    state, so that ``random.seed(SEED)`` in the reference's entry scripts
    (run_ggs.py:25-28, run_sags.py:26-27) makes a run repeatable here too."""
    return int(seed) if seed is not None else random.getrandbits(63)


class NumpyDraws:
    """Batched draws with the distributions of the reference's RNG calls.  With
    ``seed=None`` the generator is seeded from Python's ``random`` at first use
    (``resolve_seed``), not at construction: module-level sources made at import
    time still follow a later ``random.seed``."""

    def __init__(self, seed: Optional[int] = None):
        self._seed = seed
        self._rng = None

    @property
    def rng(self) -> np.random.Generator:
        if self._rng is None:
            self._rng = np.random.default_rng(resolve_seed(self._seed))
        return self._rng

    def tournament(self, P: int, k: int) -> np.ndarray:           # random.randrange (genetic.py:11)
        return self.rng.integers(0, P, (P, k))

    def shuffle(self, P: int) -> np.ndarray:                       # random.shuffle (algorithm.py:90)
        return self.rng.permutation(P)

    def uniform(self, n: int) -> np.ndarray:                       # random.random (algorithm.py:97)
        return self.rng.random(n)

    def crossover_masks(self, n: int, N: int) -> np.ndarray:       # torch.rand((N,1)) (genetic.py:18)
        return self.rng.random((n, N, 1), dtype=np.float32)

    def mutation(self, P: int, N: int, mutpb: float) -> Dict[str, np.ndarray]:
        """genetic.py:37-91: mask uniforms, one-true fallbacks, normals, swap."""
        r = self.rng
        u = lambda *s: r.random((P,) + s, dtype=np.float32)      # noqa: E731
        n = lambda *s: r.standard_normal((P,) + s, dtype=np.float32)  # noqa: E731
        return {
            "u_xy": u(N, 2), "u_ab": u(N, 2), "u_t": u(N, 1), "u_rgb": u(N, 1), "u_a": u(N, 1),
            "k_color": r.integers(0, 2 * N, P), "k_xy": r.integers(0, 2 * N, P),
            "k_ab": r.integers(0, 2 * N, P), "k_t": r.integers(0, N, P),
            "n_xy": n(N, 2), "n_ab": n(N, 2), "n_t": n(N, 1), "n_rgba": n(N, 4),
            "swap_i": r.integers(0, max(N - 1, 1), P), "swap_pick": np.full(P, -1),
            "swap_u": r.random(P),
        }

    def accept(self) -> float:                                     # random.random (annealing.py:142)
        return float(self.rng.random())

    def generation(self, cx: np.ndarray, n_off: int, N: int, mutpb: float):
        """Crossover masks for the crossing pairs + mutation draws for the offspring."""
        return self.crossover_masks(int(cx.sum()), N), self.mutation(n_off, N, mutpb)


# ---------------------------------------------------------------------------
# population.py:20-46
# ---------------------------------------------------------------------------
def new_population(batch_size: int, n_splats: int, H: int, W: int, min_scale_splats: float,
                   max_scale_splats: float, rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """[B, N, 9] axes-angle genomes with population.py's distributions."""
    rng = rng if rng is not None else np.random.default_rng(resolve_seed())
    B, N = batch_size, n_splats
    s_lo, s_hi = float(min_scale_splats), float(max_scale_splats * float(max(H, W)))

    def log_scales(m, conc=8.0, eps=1e-6):                     # population.py:6-15
        u = rng.beta(m * max(conc, eps) + eps, (1 - m) * max(conc, eps) + eps, (B, N, 1))
        return np.log((s_lo + u.astype(np.float32) * _f32(s_hi - s_lo)).astype(np.float32))

    G = np.concatenate([
        rng.random((B, N, 2), dtype=np.float32),
        log_scales(0.4), log_scales(0.6),
        rng.uniform(-np.pi, np.pi, (B, N, 1)).astype(np.float32),
        rng.uniform(0.0, 256.0, (B, N, 3)).astype(np.float32),
        rng.uniform(180.0, 256.0, (B, N, 1)).astype(np.float32),
    ], axis=-1).astype(np.float32)
    G[..., 0:2] = np.clip(G[..., 0:2], 0.0, 1.0)
    G[..., 5:9] = np.clip(G[..., 5:9], 0.0, 255.0)
    return G


# ---------------------------------------------------------------------------
# genetic.py operators, batched
# ---------------------------------------------------------------------------
def tournament(fits: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """genetic.py:8-14 for every selection at once: idx [P, k] drawn indices;
    the winner is the first drawn index with the smallest fitness."""
    return idx[np.arange(len(idx)), np.argmin(np.asarray(fits)[idx], axis=1)]


def crossover(a: np.ndarray, b: np.ndarray, u: np.ndarray, p: float = 0.5):
    """genetic.py:17-21 batched: a, b [n, N, C], u [n, N, 1] uniforms."""
    m = u < _f32(p)
    return np.where(m, a, b), np.where(m, b, a)


def _ensure_one_true(m: np.ndarray, k: np.ndarray) -> np.ndarray:
    """genetic.py:24-29 per individual: if no flag is set, set flat index k."""
    flat = m.reshape(len(m), -1)
    none = ~flat.any(axis=1)
    rows = np.nonzero(none)[0]
    flat[rows, k[rows]] = True
    return flat.reshape(m.shape)


def mutate_batch(G: np.ndarray, d: Dict[str, np.ndarray], gen: int, total_gens: int,
                 schedule: str, mut_sigma_max: Dict[str, float], mut_sigma_min: Dict[str, float],
                 mutpb: float, H: int, W: int, min_scale_splats: float,
                 max_scale_splats: float) -> np.ndarray:
    """genetic.py:32-91 for a batch [P, N, 9] (in place; returns G)."""
    SIG = build_mut_sigma(gen, total_gens, schedule, mut_sigma_max, mut_sigma_min)
    P, N = G.shape[:2]
    p = _f32(mutpb)
    m_xy = d["u_xy"] < p
    m_ab = d["u_ab"] < p
    m_t = d["u_t"] < p
    pair = _ensure_one_true(np.concatenate([d["u_rgb"] < p, d["u_a"] < p], axis=2), d["k_color"])
    m_rgba = np.concatenate([np.repeat(pair[..., 0:1], 3, axis=2), pair[..., 1:2]], axis=2)
    m_xy = _ensure_one_true(m_xy, d["k_xy"])
    m_ab = _ensure_one_true(m_ab, d["k_ab"])
    m_t = _ensure_one_true(m_t, d["k_t"])

    G[..., 0:2] += (d["n_xy"] * _f32(SIG["xy"])) * m_xy.astype(np.float32)
    sig_ab = np.array([SIG["alog"], SIG["blog"]], np.float32)
    G[..., 2:4] += (d["n_ab"] * sig_ab) * m_ab.astype(np.float32)
    G[..., 4:5] += (d["n_t"] * _f32(SIG["theta"])) * m_t.astype(np.float32)
    G[..., 4] = wrap_angle(G[..., 4])
    sig_rgba = np.array([SIG["rgb"], SIG["rgb"], SIG["rgb"], SIG["alpha"]], np.float32)
    G[..., 5:9] += (d["n_rgba"] * sig_rgba) * m_rgba.astype(np.float32)
    clamp_genome(G, H, W, min_scale_splats, max_scale_splats)

    if N >= 2:                                                    # genetic.py:79-91
        i = np.asarray(d["swap_i"], np.int64)
        rows = np.arange(P)
        size = np.exp(G[..., 2]) * np.exp(G[..., 3])
        cand = (np.arange(N)[None, :] > i[:, None]) & (size > size[rows, i][:, None])
        count = cand.sum(axis=1)
        pick = np.asarray(d["swap_pick"], np.int64).copy()
        fresh = pick < 0
        pick[fresh] = np.minimum((np.asarray(d["swap_u"])[fresh] * count[fresh]).astype(np.int64),
                                 np.maximum(count[fresh] - 1, 0))
        has = count > 0
        csum = np.cumsum(cand, axis=1)
        j = np.argmax(cand & (csum == (pick + 1)[:, None]), axis=1)   # (pick+1)-th candidate
        r = rows[has]
        gi, gj = G[r, i[has]].copy(), G[r, j[has]].copy()
        G[r, i[has]] = gj
        G[r, j[has]] = gi
    return G


# ---------------------------------------------------------------------------
# algorithm.py:17-195
# ---------------------------------------------------------------------------
def next_generation(pop: np.ndarray, fits: np.ndarray, draws, gen: int, generations: int,
                    tour_k: int, cxpb: float, mutpb: float, mut_sigma_max, mut_sigma_min,
                    schedule: str, H: int, W: int, min_scale_splats: float,
                    max_scale_splats: float) -> np.ndarray:
    """algorithm.py:86-120: selection, crossover and mutation → offspring [P, N, C]."""
    P = len(pop)
    parents = tournament(fits, draws.tournament(P, tour_k))
    parents = parents[draws.shuffle(P)]
    npairs = (P + 1) // 2
    a_idx = parents[0::2][:npairs]
    b_idx = parents[(np.arange(npairs) * 2 + 1) % P]
    cx = draws.uniform(npairs) < cxpb
    cxu, mut = draws.generation(cx, P, pop.shape[1], mutpb)
    c1 = pop[a_idx].copy()
    c2 = pop[b_idx].copy()
    if cx.any():
        c1[cx], c2[cx] = crossover(pop[a_idx[cx]], pop[b_idx[cx]], cxu)
    off = np.empty((2 * npairs,) + pop.shape[1:], pop.dtype)
    off[0::2], off[1::2] = c1, c2
    off = np.ascontiguousarray(off[:P])
    return mutate_batch(off, mut, gen, generations, schedule, mut_sigma_max, mut_sigma_min,
                        mutpb, H, W, min_scale_splats, max_scale_splats)


def _render_best_u8(best: np.ndarray, H: int, W: int, k_sigma: float, device=None) -> np.ndarray:
    """utils.py:48-58: render one axes-angle genome to uint8 [H, W, 3]."""
    from . import api
    img = api.render(api.encode(best[None]), H, W, k_sigma=k_sigma, device=device)[0]
    return (np.clip(img, 0, 1) * 255.0).astype(np.uint8)


def save_frame_png(gen: int, ind, pad: int, prefix: str, video_dir: str, H: int, W: int,
                   k_sigma: float, device=None, save_video: bool = True) -> None:
    """utils.py:61-69."""
    if not save_video:
        return
    from PIL import Image
    fname = f"{prefix}_{gen:0{pad}d}.png"
    Image.fromarray(_render_best_u8(np.asarray(ind, np.float32), H, W, k_sigma, device)).save(
        os.path.join(video_dir, fname))


def save_curves_csv(curves: Dict[str, Sequence[float]], out_csv_path: str) -> None:
    """utils.py:133-151: gen,<key1>,<key2>,..."""
    if not out_csv_path:
        return
    d = os.path.dirname(out_csv_path)
    if d:
        os.makedirs(d, exist_ok=True)
    keys = list(curves.keys())
    lens = [len(v) for v in curves.values() if len(v) > 0]
    if not lens:
        print("[warn] No values to save to CSV")
        return
    with open(out_csv_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["gen"] + keys)
        for i in range(lens[0]):
            w.writerow([i] + [curves[k][i] if i < len(curves[k]) else "" for k in keys])


def save_loss_curve_png(curves, out_path: str, title: str = "GA fitness over generations",
                        xlabel: str = "Generation", ylabel: str = "MSE", log_y: bool = False,
                        dpi: int = 144) -> None:
    """utils.py:85-130: one line per named curve against its index, written as a
    PNG.  Same contract as the reference: nothing when out_path is empty; a
    warning and no file without matplotlib or without any values; ValueError when
    the non-empty curves differ in length."""
    if not out_path:
        return
    try:
        import matplotlib
        matplotlib.use("Agg")
        from matplotlib.figure import Figure
    except Exception as e:  # noqa: BLE001 — the reference degrades to a warning too
        print(f"[warn] matplotlib not available, cannot save plot: {e}")
        return
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    series = {k: list(v) for k, v in curves.items() if len(v)}
    if not series:
        print("[warn] No values to plot")
        return
    lengths = {k: len(v) for k, v in series.items()}
    n = next(iter(lengths.values()))
    bad = [k for k, m in lengths.items() if m != n]
    if bad:
        raise ValueError(f"Curve '{bad[0]}' length {lengths[bad[0]]} does not match others {n}")
    fig = Figure()
    ax = fig.add_subplot()
    x = np.arange(n)
    for name, ys in series.items():
        ax.plot(x, ys, label=name)
    ax.set(title=title, xlabel=xlabel, ylabel=ylabel)
    if log_y:
        ax.set_yscale("log")
    ax.grid(True, which="both", alpha=0.3)
    ax.legend()
    fig.tight_layout()
    fig.savefig(out_path, dpi=dpi)


def ring_migration(pops: np.ndarray, fits: np.ndarray, m: int, refit=None):
    """One ring migration of an island group on the host (the definition the
    device applies, include/ggs.h): with every island ranked by fitness
    (ascending, ties by lower row), the row of rank j < m of island (k - 1) mod K
    overwrites the row of rank P - 1 - j of island k, genome and fitness, all
    islands at once from the pre-migration state.  ``pops`` [K, P, N, 9],
    ``fits`` [K, P]; returns new arrays.  K < 2 or m == 0: copies.

    ``refit`` (islands with a target each): ``refit(k, genomes [m, N, 9]) -> [m]``
    gives the immigrants' fitness on island k, in the order j = 0 .. m - 1 (the
    source island's ranks); it is installed instead of the fitness the rows had
    on their source island, whose target it was measured against.  Which rows
    move is decided from the pre-migration fitness either way."""
    pops, fits = np.asarray(pops), np.asarray(fits)
    K, P = fits.shape
    if not 0 <= m <= P // 2:
        raise ValueError(f"migrants must be in [0, {P // 2}], got {m}")
    new_p, new_f = pops.copy(), fits.copy()
    if K < 2 or m == 0:
        return new_p, new_f
    order = [np.argsort(fits[k], kind="stable") for k in range(K)]
    for k in range(K):
        src = (k - 1) % K
        for j in range(m):
            new_p[k, order[k][P - 1 - j]] = pops[src, order[src][j]]
            new_f[k, order[k][P - 1 - j]] = fits[src, order[src][j]]
        if refit is not None:
            rows = [order[k][P - 1 - j] for j in range(m)]
            new_f[k, rows] = np.asarray(refit(k, new_p[k, rows]), new_f.dtype).reshape(m)
    return new_p, new_f


def polish_elites(pops: np.ndarray, fits: np.ndarray, n_rows: int, refine):
    """One polish of an island group on the host (the definition the device
    applies, ``ggs_ga_islands_set_polish`` in include/ggs.h): island k's rows of
    fitness rank j < ``n_rows`` (ascending fitness, ties by lower row) are handed
    to ``refine(k, genomes [n_rows, N, 9]) -> (best [n_rows, N, 9], best_fits
    [n_rows])`` in rank order, and a refined individual and its fitness overwrite
    the row iff that fitness is strictly lower than the row's; any other row
    keeps its bits.  ``pops`` [K, P, N, 9], ``fits`` [K, P]; returns new arrays."""
    pops, fits = np.asarray(pops), np.asarray(fits)
    if fits.ndim != 2 or pops.ndim != 4 or pops.shape[:2] != fits.shape:
        raise ValueError(f"pops must be [K, P, N, 9] and fits [K, P], got {pops.shape} and {fits.shape}")
    K, P = fits.shape
    n_rows = int(n_rows)
    if not 1 <= n_rows <= P:
        raise ValueError(f"n_rows must be in [1, {P}], got {n_rows}")
    new_p, new_f = pops.copy(), fits.copy()
    for k in range(K):
        rows = np.argsort(fits[k], kind="stable")[:n_rows]
        best, bf = refine(k, pops[k, rows].copy())
        best = np.asarray(best, pops.dtype).reshape((n_rows,) + pops.shape[2:])
        bf = np.asarray(bf, fits.dtype).reshape(n_rows)
        for j, r in enumerate(rows):
            if bf[j] < fits[k, r]:
                new_p[k, r] = best[j]
                new_f[k, r] = bf[j]
    return new_p, new_f


def combine_island_curves(curves: Sequence[Dict[str, Sequence[float]]]) -> Dict[str, List[float]]:
    """An island group's saved curves from the islands' own: per generation,
    ``best`` = min over islands, ``mean`` = mean of the islands' means,
    ``median`` = median of the islands' medians."""
    best = np.asarray([c["best"] for c in curves], np.float64)
    mean = np.asarray([c["mean"] for c in curves], np.float64)
    med = np.asarray([c["median"] for c in curves], np.float64)
    return {"best": best.min(axis=0).tolist(), "mean": mean.mean(axis=0).tolist(),
            "median": np.median(med, axis=0).tolist()}


def genetic_approx(target_img_uint8, H: int, W: int, device, pop_size: int, n_splats: int,
                   generations: int, tour_k: int, elite_k: int, cxpb: float, mutpb: float,
                   mut_sigma_max: dict, mut_sigma_min: dict, schedule: str,
                   min_scale_splats: float, max_scale_splats: float, k_sigma: float,
                   mask_strength: float, boost_only: bool, save_video: bool = False,
                   frame_every: int = 5000, video_dir: str = "", prefix: str = "ga",
                   loss_png_path: str = "", loss_csv_path: str = "", loss_log_y: bool = False,
                   *, seed: Optional[int] = None, draws=None,
                   evaluate: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                   init_population: Optional[np.ndarray] = None, progress: bool = True,
                   return_state: bool = False, backend: str = "auto", chunk: int = 50,
                   islands: int = 1, migrate_every: int = 0, migrants: int = 0,
                   polish_steps: int = 0, memetic_every: int = 0, memetic_steps: int = 0,
                   memetic_rows: int = 1):
    """algorithm.py:17-195 → (best individual [N, 9] float32, best fitness).

    ``memetic_every`` = M > 0 with ``memetic_steps`` > 0 (device backend only; both
    default to 0, which changes nothing): after every generation g with g % M == 0
    each island's ``memetic_rows`` best individuals take ``memetic_steps`` Adam steps
    on the device gradient (``ggs.refine.DEFAULT_LR``) and replace their row where
    that lowered the fitness, inside the session and without a host round trip
    (``ga_device.DeviceGAIslands.set_polish``, ``polish_elites`` is the rule;
    DESIGN.md §8d).  ``islands=1`` then runs an island group of one, whose
    trajectory is the single session's.  docs/EXPERIMENTS.md §26 has what was
    measured; no setting has been tuned.

    ``polish_steps`` > 0: after the last generation the best individual is refined
    by that many Adam steps on the device gradient (``ggs.refine.refine`` with its
    default rates, same target, mask and mode) and the refined individual is
    returned if its fitness is lower.  0 (the default) changes nothing.

    Extra keyword-only hooks: ``seed`` / ``draws`` (draw source), ``evaluate``
    (population [M,N,9] → fitness [M]: the initial population, then the P -
    elite_k surviving offspring of each generation; default: one libggs launch
    with the importance mask), ``init_population``, ``return_state`` (also return the
    final population, fitnesses and curves), ``backend``: "host" (numpy
    operators, one libggs fitness launch per generation), "device" (the whole
    generation on the GPU, ggs/ga_device.py; Philox draws keyed by ``seed``, or
    the draws a ``ga_device.RecordingDraws`` holds; ``chunk`` generations per
    host call) or "auto" (device unless an ``evaluate`` or ``draws`` hook is
    given).

    ``islands`` = K > 1 (device backend only) runs K populations of ``pop_size``
    rows as one island group (``ga_device.DeviceGAIslands``): island k is seeded
    with ``(seed + k) mod 2^64`` and starts from ``new_population(...,
    default_rng(seed_k))`` (``init_population``, when given, is [K, P, N, 9]);
    every ``migrate_every`` generations the ``migrants`` best individuals of
    island k - 1 replace the worst of island k (0: never).  The call returns the
    best individual over all islands and its fitness, frames render it, and the
    saved curves are, per generation, ``best`` = min over the islands, ``mean`` =
    mean of the islands' means, ``median`` = median of the islands' medians.
    ``return_state`` then also holds ``"islands"``: the per-island ``population``
    [K, P, N, 9], ``fitness`` [K, P] and ``curves`` (a list of K dicts), while
    ``"population"`` / ``"fitness"`` are those of the best island."""
    out = _genetic_approx_search(target_img_uint8, H, W, device, pop_size, n_splats, generations, tour_k,
                                 elite_k, cxpb, mutpb, mut_sigma_max, mut_sigma_min, schedule,
                                 min_scale_splats, max_scale_splats, k_sigma, mask_strength, boost_only,
                                 save_video, frame_every, video_dir, prefix, loss_png_path, loss_csv_path,
                                 loss_log_y, seed=seed, draws=draws, evaluate=evaluate,
                                 init_population=init_population, progress=progress,
                                 return_state=return_state, backend=backend, chunk=chunk, islands=islands,
                                 migrate_every=migrate_every, migrants=migrants,
                                 memetic=(int(memetic_every), int(memetic_steps), int(memetic_rows)))
    if int(polish_steps) <= 0:
        return out
    from . import api
    from .mask import compute_importance_mask, prepare_target
    from .refine import refine
    t = prepare_target(target_img_uint8, H, W)
    imp_mask = compute_importance_mask(t, H, W, edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3,
                                       gamma=0.7, floor=0.15, smooth=3, strength=mask_strength)
    best_ind, best_fit = out[0], out[1]
    r = refine(best_ind, t, H, W, int(polish_steps), k_sigma=k_sigma, weight_mask=imp_mask,
               boost_only=boost_only, min_scale_splats=min_scale_splats,
               max_scale_splats=max_scale_splats, device=api.device_index(device))
    if float(r["best_fits"][0]) < float(best_fit):
        best_ind, best_fit = r["best"][0].copy(), float(r["best_fits"][0])
    return (best_ind, best_fit) + tuple(out[2:])


def _memetic_polish(every: int, steps: int, rows: int):
    """``DeviceGAIslands.set_polish``'s keyword arguments for the ``memetic_*`` arguments, None when off."""
    if every < 0 or steps < 0:
        raise ValueError(f"memetic_every and memetic_steps must be >= 0, got {every} and {steps}")
    if rows < 1:
        raise ValueError(f"memetic_rows must be >= 1, got {rows}")
    return dict(every=every, steps=steps, rows=rows) if every > 0 and steps > 0 else None


def _genetic_approx_search(target_img_uint8, H, W, device, pop_size, n_splats, generations, tour_k, elite_k,
                           cxpb, mutpb, mut_sigma_max, mut_sigma_min, schedule, min_scale_splats,
                           max_scale_splats, k_sigma, mask_strength, boost_only, save_video, frame_every,
                           video_dir, prefix, loss_png_path, loss_csv_path, loss_log_y, *, seed, draws,
                           evaluate, init_population, progress, return_state, backend, chunk, islands,
                           migrate_every, migrants, memetic=(0, 0, 1)):
    """``genetic_approx`` without the polish."""
    from .mask import compute_importance_mask, prepare_target

    islands = int(islands)
    if islands < 1:
        raise ValueError(f"islands must be >= 1, got {islands}")
    polish = _memetic_polish(*memetic)
    if polish is not None:
        if backend not in ("auto", "host", "device"):
            raise ValueError(f"backend must be 'host' or 'device', got {backend!r}")
        if backend == "host" or evaluate is not None or draws is not None:
            raise ValueError("memetic generations run in the device session: backend='device', no evaluate / "
                             "draws hooks")
    if islands > 1:
        if backend == "host":
            raise ValueError("islands > 1 needs backend='device': the host backend runs one population")
        if backend not in ("auto", "device"):
            raise ValueError(f"backend must be 'host' or 'device', got {backend!r}")
        if evaluate is not None or draws is not None:
            raise ValueError("islands > 1 runs on the device with Philox draws: no evaluate / draws hooks")
    seed = resolve_seed(seed)                                          # run_ggs.py:25-28 seeds `random`
    t = prepare_target(target_img_uint8, H, W)                         # algorithm.py:33-39
    imp_mask = compute_importance_mask(t, H, W, edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3,
                                       gamma=0.7, floor=0.15, smooth=3,
                                       strength=mask_strength)          # algorithm.py:42-49
    if islands > 1:
        seeds = [(seed + k) % 2**64 for k in range(islands)]
        if init_population is not None:
            pops = np.array(init_population, np.float32, copy=True)
            if pops.ndim != 4 or pops.shape[0] != islands:
                raise ValueError(f"init_population must be [islands={islands}, P, N, 9], got {pops.shape}")
        else:
            pops = np.stack([new_population(pop_size, n_splats, H, W, min_scale_splats, max_scale_splats,
                                            np.random.default_rng(sk)) for sk in seeds])
        return _genetic_approx_device(t, imp_mask, pops, H, W, generations, tour_k, elite_k, cxpb,
                                      mutpb, mut_sigma_max, mut_sigma_min, schedule,
                                      min_scale_splats, max_scale_splats, k_sigma, boost_only,
                                      save_video, frame_every, video_dir, prefix, loss_png_path,
                                      loss_csv_path, loss_log_y, seed, None, progress,
                                      return_state, chunk, device,
                                      islands=(seeds, int(migrate_every), int(migrants)), polish=polish)
    if polish is not None:      # an island group of one: the single session's trajectory
        pop = (np.array(init_population, np.float32, copy=True) if init_population is not None else
               new_population(pop_size, n_splats, H, W, min_scale_splats, max_scale_splats,
                              np.random.default_rng(seed)))
        return _genetic_approx_device(t, imp_mask, pop[None], H, W, generations, tour_k, elite_k, cxpb,
                                      mutpb, mut_sigma_max, mut_sigma_min, schedule,
                                      min_scale_splats, max_scale_splats, k_sigma, boost_only,
                                      save_video, frame_every, video_dir, prefix, loss_png_path,
                                      loss_csv_path, loss_log_y, seed, None, progress,
                                      return_state, chunk, device,
                                      islands=([seed & (2**64 - 1)], 0, 0), polish=polish)
    if evaluate is None:
        from . import api

        def evaluate(G):
            return api.fitness(G, t, H, W, k_sigma, weight_mask=imp_mask, boost_only=boost_only,
                               device=device)
    pop = (np.array(init_population, np.float32, copy=True) if init_population is not None else
           new_population(pop_size, n_splats, H, W, min_scale_splats, max_scale_splats,
                          np.random.default_rng(seed)))
    if backend == "auto":
        backend = "device" if evaluate is None and draws is None else "host"
    if backend == "device":
        return _genetic_approx_device(t, imp_mask, pop, H, W, generations, tour_k, elite_k, cxpb,
                                      mutpb, mut_sigma_max, mut_sigma_min, schedule,
                                      min_scale_splats, max_scale_splats, k_sigma, boost_only,
                                      save_video, frame_every, video_dir, prefix, loss_png_path,
                                      loss_csv_path, loss_log_y, seed, draws, progress,
                                      return_state, chunk, device)
    if backend != "host":
        raise ValueError(f"backend must be 'host' or 'device', got {backend!r}")
    draws = draws if draws is not None else NumpyDraws(seed)
    fits = np.asarray(evaluate(pop), np.float32)

    best_idx = int(np.argmin(fits))
    best_ind = pop[best_idx].copy()
    best_fit = float(fits[best_idx])
    no_improve = 0
    fl = fits.tolist()
    curves = {"best": [best_fit], "mean": [float(sum(fl) / len(fl))], "median": [float(statistics.median(fl))]}
    pad = len(str(generations))
    if save_video:
        save_frame_png(0, best_ind, pad, prefix, video_dir, H, W, k_sigma, device, save_video)

    elite_k_actual = max(1, elite_k)
    bar = range(1, generations + 1)
    if progress:
        try:
            from tqdm.auto import tqdm
            bar = tqdm(bar, desc="GA generations", leave=True)
        except ImportError:
            pass
    try:
        for gen in bar:
            off = next_generation(pop, fits, draws, gen, generations, tour_k, cxpb, mutpb,
                                  mut_sigma_max, mut_sigma_min, schedule, H, W,
                                  min_scale_splats, max_scale_splats)
            # algorithm.py:123-126 evaluates all offspring, but only off[:keep] survive
            # (:140-141) and nothing reads the rest's fitness: evaluate the survivors
            keep = pop_size - elite_k_actual
            off_fits = (np.asarray(evaluate(off[:keep]), np.float32) if keep > 0
                        else np.zeros(0, np.float32))
            elite_idx = np.argsort(fits, kind="stable")[:elite_k_actual]     # algorithm.py:129-131
            pop = np.concatenate([pop[elite_idx], off[:keep]], axis=0)
            fits = np.concatenate([fits[elite_idx], off_fits[:keep]], axis=0)  # elites: carried over
            g = int(np.argmin(fits))
            if float(fits[g]) + 1e-10 < best_fit:                            # algorithm.py:144-150
                best_fit = float(fits[g])
                best_ind = pop[g].copy()
                no_improve = 0
            else:
                no_improve += 1
            fl = fits.tolist()
            curves["best"].append(float(best_fit))
            curves["mean"].append(float(sum(fl) / len(fl)))
            curves["median"].append(float(statistics.median(fl)))
            if save_video and gen % max(1, frame_every) == 0:
                save_frame_png(gen, best_ind, pad, prefix, video_dir, H, W, k_sigma, device, save_video)
            if hasattr(bar, "set_postfix"):
                bar.set_postfix(best_mse=f"{best_fit:.6f}", stale=no_improve,
                                sigma_fac=f"{anneal_factor(gen, generations, schedule):.3f}")
    except KeyboardInterrupt:
        print("\n[Interrupted] Returning current best individual…", flush=True)
    finally:
        if hasattr(bar, "close"):
            bar.close()

    save_loss_curve_png(curves, loss_png_path, title=f"{prefix} fitness", xlabel="Generation",
                        ylabel="MSE", log_y=loss_log_y, dpi=144)
    save_curves_csv(curves, loss_csv_path)
    if return_state:
        return best_ind, best_fit, {"population": pop, "fitness": fits, "curves": curves}
    return best_ind, best_fit


def genetic_approx_many(images, H: int, W: int, device, pop_size: int, n_splats: int,
                        generations: int, tour_k: int, elite_k: int, cxpb: float, mutpb: float,
                        mut_sigma_max: dict, mut_sigma_min: dict, schedule: str,
                        min_scale_splats: float, max_scale_splats: float, k_sigma: float,
                        mask_strength: float, boost_only: bool, *, seed: Optional[int] = None,
                        migrate_every: int = 0, migrants: int = 0,
                        init_population: Optional[np.ndarray] = None, chunk: int = 50,
                        progress: bool = True, return_state: bool = False, prep: str = "host",
                        polish_steps: int = 0, memetic_every: int = 0, memetic_steps: int = 0,
                        memetic_rows: int = 1):
    """``genetic_approx`` (device backend) for K images in one session: an island
    group with a target per island (``ga_device.DeviceGAIslands`` with a 4-D
    target), one breed and one raster launch per generation for all K.

    Each image goes through ``prepare_target`` and ``compute_importance_mask`` as
    in ``genetic_approx``; image k is seeded ``(seed + k) mod 2^64`` and starts
    from ``new_population(..., default_rng(seed_k))`` (``init_population``, when
    given, is [K, P, N, 9]).  With ``migrate_every`` == 0 image k's result is that
    of ``genetic_approx(images[k], ..., seed=seed + k, backend="device")``, bit for
    bit; with migration the ``migrants`` best of image k - 1's population are
    re-scored against image k before they replace its worst (neighbouring frames
    or tiles seed each other).  ``prep="device"`` prepares the K targets and masks
    on the device (``mask.prepare_targets``, within 2e-5 of the host's; the default
    ``"host"`` keeps every earlier result).

    ``memetic_every`` / ``memetic_steps`` / ``memetic_rows`` are ``genetic_approx``'s
    (every image's best rows polished against that image, all K in one launch
    chain).  ``polish_steps`` > 0: after the last generation the K best individuals
    are refined in ONE session (``ggs_refine_create_targets``, candidate k against
    image k) and kept where lower; each result equals
    ``genetic_approx(images[k], ..., polish_steps=...)`` bit for bit.

    Returns a list of K ``(best individual [N, 9], best fitness)``; with
    ``return_state`` each entry is ``(best, best_fit, {"population", "fitness",
    "curves"})``.  No frames, CSV or PNG outputs."""
    from . import api
    from .ga_device import run_device_ga_islands
    from .mask import compute_importance_mask, prepare_target, prepare_targets

    images = list(images)
    K = len(images)
    if K < 1:
        raise ValueError("genetic_approx_many needs at least one image")
    if prep not in ("host", "device"):
        raise ValueError(f"prep must be 'host' or 'device', got {prep!r}")
    memetic = (int(memetic_every), int(memetic_steps), int(memetic_rows))
    polish = _memetic_polish(*memetic)
    seed = resolve_seed(seed)
    seeds = [(seed + k) % 2**64 for k in range(K)]
    if prep == "device":
        targets, masks = prepare_targets(images, H, W, edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3,
                                         gamma=0.7, floor=0.15, smooth=3, strength=mask_strength,
                                         backend="device", device=device)
    else:
        targets = np.stack([prepare_target(im, H, W) for im in images])
        masks = np.stack([compute_importance_mask(t, H, W, edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3,
                                                  gamma=0.7, floor=0.15, smooth=3, strength=mask_strength)
                          for t in targets])
    if init_population is not None:
        pops = np.array(init_population, np.float32, copy=True)
        if pops.ndim != 4 or pops.shape[0] != K:
            raise ValueError(f"init_population must be [K={K}, P, N, 9], got {pops.shape}")
    else:
        pops = np.stack([new_population(pop_size, n_splats, H, W, min_scale_splats, max_scale_splats,
                                        np.random.default_rng(sk)) for sk in seeds])
    bar = None
    if progress:
        try:
            from tqdm.auto import tqdm
            bar = tqdm(total=generations, desc=f"GA generations (device, {K} images)", leave=True)
        except ImportError:
            pass
    state = {"gen": 0}

    def on_chunk(gen, ga):
        if bar is not None:
            bar.update(gen - state["gen"])
        state["gen"] = gen

    try:
        st = run_device_ga_islands(targets, masks, pops, seeds, generations,
                                   migrate_every=int(migrate_every), n_migrants=int(migrants),
                                   tour_k=tour_k, elite_k=elite_k, cxpb=cxpb, mutpb=mutpb,
                                   mut_sigma_max=mut_sigma_max, mut_sigma_min=mut_sigma_min,
                                   schedule=schedule, min_scale_splats=min_scale_splats,
                                   max_scale_splats=max_scale_splats, k_sigma=k_sigma,
                                   boost_only=boost_only, chunk=max(1, chunk), on_chunk=on_chunk,
                                   device=api.device_index(device), polish=polish)
    finally:
        if bar is not None:
            bar.close()
    refined = None
    if int(polish_steps) > 0:
        from .refine import refine
        refined = refine(st["best"], targets, H, W, int(polish_steps), k_sigma=k_sigma, weight_mask=masks,
                         boost_only=boost_only, min_scale_splats=min_scale_splats,
                         max_scale_splats=max_scale_splats, device=api.device_index(device), group=1)
    out = []
    for k in range(K):
        best, bf = st["best"][k], float(st["best_fit"][k])
        if refined is not None and float(refined["best_fits"][k]) < bf:
            best, bf = refined["best"][k].copy(), float(refined["best_fits"][k])
        if return_state:
            out.append((best, bf, {"population": st["population"][k], "fitness": st["fitness"][k],
                                   "curves": st["curves"][k]}))
        else:
            out.append((best, bf))
    return out


def _genetic_approx_device(t, imp_mask, pop, H, W, generations, tour_k, elite_k, cxpb, mutpb,
                           mut_sigma_max, mut_sigma_min, schedule, min_scale_splats,
                           max_scale_splats, k_sigma, boost_only, save_video, frame_every,
                           video_dir, prefix, loss_png_path, loss_csv_path, loss_log_y, seed,
                           draws, progress, return_state, chunk, device=None, islands=None, polish=None):
    """genetic_approx with backend="device" (ggs/ga_device.py) on the GPU
    ``device`` names (api.device_index).  ``islands``: (seeds, migrate_every,
    migrants) of an island group, ``pop`` then being [K, P, N, 9]."""
    from . import api
    from .ga_device import run_device_ga, run_device_ga_islands
    pad = len(str(generations))
    every = max(1, frame_every)
    step = max(1, chunk)
    if save_video:
        step = math.gcd(step, every)                  # land on every frame generation
    bar = None
    if progress:
        try:
            from tqdm.auto import tqdm
            bar = tqdm(total=generations, desc="GA generations (device)", leave=True)
        except ImportError:
            pass
    state = {"gen": 0}

    def on_chunk(gen, ga):
        if bar is not None:
            bar.update(gen - state["gen"])
        state["gen"] = gen
        if save_video and gen % every == 0:
            st = ga.read()
            best = st["best"] if islands is None else st["best"][st["best_island"]]
            save_frame_png(gen, best, pad, prefix, video_dir, H, W, k_sigma, device, save_video)
        if bar is not None:
            bar.set_postfix(sigma_fac=f"{anneal_factor(gen, generations, schedule):.3f}")

    if save_video:
        p0 = pop.reshape(-1, *pop.shape[-2:])
        f0 = api.fitness(p0, t, H, W, k_sigma, weight_mask=imp_mask, boost_only=boost_only,
                         device=device)
        save_frame_png(0, p0[int(np.argmin(f0))], pad, prefix, video_dir, H, W, k_sigma, device,
                       save_video)
    replay = getattr(draws, "generations", None) if draws is not None else None
    try:
        if islands is not None:
            st = run_device_ga_islands(t, imp_mask, pop, islands[0], generations,
                                       migrate_every=islands[1], n_migrants=islands[2],
                                       tour_k=tour_k, elite_k=elite_k, cxpb=cxpb, mutpb=mutpb,
                                       mut_sigma_max=mut_sigma_max, mut_sigma_min=mut_sigma_min,
                                       schedule=schedule, min_scale_splats=min_scale_splats,
                                       max_scale_splats=max_scale_splats, k_sigma=k_sigma,
                                       boost_only=boost_only, chunk=step, on_chunk=on_chunk,
                                       device=api.device_index(device), polish=polish)
        else:
            st = run_device_ga(t, imp_mask, pop, generations, tour_k=tour_k, elite_k=elite_k,
                               cxpb=cxpb, mutpb=mutpb, mut_sigma_max=mut_sigma_max,
                               mut_sigma_min=mut_sigma_min, schedule=schedule,
                               min_scale_splats=min_scale_splats,
                               max_scale_splats=max_scale_splats,
                               k_sigma=k_sigma, boost_only=boost_only,
                               seed=resolve_seed(seed) & (2**64 - 1), chunk=step,
                               on_chunk=on_chunk, draws=replay, device=api.device_index(device))
    finally:
        if bar is not None:
            bar.close()
    if islands is not None:
        b = st["best_island"]
        per_island = {"population": st["population"], "fitness": st["fitness"], "curves": st["curves"]}
        st = {"population": st["population"][b], "fitness": st["fitness"][b], "best": st["best"][b],
              "best_fit": float(st["best_fit"][b]), "curves": combine_island_curves(st["curves"])}
    curves = st["curves"]
    save_loss_curve_png(curves, loss_png_path, title=f"{prefix} fitness", xlabel="Generation",
                        ylabel="MSE", log_y=loss_log_y, dpi=144)
    save_curves_csv(curves, loss_csv_path)
    best_ind, best_fit = st["best"], st["best_fit"]
    if return_state and islands is not None:
        return best_ind, best_fit, {"population": st["population"], "fitness": st["fitness"],
                                    "curves": curves, "islands": per_island}
    if return_state:
        return best_ind, best_fit, {"population": st["population"], "fitness": st["fitness"],
                                    "curves": curves}
    return best_ind, best_fit
