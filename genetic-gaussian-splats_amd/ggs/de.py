"""Differential evolution around the MI355X evaluator: a third optimiser next to
``ggs.ga`` and ``ggs.annealing``.

The numpy functions here are the specification; the device session
(``ga_device.DeviceDE``, ggs_de_* in include/ggs.h, kernels in csrc/ggs_ga.hip)
is held to them bit for bit (tests/test_gpu_de.py).

State: population ``x`` [P, N, 9] of axes-angle genomes and fitness ``f`` [P],
float32.  Generation ``gen >= 1`` is synchronous: all P trials are built from
the population as it stood at the start of the generation.

* ``de_decollide``  the three row indices of a target row: distinct, not the row
* ``de_trials``     mutant (rand/1, best/1, current-to-best/1), binomial
                    crossover per gene or per splat, clamp of the mutant's genes
* ``de_select``     trial i replaces row i iff f_trial[i] <= f[i]
* ``de_stats``      best row, sequential float64 mean, ``statistics.median`` —
                    the GA's curves arithmetic
* ``differential_evolution``  the loop, ``ggs.ga.genetic_approx``'s shape

Splats are homologous by index across individuals (the GA's crossover is per
row), so a difference of splat ``s`` between two individuals is a meaningful
direction, and the steps shrink per gene as the population converges: there is
no sigma table.  Every arithmetic operation is one float32 rounding in the
written order (the kernels are built with -ffp-contract=off).

Randomness comes from a *draw source* with ``generation(gen, P, N) -> dict``:
``r`` [P, 3] int32 (already de-collided), ``jrand`` [P] (a flat gene index
``9 s + c`` for the per-gene crossover, a splat index for the per-splat one),
``f_u`` [P] and ``cr_u`` [P, N, 9] float32 uniforms in [0, 1) (the per-splat
crossover reads ``cr_u[:, :, 0]``).  ``NumpyDeDraws`` is the default; the
device's Philox stream is restated in tests/_philox_de.py.
"""
from __future__ import annotations

import math
import statistics
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np

from .ga import (new_population, resolve_seed, save_curves_csv, save_frame_png, save_loss_curve_png,
                 scale_log_bounds, wrap_angle)

_f32 = np.float32
STRATEGIES = {"rand1": 0, "best1": 1, "current-to-best1": 2}
CROSSOVERS = {"gene": 0, "splat": 1}


def strategy_id(strategy) -> int:
    """0 rand/1, 1 best/1, 2 current-to-best/1, from a name of ``STRATEGIES`` or the number."""
    if isinstance(strategy, str):
        if strategy not in STRATEGIES:
            raise ValueError(f"strategy must be one of {sorted(STRATEGIES)}, got {strategy!r}")
        return STRATEGIES[strategy]
    return int(strategy)


def crossover_id(crossover) -> int:
    """0 per gene, 1 per splat, from a name of ``CROSSOVERS`` or the number."""
    if isinstance(crossover, str):
        if crossover not in CROSSOVERS:
            raise ValueError(f"crossover must be one of {sorted(CROSSOVERS)}, got {crossover!r}")
        return CROSSOVERS[crossover]
    return int(crossover)


def f_range(F) -> Tuple[float, float]:
    """``F`` as (f_lo, f_hi): a number is a fixed F."""
    if np.ndim(F) == 0:
        return float(F), float(F)
    f_lo, f_hi = F
    return float(f_lo), float(f_hi)


# ---------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------
def de_decollide(i: int, raw: Sequence[int]) -> Tuple[int, int, int]:
    """Row indices of target row ``i`` from the raw draws ``raw`` = (r1 in
    [0, P-1), r2 in [0, P-2), r3 in [0, P-3)): r1 must avoid {i}, r2 {i, r1}, r3
    {i, r1, r2}.  For each r, walk its excluded values in ascending order and add
    1 whenever r >= e.  The results are distinct, different from ``i`` and uniform
    over what is left."""
    out = []
    for r in raw:
        r = int(r)
        for e in sorted([int(i)] + out):
            if r >= e:
                r += 1
        out.append(r)
    return tuple(out)


class NumpyDeDraws:
    """A generation's draws from ``np.random.default_rng(seed)`` (seeded from
    Python's ``random`` at first use when ``seed`` is None, as ``ga.NumpyDraws``)."""

    def __init__(self, seed: Optional[int] = None, crossover="gene"):
        self._seed, self._rng = seed, None
        self.per_splat = crossover_id(crossover) == 1

    @property
    def rng(self) -> np.random.Generator:
        if self._rng is None:
            self._rng = np.random.default_rng(resolve_seed(self._seed))
        return self._rng

    def generation(self, gen: int, P: int, N: int) -> Dict[str, np.ndarray]:
        g = self.rng
        raw = np.stack([g.integers(0, P - 1 - k, P) for k in range(3)], axis=1)
        r = np.array([de_decollide(i, raw[i]) for i in range(P)], np.int32)
        return {"r": r, "jrand": g.integers(0, N if self.per_splat else 9 * N, P).astype(np.int32),
                "f_u": g.random(P, dtype=np.float32), "cr_u": g.random((P, N, 9), dtype=np.float32)}


# ---------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------
def best_row(fits: np.ndarray) -> int:
    """The row of lowest fitness, ties to the lowest row (a scan with a strict <,
    so a NaN is never chosen over row 0)."""
    g = 0
    for r in range(1, len(fits)):
        if fits[r] < fits[g]:
            g = r
    return g


def _clamp_mutant(v: np.ndarray, log_lo, log_hi) -> np.ndarray:
    """clamp_genome's rules on [..., 9] (utils.py:35-45) for given log-scale bounds."""
    out = np.empty_like(v)
    out[..., 0:2] = np.clip(v[..., 0:2], _f32(0.0), _f32(1.0))
    out[..., 2:4] = np.clip(v[..., 2:4], _f32(log_lo), _f32(log_hi))
    out[..., 4] = wrap_angle(v[..., 4])
    out[..., 5:9] = np.clip(v[..., 5:9], _f32(0.0), _f32(255.0))
    return out


def _diff(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a - b, the angle column through wrap_angle."""
    d = a - b
    d[..., 4] = wrap_angle(d[..., 4])
    return d


def de_trials(pop: np.ndarray, fits: np.ndarray, draws: Dict[str, np.ndarray], *, strategy, crossover,
              f_lo: float, f_hi: float, cr: float, log_lo: float, log_hi: float) -> np.ndarray:
    """The P trials of one generation, [P, N, 9] float32.

    ``F_i = f_lo + f_u (f_hi - f_lo)``; with ``best`` = ``best_row(fits)`` and d
    a difference whose angle column went through ``wrap_angle``:

    * rand/1              ``v = x[r1] + F_i (x[r2] - x[r3])``
    * best/1              ``v = x[best] + F_i (x[r1] - x[r2])``
    * current-to-best/1   ``v = (x[i] + F_i (x[best] - x[i])) + F_i (x[r1] - x[r2])``

    Gene (s, c) of trial i is the mutant's iff ``cr_u[i, s, c] < cr`` or it is the
    ``jrand`` gene (per splat: ``cr_u[i, s, 0] < cr`` or ``s == jrand``, then all
    nine genes); only those are clamped (clamp_genome's rules with the given
    log-scale bounds).  Every other gene is ``x[i][s, c]`` bit for bit: inherited
    angles are not wrapped again (re-applying ``wrap_angle`` moves about half of
    them by an ulp, and the population would drift every generation)."""
    x = np.ascontiguousarray(pop, np.float32)
    P, N, _ = x.shape
    st, per_splat = strategy_id(strategy), crossover_id(crossover) == 1
    if st not in (0, 1, 2):
        raise ValueError(f"unknown strategy {strategy!r}")
    r = np.asarray(draws["r"], np.int64).reshape(P, 3)
    jrand = np.asarray(draws["jrand"], np.int64).reshape(P)
    if (jrand < 0).any() or (jrand >= (N if per_splat else 9 * N)).any():
        raise ValueError("jrand out of range for this crossover (a splat index per splat, 9 s + c per gene)")
    f_lo, f_hi = _f32(f_lo), _f32(f_hi)
    F = (f_lo + np.asarray(draws["f_u"], np.float32).reshape(P) * (f_hi - f_lo))[:, None, None]
    r1, r2, r3 = x[r[:, 0]], x[r[:, 1]], x[r[:, 2]]
    if st == 0:
        v = r1 + F * _diff(r2, r3)
    else:
        best = x[best_row(np.asarray(fits, np.float32))][None]
        if st == 1:
            v = best + F * _diff(r1, r2)
        else:
            v = (x + F * _diff(best, x)) + F * _diff(r1, r2)
    cr_u = np.asarray(draws["cr_u"], np.float32).reshape(P, N, 9)
    if per_splat:
        take = (cr_u[:, :, 0] < _f32(cr)) | (np.arange(N)[None, :] == jrand[:, None])
        take = np.repeat(take[:, :, None], 9, axis=2)
    else:
        take = (cr_u < _f32(cr)).reshape(P, 9 * N) | (np.arange(9 * N)[None, :] == jrand[:, None])
        take = take.reshape(P, N, 9)
    return np.where(take, _clamp_mutant(v.astype(np.float32), log_lo, log_hi), x)


def de_select(pop: np.ndarray, fits: np.ndarray, trials: np.ndarray,
              trial_fits: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Trial i replaces row i iff ``trial_fits[i] <= fits[i]`` in float32 (a NaN
    keeps the parent, a tie takes the trial).  Returns new arrays."""
    f, tf = np.asarray(fits, np.float32), np.asarray(trial_fits, np.float32)
    take = tf <= f
    return np.where(take[:, None, None], trials, pop).astype(np.float32), np.where(take, tf, f)


def de_stats(fits: np.ndarray) -> Tuple[int, float, float]:
    """(best row, mean, median) of a fitness vector with the GA's arithmetic: the
    mean a sequential float64 sum in row order over P, ``statistics.median``."""
    fl = [float(v) for v in np.asarray(fits, np.float32)]
    total = fl[0]
    for v in fl[1:]:
        total += v
    return best_row(fits), total / len(fl), float(statistics.median(fl))


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
def differential_evolution(target_img_uint8, H: int, W: int, device, pop_size: int, n_splats: int,
                           generations: int, *, strategy="rand1", crossover="gene", F=(0.5, 0.9),
                           CR: float = 0.3, min_scale_splats: float, max_scale_splats: float,
                           k_sigma: float, mask_strength: float, boost_only: bool,
                           save_video: bool = False, frame_every: int = 5000, video_dir: str = "",
                           prefix: str = "de", loss_png_path: str = "", loss_csv_path: str = "",
                           loss_log_y: bool = False, seed: Optional[int] = None, draws=None,
                           evaluate: Optional[Callable[[np.ndarray], np.ndarray]] = None,
                           init_population: Optional[np.ndarray] = None, progress: bool = True,
                           return_state: bool = False, backend: str = "auto", chunk: int = 50):
    """``ggs.ga.genetic_approx`` with differential evolution as the search operator
    → (best individual [N, 9] float32, best fitness).

    ``strategy``: "rand1", "best1" or "current-to-best1"; ``crossover``: "gene" or
    "splat"; ``F``: a number or ``(f_lo, f_hi)`` (per trial uniform); ``CR`` in
    [0, 1].  The defaults of ``F`` and ``CR`` are starting values, not tuned.
    Everything else means what it means for ``genetic_approx`` (``prefix``
    defaults to "de"): ``evaluate`` (population [M, N, 9] → fitness [M]: the
    initial population, then the P trials of each generation), ``draws`` (a source
    with ``generation(gen, P, N)``; default ``NumpyDeDraws(seed, crossover)``),
    ``backend``: "host" (numpy operators, one libggs fitness launch per
    generation), "device" (``ga_device.DeviceDE``: Philox draws keyed by ``seed``,
    ``chunk`` generations per host call) or "auto" (device unless an ``evaluate``
    or ``draws`` hook is given).  4 <= pop_size (<= 512 on the device)."""
    from .mask import compute_importance_mask, prepare_target

    if pop_size < 4:
        raise ValueError(f"pop_size must be >= 4 (three distinct rows besides the target), got {pop_size}")
    f_lo, f_hi = f_range(F)
    st, cx = strategy_id(strategy), crossover_id(crossover)
    seed = resolve_seed(seed)
    t = prepare_target(target_img_uint8, H, W)
    imp_mask = compute_importance_mask(t, H, W, edge_scales=(1, 2, 4), w_edge=0.7, w_var=0.3,
                                       gamma=0.7, floor=0.15, smooth=3, strength=mask_strength)
    pop = (np.array(init_population, np.float32, copy=True) if init_population is not None else
           new_population(pop_size, n_splats, H, W, min_scale_splats, max_scale_splats,
                          np.random.default_rng(seed)))
    if backend == "auto":
        backend = "device" if evaluate is None and draws is None else "host"
    if backend not in ("host", "device"):
        raise ValueError(f"backend must be 'host' or 'device', got {backend!r}")
    pad = len(str(generations))
    every = max(1, frame_every)
    bar = None
    if progress:
        try:
            from tqdm.auto import tqdm
            bar = tqdm(total=generations, desc=f"DE generations ({backend})", leave=True)
        except ImportError:
            pass

    def frame(gen, best):
        save_frame_png(gen, best, pad, prefix, video_dir, H, W, k_sigma, device, save_video)

    try:
        if backend == "device":
            st_out = _run_device(t, imp_mask, pop, generations, st, cx, (f_lo, f_hi), CR, min_scale_splats,
                                 max_scale_splats, k_sigma, boost_only, seed, chunk, save_video, every,
                                 frame, bar, device)
        else:
            if evaluate is None:
                from . import api

                def evaluate(G):
                    return api.fitness(G, t, H, W, k_sigma, weight_mask=imp_mask, boost_only=boost_only,
                                       device=device)
            draws = draws if draws is not None else NumpyDeDraws(seed, cx)
            lo, hi = scale_log_bounds(H, W, min_scale_splats, max_scale_splats)

            def on_generation(gen, best):
                if bar is not None and gen > 0:
                    bar.update(1)
                if save_video and gen % every == 0:
                    frame(gen, best)

            st_out = run_host_de(pop, generations, draws, evaluate, strategy=st, crossover=cx, f_lo=f_lo,
                                 f_hi=f_hi, cr=CR, log_lo=lo, log_hi=hi, on_generation=on_generation)
    finally:
        if bar is not None:
            bar.close()
    curves = st_out["curves"]
    save_loss_curve_png(curves, loss_png_path, title=f"{prefix} fitness", xlabel="Generation",
                        ylabel="MSE", log_y=loss_log_y, dpi=144)
    save_curves_csv(curves, loss_csv_path)
    if return_state:
        return st_out["best"], st_out["best_fit"], {"population": st_out["population"],
                                                    "fitness": st_out["fitness"], "curves": curves}
    return st_out["best"], st_out["best_fit"]


def run_host_de(pop: np.ndarray, generations: int, draws, evaluate, *, strategy, crossover, f_lo: float,
                f_hi: float, cr: float, log_lo: float, log_hi: float, first_gen: int = 1, state=None,
                on_generation=None) -> Dict[str, object]:
    """The DE loop on the host: ``de_trials`` → ``evaluate`` → ``de_select`` →
    statistics, generations ``first_gen .. first_gen + generations - 1``.  Returns
    ``DeviceDE.read``'s dict (``trials`` / ``trial_fits`` of the last generation).
    ``state``: a dict this function returned, to continue from (other parameters,
    say); without it ``pop`` is evaluated and gives curves row 0, and
    ``on_generation(0, best)`` is called."""
    if state is None:
        pop = np.array(pop, np.float32, copy=True)
        fits = np.asarray(evaluate(pop), np.float32)
        g, mean, med = de_stats(fits)
        best_ind, best_fit = pop[g].copy(), float(fits[g])
        curves = {"best": [best_fit], "mean": [mean], "median": [med]}
        trials, tf = None, None
        if on_generation is not None:
            on_generation(0, best_ind)
    else:
        pop, fits = state["population"], state["fitness"]
        best_ind, best_fit = state["best"], state["best_fit"]
        curves = {k: list(v) for k, v in state["curves"].items()}
        trials, tf = state.get("trials"), state.get("trial_fits")
    P, N, _ = pop.shape
    try:
        for gen in range(first_gen, first_gen + generations):
            trials = de_trials(pop, fits, draws.generation(gen, P, N), strategy=strategy, crossover=crossover,
                               f_lo=f_lo, f_hi=f_hi, cr=cr, log_lo=log_lo, log_hi=log_hi)
            tf = np.asarray(evaluate(trials), np.float32)
            pop, fits = de_select(pop, fits, trials, tf)
            g, mean, med = de_stats(fits)
            if float(fits[g]) + 1e-10 < best_fit:
                best_fit, best_ind = float(fits[g]), pop[g].copy()
            curves["best"].append(best_fit)
            curves["mean"].append(mean)
            curves["median"].append(med)
            if on_generation is not None:
                on_generation(gen, best_ind)
    except KeyboardInterrupt:
        print("\n[Interrupted] Returning current best individual…", flush=True)
    return {"population": pop, "fitness": fits, "trials": trials, "trial_fits": tf, "best": best_ind,
            "best_fit": best_fit, "curves": curves}


def _run_device(t, imp_mask, pop, generations, strategy, crossover, F, CR, min_scale_splats, max_scale_splats,
                k_sigma, boost_only, seed, chunk, save_video, every, frame, bar, device):
    from . import api
    from .ga_device import DeviceDE
    step = max(1, chunk)
    if save_video:
        step = math.gcd(step, every)                  # land on every frame generation
    de = DeviceDE(t, imp_mask, pop, strategy=strategy, crossover=crossover, F=F, CR=CR,
                  min_scale_splats=min_scale_splats, max_scale_splats=max_scale_splats, k_sigma=k_sigma,
                  boost_only=boost_only, seed=seed & (2**64 - 1), device=api.device_index(device))
    try:
        if save_video:
            frame(0, de.read()["best"])
        gen = 1
        try:
            while gen <= generations:
                n = min(step, generations - gen + 1)
                de.run(gen, n)
                gen += n
                if bar is not None:
                    bar.update(n)
                if save_video and (gen - 1) % every == 0:
                    frame(gen - 1, de.read()["best"])
        except KeyboardInterrupt:
            print("\n[Interrupted] Returning current best individual…", flush=True)
        return de.read()
    finally:
        de.close()
