"""Device-resident GA loop (ggs_ga_* in include/ggs.h, kernels in csrc/ggs_ga.hip).

The whole generation of algorithm.py:85-155 — selection, crossover, mutation,
fitness, elites, best individual, curves — runs on one GPU with no host round
trip; the host only enqueues.  ``DeviceGA.step(draws=...)`` accepts explicit
draws in ggs/ga.py's layout (tests/test_gpu_parity.py feeds it the same draws as
the host path and requires identical populations); ``DeviceGA.run`` uses the
in-kernel Philox stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._lib import GaConfig, GaDraws, check, lib

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)
SIG_KEYS = ("xy", "alog", "blog", "theta", "rgb", "alpha")
SCHEDULES = {"linear": 0, "cosine": 1, "exp": 2}


def _arr(x, dt):
    return np.ascontiguousarray(x, dtype=dt)


def _config(P, N, H, W, tour_k, elite_k, cxpb, mutpb, k_sigma, min_scale_splats,
            max_scale_splats, mask, boost_only, boost_beta, schedule, mut_sigma_max,
            mut_sigma_min, seed) -> GaConfig:
    from .ga import scale_log_bounds
    lo, hi = scale_log_bounds(H, W, min_scale_splats, max_scale_splats)
    mode = (_lib.GGS_FIT_NONE if mask is None else
            _lib.GGS_FIT_BOOST if boost_only else _lib.GGS_FIT_WEIGHTED)
    return GaConfig(P, N, H, W, tour_k, elite_k, cxpb, mutpb, k_sigma, min_scale_splats,
                    max_scale_splats, float(lo), float(hi), mode, boost_beta,
                    SCHEDULES.get(schedule, 0),
                    (C.c_double * 6)(*[mut_sigma_max[k] for k in SIG_KEYS]),
                    (C.c_double * 6)(*[mut_sigma_min[k] for k in SIG_KEYS]), seed & (2**64 - 1))


def _draws_struct(draws, keep, fields=None) -> GaDraws:
    d = GaDraws()
    for name, typ in GaDraws._fields_:
        if fields is not None and name not in fields:
            continue
        dt = np.float64 if name == "swap_u" else (np.int32 if typ is _i32p else np.float32)
        a = keep[name] = _arr(draws[name], dt)
        setattr(d, name, a.ctypes.data_as(typ))
    return d


class PhiloxAcceptDraws:
    """The device SA loop's acceptance uniforms (ggs_sa_accept_uniform: Philox keyed
    by (seed, iteration, try)) for the host loop, so a host-driven run with the
    device proposer follows the device loop's trajectory exactly."""

    def __init__(self, seed: int):
        self.seed = int(seed) & (2**64 - 1)

    def accept_at(self, it: int, k: int) -> float:
        u = C.c_double()
        check(lib.ggs_sa_accept_uniform(self.seed, int(it), int(k), C.byref(u)),
              "ggs_sa_accept_uniform")
        return u.value


MUTATION_KEYS = ("u_xy", "u_ab", "u_t", "u_rgb", "u_a", "k_color", "k_xy", "k_ab", "k_t", "n_xy",
                 "n_ab", "n_t", "n_rgba", "swap_i", "swap_pick", "swap_u")


class DeviceSA:
    """Device-resident SA state (ggs_sa_* in include/ggs.h): the current and best
    individuals live in HBM; ``propose`` returns the energies of a batch of tries."""

    def __init__(self, target, mask, init_ind, *, max_tries: int, mutpb: float,
                 mut_sigma_max: Dict[str, float], mut_sigma_min: Dict[str, float],
                 schedule: str, min_scale_splats: float, max_scale_splats: float,
                 k_sigma: float = 3.0, boost_only: bool = False, boost_beta: float = 1.0,
                 seed: int = 0, device: int = 0, incremental: bool = False):
        ind = _arr(init_ind, np.float32)
        if ind.ndim != 2 or ind.shape[1] != 9:
            raise _lib.GGSInputError("the device SA keeps an [N, 9] genome")
        self.target = _arr(target, np.float32)
        H, W = self.target.shape[:2]
        self.mask = None if mask is None else _arr(mask, np.float32)
        self.N, self.cap = ind.shape[0], max(1, int(max_tries))
        cfg = _config(self.cap, self.N, H, W, 1, 0, 0.0, mutpb, k_sigma, min_scale_splats,
                      max_scale_splats, self.mask, boost_only, boost_beta, schedule,
                      mut_sigma_max, mut_sigma_min, seed)
        _lib.ensure_init()
        h = C.c_void_p()
        f = C.c_float()
        check(lib.ggs_sa_create(device, C.byref(cfg), self.target.ctypes.data_as(_f32p),
                                None if self.mask is None else self.mask.ctypes.data_as(_f32p),
                                ind.ctypes.data_as(_f32p), C.byref(h), C.byref(f)),
              "ggs_sa_create")
        self.h, self.init_fit, self.last_n = h, f.value, 0
        check(lib.ggs_sa_set_incremental(h, int(bool(incremental))), "ggs_sa_set_incremental")

    def stats(self) -> Dict[str, int]:
        """Neighbours proposed and splats changed (the incremental path's work)."""
        p, c = C.c_uint64(), C.c_uint64()
        check(lib.ggs_sa_stats(self.h, C.byref(p), C.byref(c)), "ggs_sa_stats")
        return {"proposed": p.value, "changed_splats": c.value}

    def propose(self, it: int, total: int, first_try: int, n: int, draws=None) -> np.ndarray:
        out = np.empty(n, np.float32)
        keep = {}
        d = None if draws is None else C.byref(_draws_struct(draws, keep, MUTATION_KEYS))
        check(lib.ggs_sa_propose(self.h, it, total, first_try, n, d, out.ctypes.data_as(_f32p)),
              "ggs_sa_propose")
        self.last_n = n
        return out

    def commit(self, j: int, update_best: bool) -> None:
        check(lib.ggs_sa_commit(self.h, j, int(bool(update_best))), "ggs_sa_commit")

    def run(self, first_it: int, temps, total: int, tries: int, width: int = 0) -> np.ndarray:
        """Iterations first_it .. first_it+len(temps)-1 of the SA loop on the device
        (ggs_sa_run): acceptance walk and state updates included, one host sync per
        batch of rounds.  Returns the [n, 2] (best, current) energy curves."""
        t = _arr(temps, np.float64)
        out = np.empty((len(t), 2), np.float64)
        check(lib.ggs_sa_run(self.h, int(first_it), len(t), int(total), int(tries),
                             t.ctypes.data_as(_f64p), int(width), out.ctypes.data_as(_f64p)),
              "ggs_sa_run")
        return out

    def loop_state(self) -> Dict[str, float]:
        """Energies and counters of the device loop after the last ``run``."""
        b, c = C.c_double(), C.c_double()
        r, e, a = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib.ggs_sa_loop_state(self.h, C.byref(b), C.byref(c), C.byref(r), C.byref(e),
                                    C.byref(a)), "ggs_sa_loop_state")
        return {"best_fit": b.value, "current_fit": c.value, "rounds": r.value,
                "evaluated": e.value, "accepted": a.value}

    def read(self):
        cur = np.empty((self.N, 9), np.float32)
        best = np.empty((self.N, 9), np.float32)
        nb = np.empty((max(self.last_n, 1), self.N, 9), np.float32)
        check(lib.ggs_sa_read(self.h, cur.ctypes.data_as(_f32p), best.ctypes.data_as(_f32p),
                              nb.ctypes.data_as(_f32p)), "ggs_sa_read")
        return cur, best, nb[:self.last_n]

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_sa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


class DeviceSAChains:
    """K device-resident SA chains in one session (ggs_sa_chains_* in include/ggs.h):
    one set of launches per round for all chains, one raster launch over exactly
    the neighbours they have live.  ``init_inds`` is [K, N, 9], ``seeds`` [K];
    chain k without exchange follows ``DeviceSA(seed=seeds[k], init_ind=
    init_inds[k])`` run with ``temps[k]`` bit for bit.  ``max_tries`` is the
    neighbour capacity per chain.

    A 4-D ``target`` [K, H, W, 3] (with ``mask`` [K, H, W] or None) gives every
    chain its own image (ggs_sa_chains_create_targets); a 3-D target is shared by
    all chains, and only then may ``exchange_every`` = M > 0 ask for replica
    exchange after every iteration ``it`` with (it + 1) % M == 0
    (``ggs.annealing.replica_exchange`` states the rule)."""

    def __init__(self, target, mask, init_inds, seeds, *, exchange_every: int = 0,
                 exchange_seed: int = 0, max_tries: int, mutpb: float,
                 mut_sigma_max: Dict[str, float], mut_sigma_min: Dict[str, float],
                 schedule: str, min_scale_splats: float, max_scale_splats: float,
                 k_sigma: float = 3.0, boost_only: bool = False, boost_beta: float = 1.0,
                 device: int = 0):
        inds = _arr(init_inds, np.float32)
        if inds.ndim != 3 or inds.shape[2] != 9:
            raise _lib.GGSInputError("the chain group keeps [K, N, 9] genomes")
        K, N, _ = inds.shape
        sd = np.asarray([int(s) & (2**64 - 1) for s in seeds], np.uint64)
        if sd.shape != (K,):
            raise _lib.GGSInputError(f"seeds must have one entry per chain ({K}), got {sd.shape}")
        self.target = _arr(target, np.float32)
        self.mask = None if mask is None else _arr(mask, np.float32)
        self.per_chain = self.target.ndim == 4
        if self.per_chain:
            if self.target.shape[0] != K or self.target.shape[3] != 3:
                raise _lib.GGSInputError(
                    f"per-chain targets must be [K={K}, H, W, 3], got {self.target.shape}")
            if self.mask is not None and self.mask.shape != self.target.shape[:3]:
                raise _lib.GGSInputError(
                    f"per-chain masks must be {self.target.shape[:3]}, got {self.mask.shape}")
        elif self.target.ndim != 3:
            raise _lib.GGSInputError(f"target must be [H, W, 3] or [K, H, W, 3], got {self.target.shape}")
        H, W = self.target.shape[-3:-1]
        self.K, self.N, self.H, self.W, self.cap = K, N, H, W, max(1, int(max_tries))
        cfg = _config(self.cap, N, H, W, 1, 0, 0.0, mutpb, k_sigma, min_scale_splats,
                      max_scale_splats, self.mask, boost_only, boost_beta, schedule,
                      mut_sigma_max, mut_sigma_min, 0)
        ch = _lib.SaChains(K, int(exchange_every), sd.ctypes.data_as(C.POINTER(C.c_uint64)),
                           int(exchange_seed) & (2**64 - 1))
        h = C.c_void_p()
        fits = np.empty(K, np.float32)
        # arguments are validated before the library looks for a device
        create, name = ((lib.ggs_sa_chains_create_targets, "ggs_sa_chains_create_targets")
                        if self.per_chain else (lib.ggs_sa_chains_create, "ggs_sa_chains_create"))
        check(create(device, C.byref(cfg), C.byref(ch), self.target.ctypes.data_as(_f32p),
                     None if self.mask is None else self.mask.ctypes.data_as(_f32p),
                     inds.ctypes.data_as(_f32p), C.byref(h), fits.ctypes.data_as(_f32p)), name)
        self.h, self.init_fits = h, fits

    def run(self, first_it: int, temps, total: int, tries: int, width: int = 0) -> np.ndarray:
        """Iterations first_it .. first_it+n-1 of every chain (ggs_sa_chains_run),
        ``temps`` [K, n].  Returns the [K, n, 2] (best, current) energy curves."""
        t = _arr(temps, np.float64)
        if t.ndim != 2 or t.shape[0] != self.K:
            raise _lib.GGSInputError(f"temps must be [K={self.K}, n], got {t.shape}")
        out = np.empty((self.K, t.shape[1], 2), np.float64)
        check(lib.ggs_sa_chains_run(self.h, int(first_it), t.shape[1], int(total), int(tries),
                                    t.ctypes.data_as(_f64p), int(width), out.ctypes.data_as(_f64p)),
              "ggs_sa_chains_run")
        return out

    def loop_state(self) -> Dict[str, object]:
        """Per-chain energies and counters ([K] arrays) after the last ``run``, and
        the session's exchange counts."""
        K = self.K
        b, c = np.empty(K, np.float64), np.empty(K, np.float64)
        r, e, a = np.empty(K, np.uint64), np.empty(K, np.uint64), np.empty(K, np.uint64)
        st, sa = C.c_uint64(), C.c_uint64()
        u64p = C.POINTER(C.c_uint64)
        check(lib.ggs_sa_chains_state(self.h, b.ctypes.data_as(_f64p), c.ctypes.data_as(_f64p),
                                      r.ctypes.data_as(u64p), e.ctypes.data_as(u64p),
                                      a.ctypes.data_as(u64p), C.byref(st), C.byref(sa)),
              "ggs_sa_chains_state")
        return {"best_fit": b, "current_fit": c, "rounds": r, "evaluated": e, "accepted": a,
                "swaps_tried": st.value, "swaps_accepted": sa.value}

    def read(self):
        """(current [K, N, 9], best [K, N, 9])."""
        cur = np.empty((self.K, self.N, 9), np.float32)
        best = np.empty((self.K, self.N, 9), np.float32)
        check(lib.ggs_sa_chains_read(self.h, cur.ctypes.data_as(_f32p), best.ctypes.data_as(_f32p)),
              "ggs_sa_chains_read")
        return cur, best

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_sa_chains_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


class DeviceGA:
    """One device-resident GA population (see module docstring)."""

    def __init__(self, target, mask, init_pop, *, tour_k: int, elite_k: int, cxpb: float,
                 mutpb: float, mut_sigma_max: Dict[str, float], mut_sigma_min: Dict[str, float],
                 schedule: str, min_scale_splats: float, max_scale_splats: float,
                 k_sigma: float = 3.0, boost_only: bool = False, boost_beta: float = 1.0,
                 seed: int = 0, device: int = 0):
        pop = _arr(init_pop, np.float32)
        P, N, Cc = pop.shape
        if Cc != 9:
            raise _lib.GGSInputError("the device GA keeps [P, N, 9] genomes")
        self.target = _arr(target, np.float32)
        H, W = self.target.shape[:2]
        self.mask = None if mask is None else _arr(mask, np.float32)
        cfg = _config(P, N, H, W, tour_k, elite_k, cxpb, mutpb, k_sigma, min_scale_splats,
                      max_scale_splats, self.mask, boost_only, boost_beta, schedule,
                      mut_sigma_max, mut_sigma_min, seed)
        self.P, self.N, self.H, self.W, self.tour_k, self.cxpb = P, N, H, W, tour_k, cxpb
        _lib.ensure_init()
        h = C.c_void_p()
        check(lib.ggs_ga_create(device, C.byref(cfg), self.target.ctypes.data_as(_f32p),
                                None if self.mask is None else self.mask.ctypes.data_as(_f32p),
                                pop.ctypes.data_as(_f32p), C.byref(h)), "ggs_ga_create")
        self.h = h

    def set_comm(self, gather) -> None:
        """Shard each generation's offspring evaluation over the ranks of an
        ``ggs.RcclGather`` (one process per GPU, identical sessions on every rank;
        ggs_ga_set_comm).  ``None``: evaluate every offspring here."""
        self._comm = gather                     # keeps the communicator alive
        check(lib.ggs_ga_set_comm(self.h, None if gather is None else gather.handle), "ggs_ga_set_comm")

    def step(self, gen: int, total: int, draws: Optional[Dict[str, np.ndarray]] = None) -> None:
        """One generation; ``draws`` in ggs/ga.py layout (see draws_from_host)."""
        if draws is None:
            check(lib.ggs_ga_step(self.h, gen, total, None), "ggs_ga_step")
            return
        keep = {}
        d = _draws_struct(draws, keep)
        check(lib.ggs_ga_step(self.h, gen, total, C.byref(d)), "ggs_ga_step")

    def run(self, first_gen: int, n_gens: int, total: int) -> None:
        check(lib.ggs_ga_run(self.h, first_gen, n_gens, total), "ggs_ga_run")

    def read(self) -> Dict[str, object]:
        pop = np.empty((self.P, self.N, 9), np.float32)
        fits = np.empty(self.P, np.float32)
        best = np.empty((self.N, 9), np.float32)
        bf = C.c_double()
        n = C.c_int32()
        check(lib.ggs_ga_read(self.h, None, None, None, None, None, C.byref(n)), "ggs_ga_read")
        curves = np.empty((n.value, 3), np.float64)
        check(lib.ggs_ga_read(self.h, pop.ctypes.data_as(_f32p), fits.ctypes.data_as(_f32p),
                              best.ctypes.data_as(_f32p), C.byref(bf),
                              curves.ctypes.data_as(_f64p), C.byref(n)), "ggs_ga_read")
        return {"population": pop, "fitness": fits, "best": best, "best_fit": bf.value,
                "curves": {"best": curves[:, 0].tolist(), "mean": curves[:, 1].tolist(),
                           "median": curves[:, 2].tolist()}}

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_ga_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


class DeviceGAIslands:
    """K device-resident GA populations ("islands") with ring migration in one
    session (ggs_ga_islands_* in include/ggs.h): one breed launch and one raster
    launch per generation for all islands.  ``init_pops`` is [K, P, N, 9],
    ``seeds`` [K]; island k without migration follows ``DeviceGA(seed=seeds[k],
    init_pop=init_pops[k])`` bit for bit.  Every ``migrate_every`` generations the
    ``n_migrants`` best rows of island k-1 replace the worst rows of island k.

    A 4-D ``target`` [K, H, W, 3] (with ``mask`` [K, H, W] or None) gives every
    island its own image (ggs_ga_islands_create_targets): island k is fitted to
    ``target[k]``, and an immigrant is re-scored against its new island's target
    and mask before the elites are re-ranked (``ggs.ga.ring_migration`` with
    ``refit``).  A 3-D target is shared by all islands."""

    def __init__(self, target, mask, init_pops, seeds, migrate_every: int = 0, n_migrants: int = 0,
                 *, tour_k: int, elite_k: int, cxpb: float, mutpb: float,
                 mut_sigma_max: Dict[str, float], mut_sigma_min: Dict[str, float],
                 schedule: str, min_scale_splats: float, max_scale_splats: float,
                 k_sigma: float = 3.0, boost_only: bool = False, boost_beta: float = 1.0,
                 device: int = 0):
        pops = _arr(init_pops, np.float32)
        if pops.ndim != 4 or pops.shape[3] != 9:
            raise _lib.GGSInputError("the island group keeps [K, P, N, 9] genomes")
        K, P, N, _ = pops.shape
        sd = np.asarray([int(s) & (2**64 - 1) for s in seeds], np.uint64)
        if sd.shape != (K,):
            raise _lib.GGSInputError(f"seeds must have one entry per island ({K}), got {sd.shape}")
        self.target = _arr(target, np.float32)
        self.mask = None if mask is None else _arr(mask, np.float32)
        self.per_island = self.target.ndim == 4
        if self.per_island:
            if self.target.shape[0] != K or self.target.shape[3] != 3:
                raise _lib.GGSInputError(
                    f"per-island targets must be [K={K}, H, W, 3], got {self.target.shape}")
            if self.mask is not None and self.mask.shape != self.target.shape[:3]:
                raise _lib.GGSInputError(
                    f"per-island masks must be {self.target.shape[:3]}, got {self.mask.shape}")
        elif self.target.ndim != 3:
            raise _lib.GGSInputError(f"target must be [H, W, 3] or [K, H, W, 3], got {self.target.shape}")
        H, W = self.target.shape[-3:-1]
        cfg = _config(P, N, H, W, tour_k, elite_k, cxpb, mutpb, k_sigma, min_scale_splats,
                      max_scale_splats, self.mask, boost_only, boost_beta, schedule,
                      mut_sigma_max, mut_sigma_min, 0)
        isl = _lib.GaIslands(K, int(migrate_every), int(n_migrants), 0,
                             sd.ctypes.data_as(C.POINTER(C.c_uint64)))
        self.K, self.P, self.N, self.H, self.W = K, P, N, H, W
        h = C.c_void_p()
        # arguments are validated before the library looks for a device
        create, name = ((lib.ggs_ga_islands_create_targets, "ggs_ga_islands_create_targets")
                        if self.per_island else (lib.ggs_ga_islands_create, "ggs_ga_islands_create"))
        check(create(device, C.byref(cfg), C.byref(isl), self.target.ctypes.data_as(_f32p),
                     None if self.mask is None else self.mask.ctypes.data_as(_f32p),
                     pops.ctypes.data_as(_f32p), C.byref(h)), name)
        self.h = h

    def set_polish(self, every: int, steps: int, rows: int = 1, lr=None, beta1: float = 0.9,
                   beta2: float = 0.999, eps: float = 1e-8) -> None:
        """Memetic generations (ggs_ga_islands_set_polish): after every generation g with
        ``g % every == 0`` (and its migration) each island's ``rows`` best-ranked rows take
        ``steps`` Adam steps against the island's image and replace the row where strictly
        better (``ggs.ga.polish_elites`` is the rule).  ``every`` or ``steps`` 0: off.
        ``lr=None``: ``ggs.refine.DEFAULT_LR``."""
        if lr is None:
            from .refine import DEFAULT_LR as lr
        lr = np.asarray(lr, np.float32).reshape(-1)
        if lr.shape != (9,):
            raise _lib.GGSInputError("lr must have nine entries, one per genome column")
        adam = _lib.RefineParams((C.c_float * 9)(*[float(v) for v in lr]), float(beta1), float(beta2), float(eps))
        pol = _lib.GaPolish(int(every), int(steps), int(rows), adam)
        check(lib.ggs_ga_islands_set_polish(self.h, C.byref(pol)), "ggs_ga_islands_set_polish")

    def clear_polish(self) -> None:
        check(lib.ggs_ga_islands_set_polish(self.h, None), "ggs_ga_islands_set_polish")

    def run(self, first_gen: int, n_gens: int, total: int) -> None:
        check(lib.ggs_ga_islands_run(self.h, first_gen, n_gens, total), "ggs_ga_islands_run")

    def read(self) -> Dict[str, object]:
        """Per-island arrays (leading dimension K) and ``best_island``: the island
        with the lowest ``best_fit`` (the first one on ties)."""
        K = self.K
        pop = np.empty((K, self.P, self.N, 9), np.float32)
        fits = np.empty((K, self.P), np.float32)
        best = np.empty((K, self.N, 9), np.float32)
        bf = np.empty(K, np.float64)
        n = C.c_int32()
        check(lib.ggs_ga_islands_read(self.h, None, None, None, None, None, C.byref(n)),
              "ggs_ga_islands_read")
        curves = np.empty((K, n.value, 3), np.float64)
        check(lib.ggs_ga_islands_read(self.h, pop.ctypes.data_as(_f32p), fits.ctypes.data_as(_f32p),
                                      best.ctypes.data_as(_f32p), bf.ctypes.data_as(_f64p),
                                      curves.ctypes.data_as(_f64p), C.byref(n)), "ggs_ga_islands_read")
        return {"population": pop, "fitness": fits, "best": best, "best_fit": bf,
                "best_island": int(np.argmin(bf)),
                "curves": [{"best": c[:, 0].tolist(), "mean": c[:, 1].tolist(),
                            "median": c[:, 2].tolist()} for c in curves]}

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_ga_islands_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


class DeviceDE:
    """One device-resident differential-evolution population (ggs_de_* in
    include/ggs.h; ``ggs.de`` states the algorithm in numpy and names the
    strategies and crossovers).  ``F``: a number (fixed) or ``(f_lo, f_hi)`` (per
    trial uniform in that range); ``CR`` in [0, 1].  4 <= P <= 512."""

    def __init__(self, target, mask, init_pop, *, strategy="rand1", crossover="gene", F=(0.5, 0.9),
                 CR: float = 0.3, min_scale_splats: float, max_scale_splats: float,
                 k_sigma: float = 3.0, boost_only: bool = False, boost_beta: float = 1.0,
                 seed: int = 0, device: int = 0):
        pop = _arr(init_pop, np.float32)
        if pop.ndim != 3 or pop.shape[2] != 9:
            raise _lib.GGSInputError("the device DE keeps [P, N, 9] genomes")
        P, N, _ = pop.shape
        self.target = _arr(target, np.float32)
        H, W = self.target.shape[:2]
        self.mask = None if mask is None else _arr(mask, np.float32)
        zero = dict.fromkeys(SIG_KEYS, 0.0)             # the GA's operator fields are not read
        cfg = _config(P, N, H, W, 1, 0, 0.0, 0.0, k_sigma, min_scale_splats, max_scale_splats,
                      self.mask, boost_only, boost_beta, "linear", zero, zero, seed)
        self.P, self.N, self.H, self.W = P, N, H, W
        h = C.c_void_p()
        # arguments are validated before the library looks for a device
        check(lib.ggs_de_create(device, C.byref(cfg), C.byref(self._params(strategy, crossover, F, CR)),
                                self.target.ctypes.data_as(_f32p),
                                None if self.mask is None else self.mask.ctypes.data_as(_f32p),
                                pop.ctypes.data_as(_f32p), C.byref(h)), "ggs_de_create")
        self.h = h

    @staticmethod
    def _params(strategy, crossover, F, CR) -> "_lib.DeParams":
        from .de import crossover_id, f_range, strategy_id
        f_lo, f_hi = f_range(F)
        return _lib.DeParams(strategy_id(strategy), crossover_id(crossover), f_lo, f_hi, float(CR))

    def set_params(self, *, strategy="rand1", crossover="gene", F=(0.5, 0.9), CR: float = 0.3) -> None:
        """The operator parameters of the generations run from now on."""
        check(lib.ggs_de_set_params(self.h, C.byref(self._params(strategy, crossover, F, CR))),
              "ggs_de_set_params")

    def run(self, first_gen: int, n_gens: int) -> None:
        check(lib.ggs_de_run(self.h, int(first_gen), int(n_gens)), "ggs_de_run")

    def read(self) -> Dict[str, object]:
        """``DeviceGA.read``'s dict plus ``trials`` / ``trial_fits`` of the last
        generation run (unspecified before the first)."""
        pop = np.empty((self.P, self.N, 9), np.float32)
        trials = np.empty((self.P, self.N, 9), np.float32)
        fits, tf = np.empty(self.P, np.float32), np.empty(self.P, np.float32)
        best = np.empty((self.N, 9), np.float32)
        bf = C.c_double()
        n = C.c_int32()
        check(lib.ggs_de_read(self.h, None, None, None, None, None, None, None, C.byref(n)), "ggs_de_read")
        curves = np.empty((n.value, 3), np.float64)
        check(lib.ggs_de_read(self.h, pop.ctypes.data_as(_f32p), fits.ctypes.data_as(_f32p),
                              trials.ctypes.data_as(_f32p), tf.ctypes.data_as(_f32p),
                              best.ctypes.data_as(_f32p), C.byref(bf), curves.ctypes.data_as(_f64p),
                              C.byref(n)), "ggs_de_read")
        return {"population": pop, "fitness": fits, "trials": trials, "trial_fits": tf, "best": best,
                "best_fit": bf.value,
                "curves": {"best": curves[:, 0].tolist(), "mean": curves[:, 1].tolist(),
                           "median": curves[:, 2].tolist()}}

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_de_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


class DeviceRefine:
    """B candidates refined by Adam on the device (ggs_refine_* in include/ggs.h;
    ``ggs.refine.adam_step`` states the update in numpy).  ``lr``: nine per-column
    rates.  A 4-D ``target`` [K, H, W, 3] (``mask`` [K, H, W] or None) refines candidate
    b against image ``b // group`` in one session (ggs_refine_create_targets; ``group``
    defaults to B // K); what ``read`` returns for a candidate has the bits of a
    session on that genome and image alone.

    ``loss`` (an ``api.LossParams``; default None: the fitness above) descends the image
    loss L1 / MSE / SSIM of DESIGN.md §8f instead (ggs_refine_create_loss): ``mask`` must
    then be None, ``fitness`` / ``best_fits`` are the loss, ``background`` is the render's,
    and a step is ``api.loss_grad`` followed by ``adam_step``, bit for bit."""

    def __init__(self, target, mask, genomes, *, lr, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8, min_scale_splats: float, max_scale_splats: float,
                 k_sigma: float = 3.0, boost_only: bool = False, boost_beta: float = 1.0, device: int = 0,
                 group: Optional[int] = None, loss=None, background=(1.0, 1.0, 1.0)):
        x = _arr(genomes, np.float32)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[2] != 9:
            raise _lib.GGSInputError("the device refiner keeps [B, N, 9] genomes")
        if loss is not None and mask is not None:
            raise _lib.GGSInputError("the image loss takes no weight mask")
        B, N, _ = x.shape
        self.target = _arr(target, np.float32)
        many = self.target.ndim == 4
        if not many and group is not None:
            raise _lib.GGSInputError("group= needs a 4-D target [K, H, W, 3]")
        if self.target.ndim not in (3, 4) or self.target.shape[-1] != 3:
            raise _lib.GGSInputError(f"target must be [H, W, 3] or [K, H, W, 3], got {self.target.shape}")
        H, W = self.target.shape[-3:-1]
        self.mask = None if mask is None else _arr(mask, np.float32)
        if self.mask is not None and self.mask.shape != self.target.shape[:-1]:
            raise _lib.GGSInputError(f"mask must be {self.target.shape[:-1]}, got {self.mask.shape}")
        zero = dict.fromkeys(SIG_KEYS, 0.0)             # the GA's operator fields are not read
        cfg = _config(max(B, 1), N, H, W, 1, 0, 0.0, 0.0, k_sigma, min_scale_splats, max_scale_splats,
                      self.mask, boost_only, boost_beta, "linear", zero, zero, 0)
        lr = np.asarray(lr, np.float32).reshape(-1)
        if lr.shape != (9,):
            raise _lib.GGSInputError("lr must have nine entries, one per genome column")
        prm = _lib.RefineParams((C.c_float * 9)(*[float(v) for v in lr]), float(beta1), float(beta2), float(eps))
        self.B, self.N, self.H, self.W = B, N, H, W
        h = C.c_void_p()
        # arguments are validated before the library looks for a device
        mask_p = None if self.mask is None else self.mask.ctypes.data_as(_f32p)
        if loss is not None:
            from .api import loss_params_c
            K = self.target.shape[0] if many else 1
            if group is None:
                group = max(B // max(K, 1), 1) if many else B
            lp = loss_params_c(loss)
            bg = np.ascontiguousarray(np.broadcast_to(np.asarray(background, np.float32), (3,)))
            check(lib.ggs_refine_create_loss(device, C.byref(cfg), C.byref(prm), C.byref(lp),
                                             bg.ctypes.data_as(_f32p), self.target.ctypes.data_as(_f32p), K,
                                             x.ctypes.data_as(_f32p), B, int(group), C.byref(h)),
                  "ggs_refine_create_loss")
        elif many:
            K = self.target.shape[0]
            if group is None:
                group = max(B // max(K, 1), 1)
            check(lib.ggs_refine_create_targets(device, C.byref(cfg), C.byref(prm),
                                                self.target.ctypes.data_as(_f32p), mask_p, K,
                                                x.ctypes.data_as(_f32p), B, int(group), C.byref(h)),
                  "ggs_refine_create_targets")
        else:
            check(lib.ggs_refine_create(device, C.byref(cfg), C.byref(prm), self.target.ctypes.data_as(_f32p),
                                        mask_p, x.ctypes.data_as(_f32p), B, C.byref(h)), "ggs_refine_create")
        self.h = h

    def run(self, n_steps: int) -> None:
        check(lib.ggs_refine_run(self.h, int(n_steps)), "ggs_refine_run")

    def read(self) -> Dict[str, np.ndarray]:
        """The current state with its fitness, the best so far per candidate and the
        gradient of the last step run (zeros before the first)."""
        shape = (self.B, self.N, 9)
        x, best, grad = (np.empty(shape, np.float32) for _ in range(3))
        fits, bf = np.empty(self.B, np.float32), np.empty(self.B, np.float32)
        check(lib.ggs_refine_read(self.h, x.ctypes.data_as(_f32p), fits.ctypes.data_as(_f32p),
                                  best.ctypes.data_as(_f32p), bf.ctypes.data_as(_f32p),
                                  grad.ctypes.data_as(_f32p)), "ggs_refine_read")
        return {"genomes": x, "fitness": fits, "best": best, "best_fits": bf, "last_grad": grad}

    def set_density(self, params=None) -> None:
        """Density control (ggs_refine_set_density; ``ggs.DensityParams``) for the steps run
        after the call, with the accumulator and ``density_stats`` started from zero.  None or
        ``every = 0``: off, and a session that never had it on keeps its bits."""
        from .refine import density_moves, density_params_c
        prm = None if params is None else density_params_c(params)
        check(lib.ggs_refine_set_density(self.h, None if prm is None else C.byref(prm)), "ggs_refine_set_density")
        self._moves = 0 if prm is None else density_moves(prm, self.N)

    def density_stats(self) -> Dict[str, np.ndarray]:
        """ggs_refine_density_read: ``acc`` [B, N] and ``n_acc`` as they stand, ``moves`` /
        ``splits`` int64 [B] since ``set_density``, and the last event's ``last_pairs`` int32
        [B, M, 2] ((dead, source) rows, (-1, -1) past ``last_n`` [B]).  Refused while off."""
        M = getattr(self, "_moves", 0)
        acc = np.empty((self.B, self.N), np.float32)
        n_acc = C.c_int32(0)
        moves, splits = np.empty(self.B, np.int64), np.empty(self.B, np.int64)
        pairs, last_n = np.full((self.B, M, 2), -1, np.int32), np.empty(self.B, np.int32)
        i64p = C.POINTER(C.c_int64)
        check(lib.ggs_refine_density_read(self.h, acc.ctypes.data_as(_f32p), C.byref(n_acc),
                                          moves.ctypes.data_as(i64p), splits.ctypes.data_as(i64p),
                                          pairs.ctypes.data_as(_i32p), last_n.ctypes.data_as(_i32p)),
              "ggs_refine_density_read")
        return {"acc": acc, "n_acc": int(n_acc.value), "moves": moves, "splits": splits, "last_pairs": pairs,
                "last_n": last_n}

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_refine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


def draws_from_host(tour_idx, perm, cx, cxu_compact, mut, N: int) -> Dict[str, np.ndarray]:
    """Pack the draws ggs/ga.py's next_generation consumed into the device layout
    (crossover masks expanded to one row per pair)."""
    npairs = len(cx)
    cx_u = np.ones((npairs, N), np.float32)
    cx_u[np.asarray(cx, bool)] = np.asarray(cxu_compact, np.float32).reshape(-1, N)
    out = {"tour_idx": tour_idx, "perm": perm, "cx": np.asarray(cx, np.int32), "cx_u": cx_u}
    out.update({k: mut[k] for k in MUTATION_KEYS})
    return out


def philox_draws(seed: int, gen: int, n_off: int, P: int, N: int, tour_k: int, cxpb: float,
                 first: int = 0, device: int = 0) -> Dict[str, np.ndarray]:
    """ggs_ga_philox_draws (a stage export for parity tests): the draws the
    variation kernels take from the in-kernel Philox stream keyed by ``seed`` for
    generation ``gen`` (SA: iteration) and offspring ``first .. first+n_off-1``
    (SA: tries), computed on the device by the kernels' own draw functions, as the
    dict ``DeviceGA.step`` / ``DeviceSA.propose`` accept (ggs/ga.py's shapes, the
    crossover masks one row per pair).  A Philox run is the explicit run on these
    draws: ``DeviceGA(seed=s).run(g, 1, G)`` equals ``step(g, G, philox_draws(s, g,
    P, P, N, tour_k, cxpb))``, and ``propose(it, total, first_try, n)`` equals
    ``propose(..., draws=philox_draws(s, it, n, n, N, 1, 0.0, first=first_try))``."""
    n, np2 = int(n_off), (int(n_off) + 1) // 2
    shapes = {"tour_idx": (P, tour_k), "perm": (P,), "cx": (np2,), "cx_u": (np2, N),
              "u_xy": (n, N, 2), "u_ab": (n, N, 2), "u_t": (n, N, 1), "u_rgb": (n, N, 1), "u_a": (n, N, 1),
              "k_color": (n,), "k_xy": (n,), "k_ab": (n,), "k_t": (n,),
              "n_xy": (n, N, 2), "n_ab": (n, N, 2), "n_t": (n, N, 1), "n_rgba": (n, N, 4),
              "swap_i": (n,), "swap_pick": (n,), "swap_u": (n,)}
    out, d = {}, GaDraws()
    for name, typ in GaDraws._fields_:
        dt = np.float64 if name == "swap_u" else (np.int32 if typ is _i32p else np.float32)
        out[name] = np.empty([max(int(v), 0) for v in shapes[name]], dt)
        setattr(d, name, out[name].ctypes.data_as(typ))
    # arguments are validated before the library looks for a device
    check(lib.ggs_ga_philox_draws(int(device), int(seed) & (2**64 - 1), int(gen), int(first), n, int(P),
                                  int(N), int(tour_k), float(cxpb), C.byref(d)), "ggs_ga_philox_draws")
    return out


class RecordingDraws:
    """Wraps a ggs.ga draw source and keeps, per generation, the draws
    ``next_generation`` consumed — in the device layout (``draws_from_host``)."""

    def __init__(self, inner, cxpb: float):
        self.inner, self.cxpb = inner, cxpb
        self.generations = []
        self._cur = {}

    def tournament(self, P, k):
        self._cur = {"tour_idx": np.asarray(self.inner.tournament(P, k))}
        return self._cur["tour_idx"]

    def shuffle(self, P):
        self._cur["perm"] = np.asarray(self.inner.shuffle(P))
        return self._cur["perm"]

    def uniform(self, n):
        u = np.asarray(self.inner.uniform(n))
        self._cur["cx"] = u < self.cxpb
        return u

    def generation(self, cx, n_off, N, mutpb):
        cxu, mut = self.inner.generation(cx, n_off, N, mutpb)
        c = self._cur
        self.generations.append(draws_from_host(c["tour_idx"], c["perm"], c["cx"], cxu, mut, N))
        return cxu, mut


def run_device_ga(target, imp_mask, init_pop, generations: int, *, tour_k: int, elite_k: int,
                  cxpb: float, mutpb: float, mut_sigma_max, mut_sigma_min, schedule: str,
                  min_scale_splats: float, max_scale_splats: float, k_sigma: float,
                  boost_only: bool, seed: int, chunk: int, on_chunk=None, draws=None,
                  device: int = 0):
    """algorithm.py:85-155 for ``generations`` generations on one GPU.

    ``draws``: optional list of per-generation draw dicts (replay); otherwise the
    Philox stream keyed by ``seed``.  ``on_chunk(gen, ga)`` runs every ``chunk``
    generations (progress bar, video frames)."""
    ga = DeviceGA(target, imp_mask, init_pop, tour_k=tour_k, elite_k=elite_k, cxpb=cxpb,
                  mutpb=mutpb, mut_sigma_max=mut_sigma_max, mut_sigma_min=mut_sigma_min,
                  schedule=schedule, min_scale_splats=min_scale_splats,
                  max_scale_splats=max_scale_splats, k_sigma=k_sigma, boost_only=boost_only,
                  seed=seed, device=device)
    try:
        gen = 1
        try:
            while gen <= generations:
                n = min(max(1, chunk), generations - gen + 1)
                if draws is not None:
                    for g in range(gen, gen + n):
                        ga.step(g, generations, draws[g - 1])
                else:
                    ga.run(gen, n, generations)
                gen += n
                if on_chunk is not None:
                    on_chunk(gen - 1, ga)
        except KeyboardInterrupt:                                  # algorithm.py:157-158
            print("\n[Interrupted] Returning current best individual…", flush=True)
        return ga.read()
    finally:
        ga.close()


def run_device_ga_islands(target, imp_mask, init_pops, seeds, generations: int, *, migrate_every: int,
                          n_migrants: int, tour_k: int, elite_k: int, cxpb: float, mutpb: float,
                          mut_sigma_max, mut_sigma_min, schedule: str, min_scale_splats: float,
                          max_scale_splats: float, k_sigma: float, boost_only: bool, chunk: int,
                          on_chunk=None, device: int = 0, polish: Optional[Dict[str, object]] = None):
    """``run_device_ga`` for an island group (``DeviceGAIslands``).  Migrations are
    keyed to the generation number, so the result does not depend on ``chunk``.
    ``polish``: keyword arguments of ``DeviceGAIslands.set_polish`` (memetic generations)."""
    ga = DeviceGAIslands(target, imp_mask, init_pops, seeds, migrate_every, n_migrants,
                         tour_k=tour_k, elite_k=elite_k, cxpb=cxpb, mutpb=mutpb,
                         mut_sigma_max=mut_sigma_max, mut_sigma_min=mut_sigma_min, schedule=schedule,
                         min_scale_splats=min_scale_splats, max_scale_splats=max_scale_splats,
                         k_sigma=k_sigma, boost_only=boost_only, device=device)
    try:
        if polish:
            ga.set_polish(**polish)
        gen = 1
        try:
            while gen <= generations:
                n = min(max(1, chunk), generations - gen + 1)
                ga.run(gen, n, generations)
                gen += n
                if on_chunk is not None:
                    on_chunk(gen - 1, ga)
        except KeyboardInterrupt:                                  # algorithm.py:157-158
            print("\n[Interrupted] Returning current best individual…", flush=True)
        return ga.read()
    finally:
        ga.close()
