"""Inputs of the density-control tests (tests/test_density_host.py on the CPU,
tests/test_gpu_density_relocate.py on the device): seeded genomes with planted alphas
(ties, values exactly at ``alpha_dead``), a crafted accumulator (ties, +-0.0, NaN, inf) and
``split_log`` at the median of max(log a, log b) so that clones and splits both occur."""
from __future__ import annotations

import numpy as np

import detmath
import ggs_oracle as oracle
from ggs import ga
from ggs.refine import DensityParams

MIN_S, MAX_S = 0.5, 0.5
ALPHA_DEAD = 16.0
N_ACC = 4
# exp, sin, cos of csrc/ggs_detmath.h as the oracle states them (bit-identical to the
# device: tests/test_gpu_parity.py::test_detmath_bit_exact)
ORACLE_DETMATH = (detmath.exp_f32, lambda a: detmath.sincos_f32(a)[0], lambda a: detmath.sincos_f32(a)[1])


def case(B: int, N: int, H: int, W: int, seed: int):
    """→ x, m, v [B,N,9], acc [B,N] float32, (log_lo, log_hi), split_log."""
    rng = np.random.default_rng(seed)
    x = np.ascontiguousarray(ga.clamp_genome(oracle.synthetic_population(B, N, H, W, seed=seed), H, W, MIN_S, MAX_S))
    x[..., 8] = rng.uniform(40.0, 255.0, (B, N)).astype(np.float32)
    acc = rng.uniform(0.05, 1.0, (B, N)).astype(np.float32)
    for b in range(B):
        p = rng.permutation(N)
        nd = max(N // 4, 4)
        dead = p[:nd]
        # dead alphas: two tied pairs (one at zero), the rest distinct
        x[b, dead, 8] = rng.uniform(0.0, ALPHA_DEAD * 0.99, nd).astype(np.float32)
        x[b, dead[0], 8] = x[b, dead[1], 8] = 0.0
        x[b, dead[2], 8] = x[b, dead[3], 8]
        live = p[nd:]
        x[b, live[0], 8] = ALPHA_DEAD                       # exactly at the threshold: alive
        x[b, live[1], 8] = np.nextafter(np.float32(ALPHA_DEAD), np.float32(0.0))   # one ulp below: dead
        acc[b, live[2]] = acc[b, live[3]] = acc[b, live[4]]                          # a three-way tie
        acc[b, live[5]] = np.float32(np.nan)                                          # never a source
        acc[b, live[6]] = np.float32(np.inf)                                          # the first source
        acc[b, live[7]], acc[b, live[8]] = np.float32(0.0), np.float32(-0.0)          # below any grad_min >= 0
        acc[b, live[9]] = acc[b, live[0]] = np.float32(2.0)                           # a tie at the top of the finite ones
        acc[b, dead[4 % nd]] = np.float32(50.0)                                       # a dead splat is never a source
    m = rng.normal(0, 1, x.shape).astype(np.float32)
    v = rng.uniform(0, 1, x.shape).astype(np.float32)
    lo, hi = ga.scale_log_bounds(H, W, MIN_S, MAX_S)
    split_log = float(np.median(np.maximum(x[..., 2], x[..., 3])))
    return x, m, v, acc, (float(lo), float(hi)), split_log


def params(split_log: float, max_moves: int, **kw) -> DensityParams:
    base = dict(every=1, start=0, stop=0, max_moves=max_moves, alpha_dead=ALPHA_DEAD, grad_min=0.02,
                split_log=split_log, shrink=1.6, split_offset=0.5)
    base.update(kw)
    return DensityParams(**base)
