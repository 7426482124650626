"""The density-control event on an MI355X: the stage export ``api.density_relocate``
(ggs_density_relocate: the session's rank and apply kernels on host arrays) against the
numpy statement ``ggs.refine.relocate``, bytewise for x, m, v, pairs, n_pairs and is_split.
N = 1100 crosses the 1,024 boundary and several 256-thread blocks; the accumulator carries
ties, +-0.0, NaN and inf, the alphas ties and values exactly at ``alpha_dead``, ``split_log``
is the median of max(log a, log b); ``max_moves`` is 1, binding, and larger than N."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from _density_cases import N_ACC, case, params
from ggs import api
from ggs.refine import density_moves, relocate

pytestmark = pytest.mark.gpu
SHAPES = [(3, 24, 33, 47), (2, 130, 64, 64), (2, 1100, 32, 32)]
MOVES = {"one": lambda N: 1, "binding": lambda N: 3, "above_n": lambda N: N + 7}


@functools.lru_cache(maxsize=None)
def _reference(B, N, H, W, which):
    """The inputs and the numpy statement's event, made once and left unchanged."""
    x, m, v, acc, (lo, hi), split_log = case(B, N, H, W, seed=100 + N)
    p = params(split_log, MOVES[which](N))
    ref = relocate(x, m, v, acc, N_ACC, H, W, p, lo, hi)
    for a in (x, m, v, acc, *ref):
        a.setflags(write=False)
    return (x, m, v, acc, lo, hi, p, H, W), ref


def _device(inp, rows=slice(None)):
    x, m, v, acc, lo, hi, p, H, W = inp
    return api.density_relocate(x[rows], m[rows], v[rows], acc[rows], N_ACC, H, W, p, lo, hi)



@pytest.mark.parametrize("which", sorted(MOVES))
@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_the_stage_export_is_the_numpy_statement_bytewise(B, N, H, W, which):
    inp, (rx, rm, rv, rpairs, rsplit) = _reference(B, N, H, W, which)
    M = density_moves(inp[6], N)
    assert M == min(MOVES[which](N), N // 2) and rpairs.shape == (B, M, 2)
    rn = (rpairs[:, :, 0] >= 0).sum(1).astype(np.int32)
    print(f"B={B} N={N} max_moves={which}: pairs per candidate {rn.tolist()}, splits {rsplit.sum(1).tolist()}")
    # the case moves something in every candidate and, unless one pair is all there is, both ways
    assert (rn >= 1).all() and (which == "one" or (rsplit.any() and (rsplit.sum() < rn.sum())))
    if which != "above_n":
        assert (rn == M).all()                               # max_moves binds
    x2, m2, v2, pairs, n_pairs, is_split = _device(inp)
    assert n_pairs.tobytes() == rn.tobytes()
    assert pairs.tobytes() == rpairs.tobytes()
    assert is_split.tobytes() == rsplit.tobytes()
    assert x2.tobytes() == rx.tobytes() and m2.tobytes() == rm.tobytes() and v2.tobytes() == rv.tobytes()
    # a rerun, and every candidate alone against itself in the batch
    again = _device(inp)
    for a, b in zip(again, (x2, m2, v2, pairs, n_pairs, is_split)):
        assert a.tobytes() == b.tobytes()
    for b in range(B):
        solo = _device(inp, slice(b, b + 1))
        for a, full in zip(solo, (x2, m2, v2, pairs, n_pairs, is_split)):
            assert a[0].tobytes() == full[b].tobytes(), b


def test_nothing_dead_or_no_source_moves_nothing():
    B, N, H, W = 2, 24, 33, 47
    (x, m, v, acc, lo, hi, p, _, _), _ = _reference(B, N, H, W, "binding")
    alive = x.copy()
    alive[..., 8] = 200.0
    for xx, aa in ((alive, acc), (x, np.full_like(acc, np.nan)), (x, np.zeros_like(acc))):
        x2, m2, v2, pairs, n_pairs, is_split = api.density_relocate(xx, m, v, aa, N_ACC, H, W, p, lo, hi)
        assert not n_pairs.any() and (pairs == -1).all() and not is_split.any()
        assert x2.tobytes() == xx.tobytes() and m2.tobytes() == m.tobytes() and v2.tobytes() == v.tobytes()
