"""The numpy statement of density control (ggs.refine.density_accumulate / relocate,
DESIGN.md §8g) on seeded inputs, N = 24 and 130, without a GPU: exp, sin and cos are the
oracle's restatement of csrc/ggs_detmath.h, handed in through ``detmath=``."""
from __future__ import annotations

import numpy as np
import pytest

from _density_cases import ALPHA_DEAD, N_ACC, ORACLE_DETMATH, case, params
from ggs.refine import DensityParams, density_accumulate, density_moves, relocate

_f32 = np.float32
SHAPES = [(3, 24, 33, 47), (2, 130, 64, 64)]


def _event(B, N, H, W, max_moves, **kw):
    x, m, v, acc, (lo, hi), split_log = case(B, N, H, W, seed=100 + N)
    p = params(split_log, max_moves, **kw)
    out = relocate(x, m, v, acc, N_ACC, H, W, p, lo, hi, detmath=ORACLE_DETMATH)
    return (x, m, v, acc, lo, hi, p), out


def _sets(x, acc, p):
    dead = x[:, 8] < _f32(p.alpha_dead)
    with np.errstate(invalid="ignore"):
        src = ~dead & (acc / _f32(N_ACC) > _f32(p.grad_min))
    return dead, src


@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_rows_sets_and_untouched_rows(B, N, H, W):
    (x, m, v, acc, lo, hi, p), (x2, m2, v2, pairs, is_split) = _event(B, N, H, W, N)
    M = density_moves(p, N)
    assert M == N // 2 and x2.shape == x.shape and pairs.shape == (B, M, 2) and is_split.shape == (B, M)
    n_clone = n_split = 0
    for b in range(B):
        dead, src = _sets(x[b], acc[b], p)
        assert not (dead & src).any()
        n = int((pairs[b, :, 0] >= 0).sum())
        assert n == min(dead.sum(), src.sum(), M) and n > 0
        assert (pairs[b, n:] == -1).all() and not is_split[b, n:].any()
        d, s = pairs[b, :n, 0], pairs[b, :n, 1]
        assert dead[d].all() and src[s].all()
        assert len(set(d) | set(s)) == 2 * n                     # the pairs touch disjoint rows
        # the dead list ascends by (alpha, index), the sources descend by acc with ties to the lower index
        ka = list(zip(x[b, d, 8].tolist(), d.tolist()))
        assert ka == sorted(ka)
        ks = list(zip((-acc[b, s]).tolist(), s.tolist()))
        assert ks == sorted(ks)
        # ... and they are the first n of the whole lists
        all_d = sorted(zip(x[b, dead, 8].tolist(), np.flatnonzero(dead).tolist()))
        all_s = sorted(zip((-acc[b, src]).tolist(), np.flatnonzero(src).tolist()))
        assert [i for _, i in all_d[:n]] == d.tolist() and [i for _, i in all_s[:n]] == s.tolist()
        assert not np.isnan(acc[b, s]).any() and np.isinf(acc[b, s[0]])
        touched = np.zeros(N, bool)
        touched[d] = True
        touched[s[is_split[b, :n] == 1]] = True
        for a, a2 in ((x, x2), (m, m2), (v, v2)):
            assert a2[b, ~touched].tobytes() == a[b, ~touched].tobytes()
        for j in range(n):
            if is_split[b, j]:
                n_split += 1
                assert max(x[b, s[j], 2], x[b, s[j], 3]) > _f32(p.split_log)
                assert not m2[b, s[j]].any() and not v2[b, s[j]].any()
            else:
                n_clone += 1
                assert max(x[b, s[j], 2], x[b, s[j], 3]) <= _f32(p.split_log)
                assert x2[b, d[j]].tobytes() == x[b, s[j]].tobytes()           # a bytewise copy
                assert x2[b, s[j]].tobytes() == x[b, s[j]].tobytes()
                assert m2[b, s[j]].tobytes() == m[b, s[j]].tobytes() and v2[b, s[j]].tobytes() == v[b, s[j]].tobytes()
            assert not m2[b, d[j]].any() and not v2[b, d[j]].any()
    assert n_clone >= 1 and n_split >= 1, (n_clone, n_split)


@pytest.mark.parametrize("B,N,H,W", SHAPES)
def test_split_halves_are_a_scalar_restatement_and_symmetric(B, N, H, W):
    import detmath
    (x, m, v, acc, lo, hi, p), (x2, _, _, pairs, is_split) = _event(B, N, H, W, N)
    wm, hm = _f32(max(W - 1, 1)), _f32(max(H - 1, 1))
    shrink = _f32(np.log(p.shrink))
    seen = unclipped = 0
    for b in range(B):
        for j in np.flatnonzero(is_split[b]):
            d, s = pairs[b, j]
            r = x[b, s]
            a_major = r[2] >= r[3]
            L = r[2] if a_major else r[3]
            sig = detmath.exp_f32(np.array([L], _f32))[0]
            sn, cs = (t[0] for t in detmath.sincos_f32(np.array([r[4]], _f32)))
            ux, uy = (cs, sn) if a_major else (-sn, cs)
            dlt = _f32(p.split_offset) * sig
            dx, dy = _f32(dlt * ux) / wm, _f32(dlt * uy) / hm
            for row, sg in ((s, 1), (d, -1)):
                want = r.copy()
                want[0] = np.clip(_f32(r[0] + dx) if sg > 0 else _f32(r[0] - dx), _f32(0), _f32(1))
                want[1] = np.clip(_f32(r[1] + dy) if sg > 0 else _f32(r[1] - dy), _f32(0), _f32(1))
                want[2] = np.clip(_f32(r[2] - shrink), _f32(lo), _f32(hi))
                want[3] = np.clip(_f32(r[3] - shrink), _f32(lo), _f32(hi))
                assert x2[b, row].tobytes() == want.tobytes(), (b, j, row)
            seen += 1
            xy = np.stack([x2[b, s, :2], x2[b, d, :2]]).astype(np.float64)
            if ((xy > 0) & (xy < 1)).all():
                # two roundings of at most half an ulp of 1.0 each, halved by the mean
                assert np.abs(xy.mean(0) - r[:2].astype(np.float64)).max() <= 2.0 ** -24
                unclipped += 1
    assert seen >= 1 and unclipped >= 1


def test_ties_go_to_the_lower_index_and_nan_is_never_a_source():
    N, H, W = 24, 33, 47
    x, m, v, acc, (lo, hi), split_log = case(1, N, H, W, seed=7)
    x, m, v, acc = x[0], m[0], v[0], acc[0]
    x[:, 8] = 200.0
    x[[5, 3, 11, 9], 8] = [1.0, 1.0, 0.0, -0.0]               # dead: 9 and 11 tie at zero, then 3 and 5
    acc[:] = 0.5
    acc[[20, 2, 7]] = [np.nan, 3.0, 3.0]                       # sources: 2, 7, then 0, 1, 4, ... at 0.5
    p = params(split_log, 4)
    _, _, _, pairs, _ = relocate(x, m, v, acc, N_ACC, H, W, p, lo, hi, detmath=ORACLE_DETMATH)
    assert pairs.tolist() == [[9, 2], [11, 7], [3, 0], [5, 1]]
    acc[:] = np.nan
    x2, m2, v2, pairs, is_split = relocate(x, m, v, acc, N_ACC, H, W, p, lo, hi, detmath=ORACLE_DETMATH)
    assert (pairs == -1).all() and x2.tobytes() == x.tobytes() and m2.tobytes() == m.tobytes()


def test_n_is_the_minimum_under_each_binding_term():
    N, H, W = 24, 33, 47
    x, m, v, acc, (lo, hi), split_log = case(1, N, H, W, seed=8)
    x[0, :, 8] = 200.0
    x[0, :5, 8] = 1.0                                          # five dead
    acc[0] = 1.0                                               # nineteen sources

    def n_moved(xx, aa, max_moves):
        out = relocate(xx, m, v, aa, N_ACC, H, W, params(split_log, max_moves), lo, hi, detmath=ORACLE_DETMATH)
        return int((out[3][0, :, 0] >= 0).sum())
    assert n_moved(x, acc, 12) == 5                            # the dead bind
    assert n_moved(x, acc, 3) == 3                             # max_moves binds
    few = np.zeros_like(acc)
    few[0, [10, 12]] = 1.0
    assert n_moved(x, few, 12) == 2                            # the sources bind
    assert n_moved(x, acc, 1000) == 5 and density_moves(params(split_log, 1000), N) == N // 2


def test_every_zero_is_the_identity():
    N, H, W = 24, 33, 47
    x, m, v, acc, (lo, hi), split_log = case(2, N, H, W, seed=9)
    p = params(split_log, 8, every=0)
    x2, m2, v2, pairs, is_split = relocate(x, m, v, acc, N_ACC, H, W, p, lo, hi, detmath=ORACLE_DETMATH)
    assert pairs.shape == (2, 0, 2) and is_split.shape == (2, 0)
    assert x2.tobytes() == x.tobytes() and m2.tobytes() == m.tobytes() and v2.tobytes() == v.tobytes()
    assert x2 is not x


def test_accumulate_is_the_scalar_loop():
    rng = np.random.default_rng(3)
    B, N, H, W = 2, 24, 33, 47
    g = (rng.normal(0, 1, (B, N, 9)) * 10.0 ** rng.integers(-6, 3, (B, N, 1))).astype(np.float32)
    acc = rng.uniform(0, 2, (B, N)).astype(np.float32)
    got = density_accumulate(acc, g, H, W)
    assert got.dtype == np.float32 and got is not acc
    for b in range(B):
        for s in range(N):
            px = _f32(g[b, s, 0] / _f32(W - 1))
            py = _f32(g[b, s, 1] / _f32(H - 1))
            n = _f32(np.sqrt(_f32(_f32(px * px) + _f32(py * py))))
            assert got[b, s].tobytes() == _f32(acc[b, s] + n).tobytes(), (b, s)
    # a one-pixel axis divides by one
    one = density_accumulate(np.zeros(1, _f32), np.array([[3.0, 4.0, 0, 0, 0, 0, 0, 0, 0]], _f32), 1, 1)
    assert one.tolist() == [5.0]


def test_defaults_are_off_only_when_every_is_zero():
    assert DensityParams().every > 0 and DensityParams().shrink == 1.6
    assert density_moves(DensityParams(every=0), 24) == 0
    assert ALPHA_DEAD == 16.0
