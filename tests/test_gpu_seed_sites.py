"""Residual-driven placement on an MI355X: the stage export ``api.seed_sites``
(ggs_seed_sites: the cell, rank and apply kernels on host arrays) against the numpy statement
``ggs.seed.place_sites``, bytewise for the rows, the sites, n and the error grid.  The shapes
are the smallest that reach every path of the cell kernel: partial cells on both axes, a
canvas one pixel wide, a whole wave per cell, 32 cells per wave, two waves per cell row.
``flat`` and ``none`` inputs are flat blocks of eighths, so cells and pixels tie exactly;
``noisy`` ones make every sum inexact, so the summation order shows.  ``max_sites`` is 1,
binding, and above the cell count."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import _seed_cases as cases
from ggs import api
from ggs.seed import SeedParams, place_sites

pytestmark = pytest.mark.gpu
MODES = ("flat_w", "noisy", "noisy_w", "none")
SITES = {"one": lambda G: 1, "binding": lambda G: max(1, min(G // 2, 7)), "above": lambda G: G + 5}
FIRST = 2


def _inputs(B, H, W, c, mode, K=None, group=1):
    K = B if K is None else K
    seed = 1000 * H + 10 * W + c
    tgt = cases.flat_blocks(K, H, W, 2 * c, seed)
    if mode == "none":
        img, w = None, None
    elif mode == "flat_w":
        img = cases.flat_blocks(B, H, W, 4 * c, seed + 1)
        w = cases.flat_blocks(K, H, W, 2 * c, seed + 2, channels=1)[..., 0]
    else:
        img = cases.noisy_image(B, H, W, seed + 3)
        w = cases.weights(K, H, W, seed + 4) if mode == "noisy_w" else None
    return img, tgt, w, group


@functools.lru_cache(maxsize=None)
def _reference(B, H, W, c, mode, which):
    """The inputs and the numpy statement's placement, made once and left unchanged."""
    img, tgt, w, group = _inputs(B, H, W, c, mode)
    G = -(-H // c) * -(-W // c)
    M = SITES[which](G)
    p = SeedParams(c, M, FIRST, 0.0, 1.25, 180.0)
    x = cases.genomes(B, M + FIRST + 1, 7)
    ref = place_sites(x, img, tgt, p, weights=w, group=group, background=(0.0, 0.0, 0.0))
    for a in (x, tgt, *ref) + tuple(a for a in (img, w) if a is not None):
        a.setflags(write=False)
    return (x, img, tgt, w, group, p), ref


def _device(inp, rows=slice(None)):
    x, img, tgt, w, group, p = inp
    # a candidate alone takes its own image, target and weights (group = 1: candidate b has target b)
    return api.seed_sites(x[rows], None if img is None else img[rows], tgt[rows], p,
                          weights=None if w is None else w[rows], group=group, background=(0.0, 0.0, 0.0))


@pytest.mark.parametrize("which", sorted(SITES))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,W,c", cases.SITE_SHAPES)
def test_the_stage_export_is_the_numpy_statement_bytewise(B, H, W, c, mode, which):
    inp, (rx, rsites, rn, rerr) = _reference(B, H, W, c, mode, which)
    G = rerr.shape[1]
    M = inp[5].max_sites
    elig = rerr > 0.0
    print(f"B={B} {H}x{W} c={c} {mode} M={M}: G={G}, eligible {elig.sum(1).tolist()}, n {rn.tolist()}")
    assert (rn >= 1).all() and (rn == np.minimum(elig.sum(1), M)).all()
    if which == "binding" and G >= 4:
        assert (rn == M).all() and (elig.sum(1) > M).all()          # max_sites binds
    if which == "above":
        assert (rn < M).all() and (rsites[:, -1] == -1).all()
    if mode in ("flat_w", "none") and G >= 16:
        # exact ties among the eligible cells of every candidate: the tie rule decides the order
        for b in range(B):
            assert len(np.unique(rerr[b][elig[b]])) < elig[b].sum(), b
    x2, sites, n, err = _device(inp)
    assert err.tobytes() == rerr.tobytes()
    assert n.tobytes() == rn.tobytes()
    assert sites.tobytes() == rsites.tobytes()
    assert x2.tobytes() == rx.tobytes()
    # a rerun, and every candidate alone against itself in the batch
    for a, b in zip(_device(inp), (x2, sites, n, err)):
        assert a.tobytes() == b.tobytes()
    for b in range(B):
        solo = _device(inp, slice(b, b + 1))
        for a, full in zip(solo, (x2, sites, n, err)):
            assert a[0].tobytes() == full[b].tobytes(), b


def test_group_picks_the_target_of_every_candidate():
    B, K, group, H, W, c = 4, 2, 2, 33, 47, 8
    for mode in ("noisy_w", "none"):
        img, tgt, w, _ = _inputs(B, H, W, c, mode, K=K, group=group)
        p = SeedParams(c, 5, 0, 0.0, 1.0, 255.0)
        x = cases.genomes(B, 6, 9)
        ref = place_sites(x, img, tgt, p, weights=w, group=group)
        got = api.seed_sites(x, img, tgt, p, weights=w, group=group)
        for a, r in zip(got, ref):
            assert a.tobytes() == r.tobytes()
        assert ref[3][0].tobytes() != ref[3][2].tobytes()            # the two targets give different grids
        if img is None:
            assert ref[3][0].tobytes() == ref[3][1].tobytes()        # ... and one target the same grid


def test_a_row_list_writes_the_same_sites_to_the_rows_it_names():
    B, H, W, c = 3, 33, 47, 8
    inp, (rx, rsites, rn, _) = _reference(B, H, W, c, "noisy_w", "binding")
    x, img, tgt, w, group, p = inp
    M, N = p.max_sites, x.shape[1]
    rows = np.stack([np.random.default_rng(b).permutation(N)[:M] for b in range(B)]).astype(np.int32)
    ref = place_sites(x, img, tgt, p, weights=w, group=group, background=(0.0, 0.0, 0.0), rows=rows)
    got = api.seed_sites(x, img, tgt, p, weights=w, group=group, background=(0.0, 0.0, 0.0), rows=rows)
    for a, r in zip(got, ref):
        assert a.tobytes() == r.tobytes()
    assert got[1].tobytes() == rsites.tobytes() and got[2].tobytes() == rn.tobytes()
    for b in range(B):
        assert got[0][b, rows[b]].tobytes() == rx[b, FIRST:FIRST + M].tobytes()
        rest = np.setdiff1d(np.arange(N), rows[b])
        assert got[0][b, rest].tobytes() == x[b, rest].tobytes()      # every other row keeps its bytes


def test_sites_only_and_a_perfect_render():
    B, H, W, c = 2, 33, 47, 8
    inp, (_, rsites, rn, rerr) = _reference(B, H, W, c, "noisy", "binding")
    x, img, tgt, w, group, p = inp
    none, sites, n, err = api.seed_sites(None, img, tgt[:B], p, group=group, background=(0.0, 0.0, 0.0))
    assert none is None and sites.tobytes() == rsites[:B].tobytes() and err.tobytes() == rerr[:B].tobytes()
    out, sites, n, err = api.seed_sites(x[:B], tgt[:B], tgt[:B], p)
    assert not n.any() and (sites == -1).all() and not err.any() and out.tobytes() == x[:B].tobytes()
    # err_min excludes what is at or below it: above the largest cell nothing is placed
    out, sites, n, _ = api.seed_sites(x[:B], img[:B], tgt[:B], p._replace(err_min=float(rerr.max())))
    assert not n.any() and out.tobytes() == x[:B].tobytes()
