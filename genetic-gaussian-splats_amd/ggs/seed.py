"""Seeding from the target: residual-driven placement.

Given a render and a target, ``cell_grid`` says where the error is and ``place_sites``
what the splats placed there look like; ``seed_genomes_host`` is the greedy
coarse-to-fine seeding built on them.  These three are the numpy statement of
ggs_seed_sites / ggs_seed_genomes (include/ggs.h): the device (``seed_sites``,
``seed_genomes``) is held to them bit for bit.  Float32 throughout, every operation
rounded once in the written order.

``seed_schedule`` supplies default rounds and ``seeded_population`` turns one seeded
genome into what the optimisers take as ``init_population``.  The schedule's values
(cells, shares, sigma = cell, alpha 255) are starting values: the best of one coarse sweep
on two synthetic targets (docs/EXPERIMENTS.md §32), not tuned beyond it.
"""
from __future__ import annotations

import math
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .ga import new_population, scale_log_bounds

_f32 = np.float32
CELLS = (2, 4, 8, 16, 32, 64)


class SeedParams(NamedTuple):
    """One placement (ggs_seed_params): cells of ``cell`` x ``cell`` pixels, at most
    ``max_sites`` sites per candidate among the cells whose error exceeds ``err_min``, each
    written as a round splat of log-scale ``log_sigma`` (the caller clips it to the scale
    bounds) and opacity ``alpha`` to rows ``first_row + j`` unless a row list is given."""
    cell: int = 16
    max_sites: int = 64
    first_row: int = 0
    err_min: float = 0.0
    log_sigma: float = 2.0
    alpha: float = 255.0


class SeedRound(NamedTuple):
    """One round of the greedy seeding (ggs_seed_round)."""
    cell: int
    count: int
    log_sigma: float
    alpha: float


def _input_error(msg: str):
    from . import _lib
    return _lib.GGSInputError(msg)


def _check_floats(what: str, **vals) -> None:
    for k, v in vals.items():
        if not math.isfinite(float(v)) or abs(float(v)) > float(np.finfo(np.float32).max):
            raise _input_error(f"{what}: {k}={v!r} must be finite")


def seed_params_c(params) -> "_lib.SeedParamsC":
    """ggs_seed_params of a ``SeedParams`` (or its six values in order); the parameter
    rules of ggs_seed_sites are checked here as well."""
    from . import _lib
    p = params if isinstance(params, SeedParams) else SeedParams(*params)
    for k in ("cell", "max_sites", "first_row"):
        v = getattr(p, k)
        if int(v) != v or abs(v) >= 2 ** 31:
            raise _input_error(f"seed: {k}={v!r} must be an integer")
    if int(p.cell) not in CELLS:
        raise _input_error(f"seed: cell={p.cell!r} must be one of {CELLS}")
    if p.max_sites < 1:
        raise _input_error(f"seed: max_sites={p.max_sites!r} must be >= 1")
    if p.first_row < 0:
        raise _input_error(f"seed: first_row={p.first_row!r} must be >= 0")
    _check_floats("seed", err_min=p.err_min, log_sigma=p.log_sigma, alpha=p.alpha)
    if p.err_min < 0.0:
        raise _input_error(f"seed: err_min={p.err_min!r} must be >= 0")
    if not 0.0 <= p.alpha <= 255.0:
        raise _input_error(f"seed: alpha={p.alpha!r} must be in [0, 255]")
    return _lib.SeedParamsC(int(p.cell), int(p.max_sites), int(p.first_row), float(p.err_min), float(p.log_sigma),
                            float(p.alpha))


def seed_rounds_c(rounds, N: int):
    """A ctypes array of ggs_seed_round from ``SeedRound``s, with ggs_seed_genomes's rules."""
    from . import _lib
    rs = [r if isinstance(r, SeedRound) else SeedRound(*r) for r in rounds]
    if not rs:
        raise _input_error("seed: at least one round is needed")
    for i, r in enumerate(rs):
        if int(r.cell) != r.cell or int(r.cell) not in CELLS:
            raise _input_error(f"seed: round {i}: cell={r.cell!r} must be one of {CELLS}")
        if int(r.count) != r.count or not 0 <= r.count < 2 ** 31:
            raise _input_error(f"seed: round {i}: count={r.count!r} must be an integer >= 0")
        _check_floats(f"seed: round {i}", log_sigma=r.log_sigma, alpha=r.alpha)
        if not 0.0 <= r.alpha <= 255.0:
            raise _input_error(f"seed: round {i}: alpha={r.alpha!r} must be in [0, 255]")
    if sum(int(r.count) for r in rs) != int(N):
        raise _input_error(f"seed: the rounds' counts sum to {sum(int(r.count) for r in rs)}, not N={N}")
    arr = (_lib.SeedRoundC * len(rs))(*[_lib.SeedRoundC(int(r.cell), int(r.count), float(r.log_sigma),
                                                         float(r.alpha)) for r in rs])
    return arr, rs


# ---- the numpy statement ------------------------------------------------------------

def _as_batch(image, targets, weights, group, background):
    """(img [B,H,W,3], tgt [B,H,W,3], w [B,H,W] or None), each candidate's own arrays."""
    tgt = np.asarray(targets, np.float32)
    if tgt.ndim == 3:
        tgt = tgt[None]
    if tgt.ndim != 4 or tgt.shape[3] != 3:
        raise _input_error(f"targets must be [K,H,W,3] or [H,W,3], got {tuple(tgt.shape)}")
    K, H, W, _ = tgt.shape
    if image is None:
        B = K * (1 if group is None else int(group))
        img = np.broadcast_to(np.asarray(background, np.float32).reshape(1, 1, 1, 3), (B, H, W, 3))
    else:
        img = np.asarray(image, np.float32)
        if img.ndim == 3:
            img = img[None]
        if img.ndim != 4 or img.shape[1:] != (H, W, 3):
            raise _input_error(f"image must be [B,H,W,3] with (H, W) = {(H, W)}, got {tuple(img.shape)}")
        B = img.shape[0]
    if group is None:
        group = max(B // K, 1)
    group = int(group)
    if group < 1 or B % group != 0 or B // group > K:
        raise _input_error(f"group={group}: needs group >= 1, B={B} a multiple of it and B / group <= K={K}")
    which = np.arange(B) // group
    w = None
    if weights is not None:
        w = np.asarray(weights, np.float32)
        if w.ndim == 2:
            w = w[None]
        if w.shape != (K, H, W):
            raise _input_error(f"weights must be [K,H,W] = {(K, H, W)}, got {tuple(w.shape)}")
        w = w[which]
    return img, tgt[which], w


def tree_sum(v: np.ndarray) -> np.ndarray:
    """The balanced tree over the last axis (a power of two long): adjacent pairs, then
    pairs of pairs, ...; what a lane xor-butterfly with strides 1, 2, 4, ... computes."""
    v = np.asarray(v, np.float32)
    while v.shape[-1] > 1:
        v = (v[..., 0::2] + v[..., 1::2]).astype(np.float32)
    return v[..., 0]


def _cell_sums(a: np.ndarray, c: int) -> np.ndarray:
    """[B,H,W] -> [B,Gy,Gx]: pixels past the image are +0.0, each of a cell's c columns is
    summed over y ascending from +0.0, the c column sums go through ``tree_sum``."""
    B, H, W = a.shape
    Gy, Gx = -(-H // c), -(-W // c)
    pad = np.zeros((B, Gy * c, Gx * c), np.float32)
    pad[:, :H, :W] = a
    pad = pad.reshape(B, Gy, c, Gx, c)
    col = np.zeros((B, Gy, Gx, c), np.float32)
    for i in range(c):
        col = (col + pad[:, :, i, :, :]).astype(np.float32)
    return tree_sum(col)


def pixel_residual(img: np.ndarray, tgt: np.ndarray, w: Optional[np.ndarray]) -> np.ndarray:
    """e = w ((dr dr + dg dg) + db db), d = img - target, float32 [B,H,W]."""
    d = (np.asarray(img, np.float32) - np.asarray(tgt, np.float32)).astype(np.float32)
    dr, dg, db = d[..., 0], d[..., 1], d[..., 2]
    e = ((dr * dr + dg * dg) + db * db).astype(np.float32)
    return e if w is None else (np.asarray(w, np.float32) * e).astype(np.float32)


def cell_grid(image, targets, cell: int, *, weights=None, group: Optional[int] = None,
              background=(1.0, 1.0, 1.0)) -> dict:
    """The cells of ``image`` [B,H,W,3] (None: the constant ``background``) against
    ``targets`` [K,H,W,3] (candidate b against image ``b // group``): ``err`` [B,G] the
    cell's summed residual, ``sums`` [B,G,3] its summed target colour, ``count`` [G] its
    in-image pixels and ``peak`` int32 [B,G,2] the (y, x) of its largest residual, ties to
    the smaller (y, x); G = ceil(H / cell) ceil(W / cell), cell index gy Gx + gx."""
    c = int(cell)
    if c not in CELLS:
        raise _input_error(f"seed: cell={cell!r} must be one of {CELLS}")
    img, tgt, w = _as_batch(image, targets, weights, group, background)
    B, H, W, _ = tgt.shape
    Gy, Gx = -(-H // c), -(-W // c)
    e = pixel_residual(img, tgt, w)
    err = _cell_sums(e, c).reshape(B, Gy * Gx)
    sums = np.stack([_cell_sums(np.ascontiguousarray(tgt[..., k]), c) for k in range(3)], -1).reshape(B, Gy * Gx, 3)
    ys = np.minimum(H, (np.arange(Gy) + 1) * c) - np.arange(Gy) * c
    xs = np.minimum(W, (np.arange(Gx) + 1) * c) - np.arange(Gx) * c
    count = (ys[:, None] * xs[None, :]).reshape(-1).astype(np.int32)
    # the peak: -inf past the image, the first largest in (y, x) order
    pad = np.full((B, Gy * c, Gx * c), -np.inf, np.float32)
    pad[:, :H, :W] = e
    flat = pad.reshape(B, Gy, c, Gx, c).transpose(0, 1, 3, 2, 4).reshape(B, Gy * Gx, c * c)
    k = np.argmax(flat, axis=2)                                  # first occurrence
    g = np.arange(Gy * Gx)
    peak = np.stack([(g // Gx)[None] * c + k // c, (g % Gx)[None] * c + k % c], -1).astype(np.int32)
    return {"err": err, "sums": sums, "count": count, "peak": peak, "Gy": Gy, "Gx": Gx}


def rank_sites(err: np.ndarray, err_min: float, max_sites: int) -> Tuple[np.ndarray, np.ndarray]:
    """``err`` [B,G] -> (sites int32 [B,M], n int32 [B]): the cells with err > err_min
    descending by err, ties to the lower cell, the first M of them; -1 past n."""
    err = np.asarray(err, np.float32)
    B, G = err.shape
    M = int(max_sites)
    sites = np.full((B, M), -1, np.int32)
    n = np.zeros((B,), np.int32)
    idx = np.arange(G)
    for b in range(B):
        el = idx[err[b] > _f32(err_min)]                         # False for a NaN
        el = el[np.lexsort((el, -err[b][el]))]
        n[b] = min(len(el), M)
        sites[b, :n[b]] = el[:n[b]]
    return sites, n


def place_sites(genomes, image, targets, params, *, weights=None, group: Optional[int] = None,
                background=(1.0, 1.0, 1.0), rows=None):
    """One placement (include/ggs.h, ggs_seed_params) → ``(genomes, sites, n, err)``:
    new [B,N,9] genomes (None in, None out: sites only) with the sites' rows written,
    ``sites`` int32 [B,M], ``n`` int32 [B] and the error grid [B,G].  ``rows`` int [B,M]
    names the row of every slot instead of ``first_row + j``."""
    p = params if isinstance(params, SeedParams) else SeedParams(*params)
    seed_params_c(p)
    cg = cell_grid(image, targets, p.cell, weights=weights, group=group, background=background)
    err = cg["err"]
    B = err.shape[0]
    H, W = np.asarray(targets).shape[-3:-1]
    sites, n = rank_sites(err, p.err_min, p.max_sites)
    if genomes is None:
        return None, sites, n, err
    x = np.array(genomes, np.float32)
    if x.ndim != 3 or x.shape[0] != B or x.shape[2] != 9:
        raise _input_error(f"genomes must be [B,N,9] with B = {B}, got {tuple(x.shape)}")
    N = x.shape[1]
    M = int(p.max_sites)
    if rows is None:
        if p.first_row + M > N:
            raise _input_error(f"seed: rows first_row={p.first_row} .. + max_sites={M} lie outside [0, N={N})")
        rows = np.broadcast_to(p.first_row + np.arange(M), (B, M))
    rows = np.asarray(rows)
    if rows.shape != (B, M) or rows.min() < 0 or rows.max() >= N:
        raise _input_error(f"seed: rows must be [B,M] = {(B, M)} with every row inside [0, N={N})")
    wm, hm = _f32(max(int(W) - 1, 1)), _f32(max(int(H) - 1, 1))
    for b in range(B):
        for j in range(int(n[b])):
            g = int(sites[b, j])
            py, px = cg["peak"][b, g]
            mean = cg["sums"][b, g] / _f32(cg["count"][g])
            x[b, rows[b, j]] = (_f32(px) / wm, _f32(py) / hm, _f32(p.log_sigma), _f32(p.log_sigma), _f32(0.0),
                                *np.clip(_f32(255.0) * mean, _f32(0.0), _f32(255.0)), _f32(p.alpha))
    return x, sites, n, err


def empty_genome(N: int, log_lo: float, K: Optional[int] = None) -> np.ndarray:
    """N empty rows (0.5, 0.5, log_lo, log_lo, 0, 0, 0, 0, 0), [N,9] or [K,N,9].  An empty
    row has alpha 0, so it blends as the identity: N of them render exactly the background."""
    g = np.zeros((int(N), 9), np.float32)
    g[:, 0:2] = _f32(0.5)
    g[:, 2:4] = _f32(log_lo)
    return g if K is None else np.repeat(g[None], int(K), axis=0)


def seed_schedule(N: int, H: int, W: int, *, min_scale_splats: float = 3.0, max_scale_splats: float = 0.1,
                  alpha: float = 255.0) -> List[SeedRound]:
    """A default coarse-to-fine schedule for N splats on an H x W canvas: up to four rounds
    whose cell halves each time, down to 4 pixels at the finest, starting from the largest
    cell that still leaves at least 2 x 2 cells; shares 1 : 2 : 4 : 8 of N, a round never
    asking for more sites than it has cells (what it gives up goes to the finer rounds, the
    last one takes what is left); sigma = cell clipped to the scale bounds.  The counts sum
    to N.  Untuned starting values (one coarse sweep chose sigma and alpha, docs/EXPERIMENTS.md §32)."""
    N, H, W = int(N), int(H), int(W)
    if N < 1 or H < 1 or W < 1:
        raise _input_error(f"seed_schedule: N={N}, H={H}, W={W} must be >= 1")
    lo, hi = scale_log_bounds(H, W, min_scale_splats, max_scale_splats)
    top = [c for c in CELLS if c >= 4 and 2 * c <= max(min(H, W), 8)]
    cells = sorted(top[-4:] if top else [4], reverse=True)
    shares = [2 ** i for i in range(len(cells))]
    out, left = [], N
    for i, c in enumerate(cells):
        if i == len(cells) - 1:
            cnt = left
        else:
            want = (left * shares[i]) // sum(shares[i:])
            cnt = min(want, -(-H // c) * -(-W // c))
        left -= cnt
        ls = float(np.clip(np.log(_f32(c)), lo, hi))
        out.append(SeedRound(c, int(cnt), ls, float(alpha)))
    return out


def seed_genomes_host(targets, N: int, rounds: Sequence, render: Callable[[np.ndarray], np.ndarray], *,
                      weights=None, err_min: float = 0.0, log_lo: float = 0.0, background=(1.0, 1.0, 1.0)):
    """The greedy seeding as a host loop → ``(genomes [K,N,9], placed int32 [R,K])``: from N
    empty rows, round r renders the genomes as they stand (``render``: [K,N,9] axes-angle
    genomes → [K,H,W,3]), places up to ``count`` sites against image k and writes them to
    the next ``count`` rows; a round with count 0 is skipped.  ``seed_genomes`` does the
    same on the device with the device's render."""
    tgt = np.asarray(targets, np.float32)
    if tgt.ndim == 3:
        tgt = tgt[None]
    K = tgt.shape[0]
    _, rs = seed_rounds_c(rounds, N)
    x = empty_genome(N, log_lo, K)
    placed = np.zeros((len(rs), K), np.int32)
    first = 0
    for r, rd in enumerate(rs):
        if rd.count == 0:
            continue
        img = np.asarray(render(x), np.float32)
        p = SeedParams(rd.cell, rd.count, first, err_min, rd.log_sigma, rd.alpha)
        x, _, n, _ = place_sites(x, img, tgt, p, weights=weights, group=1, background=background)
        placed[r] = n
        first += rd.count
    return x, placed


def seeded_population(P: int, genome, H: int, W: int, rng: np.random.Generator, *, keep: float = 0.5,
                      min_scale_splats: float = 3.0, max_scale_splats: float = 0.1) -> np.ndarray:
    """[P,N,9] from one seeded ``genome`` [N,9]: individual 0 is the genome; every other
    individual keeps a random subset of its rows (each row with probability ``keep``, drawn
    from ``rng``) and takes ``new_population`` rows, from the same ``rng``, for the rest.
    Host numpy; the result is what a search takes as ``init_population``."""
    g = np.asarray(genome, np.float32)
    if g.ndim != 2 or g.shape[1] != 9:
        raise _input_error(f"genome must be [N,9], got {tuple(g.shape)}")
    if int(P) < 1 or not 0.0 <= float(keep) <= 1.0:
        raise _input_error(f"seeded_population: P={P!r} must be >= 1 and keep={keep!r} in [0, 1]")
    N = g.shape[0]
    pop = np.empty((int(P), N, 9), np.float32)
    pop[0] = g
    if P > 1:
        pop[1:] = new_population(int(P) - 1, N, int(H), int(W), min_scale_splats, max_scale_splats, rng)
        kept = rng.random((int(P) - 1, N)) < float(keep)
        pop[1:][kept] = np.broadcast_to(g, (int(P) - 1, N, 9))[kept]
    return pop


# ---- the device ---------------------------------------------------------------------

def seed_sites(genomes, image, targets, params, *, weights=None, group: Optional[int] = None,
               background=(1.0, 1.0, 1.0), rows=None, device=None):
    """``place_sites`` by the device's cell, rank and apply kernels (ggs_seed_sites)."""
    from .api import seed_sites as _seed_sites
    return _seed_sites(genomes, image, targets, params, weights=weights, group=group, background=background,
                       rows=rows, device=device)


def seed_genomes(targets, N: int, rounds: Optional[Sequence] = None, *, weights=None, err_min: float = 0.0,
                 k_sigma: float = 3.0, background=(1.0, 1.0, 1.0), min_scale_splats: float = 3.0,
                 max_scale_splats: float = 0.1, device=None):
    """Greedy coarse-to-fine seeding of ``targets`` [K,H,W,3] ([H,W,3]: one image) on the
    device (ggs_seed_genomes) → ``(genomes [K,N,9], placed int32 [R,K])``; every round's
    render, placement and row writes are enqueued on one stream with one synchronisation at
    the end.  ``rounds``: ``SeedRound``s whose counts sum to N (None: ``seed_schedule``);
    ``weights`` [K,H,W]: the importance mask.  The empty rows' log-scale is the lower scale
    bound of ``min_scale_splats``."""
    import ctypes as C
    from . import _lib
    from .api import _background3, _fp, as_f32, device_index
    tgt = as_f32(targets)
    if tgt.ndim == 3:
        tgt = tgt[None]
    if tgt.ndim != 4 or tgt.shape[3] != 3:
        raise _input_error(f"targets must be [K,H,W,3] or [H,W,3], got {tuple(tgt.shape)}")
    K, H, W, _ = tgt.shape
    w = None
    if weights is not None:
        w = as_f32(weights)
        if w.ndim == 2:
            w = w[None]
        if w.shape != (K, H, W):
            raise _input_error(f"weights must be [K,H,W] = {(K, H, W)}, got {tuple(w.shape)}")
    if rounds is None:
        rounds = seed_schedule(N, H, W, min_scale_splats=min_scale_splats, max_scale_splats=max_scale_splats)
    arr, rs = seed_rounds_c(rounds, N)
    lo, _hi = scale_log_bounds(H, W, min_scale_splats, max_scale_splats)
    bg = _background3(background)
    out = np.empty((K, int(N), 9), np.float32)
    placed = np.zeros((len(rs), K), np.int32)
    # arguments are validated before the library looks for a device
    _lib.check(_lib.lib.ggs_seed_genomes(device_index(device), _fp(tgt), None if w is None else _fp(w), K, H, W,
                                         int(N), arr, len(rs), float(err_min), float(lo), float(k_sigma), _fp(bg),
                                         _fp(out), placed.ctypes.data_as(C.POINTER(C.c_int32))),
               "ggs_seed_genomes")
    return out, placed
