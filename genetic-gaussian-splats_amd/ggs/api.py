"""Host side of the hot path: numpy in, numpy out, libggs.so (HIP, gfx950) underneath.

Mirrors the reference operator interface (modules/render.py, modules/fitness.py,
modules/encode.py) with plain Python + numpy; torch tensors are accepted by duck
typing (``.detach().cpu().numpy()``) so the reference's own callers work
unchanged.  Every compute call goes through ctypes into libggs.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import GGSInputError, check, lib

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)


def as_f32(x) -> np.ndarray:
    """float32, C-contiguous host array from numpy / lists / torch tensors."""
    if hasattr(x, "detach") and hasattr(x, "cpu"):          # torch.Tensor (duck-typed)
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_f32p)


def _genomes3d(genomes, what: str) -> np.ndarray:
    g = as_f32(genomes)
    if g.ndim not in (2, 3):                                  # render.py:219
        raise GGSInputError(f"genomes must be [B,N,9] or [N,9], got {tuple(g.shape)}")
    if g.ndim == 2:                                           # render.py:220-221
        g = g[None]
    if g.shape[2] < 9:                                        # render.py:223
        raise GGSInputError(f"expected at least 9 genome cols, got {g.shape[2]} ({what})")
    return g


def device_index(device=None) -> int:
    """The HIP device a reference-style ``device`` argument names (render.py:215-217
    resolves ``device or 'cuda'`` the same way): an explicit index ('cuda:k',
    torch.device('cuda', k), k) wins; without one, LOCAL_RANK under a launcher
    (one process per GPU), else device 0.  Never "every GPU"."""
    idx = None
    if isinstance(device, int):
        idx = device
    elif isinstance(device, str):
        parts = device.split(":")
        if len(parts) == 2 and parts[1].strip().isdigit():
            idx = int(parts[1])
    elif device is not None:                                   # torch.device (duck-typed)
        idx = getattr(device, "index", None)
    if idx is None:
        idx = int(os.environ.get("LOCAL_RANK", "0") or 0)
    return int(idx)


@contextlib.contextmanager
def _on_devices(device, n_devices: int):
    """Point the host API at the devices of one call and yield the n_devices
    argument for the C layer; the selection and the call happen under one lock
    (another thread, or a direct ``ggs.select_devices``, cannot change the
    library's device list in between).  n_devices == 1 (default): the single
    device ``device`` names; n_devices > 1: fan the batch out over the first
    n_devices GPUs (opt-in; one RCCL gather returns the scalars); n_devices <= 0:
    all GPUs.

    The lock is process-wide and held for the whole C call, so the host API
    (render / fitness / encode / preprocess) is serialised across Python threads:
    concurrent host-API calls run one after another (the library's per-device
    pipeline is one stream anyway).  Threads that want concurrent GPU work use the
    device-pointer API (``fitness_device`` / ``TargetPlan`` on their own HIP
    streams), which takes no such lock."""
    n = _lib.ensure_init()
    if n_devices == 1:
        ids = (device_index(device),)
        if not 0 <= ids[0] < n:
            raise _lib.GGSDeviceError(f"device {device!r} -> HIP device {ids[0]}, but {n} visible")
    else:
        ids = tuple(range(n if n_devices <= 0 else min(int(n_devices), n)))
    with _lib.device_lock:
        if _lib.selected[0] != ids:
            _lib.select_devices(list(ids))
        yield len(ids)


_LAYOUTS = {"renderer": _lib.GGS_LAYOUT_RENDERER, "axes": _lib.GGS_LAYOUT_AXES}


def layout_id(layout) -> int:
    """GGS_LAYOUT_* of a layout name ("renderer" / "axes") or of the constant itself."""
    if isinstance(layout, str) and layout in _LAYOUTS:
        return _LAYOUTS[layout]
    if not isinstance(layout, (str, bool)) and layout in _LAYOUTS.values():
        return int(layout)
    raise GGSInputError(f"layout must be 'renderer' or 'axes', got {layout!r}")


def render(genomes, H: int, W: int, *, k_sigma: float = 3.0,
           background=(1.0, 1.0, 1.0), device=None, n_devices: int = 1,
           fp16_canvas: bool = False, layout="renderer") -> np.ndarray:
    """render.py:203-252 → float32 [B,H,W,3] in [0,1] (renderer-layout genomes;
    ``layout="axes"``: axes-angle genomes, the render of ``encode(genomes)``).

    ``fp16_canvas`` (render.py:213 ``use_fp16_canvas``): the reference's canvas is
    then float16 — the background is stored in half precision, the Triton kernel
    blends in fp32 registers and stores each pixel once as float16 (round to
    nearest even), then clamps and converts back (render.py:234-237, :252).
    Here: background rounded to half, fp32 render, result rounded to half."""
    g = _genomes3d(genomes, "render")
    if layout_id(layout) == _lib.GGS_LAYOUT_AXES:
        g = encode(g)
    B, N, Cc = g.shape
    H, W = int(H), int(W)
    out = np.empty((B, H, W, 3), np.float32)
    bg = np.ascontiguousarray(np.broadcast_to(np.asarray(background, np.float32), (3,)))
    if fp16_canvas:
        bg = bg.astype(np.float16).astype(np.float32)
    with _on_devices(device, n_devices) as nd:
        check(lib.ggs_render(_fp(g), B, N, Cc, H, W, float(k_sigma), _fp(bg), _fp(out), nd),
              "ggs_render")
    if fp16_canvas:
        out = out.astype(np.float16).astype(np.float32)
    return out


def fitness(genomes_axes, target, H: int, W: int, k_sigma: float = 3.0,
            weight_mask=None, boost_only: bool = False, boost_beta: float = 1.0,
            device=None, n_devices: int = 1) -> np.ndarray:
    """fitness.py:7-31 on a stacked [B,N,C] axes-angle batch → float32 [B]
    (on the GPU ``device`` names; ``n_devices`` > 1 opts into the multi-GPU
    fan-out, see ``_on_devices``)."""
    g = _genomes3d(genomes_axes, "fitness")
    B, N, Cc = g.shape
    H, W = int(H), int(W)
    tgt = as_f32(target)
    if tgt.shape != (H, W, 3):
        raise GGSInputError(f"target must be [H,W,3] = {(H, W, 3)}, got {tuple(tgt.shape)}")
    if weight_mask is None:
        mode, mask_p = _lib.GGS_FIT_NONE, None
    else:
        mask = as_f32(weight_mask)
        if mask.shape != (H, W):
            raise GGSInputError(f"weight_mask must be [H,W] = {(H, W)}, got {tuple(mask.shape)}")
        mode = _lib.GGS_FIT_BOOST if boost_only else _lib.GGS_FIT_WEIGHTED
        mask_p = _fp(mask)
    out = np.empty((B,), np.float32)
    with _on_devices(device, n_devices) as nd:
        check(lib.ggs_fitness(_fp(g), B, N, Cc, _fp(tgt), mask_p, mode, float(boost_beta), H, W,
                              float(k_sigma), _fp(out), nd), "ggs_fitness")
    return out


def fitness_grad(genomes_axes, target, H: int, W: int, k_sigma: float = 3.0,
                 weight_mask=None, boost_only: bool = False, boost_beta: float = 1.0,
                 device=None, group: Optional[int] = None):
    """``fitness`` and its gradient with respect to the nine axes-angle genes of
    every splat → (fit float32 [B], grad float32 [B,N,9]); DESIGN.md §8c has the
    conventions.  ``fit`` has the bits ``fitness`` returns.  One device.

    A 4-D ``target`` [K,H,W,3] (``weight_mask`` [K,H,W] or None) differentiates
    candidate b against image ``b // group`` in one launch chain (DESIGN.md §8d;
    ``group`` defaults to B // K); a candidate's bits are those of the call against
    that image alone."""
    g = _genomes3d(genomes_axes, "fitness_grad")
    B, N, Cc = g.shape
    H, W = int(H), int(W)
    tgt = as_f32(target)
    many = tgt.ndim == 4
    if many:
        K = tgt.shape[0]
        if tgt.shape != (K, H, W, 3):
            raise GGSInputError(f"targets must be [K,H,W,3] = {(K, H, W, 3)}, got {tuple(tgt.shape)}")
        if group is None:
            group = max(B // max(K, 1), 1)
        mshape = (K, H, W)
    else:
        if group is not None:
            raise GGSInputError("group= needs a 4-D target [K,H,W,3]")
        if tgt.shape != (H, W, 3):
            raise GGSInputError(f"target must be [H,W,3] = {(H, W, 3)}, got {tuple(tgt.shape)}")
        mshape = (H, W)
    if weight_mask is None:
        mode, mask_p = _lib.GGS_FIT_NONE, None
    else:
        mask = as_f32(weight_mask)
        if mask.shape != mshape:
            raise GGSInputError(f"weight_mask must be {mshape}, got {tuple(mask.shape)}")
        mode = _lib.GGS_FIT_BOOST if boost_only else _lib.GGS_FIT_WEIGHTED
        mask_p = _fp(mask)
    out = np.empty((B,), np.float32)
    grad = np.empty((B, N, 9), np.float32)
    with _on_devices(device, 1):
        if many:
            check(lib.ggs_fitness_grad_targets(_fp(g), B, N, Cc, _fp(tgt), mask_p, K, int(group), mode,
                                               float(boost_beta), H, W, float(k_sigma), _fp(out), _fp(grad)),
                  "ggs_fitness_grad_targets")
        else:
            check(lib.ggs_fitness_grad(_fp(g), B, N, Cc, _fp(tgt), mask_p, mode, float(boost_beta), H, W,
                                       float(k_sigma), _fp(out), _fp(grad)), "ggs_fitness_grad")
    return out, grad


def _background3(background) -> np.ndarray:
    return np.ascontiguousarray(np.broadcast_to(np.asarray(background, np.float32), (3,)))


def render_vjp(genomes, cot, H: int, W: int, *, k_sigma: float = 3.0, background=(1.0, 1.0, 1.0),
               layout="renderer", device=None) -> np.ndarray:
    """The renderer's vector-Jacobian product → float32 [B,N,9]:
    ``sum(cot * d render(genomes) / d genomes[b,s,0:9])`` for a cotangent ``cot``
    [B,H,W,3] ([H,W,3] for [N,C] genomes), i.e. the gradient of any loss of the
    image whose ``d loss / d image`` is ``cot``.  ``layout`` names what the rows
    are ("renderer": ``render``'s input; "axes": axes-angle rows, encoded first).
    DESIGN.md §8e has the conventions (those of ``fitness_grad``).  One device."""
    g = _genomes3d(genomes, "render_vjp")
    B, N, Cc = g.shape
    H, W = int(H), int(W)
    lay = layout_id(layout)
    v = as_f32(cot)
    if v.ndim == 3 and B == 1:
        v = v[None]
    if v.shape != (B, H, W, 3):
        raise GGSInputError(f"cot must be [B,H,W,3] = {(B, H, W, 3)}, got {tuple(v.shape)}")
    bg = _background3(background)
    grad = np.empty((B, N, 9), np.float32)
    n = _lib.ensure_init()
    dev = device_index(device)
    if not 0 <= dev < n:
        raise _lib.GGSDeviceError(f"device {device!r} -> HIP device {dev}, but {n} visible")
    check(lib.ggs_render_vjp(_fp(g), B, N, Cc, lay, H, W, float(k_sigma), _fp(bg), _fp(v), _fp(grad), dev),
          "ggs_render_vjp")
    return grad


class LossParams(NamedTuple):
    """Weights of the image loss ``l1 * mean|x - y| + mse * mean (x - y)^2 + ssim * (1 - mean
    SSIM(x, y))``; the default is the 3DGS / GaussianImage loss, lambda 0.2."""
    l1: float = 0.8
    mse: float = 0.0
    ssim: float = 0.2


def loss_params_c(params) -> "_lib.LossParamsC":
    """ggs_loss_params of a ``LossParams`` (or any three weights l1, mse, ssim; None: the default)."""
    p = LossParams() if params is None else LossParams(*params)
    return _lib.LossParamsC(float(p.l1), float(p.mse), float(p.ssim))


def _targets4d(targets, B: int, H: int, W: int, group: Optional[int]):
    """[K,H,W,3] float32 targets ([H,W,3]: one image for every candidate) and the group."""
    tgt = as_f32(targets)
    if tgt.ndim == 3:
        if group is not None:
            raise GGSInputError("group= needs 4-D targets [K,H,W,3]")
        tgt, group = tgt[None], B
    K = tgt.shape[0]
    if tgt.ndim != 4 or tgt.shape != (K, H, W, 3):
        raise GGSInputError(f"targets must be [K,H,W,3] or [H,W,3] with (H, W) = {(H, W)}, got {tuple(tgt.shape)}")
    if group is None:
        group = max(B // max(K, 1), 1)
    return tgt, K, int(group)


def image_loss(img, targets, params=None, *, group: Optional[int] = None, cot: bool = True, device=None):
    """The image loss of ``img`` [B,H,W,3] ([H,W,3]: one image) against ``targets`` [K,H,W,3]
    (image b against target ``b // group``, ``group`` defaults to B // K) or [H,W,3] (one
    target for all) → (loss float32 [B], cot float32 [B,H,W,3] = d loss / d img), or the loss
    alone with ``cot=False`` (the same bits).  DESIGN.md §8f has the definition; float64
    between the float32 inputs and outputs.  One device."""
    x = as_f32(img)
    if x.ndim == 3:
        x = x[None]
    if x.ndim != 4 or x.shape[3] != 3:
        raise GGSInputError(f"img must be [B,H,W,3] or [H,W,3], got {tuple(x.shape)}")
    B, H, W, _ = x.shape
    tgt, K, group = _targets4d(targets, B, H, W, group)
    prm = loss_params_c(params)
    loss = np.empty((B,), np.float32)
    v = np.empty((B, H, W, 3), np.float32) if cot else None
    # arguments are validated before the library looks for a device
    check(lib.ggs_image_loss(_fp(x), B, _fp(tgt), K, group, H, W, C.byref(prm), _fp(loss),
                             None if v is None else _fp(v), device_index(device)), "ggs_image_loss")
    return (loss, v) if cot else loss


def loss_grad(genomes, targets, H: int, W: int, params=None, *, k_sigma: float = 3.0,
              background=(1.0, 1.0, 1.0), layout="axes", group: Optional[int] = None, device=None):
    """The image loss of the render of ``genomes`` [B,N,C] ([N,C]) and its gradient with
    respect to the nine genes of every splat → (loss float32 [B], grad float32 [B,N,9]):
    ``render`` → ``image_loss`` → ``render_vjp`` in one call, with their bits.  ``targets``
    and ``group`` as ``image_loss``; ``layout`` as ``render_vjp`` (default: axes-angle
    genomes, what the optimisers keep).  One device."""
    g = _genomes3d(genomes, "loss_grad")
    B, N, Cc = g.shape
    H, W = int(H), int(W)
    lay = layout_id(layout)
    tgt, K, group = _targets4d(targets, B, H, W, group)
    prm = loss_params_c(params)
    bg = _background3(background)
    loss = np.empty((B,), np.float32)
    grad = np.empty((B, N, 9), np.float32)
    check(lib.ggs_loss_grad(_fp(g), B, N, Cc, lay, _fp(tgt), K, group, H, W, float(k_sigma), _fp(bg),
                            C.byref(prm), _fp(loss), _fp(grad), device_index(device)), "ggs_loss_grad")
    return loss, grad


def density_relocate(x, m, v, acc, n_acc: int, H: int, W: int, params, log_lo: float, log_hi: float, *,
                     device=None):
    """ggs_density_relocate, a stage export: one density-control event by
    the refine session's own rank and apply kernels on host arrays ``x``, ``m``, ``v``
    [B,N,9] and ``acc`` [B,N] → ``(x, m, v, pairs, n_pairs, is_split)``, new arrays;
    ``ggs.refine.relocate`` states the same event in numpy.  One device."""
    from .refine import density_moves, density_params_c
    prm = density_params_c(params)
    xs = [as_f32(a) for a in (x, m, v)]
    if xs[0].ndim != 3 or xs[0].shape[2] != 9 or any(a.shape != xs[0].shape for a in xs):
        raise GGSInputError(f"x, m, v must be [B,N,9] alike, got {[tuple(a.shape) for a in xs]}")
    B, N, _ = xs[0].shape
    a = as_f32(acc)
    if a.shape != (B, N):
        raise GGSInputError(f"acc must be [B,N] = {(B, N)}, got {tuple(a.shape)}")
    M = density_moves(prm, N)
    outs = [np.empty_like(b) for b in xs]
    pairs, is_split = np.full((B, M, 2), -1, np.int32), np.zeros((B, M), np.int32)
    n_pairs = np.zeros((B,), np.int32)
    ip = lambda b: b.ctypes.data_as(_i32p)  # noqa: E731
    # arguments are validated before the library looks for a device
    check(lib.ggs_density_relocate(device_index(device), _fp(xs[0]), _fp(xs[1]), _fp(xs[2]), _fp(a), int(n_acc), B,
                                   N, int(H), int(W), float(log_lo), float(log_hi), C.byref(prm), _fp(outs[0]),
                                   _fp(outs[1]), _fp(outs[2]), ip(pairs), ip(n_pairs), ip(is_split)),
          "ggs_density_relocate")
    return outs[0], outs[1], outs[2], pairs, n_pairs, is_split


def seed_sites(genomes, image, targets, params, *, weights=None, group: Optional[int] = None,
               background=(1.0, 1.0, 1.0), rows=None, device=None):
    """ggs_seed_sites, a stage export: one residual-driven placement by the
    cell, rank and apply kernels on host arrays → ``(genomes, sites, n, err)``, new arrays:
    ``genomes`` [B,N,9] with the sites' rows written (None in, None out: sites only),
    ``sites`` int32 [B,M], ``n`` int32 [B], ``err`` [B, Gy Gx].  ``image`` [B,H,W,3] or None
    (the constant ``background``; B is then K ``group``), ``targets`` [K,H,W,3] ([H,W,3]),
    ``weights`` [K,H,W] or None, ``rows`` int [B,M] or None (``first_row + j``);
    ``ggs.seed.place_sites`` states the same call in numpy.  One device."""
    from .seed import seed_params_c
    prm = seed_params_c(params)
    tgt = as_f32(targets)
    if tgt.ndim == 3:
        tgt = tgt[None]
    if tgt.ndim != 4 or tgt.shape[3] != 3:
        raise GGSInputError(f"targets must be [K,H,W,3] or [H,W,3], got {tuple(tgt.shape)}")
    K, H, W, _ = tgt.shape
    img = None
    if image is not None:
        img = as_f32(image)
        if img.ndim == 3:
            img = img[None]
        if img.ndim != 4 or img.shape[1:] != (H, W, 3):
            raise GGSInputError(f"image must be [B,H,W,3] with (H, W) = {(H, W)}, got {tuple(img.shape)}")
    B = img.shape[0] if img is not None else K * (1 if group is None else int(group))
    if group is None:
        group = max(B // K, 1)
    w = None
    if weights is not None:
        w = as_f32(weights)
        if w.ndim == 2:
            w = w[None]
        if w.shape != (K, H, W):
            raise GGSInputError(f"weights must be [K,H,W] = {(K, H, W)}, got {tuple(w.shape)}")
    x = out = None
    N = 0
    if genomes is not None:
        x = as_f32(genomes)
        if x.ndim != 3 or x.shape[0] != B or x.shape[2] != 9:
            raise GGSInputError(f"genomes must be [B,N,9] with B = {B}, got {tuple(x.shape)}")
        N = x.shape[1]
        out = np.empty_like(x)
    M = int(prm.max_sites)
    r = None
    if rows is not None:
        r = np.ascontiguousarray(rows, np.int32)
        if r.shape != (B, M):
            raise GGSInputError(f"rows must be [B,M] = {(B, M)}, got {tuple(r.shape)}")
    c = int(prm.cell)
    sites = np.full((B, M), -1, np.int32)
    n = np.zeros((B,), np.int32)
    err = np.empty((B, -(-H // c) * -(-W // c)), np.float32)
    bg = _background3(background)
    ip = lambda b: b.ctypes.data_as(_i32p)  # noqa: E731
    # arguments are validated before the library looks for a device
    check(lib.ggs_seed_sites(device_index(device), None if img is None else _fp(img), _fp(bg), _fp(tgt),
                             None if w is None else _fp(w), B, K, int(group), H, W, C.byref(prm),
                             None if r is None else ip(r), None if x is None else _fp(x), N,
                             None if out is None else _fp(out), ip(sites), ip(n), _fp(err)), "ggs_seed_sites")
    return out, sites, n, err


def encode(G_axes) -> np.ndarray:
    """encode.py:62-79 genome_to_renderer_batched (any leading shape, C ≥ 9) → [..., 9]."""
    g = as_f32(G_axes)
    if g.ndim == 1:
        g = g[None]
    if g.shape[-1] < 9:
        raise GGSInputError(f"expected at least 9 genome cols, got {g.shape[-1]}")
    lead = g.shape[:-1]
    flat = np.ascontiguousarray(g.reshape(-1, g.shape[-1]))
    out = np.empty((flat.shape[0], 9), np.float32)
    with _on_devices(None, 1):
        check(lib.ggs_encode(_fp(flat), flat.shape[0], flat.shape[1], _fp(out)), "ggs_encode")
    return out.reshape(*lead, 9)


def preprocess(genome, H: int, W: int, k_sigma: float = 3.0) -> Dict[str, np.ndarray]:
    """render.py:8-47 _preprocess_genome → dict of the 13 per-splat arrays."""
    g = as_f32(genome)
    if g.ndim == 1:
        g = g[None]
    g = np.ascontiguousarray(g.reshape(-1, g.shape[-1]))
    S = g.shape[0]
    f9 = np.empty((9, S), np.float32)
    i4 = np.empty((4, S), np.int32)
    with _on_devices(None, 1):
        check(lib.ggs_preprocess(_fp(g), S, g.shape[1], int(H), int(W), float(k_sigma), _fp(f9),
                                 i4.ctypes.data_as(_i32p)), "ggs_preprocess")
    keys = ("cx", "cy", "sxx", "sxy", "syy", "rc", "gc", "bc", "a")
    out = {k: f9[i] for i, k in enumerate(keys)}
    out.update({k: i4[i] for i, k in enumerate(("x0", "x1", "y0", "y1"))})
    return out


def fitness_population(population: Sequence, target, H: int, W: int, k_sigma: float = 3.0,
                       chunk: Optional[int] = None, weight_mask=None,
                       boost_only: bool = False, device=None, n_devices: int = 1) -> List[float]:
    """fitness.py:34-47 → List[float]; chunking only bounds the batch size."""
    if len(population) == 0:
        return []
    G = np.stack([as_f32(p) for p in population], 0)
    if chunk is None or chunk >= len(population):
        return fitness(G, target, H, W, k_sigma, weight_mask, boost_only,
                       device=device, n_devices=n_devices).tolist()
    out: List[float] = []
    for i in range(0, len(population), int(chunk)):
        out.extend(fitness(G[i:i + chunk], target, H, W, k_sigma, weight_mask, boost_only,
                           device=device, n_devices=n_devices).tolist())
    return out


# ---- device-pointer entry points (inputs resident in HBM) ----------------------
def fitness_device(device: int, stream: int, d_genomes: int, B: int, N: int, Cc: int,
                   d_target: int, d_mask: int, mode: int, boost_beta: float, H: int, W: int,
                   k_sigma: float, d_out: int) -> None:
    """Enqueue the fused fitness pipeline on `stream` over device pointers."""
    check(lib.ggs_fitness_device(device, C.c_void_p(stream), C.c_void_p(d_genomes), B, N, Cc,
                                 C.c_void_p(d_target), C.c_void_p(d_mask or None), mode,
                                 float(boost_beta), H, W, float(k_sigma), C.c_void_p(d_out)),
          "ggs_fitness_device")


def fitness_grad_device(device: int, stream: int, d_genomes: int, B: int, N: int, Cc: int,
                        d_target: int, d_mask: int, mode: int, boost_beta: float, H: int, W: int,
                        k_sigma: float, d_out: int, d_grad: int) -> None:
    """Enqueue fitness (d_out [B], may be 0) and gradient (d_grad [B,N,9]) on `stream`."""
    check(lib.ggs_fitness_grad_device(device, C.c_void_p(stream), C.c_void_p(d_genomes), B, N, Cc,
                                      C.c_void_p(d_target), C.c_void_p(d_mask or None), mode,
                                      float(boost_beta), H, W, float(k_sigma), C.c_void_p(d_out or None),
                                      C.c_void_p(d_grad)), "ggs_fitness_grad_device")


class TargetPlan:
    """A target/mask prepared once for ``ggs_fitness_device_planned`` (the GA's
    fixed target over a run).  Pointers are device pointers on ``device``; the
    plan is built on ``stream``."""

    def __init__(self, device: int, stream: int, d_target: int, d_mask: int, mode: int,
                 boost_beta: float, H: int, W: int):
        h = C.c_void_p()
        check(lib.ggs_plan_create(device, C.c_void_p(stream), C.c_void_p(d_target),
                                  C.c_void_p(d_mask or None), mode, float(boost_beta), H, W,
                                  C.byref(h)), "ggs_plan_create")
        self.h, self.H, self.W = h, H, W

    def fitness_device(self, stream: int, d_genomes: int, B: int, N: int, Cc: int,
                       k_sigma: float, d_out: int) -> None:
        check(lib.ggs_fitness_device_planned(self.h, C.c_void_p(stream), C.c_void_p(d_genomes), B,
                                             N, Cc, float(k_sigma), C.c_void_p(d_out)),
              "ggs_fitness_device_planned")

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


class TargetPlanSet:
    """K targets/masks of one (H, W, mode, beta) prepared once (``ggs_planset_*``):
    ``d_targets`` [K, H, W, 3] and ``d_masks`` [K, H, W] (0 for mode 0) are device
    pointers on ``device``.  ``fitness_device`` scores candidate b against plan
    ``b // group`` in one launch sequence: a folder of images, the frames of a clip
    or the tiles of a picture evaluated as one batch."""

    def __init__(self, device: int, stream: int, d_targets: int, d_masks: int, mode: int,
                 boost_beta: float, H: int, W: int, K: int):
        h = C.c_void_p()
        check(lib.ggs_planset_create(device, C.c_void_p(stream), C.c_void_p(d_targets or None),
                                     C.c_void_p(d_masks or None), mode, float(boost_beta), H, W, K,
                                     C.byref(h)), "ggs_planset_create")
        self.h, self.H, self.W, self.K = h, H, W, K

    def fitness_device(self, stream: int, d_genomes: int, B: int, N: int, Cc: int, group: int,
                       k_sigma: float, d_out: int) -> None:
        check(lib.ggs_fitness_device_planset(self.h, C.c_void_p(stream), C.c_void_p(d_genomes or None), B,
                                             N, Cc, group, float(k_sigma), C.c_void_p(d_out or None)),
              "ggs_fitness_device_planset")

    def fitness_grad(self, stream: int, d_genomes: int, B: int, N: int, Cc: int, group: int, d_targets: int,
                     d_masks: int, k_sigma: float, d_out: int, d_grad: int) -> None:
        """Enqueue fitness (d_out [B], may be 0) and gradient (d_grad [B,N,9]) of candidate
        b against plan ``b // group``.  ``d_targets`` / ``d_masks``: the arrays the set was
        created from (the set keeps the pixels only in the raster's lane order)."""
        check(lib.ggs_fitness_grad_device_planset(self.h, C.c_void_p(stream), C.c_void_p(d_genomes or None), B, N,
                                                  Cc, group, C.c_void_p(d_targets or None),
                                                  C.c_void_p(d_masks or None), float(k_sigma),
                                                  C.c_void_p(d_out or None), C.c_void_p(d_grad or None)),
              "ggs_fitness_grad_device_planset")

    def close(self) -> None:
        if getattr(self, "h", None):
            lib.ggs_planset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 — interpreter shutdown
            pass


def render_device(device: int, stream: int, d_genomes: int, B: int, N: int, Cc: int, H: int,
                  W: int, k_sigma: float, d_out: int, background=(1.0, 1.0, 1.0)) -> None:
    bg = np.ascontiguousarray(np.broadcast_to(np.asarray(background, np.float32), (3,)))
    check(lib.ggs_render_device(device, C.c_void_p(stream), C.c_void_p(d_genomes), B, N, Cc, H,
                                W, float(k_sigma), _fp(bg), C.c_void_p(d_out)),
          "ggs_render_device")


def render_layout_device(device: int, stream: int, d_genomes: int, B: int, N: int, Cc: int, layout: int, H: int,
                         W: int, k_sigma: float, d_out: int, background=(1.0, 1.0, 1.0)) -> None:
    """Enqueue the render of rows in ``layout`` (GGS_LAYOUT_*) on `stream`: layout 0 is ``render_device``."""
    check(lib.ggs_render_layout_device(device, C.c_void_p(stream), C.c_void_p(d_genomes), B, N, Cc, int(layout), H,
                                       W, float(k_sigma), _fp(_background3(background)), C.c_void_p(d_out)),
          "ggs_render_layout_device")


def render_vjp_device(device: int, stream: int, d_genomes: int, B: int, N: int, Cc: int, layout: int, H: int,
                      W: int, k_sigma: float, d_cot: int, d_grad: int, background=(1.0, 1.0, 1.0)) -> None:
    """Enqueue the render's vector-Jacobian product (d_cot [B,H,W,3] -> d_grad [B,N,9]) on `stream`."""
    check(lib.ggs_render_vjp_device(device, C.c_void_p(stream), C.c_void_p(d_genomes or None), B, N, Cc, int(layout),
                                    H, W, float(k_sigma), _fp(_background3(background)),
                                    C.c_void_p(d_cot or None), C.c_void_p(d_grad or None)),
          "ggs_render_vjp_device")


def image_loss_device(device: int, stream: int, d_img: int, B: int, d_targets: int, K: int, group: int, H: int,
                      W: int, params, d_loss: int, d_cot: int = 0) -> None:
    """Enqueue the image loss (d_img [B,H,W,3] against d_targets [K,H,W,3] -> d_loss [B] and,
    unless 0, d_cot [B,H,W,3]) on `stream`."""
    prm = loss_params_c(params)
    check(lib.ggs_image_loss_device(device, C.c_void_p(stream), C.c_void_p(d_img or None), B,
                                    C.c_void_p(d_targets or None), K, int(group), H, W, C.byref(prm),
                                    C.c_void_p(d_loss or None), C.c_void_p(d_cot or None)),
          "ggs_image_loss_device")


def loss_grad_device(device: int, stream: int, d_genomes: int, B: int, N: int, Cc: int, layout: int,
                     d_targets: int, K: int, group: int, H: int, W: int, k_sigma: float, params, d_loss: int,
                     d_grad: int, background=(1.0, 1.0, 1.0)) -> None:
    """Enqueue render -> image loss -> VJP (d_loss [B], d_grad [B,N,9]) on `stream`."""
    prm = loss_params_c(params)
    check(lib.ggs_loss_grad_device(device, C.c_void_p(stream), C.c_void_p(d_genomes or None), B, N, Cc,
                                   int(layout), C.c_void_p(d_targets or None), K, int(group), H, W,
                                   float(k_sigma), _fp(_background3(background)), C.byref(prm),
                                   C.c_void_p(d_loss or None), C.c_void_p(d_grad or None)),
          "ggs_loss_grad_device")


def profile_enable(on: bool = True) -> None:
    check(lib.ggs_profile_enable(1 if on else 0), "ggs_profile_enable")


def profile_read(kernel: str):
    ms, n = C.c_double(0.0), C.c_int64(0)
    check(lib.ggs_profile_read(kernel.encode(), C.byref(ms), C.byref(n)), "ggs_profile_read")
    return ms.value, n.value


def profile_reset() -> None:
    lib.ggs_profile_reset()

