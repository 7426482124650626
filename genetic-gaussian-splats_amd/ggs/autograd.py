"""torch.autograd bridge: the splat fitness and the render as differentiable functions.

``splat_fitness(genomes, target, mask)`` returns the fitness [B] of [B,N,C]
axes-angle genomes; ``.backward()`` leaves d fitness / d genomes in
``genomes.grad`` (columns 9.. of a wider genome get zeros).  On HIP tensors the
device entry point (ggs_fitness_grad_device) runs on torch's current stream with
no host copy; CPU tensors go through the host-pointer call.  The gradient is
computed with the fitness in ``forward`` and only scaled in ``backward``.

``render_splats(genomes, H, W)`` returns the image [B,H,W,3] itself, so that any
loss written in torch (L1, SSIM, a perceptual network, a crop ...) backpropagates
into ``genomes.grad``: ``backward`` hands ``grad_output`` to the renderer's
vector-Jacobian product (ggs_render_vjp_device), again on torch's
current stream with no host copy.

``image_loss(img, targets, params)`` is the library's own L1 / MSE / SSIM loss [B]
 of images [B,H,W,3]: ``forward`` computes loss and cotangent in one
device call, ``backward`` scales the cotangent, so
``image_loss(render_splats(g, H, W), t).sum().backward()`` needs no loss written in torch.

torch is imported here, never by ``import ggs``.
"""
from __future__ import annotations

import torch

from . import _lib, api


def _mode(mask, boost_only: bool) -> int:
    if mask is None:
        return _lib.GGS_FIT_NONE
    return _lib.GGS_FIT_BOOST if boost_only else _lib.GGS_FIT_WEIGHTED


class SplatFitness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, genomes, target, mask, k_sigma, boost_only, boost_beta):
        if genomes.dim() != 3 or genomes.shape[2] < 9:
            raise _lib.GGSInputError(f"genomes must be [B,N,C>=9], got {tuple(genomes.shape)}")
        if target.dim() != 3 or target.shape[2] != 3:
            raise _lib.GGSInputError(f"target must be [H,W,3], got {tuple(target.shape)}")
        B, N, Cc = genomes.shape
        H, W = int(target.shape[0]), int(target.shape[1])
        if mask is not None and tuple(mask.shape) != (H, W):
            raise _lib.GGSInputError(f"mask must be [H,W] = {(H, W)}, got {tuple(mask.shape)}")
        if genomes.is_cuda:
            dev = genomes.device
            g = genomes.detach().to(torch.float32).contiguous()
            t = target.detach().to(device=dev, dtype=torch.float32).contiguous()
            m = None if mask is None else mask.detach().to(device=dev, dtype=torch.float32).contiguous()
            fit = torch.empty(B, dtype=torch.float32, device=dev)
            grad9 = torch.empty((B, N, 9), dtype=torch.float32, device=dev)
            _lib.ensure_init()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                api.fitness_grad_device(dev.index or 0, stream, g.data_ptr(), B, N, Cc, t.data_ptr(),
                                        0 if m is None else m.data_ptr(), _mode(m, boost_only), boost_beta,
                                        H, W, k_sigma, fit.data_ptr(), grad9.data_ptr())
        else:
            f, g9 = api.fitness_grad(genomes.detach(), target.detach(), H, W, k_sigma,
                                     weight_mask=None if mask is None else mask.detach(),
                                     boost_only=boost_only, boost_beta=boost_beta)
            fit, grad9 = torch.from_numpy(f), torch.from_numpy(g9)
        if Cc > 9:
            grad = torch.zeros((B, N, Cc), dtype=torch.float32, device=grad9.device)
            grad[:, :, :9] = grad9
        else:
            grad = grad9
        ctx.save_for_backward(grad)
        ctx.in_dtype = genomes.dtype
        return fit.to(genomes.dtype) if genomes.dtype != torch.float32 else fit

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        g = grad * grad_output.to(grad.dtype)[:, None, None]
        return g.to(ctx.in_dtype), None, None, None, None, None


def splat_fitness(genomes, target, mask=None, *, k_sigma: float = 3.0, boost_only: bool = False,
                  boost_beta: float = 1.0):
    """Fitness [B] of [B,N,C] (or [N,C]: then a scalar) axes-angle genomes, differentiable
    with respect to ``genomes`` (DESIGN.md §8c names the derivative's conventions)."""
    if genomes.dim() == 2:
        return SplatFitness.apply(genomes[None], target, mask, float(k_sigma), bool(boost_only),
                                  float(boost_beta))[0]
    return SplatFitness.apply(genomes, target, mask, float(k_sigma), bool(boost_only), float(boost_beta))


class RenderSplats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, genomes, H, W, k_sigma, background, layout):
        if genomes.dim() != 3 or genomes.shape[2] < 9:
            raise _lib.GGSInputError(f"genomes must be [B,N,C>=9], got {tuple(genomes.shape)}")
        B, N, Cc = genomes.shape
        g = genomes.detach().to(torch.float32).contiguous()
        if g.is_cuda:
            dev = g.device
            img = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
            _lib.ensure_init()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                api.render_layout_device(dev.index or 0, stream, g.data_ptr(), B, N, Cc, layout, H, W, k_sigma,
                                         img.data_ptr(), background)
        else:
            img = torch.from_numpy(api.render(g, H, W, k_sigma=k_sigma, background=background, layout=layout))
        ctx.save_for_backward(g)
        ctx.args = (H, W, k_sigma, background, layout)
        ctx.in_dtype = genomes.dtype
        return img.to(genomes.dtype) if genomes.dtype != torch.float32 else img

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        H, W, k_sigma, background, layout = ctx.args
        B, N, Cc = g.shape
        v = grad_output.detach().to(torch.float32).contiguous()
        if g.is_cuda:
            dev = g.device
            grad9 = torch.empty((B, N, 9), dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                api.render_vjp_device(dev.index or 0, stream, g.data_ptr(), B, N, Cc, layout, H, W, k_sigma,
                                      v.data_ptr(), grad9.data_ptr(), background)
        else:
            grad9 = torch.from_numpy(api.render_vjp(g, v, H, W, k_sigma=k_sigma, background=background,
                                                    layout=layout))
        if Cc > 9:
            grad = torch.zeros((B, N, Cc), dtype=torch.float32, device=grad9.device)
            grad[:, :, :9] = grad9
        else:
            grad = grad9
        return grad.to(ctx.in_dtype), None, None, None, None, None


def render_splats(genomes, H: int, W: int, *, k_sigma: float = 3.0, background=(1.0, 1.0, 1.0),
                  layout="renderer"):
    """The image [B,H,W,3] of [B,N,C] genomes ([H,W,3] of [N,C]), differentiable with
    respect to ``genomes``: ``layout="renderer"`` rows are ``ggs.render``'s
    input, ``"axes"`` rows are axes-angle genomes.  No gradient reaches ``background``."""
    bg = tuple(float(x) for x in api._background3(background))
    args = (int(H), int(W), float(k_sigma), bg, api.layout_id(layout))
    if genomes.dim() == 2:
        return RenderSplats.apply(genomes[None], *args)[0]
    return RenderSplats.apply(genomes, *args)


class ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, targets, params, group):
        if img.dim() != 4 or img.shape[3] != 3:
            raise _lib.GGSInputError(f"img must be [B,H,W,3], got {tuple(img.shape)}")
        B, H, W, _ = (int(v) for v in img.shape)
        if targets.dim() != 4 or tuple(targets.shape[1:]) != (H, W, 3):
            raise _lib.GGSInputError(f"targets must be [K,H,W,3] with (H, W) = {(H, W)}, got {tuple(targets.shape)}")
        K = int(targets.shape[0])
        x = img.detach().to(torch.float32).contiguous()
        if x.is_cuda:
            dev = x.device
            t = targets.detach().to(device=dev, dtype=torch.float32).contiguous()
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            cot = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
            _lib.ensure_init()
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                api.image_loss_device(dev.index or 0, stream, x.data_ptr(), B, t.data_ptr(), K, group, H, W, params,
                                      loss.data_ptr(), cot.data_ptr())
        else:
            lo, co = api.image_loss(x, targets.detach(), params, group=group)
            loss, cot = torch.from_numpy(lo), torch.from_numpy(co)
        ctx.save_for_backward(cot)
        ctx.in_dtype = img.dtype
        return loss.to(img.dtype) if img.dtype != torch.float32 else loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (cot,) = ctx.saved_tensors
        g = cot * grad_output.to(cot.dtype)[:, None, None, None]
        return g.to(ctx.in_dtype), None, None, None


def image_loss(img, targets, params=None, group=None):
    """The image loss [B] of ``img`` [B,H,W,3] ([H,W,3]: a scalar) against ``targets``
    [K,H,W,3] (image b against target ``b // group``, default B // K) or [H,W,3] (one target
    for all), differentiable with respect to ``img``; no gradient reaches the targets.
    ``params``: ``ggs.LossParams`` (default 0.8 L1 + 0.2 (1 - SSIM))."""
    p = api.LossParams() if params is None else api.LossParams(*params)
    single = img.dim() == 3
    x = img[None] if single else img
    B = int(x.shape[0])
    if targets.dim() == 3:
        if group is not None:
            raise _lib.GGSInputError("group= needs 4-D targets [K,H,W,3]")
        targets, group = targets[None], B
    elif group is None:
        group = max(B // max(int(targets.shape[0]), 1), 1)
    out = ImageLoss.apply(x, targets, p, int(group))
    return out[0] if single else out
