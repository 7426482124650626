"""ggs.autograd.render_splats on an MI355X: the forward has the render's bits,
``.backward()`` leaves api.render_vjp's bits in ``.grad`` (HIP tensors: the device
entry points on torch's stream), an MSE written in torch reproduces the fused
fitness gradient, and torch.optim.Adam lowers an L1 loss the library has no kernel
for."""
from __future__ import annotations

import numpy as np
import pytest

import _grad_cases as cases
import _render_vjp_cases as vc
from ggs import api
from test_gpu_render_vjp import FIT_BAR, _fmt, _ratios

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SHAPE = "48x40"
W, H, N = cases.SHAPES[SHAPE]


@pytest.mark.parametrize("layout,bg", [("renderer", vc.COLOUR), ("axes", vc.WHITE)])
@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_forward_and_backward_have_the_library_bits(device, layout, bg):
    from ggs.autograd import render_splats
    R = vc.widen(vc.rows(SHAPE, layout, encode=api.encode), 12)
    V = vc.normal_cotangent(SHAPE)
    kw = dict(k_sigma=cases.K_SIGMA, background=bg, layout=layout)
    g = torch.tensor(R, device=device, requires_grad=True)
    img = render_splats(g, H, W, **kw)
    assert img.shape == (3, H, W, 3) and img.dtype == torch.float32
    assert img.detach().cpu().numpy().tobytes() == api.render(R, H, W, **kw).tobytes()
    (img * torch.tensor(V, device=device)).sum().backward()
    got = g.grad.detach().cpu().numpy()
    assert got.shape == R.shape
    assert got[..., :9].tobytes() == api.render_vjp(R, V, H, W, **kw).tobytes() and not got[..., 9:].any()
    # one candidate as [N,C]
    g1 = torch.tensor(R[1], device=device, requires_grad=True)
    img1 = render_splats(g1, H, W, **kw)
    assert img1.shape == (H, W, 3) and torch.equal(img1.detach(), img.detach()[1])
    (img1 * torch.tensor(V[1], device=device)).sum().backward()
    assert np.array_equal(g1.grad.cpu().numpy(), got[1])


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_a_float64_input_keeps_its_dtype(device):
    from ggs.autograd import render_splats
    R = vc.rows(SHAPE, "axes")
    V = vc.normal_cotangent(SHAPE)
    g = torch.tensor(R, device=device, dtype=torch.float64, requires_grad=True)
    img = render_splats(g, H, W, k_sigma=cases.K_SIGMA, layout="axes")
    assert img.dtype == torch.float64
    (img * torch.tensor(V, device=device, dtype=torch.float64)).sum().backward()
    assert g.grad.dtype == torch.float64 and g.grad.shape == g.shape
    want = api.render_vjp(R, V, H, W, k_sigma=cases.K_SIGMA, layout="axes")
    assert np.array_equal(g.grad.cpu().numpy(), want.astype(np.float64))


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_an_mse_written_in_torch_gives_the_fitness_gradient(device):
    from ggs.autograd import render_splats, splat_fitness
    G, target, _ = cases.problem(SHAPE)
    t = torch.tensor(target, device=device)
    g = torch.tensor(np.ascontiguousarray(G), device=device, requires_grad=True)
    img = render_splats(g, H, W, k_sigma=cases.K_SIGMA, layout="axes")
    ((img - t) ** 2).mean(dim=(1, 2, 3)).sum().backward()
    got = g.grad.detach().cpu().numpy()
    g2 = torch.tensor(np.ascontiguousarray(G), device=device, requires_grad=True)
    splat_fitness(g2, t, None, k_sigma=cases.K_SIGMA).sum().backward()
    r = _ratios(got, g2.grad.detach().cpu().numpy().astype(np.float64))
    print(f"{device}: torch MSE through render_splats vs splat_fitness ratios {_fmt(r)}")
    assert r.max() <= FIT_BAR


def test_torch_adam_lowers_an_l1_loss():
    from ggs.autograd import render_splats
    G, target, _ = cases.problem(SHAPE)
    g = torch.tensor(np.ascontiguousarray(G), device="cuda")
    t = torch.tensor(target, device="cuda")
    lr = torch.tensor([0.002, 0.002, 0.02, 0.02, 0.02, 2.0, 2.0, 2.0, 2.0], device="cuda")
    z = torch.zeros_like(g, requires_grad=True)           # g + lr * z: one rate per column through one optimiser
    opt = torch.optim.Adam([z], lr=1.0)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = (render_splats(g + lr * z, H, W, k_sigma=cases.K_SIGMA, layout="axes") - t).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert losses[-1] < losses[0]
