"""ggs.autograd.image_loss on an MI355X: the forward has ``api.image_loss``'s bits,
``backward`` returns the cotangent times ``grad_output[b]`` and nothing for the targets;
``image_loss(render_splats(g))`` with ``.sum().backward()`` leaves ``api.loss_grad``'s bits
in ``g.grad``; and an L1 + SSIM written in torch (float64, zero padding) over
``render_splats`` agrees with it within the bar of tests/test_gpu_loss_grad.py (measured on
the MI355X: 2.05e-7 at worst over the nine columns, the loss within 1.80e-8)."""
from __future__ import annotations

import numpy as np
import pytest

import _grad_cases as cases
import _loss_cases as lc
import _loss_ref as lref
import _render_vjp_cases as vc
from ggs import api
from test_gpu_loss_grad import BAR, LOSS_BAR, MAIN, _fmt, _ratios, _targets

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SHAPE = "48x40"
W, H, N = cases.SHAPES[SHAPE]


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_forward_and_backward_are_the_library_loss_and_cotangent(device):
    from ggs.autograd import image_loss
    h, w = 33, 47
    B, K, group = 4, 2, 2
    tg = np.ascontiguousarray(lc.targets(h, w, "flat")[:K])
    img = lc.images(h, w, "flat", B, group)
    want_l, want_c = api.image_loss(img, tg, MAIN, group=group)
    x = torch.tensor(img, device=device, requires_grad=True)
    t = torch.tensor(tg, device=device, requires_grad=True)
    loss = image_loss(x, t, MAIN, group)
    assert loss.shape == (B,) and loss.dtype == torch.float32
    assert loss.detach().cpu().numpy().tobytes() == want_l.tobytes()
    scale = torch.tensor([1.0, 2.0, -0.5, 0.0], device=device)
    (loss * scale).sum().backward()
    got = x.grad.detach().cpu().numpy()
    assert got.tobytes() == (want_c * scale.cpu().numpy()[:, None, None, None]).astype(np.float32).tobytes()
    assert t.grad is None                                   # no gradient reaches the targets
    # one image [H,W,3] against one target [H,W,3]: a scalar
    x1 = torch.tensor(img[1], device=device, requires_grad=True)
    l1 = image_loss(x1, torch.tensor(tg[0], device=device), MAIN)
    assert l1.shape == () and float(l1.detach()) == float(want_l[1])
    l1.backward()
    assert x1.grad.cpu().numpy().tobytes() == want_c[1].tobytes()


@pytest.mark.parametrize("layout,bg", [("axes", vc.WHITE), ("renderer", vc.COLOUR)])
@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_the_loss_of_a_render_leaves_loss_grad_bits(device, layout, bg):
    from ggs.autograd import image_loss, render_splats
    R = vc.widen(vc.rows(SHAPE, layout, encode=api.encode), 12)
    tg = _targets(SHAPE)
    kw = dict(k_sigma=cases.K_SIGMA, background=bg, layout=layout)
    want_l, want_g = api.loss_grad(R, tg, H, W, MAIN, group=1, **kw)
    g = torch.tensor(R, device=device, requires_grad=True)
    loss = image_loss(render_splats(g, H, W, **kw), torch.tensor(np.array(tg), device=device), MAIN)
    assert loss.detach().cpu().numpy().tobytes() == want_l.tobytes()
    loss.sum().backward()
    got = g.grad.detach().cpu().numpy()
    assert got[..., :9].tobytes() == want_g.tobytes() and not got[..., 9:].any()


def test_a_torch_written_l1_ssim_agrees():
    from ggs.autograd import render_splats
    G = np.ascontiguousarray(cases.problem(SHAPE)[0])
    tg = _targets(SHAPE)
    want_l, want_g = api.loss_grad(G, tg, H, W, MAIN, k_sigma=cases.K_SIGMA, layout="axes", group=1)
    g = torch.tensor(G, device="cuda", requires_grad=True)
    img = render_splats(g, H, W, k_sigma=cases.K_SIGMA, layout="axes")
    x = img.to(dtype=torch.float64, device="cpu")
    losses = [lref.loss_tensor(x[b], torch.from_numpy(tg[b].astype(np.float64)), MAIN) for b in range(3)]
    torch.stack(losses).sum().backward()
    r = _ratios(want_g, g.grad.detach().cpu().numpy().astype(np.float64))
    rl = float(np.max(np.abs(want_l - np.array([float(v.detach()) for v in losses])) / want_l))
    print(f"torch-written L1 + SSIM (float64) vs loss_grad: ratios {_fmt(r)}  loss {rl:.2e}")
    assert r.max() <= BAR and rl <= LOSS_BAR
