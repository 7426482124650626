"""ggs.autograd.splat_fitness on an MI355X: ``.backward()`` leaves api.fitness_grad's
bits in ``.grad`` (HIP tensors: the device entry point on torch's stream), a scaled
``grad_output`` scales them, and torch.optim.Adam lowers the loss."""
from __future__ import annotations

import numpy as np
import pytest

import _grad_cases as cases
from ggs import api

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
SHAPE = "48x40"


def _tensors(device, C=9):
    G, target, mask = cases.problem(SHAPE)
    if C > 9:
        G = np.concatenate([G, np.zeros(G.shape[:2] + (C - 9,), np.float32)], axis=2)
    g = torch.tensor(np.ascontiguousarray(G), device=device, requires_grad=True)
    return G, target, mask, g, torch.tensor(target, device=device), torch.tensor(mask, device=device)


@pytest.mark.parametrize("device", ["cuda", "cpu"])
def test_backward_leaves_the_library_gradient(device):
    from ggs.autograd import splat_fitness
    W, H, N = cases.SHAPES[SHAPE]
    G, target, mask, g, t, m = _tensors(device, C=12)
    fit, grad = api.fitness_grad(G, target, H, W, cases.K_SIGMA, weight_mask=mask)
    out = splat_fitness(g, t, m, k_sigma=cases.K_SIGMA)
    assert out.shape == (3,) and out.detach().cpu().numpy().tobytes() == fit.tobytes()
    out.sum().backward()
    got = g.grad.detach().cpu().numpy()
    assert got[..., :9].tobytes() == np.ascontiguousarray(grad).tobytes() and not got[..., 9:].any()
    g.grad = None
    w = torch.tensor([2.0, 0.0, -0.5], device=device)
    (splat_fitness(g, t, m, k_sigma=cases.K_SIGMA) * w).sum().backward()
    want = grad * np.array([2.0, 0.0, -0.5], np.float32)[:, None, None]
    assert np.array_equal(g.grad.detach().cpu().numpy()[..., :9], want)


def test_torch_adam_lowers_the_loss():
    from ggs.autograd import splat_fitness
    G, target, mask, g, t, m = _tensors("cuda")
    lr = torch.tensor([0.002, 0.002, 0.02, 0.02, 0.02, 2.0, 2.0, 2.0, 2.0], device="cuda")
    z = torch.zeros_like(g, requires_grad=True)           # g + lr * z: one rate per column through one optimiser
    opt = torch.optim.Adam([z], lr=1.0)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = splat_fitness(g.detach() + lr * z, t, None).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert losses[-1] < losses[0]
