"""The image-loss C ABI without a GPU: the exports exist, every invalid argument of
ggs_image_loss, ggs_image_loss_device, ggs_loss_grad, ggs_loss_grad_device and
ggs_refine_create_loss is GGS_EINVAL (the VJP's workspace budget: GGS_ENOMEM) with a
message before the library looks for a device (the pattern of
tests/test_render_vjp_args.py), and the Python wrappers report shape errors themselves."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ggs
from ggs import _lib, api
from ggs.ga_device import DeviceRefine

_f32p = C.POINTER(C.c_float)
# the pointers are never read: every call below fails its argument checks
_FAKE = C.cast(0x1000, _f32p)
_VFAKE = C.c_void_p(0x1000)
EXPORTS = ("ggs_image_loss", "ggs_image_loss_device", "ggs_loss_grad", "ggs_loss_grad_device",
           "ggs_refine_create_loss")
NAN, INF = float("nan"), float("inf")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    for name in ("image_loss", "image_loss_device", "loss_grad", "loss_grad_device", "LossParams"):
        assert callable(getattr(ggs, name)), name
    assert tuple(ggs.LossParams()) == (0.8, 0.0, 0.2)
    assert C.sizeof(_lib.LossParamsC) == 12


def _prm(w):
    return None if w is None else C.byref(_lib.LossParamsC(*w))


# ---- ggs_image_loss / ggs_image_loss_device ---------------------------------------
LOSS_GOOD = dict(img=True, B=4, tg=True, K=2, group=2, H=16, W=24, w=(0.8, 0.0, 0.2), loss=True)
LOSS_BAD = [
    (dict(img=False), "null"), (dict(tg=False), "null"), (dict(loss=False), "null"), (dict(w=None), "null"),
    (dict(B=0), "B="), (dict(B=-1), "B="), (dict(H=0), "H="), (dict(W=0), "W="), (dict(W=-2), "W="),
    (dict(group=0), "group"), (dict(group=-1), "group"), (dict(K=0), "K="),
    (dict(B=3), "multiple"), (dict(group=1), "images wanted"), (dict(B=3, K=2, group=1), "images wanted"),
    (dict(w=(0.0, 0.0, 0.0)), "all zero"), (dict(w=(-0.1, 0.0, 1.0)), "weights"), (dict(w=(0.5, NAN, 0.0)), "weights"),
    (dict(w=(0.5, 0.0, INF)), "weights"),
    (dict(B=1 << 20, K=1 << 20, group=1, H=1024, W=1024), "grid limit"),
]


def _args(good, over):
    a = dict(good)
    a.update(over)
    return a


@pytest.mark.parametrize("over,word", LOSS_BAD)
@pytest.mark.parametrize("cot", [False, True])
def test_image_loss_host_call_reports_bad_arguments_without_a_device(over, word, cot):
    a = _args(LOSS_GOOD, over)
    rc = _lib.lib.ggs_image_loss(_FAKE if a["img"] else None, a["B"], _FAKE if a["tg"] else None, a["K"], a["group"],
                                 a["H"], a["W"], _prm(a["w"]), _FAKE if a["loss"] else None,
                                 _FAKE if cot else None, 0)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("over,word", LOSS_BAD)
def test_image_loss_device_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(LOSS_GOOD, over)
    rc = _lib.lib.ggs_image_loss_device(0, None, _VFAKE if a["img"] else None, a["B"], _VFAKE if a["tg"] else None,
                                        a["K"], a["group"], a["H"], a["W"], _prm(a["w"]),
                                        _VFAKE if a["loss"] else None, None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


# ---- ggs_loss_grad / ggs_loss_grad_device ------------------------------------------
GRAD_GOOD = dict(g=True, B=4, N=5, C=9, layout=_lib.GGS_LAYOUT_AXES, tg=True, K=2, group=2, H=16, W=24,
                 w=(0.8, 0.0, 0.2), loss=True, grad=True)
GRAD_BAD = [
    (dict(g=False), "null"), (dict(tg=False), "null"), (dict(loss=False), "null"), (dict(grad=False), "null"),
    (dict(w=None), "null"),
    # the dimension rules of ggs_render_vjp_device
    (dict(C=8), "genome cols"), (dict(B=0), "B="), (dict(B=-1), "B="), (dict(N=0), "N="), (dict(N=-3), "N="),
    (dict(H=0), "H="), (dict(W=0), "W="), (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
    (dict(B=1 << 20, N=1 << 11, H=1, W=1, K=1 << 20, group=1), "B*N"),
    # the group rule and the weights
    (dict(group=0), "group"), (dict(K=0), "K="), (dict(B=3), "multiple"), (dict(group=1), "images wanted"),
    (dict(w=(0.0, 0.0, 0.0)), "all zero"), (dict(w=(0.0, -1.0, 0.0)), "weights"), (dict(w=(NAN, 0.0, 0.0)), "weights"),
]


@pytest.mark.parametrize("over,word", GRAD_BAD)
def test_loss_grad_host_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(GRAD_GOOD, over)
    rc = _lib.lib.ggs_loss_grad(_FAKE if a["g"] else None, a["B"], a["N"], a["C"], a["layout"],
                                _FAKE if a["tg"] else None, a["K"], a["group"], a["H"], a["W"], 3.0, None,
                                _prm(a["w"]), _FAKE if a["loss"] else None, _FAKE if a["grad"] else None, 0)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("over,word", GRAD_BAD)
def test_loss_grad_device_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(GRAD_GOOD, over)
    rc = _lib.lib.ggs_loss_grad_device(0, None, _VFAKE if a["g"] else None, a["B"], a["N"], a["C"], a["layout"],
                                       _VFAKE if a["tg"] else None, a["K"], a["group"], a["H"], a["W"], 3.0, None,
                                       _prm(a["w"]), _VFAKE if a["loss"] else None, _VFAKE if a["grad"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


def test_a_candidate_above_the_vjp_workspace_budget_is_enomem_without_a_device():
    p = _prm((0.8, 0.0, 0.2))
    rc = _lib.lib.ggs_loss_grad(_FAKE, 1, 4096, 9, 1, _FAKE, 1, 1, 2048, 2048, 3.0, None, p, _FAKE, _FAKE, 0)
    assert rc == _lib.GGS_ENOMEM and "budget" in _lib.last_error(), _lib.last_error()
    rc = _lib.lib.ggs_loss_grad_device(0, None, _VFAKE, 1, 4096, 9, 1, _VFAKE, 1, 1, 2048, 2048, 3.0, None, p, _VFAKE,
                                       _VFAKE)
    assert rc == _lib.GGS_ENOMEM and "budget" in _lib.last_error(), _lib.last_error()


# ---- ggs_refine_create_loss ---------------------------------------------------------
def _cfg(N=5, H=16, W=24):
    cfg = _lib.GaConfig()
    cfg.pop_size, cfg.n_splats, cfg.H, cfg.W = 4, N, H, W
    cfg.k_sigma, cfg.min_scale_splats, cfg.max_scale_splats = 3.0, 0.5, 0.5
    return cfg


def _adam(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8):
    return _lib.RefineParams((C.c_float * 9)(*([lr] * 9)), beta1, beta2, eps)


REFINE_GOOD = dict(cfg=True, adam={}, w=(0.8, 0.0, 0.2), tg=True, K=2, g=True, B=4, group=2, handle=True, N=5, H=16)
REFINE_BAD = [
    (dict(cfg=False), "null"), (dict(adam=None), "null"), (dict(w=None), "null"), (dict(tg=False), "null"),
    (dict(g=False), "null"), (dict(handle=False), "null"),
    (dict(B=0), "B="), (dict(N=0), "N="), (dict(H=0), "H="),
    (dict(group=0), "group"), (dict(K=0), "K="), (dict(B=3), "multiple"),
    (dict(B=3, K=2, group=1), "images wanted"),          # 3 % 1 is fine, but 3 images > K
    (dict(w=(0.0, 0.0, 0.0)), "all zero"), (dict(w=(0.0, 0.0, -1.0)), "weights"),
    (dict(adam=dict(lr=-1.0)), "lr"), (dict(adam=dict(beta1=1.0)), "beta1"), (dict(adam=dict(eps=0.0)), "eps"),
]


@pytest.mark.parametrize("over,word", REFINE_BAD)
def test_refine_create_loss_reports_bad_arguments_without_a_device(over, word):
    a = _args(REFINE_GOOD, over)
    h = C.c_void_p()
    cfg = _cfg(N=a["N"], H=a["H"])
    rc = _lib.lib.ggs_refine_create_loss(0, C.byref(cfg) if a["cfg"] else None,
                                         None if a["adam"] is None else C.byref(_adam(**a["adam"])), _prm(a["w"]),
                                         None, _FAKE if a["tg"] else None, a["K"], _FAKE if a["g"] else None, a["B"],
                                         a["group"], C.byref(h) if a["handle"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()
    assert not h.value


# ---- the Python wrappers --------------------------------------------------------------
def test_python_wrappers_report_shape_errors():
    img = np.zeros((4, 16, 24, 3), np.float32)
    with pytest.raises(ggs.GGSInputError, match="img must be"):
        api.image_loss(np.zeros((4, 16, 24), np.float32), img[:2])
    for bad in (np.zeros((2, 16, 24), np.float32), np.zeros((2, 24, 16, 3), np.float32),
                np.zeros((2, 16, 24, 4), np.float32)):
        with pytest.raises(ggs.GGSInputError, match="targets must be"):
            api.image_loss(img, bad)
        with pytest.raises(ggs.GGSInputError, match="targets must be"):
            api.loss_grad(np.zeros((4, 5, 9), np.float32), bad, 16, 24)
    with pytest.raises(ggs.GGSInputError, match="group="):
        api.image_loss(img, img[0], group=2)
    with pytest.raises(ggs.GGSInputError, match="multiple"):
        api.image_loss(img[:3], img[:2], group=2)
    with pytest.raises(ggs.GGSInputError, match="all zero"):
        api.image_loss(img, img[:2], (0.0, 0.0, 0.0))
    with pytest.raises(ggs.GGSInputError, match="genome cols"):
        api.loss_grad(np.zeros((4, 5, 8), np.float32), img[:2], 16, 24)
    with pytest.raises(ggs.GGSInputError, match="layout"):
        api.loss_grad(np.zeros((4, 5, 9), np.float32), img[:2], 16, 24, layout="polar")


def test_device_refine_reports_loss_argument_errors():
    G = np.zeros((3, 5, 9), np.float32)
    tg = np.zeros((2, 16, 24, 3), np.float32)
    kw = dict(lr=[0.01] * 9, min_scale_splats=0.5, max_scale_splats=0.5)
    with pytest.raises(ggs.GGSInputError, match="images wanted"):
        DeviceRefine(tg, None, G, loss=ggs.LossParams(), group=1, **kw)
    with pytest.raises(ggs.GGSInputError, match="no weight mask"):
        DeviceRefine(tg, np.ones((2, 16, 24), np.float32), G, loss=ggs.LossParams(), **kw)
    with pytest.raises(ggs.GGSInputError, match="all zero"):
        DeviceRefine(tg, None, G[:2], loss=(0.0, 0.0, 0.0), **kw)
