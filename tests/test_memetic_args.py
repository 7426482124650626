"""The plan-set gradient, the K-image refiner and the island polish without a GPU:
the exports exist, and every invalid argument of ggs_fitness_grad_targets,
ggs_fitness_grad_device_planset and ggs_refine_create_targets is GGS_EINVAL (the
workspace budget: GGS_ENOMEM) with a message before the library looks for a device
(the pattern of tests/test_grad_args.py)."""
from __future__ import annotations

import ctypes as C

import pytest

from ggs import _lib
from ggs.ga_device import _config

_f32p = C.POINTER(C.c_float)
ZERO = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
# the pointers are never read: every call below fails its argument checks
_FAKE = C.cast(0x1000, _f32p)
_VFAKE = C.c_void_p(0x1000)
EXPORTS = ("ggs_fitness_grad_device_planset", "ggs_fitness_grad_targets", "ggs_refine_create_targets",
           "ggs_ga_islands_set_polish")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert [f[0] for f in _lib.GaPolish._fields_] == ["every", "n_steps", "n_rows", "adam"]
    assert C.sizeof(_lib.GaPolish) == 60


GOOD = dict(g=True, B=6, N=5, C=9, t=True, m=True, K=3, group=2, mode=_lib.GGS_FIT_WEIGHTED, H=16, W=24,
            out=True, grad=True)
BAD = [
    (dict(g=False), "null"), (dict(t=False), "null"), (dict(grad=False), "null"), (dict(out=False), "null"),
    (dict(group=0), "group="), (dict(group=-2), "group="), (dict(B=5), "multiple"), (dict(B=8), "holds"),
    (dict(group=1), "holds"), (dict(K=0), "K="), (dict(K=-1), "K="),
    (dict(m=False), "mask"), (dict(m=False, mode=_lib.GGS_FIT_BOOST), "mask"), (dict(mode=3), "mode"),
    (dict(C=8), "genome cols"), (dict(B=0), "B="), (dict(N=0), "N="), (dict(H=0), "H="), (dict(W=0), "W="),
]


def _args(over):
    a = dict(GOOD)
    a.update(over)
    return a


@pytest.mark.parametrize("over,word", BAD)
def test_host_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(over)
    rc = _lib.lib.ggs_fitness_grad_targets(_FAKE if a["g"] else None, a["B"], a["N"], a["C"],
                                           _FAKE if a["t"] else None, _FAKE if a["m"] else None, a["K"], a["group"],
                                           a["mode"], 1.0, a["H"], a["W"], 3.0, _FAKE if a["out"] else None,
                                           _FAKE if a["grad"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


def test_host_call_above_the_workspace_budget_is_enomem_without_a_device():
    rc = _lib.lib.ggs_fitness_grad_targets(_FAKE, 2, 4096, 9, _FAKE, None, 2, 1, _lib.GGS_FIT_NONE, 1.0, 2048, 2048,
                                           3.0, _FAKE, _FAKE)
    assert rc == _lib.GGS_ENOMEM and "budget" in _lib.last_error(), _lib.last_error()


def test_device_call_without_a_set_is_einval():
    # a set exists only on a device: its other rules are the host call's, checked above
    rc = _lib.lib.ggs_fitness_grad_device_planset(None, None, _VFAKE, 6, 5, 9, 2, _VFAKE, _VFAKE, 3.0, None, _VFAKE)
    assert rc == _lib.GGS_EINVAL and "null plan set" in _lib.last_error(), _lib.last_error()


def _create(cfg_over=None, prm_over=None, B=6, K=3, group=2, mask=True, target=True, pop=True, handle=True,
            cfg=True, prm=True):
    kw = dict(P=2, N=3, H=16, W=24, tour_k=1, elite_k=0, cxpb=0.0, mutpb=0.0, k_sigma=3.0,
              min_scale_splats=0.5, max_scale_splats=0.5, boost_only=False, boost_beta=1.0,
              schedule="linear", mut_sigma_max=ZERO, mut_sigma_min=ZERO, seed=0, mask=True)
    kw.update(cfg_over or {})
    c = _config(**kw)
    pk = dict(lr=[0.01] * 9, beta1=0.9, beta2=0.999, eps=1e-8)
    pk.update(prm_over or {})
    p = _lib.RefineParams((C.c_float * 9)(*pk["lr"]), pk["beta1"], pk["beta2"], pk["eps"])
    h = C.c_void_p()
    rc = _lib.lib.ggs_refine_create_targets(0, C.byref(c) if cfg else None, C.byref(p) if prm else None,
                                            _FAKE if target else None, _FAKE if mask else None, K,
                                            _FAKE if pop else None, B, group, C.byref(h) if handle else None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(cfg=False), "null"), (dict(prm=False), "null"), (dict(target=False), "null"), (dict(pop=False), "null"),
    (dict(handle=False), "null"),
    (dict(group=0), "group="), (dict(group=-1), "group="), (dict(B=5), "multiple"), (dict(B=8), "holds"),
    (dict(group=1), "holds"), (dict(K=0), "K="), (dict(mask=False), "mask"),
    (dict(B=0), "B="), (dict(cfg_over=dict(N=0)), "N="), (dict(cfg_over=dict(H=0)), "H="),
    (dict(cfg_over=dict(W=0)), "W="),
    (dict(prm_over=dict(lr=[-1.0] + [0.01] * 8)), "lr"), (dict(prm_over=dict(beta1=1.0)), "beta1"),
    (dict(prm_over=dict(beta2=-0.1)), "beta2"), (dict(prm_over=dict(eps=0.0)), "eps"),
])
def test_refine_create_targets_reports_bad_arguments_without_a_device(kw, word):
    rc, msg = _create(**kw)
    assert rc == _lib.GGS_EINVAL and word in msg, msg


def test_refine_create_targets_above_the_workspace_budget_is_enomem_without_a_device():
    rc, msg = _create(cfg_over=dict(N=4096, H=2048, W=2048))
    assert rc == _lib.GGS_ENOMEM and "budget" in msg, msg


def test_set_polish_without_a_session_is_einval():
    adam = _lib.RefineParams((C.c_float * 9)(*[0.01] * 9), 0.9, 0.999, 1e-8)
    pol = _lib.GaPolish(2, 3, 1, adam)
    assert _lib.lib.ggs_ga_islands_set_polish(None, C.byref(pol)) == _lib.GGS_EINVAL
    assert "null" in _lib.last_error()
    assert _lib.lib.ggs_ga_islands_set_polish(None, None) == _lib.GGS_EINVAL
