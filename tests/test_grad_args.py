"""The gradient and refine C ABI without a GPU: the exports exist, and every invalid
argument of ggs_fitness_grad, ggs_fitness_grad_device and ggs_refine_* is GGS_EINVAL
(the workspace budget: GGS_ENOMEM) with a message before the library looks for a
device (the pattern of tests/test_planset_args.py)."""
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
EXPORTS = ("ggs_fitness_grad", "ggs_fitness_grad_device", "ggs_refine_create", "ggs_refine_run",
           "ggs_refine_read", "ggs_refine_destroy")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert [f[0] for f in _lib.RefineParams._fields_] == ["lr", "beta1", "beta2", "eps"]
    assert C.sizeof(_lib.RefineParams) == 48


GOOD = dict(g=True, B=2, N=5, C=9, t=True, m=True, mode=_lib.GGS_FIT_WEIGHTED, H=16, W=24, out=True, grad=True)
BAD = [
    (dict(g=False), "null"), (dict(t=False), "null"), (dict(grad=False), "null"),
    (dict(C=8), "genome cols"), (dict(B=0), "B="), (dict(B=-1), "B="), (dict(N=0), "N="),
    (dict(H=0), "H="), (dict(W=0), "W="), (dict(m=False), "mask"),
    (dict(m=False, mode=_lib.GGS_FIT_BOOST), "mask"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
]


def _args(over):
    a = dict(GOOD)
    a.update(over)
    return a


@pytest.mark.parametrize("over,word", BAD + [(dict(out=False), "null")])
def test_host_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(over)
    rc = _lib.lib.ggs_fitness_grad(_FAKE if a["g"] else None, a["B"], a["N"], a["C"], _FAKE if a["t"] else None,
                                   _FAKE if a["m"] else None, a["mode"], 1.0, a["H"], a["W"], 3.0,
                                   _FAKE if a["out"] else None, _FAKE if a["grad"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("over,word", BAD)
def test_device_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(over)
    rc = _lib.lib.ggs_fitness_grad_device(0, None, _VFAKE if a["g"] else None, a["B"], a["N"], a["C"],
                                          _VFAKE if a["t"] else None, _VFAKE if a["m"] else None, a["mode"], 1.0,
                                          a["H"], a["W"], 3.0, None, _VFAKE if a["grad"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


def test_a_candidate_above_the_workspace_budget_is_enomem_without_a_device():
    rc = _lib.lib.ggs_fitness_grad(_FAKE, 1, 4096, 9, _FAKE, None, _lib.GGS_FIT_NONE, 1.0, 2048, 2048, 3.0,
                                   _FAKE, _FAKE)
    assert rc == _lib.GGS_ENOMEM and "budget" in _lib.last_error(), _lib.last_error()


def _create(cfg_over=None, prm_over=None, B=2, mask=True, target=True, pop=True, handle=True, cfg=True, prm=True):
    kw = dict(P=2, N=3, H=16, W=24, tour_k=1, elite_k=0, cxpb=0.0, mutpb=0.0, k_sigma=3.0,
              min_scale_splats=0.5, max_scale_splats=0.5, boost_only=False, boost_beta=1.0,
              schedule="linear", mut_sigma_max=ZERO, mut_sigma_min=ZERO, seed=0, mask=True)
    kw.update(cfg_over or {})
    c = _config(**kw)
    pk = dict(lr=[0.01] * 9, beta1=0.9, beta2=0.999, eps=1e-8)
    pk.update(prm_over or {})
    p = _lib.RefineParams((C.c_float * 9)(*pk["lr"]), pk["beta1"], pk["beta2"], pk["eps"])
    h = C.c_void_p()
    rc = _lib.lib.ggs_refine_create(0, C.byref(c) if cfg else None, C.byref(p) if prm else None,
                                    _FAKE if target else None, _FAKE if mask else None, _FAKE if pop else None, B,
                                    C.byref(h) if handle else None)
    assert rc != _lib.GGS_OK
    return rc, _lib.last_error()


@pytest.mark.parametrize("over,word", [
    (dict(cfg=False), "null"), (dict(prm=False), "null"), (dict(target=False), "null"), (dict(pop=False), "null"),
    (dict(handle=False), "null"), (dict(B=0), "B="), (dict(cfg_over=dict(N=0)), "N="),
    (dict(cfg_over=dict(H=0)), "H="), (dict(mask=False), "mask"),
    (dict(prm_over=dict(lr=[0.01] * 8 + [-1.0])), "lr[8]"), (dict(prm_over=dict(lr=[float("nan")] + [0.0] * 8)), "lr[0]"),
    (dict(prm_over=dict(beta1=1.0)), "beta1"), (dict(prm_over=dict(beta2=-0.1)), "beta2"),
    (dict(prm_over=dict(eps=0.0)), "eps"),
])
def test_refine_create_reports_bad_arguments_without_a_device(over, word):
    rc, msg = _create(**over)
    assert rc == _lib.GGS_EINVAL and word in msg, msg


def test_refine_calls_refuse_a_null_handle():
    assert _lib.lib.ggs_refine_run(None, 1) == _lib.GGS_EINVAL
    assert _lib.lib.ggs_refine_read(None, None, None, None, None, None) == _lib.GGS_EINVAL
    _lib.lib.ggs_refine_destroy(None)
