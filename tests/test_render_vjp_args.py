"""The render-VJP C ABI without a GPU: the exports exist, every invalid argument of
ggs_render_vjp, ggs_render_vjp_device and ggs_render_layout_device is GGS_EINVAL (the
workspace budget: GGS_ENOMEM) with a message before the library looks for a device
(the pattern of tests/test_grad_args.py), and the Python wrappers report shape and
layout errors themselves."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ggs
from ggs import _lib, api

_f32p = C.POINTER(C.c_float)
# the pointers are never read: every call below fails its argument checks
_FAKE = C.cast(0x1000, _f32p)
_VFAKE = C.c_void_p(0x1000)
EXPORTS = ("ggs_render_vjp", "ggs_render_vjp_device", "ggs_render_layout_device")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert (ggs.GGS_LAYOUT_RENDERER, ggs.GGS_LAYOUT_AXES) == (0, 1)
    for name in ("render_vjp", "render_vjp_device", "render_layout_device"):
        assert callable(getattr(ggs, name)), name


GOOD = dict(g=True, B=2, N=5, C=9, layout=_lib.GGS_LAYOUT_AXES, H=16, W=24, cot=True, grad=True)
BAD = [
    (dict(g=False), "null"), (dict(cot=False), "null"), (dict(grad=False), "null"),
    (dict(C=8), "genome cols"), (dict(B=0), "B="), (dict(B=-1), "B="), (dict(N=0), "N="), (dict(N=-3), "N="),
    (dict(H=0), "H="), (dict(W=0), "W="), (dict(layout=2), "layout"), (dict(layout=-1), "layout"),
    (dict(B=1 << 20, N=1 << 11, H=1, W=1), "B*N"),
]


def _args(over):
    a = dict(GOOD)
    a.update(over)
    return a


@pytest.mark.parametrize("over,word", BAD)
def test_host_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(over)
    rc = _lib.lib.ggs_render_vjp(_FAKE if a["g"] else None, a["B"], a["N"], a["C"], a["layout"], a["H"], a["W"], 3.0,
                                 None, _FAKE if a["cot"] else None, _FAKE if a["grad"] else None, 0)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("over,word", BAD)
def test_device_call_reports_bad_arguments_without_a_device(over, word):
    a = _args(over)
    rc = _lib.lib.ggs_render_vjp_device(0, None, _VFAKE if a["g"] else None, a["B"], a["N"], a["C"], a["layout"],
                                        a["H"], a["W"], 3.0, None, _VFAKE if a["cot"] else None,
                                        _VFAKE if a["grad"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("layout", [_lib.GGS_LAYOUT_RENDERER, _lib.GGS_LAYOUT_AXES])
def test_a_candidate_above_the_workspace_budget_is_enomem_without_a_device(layout):
    rc = _lib.lib.ggs_render_vjp(_FAKE, 1, 4096, 9, layout, 2048, 2048, 3.0, None, _FAKE, _FAKE, 0)
    assert rc == _lib.GGS_ENOMEM and "budget" in _lib.last_error(), _lib.last_error()
    rc = _lib.lib.ggs_render_vjp_device(0, None, _VFAKE, 1, 4096, 9, layout, 2048, 2048, 3.0, None, _VFAKE, _VFAKE)
    assert rc == _lib.GGS_ENOMEM and "budget" in _lib.last_error(), _lib.last_error()


@pytest.mark.parametrize("over,word", [(dict(layout=2), "layout"), (dict(C=8), "genome cols"), (dict(H=0), "H="),
                                       (dict(g=False), "null"), (dict(grad=False), "null")])
def test_layout_render_reports_bad_arguments_without_a_device(over, word):
    a = _args(over)
    rc = _lib.lib.ggs_render_layout_device(0, None, _VFAKE if a["g"] else None, a["B"], a["N"], a["C"], a["layout"],
                                           a["H"], a["W"], 3.0, None, _VFAKE if a["grad"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


def test_python_wrappers_report_shape_and_layout_errors():
    G = np.zeros((2, 5, 9), np.float32)
    for bad in (np.zeros((2, 16, 24), np.float32), np.zeros((1, 16, 24, 3), np.float32),
                np.zeros((2, 24, 16, 3), np.float32), np.zeros((2, 16, 24, 4), np.float32)):
        with pytest.raises(ggs.GGSInputError, match="cot must be"):
            api.render_vjp(G, bad, 16, 24)
    with pytest.raises(ggs.GGSInputError, match="genome cols"):
        api.render_vjp(np.zeros((2, 5, 8), np.float32), np.zeros((2, 16, 24, 3), np.float32), 16, 24)
    for call in (lambda: api.render_vjp(G, np.zeros((2, 16, 24, 3), np.float32), 16, 24, layout="polar"),
                 lambda: api.render(G, 16, 24, layout="polar"),
                 lambda: api.render_vjp(G, np.zeros((2, 16, 24, 3), np.float32), 16, 24, layout=2)):
        with pytest.raises(ggs.GGSInputError, match="layout"):
            call()
