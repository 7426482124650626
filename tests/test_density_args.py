"""Density control's C ABI without a GPU: the exports exist, every refusal of
ggs_density_relocate is GGS_EINVAL with a message before the library looks for a device
(the pattern of tests/test_loss_args.py), ``every = 0`` is the identity without a device,
and ``DensityParams`` / the Python wrappers refuse the same values themselves."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import ggs
from ggs import _lib, api
from ggs.refine import DensityParams, density_params_c, relocate

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
# the pointers are never read: every call below fails its argument checks
_FAKE = C.cast(0x1000, _f32p)
_IFAKE = C.cast(0x1000, _i32p)
NAN, INF = float("nan"), float("inf")
EXPORTS = ("ggs_refine_set_density", "ggs_refine_density_read", "ggs_density_relocate")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert callable(ggs.density_relocate) and ggs.DensityParams is DensityParams
    assert C.sizeof(_lib.RefineDensity) == 36
    c = density_params_c(DensityParams())
    assert c.log_shrink == float(np.float32(math.log(1.6))) and c.every == DensityParams().every


def _prm(p):
    if p is None:
        return None
    base = dict(every=4, start=0, stop=0, max_moves=8, alpha_dead=16.0, grad_min=0.01, split_log=2.0,
                log_shrink=0.47, split_offset=0.5)
    base.update(p)
    return C.byref(_lib.RefineDensity(*[base[k] for k, _ in _lib.RefineDensity._fields_]))


GOOD = dict(x=True, m=True, v=True, acc=True, n_acc=4, B=2, N=24, H=33, W=47, lo=-0.7, hi=3.1, p={},
            xo=True, mo=True, vo=True, pairs=True, n_pairs=True, is_split=True)
BAD = [
    (dict(p=None), "null"),
    (dict(x=False), "null"), (dict(m=False), "null"), (dict(v=False), "null"), (dict(acc=False), "null"),
    (dict(xo=False), "null"), (dict(mo=False), "null"), (dict(vo=False), "null"), (dict(pairs=False), "null"),
    (dict(n_pairs=False), "null"), (dict(is_split=False), "null"),
    (dict(p=dict(every=-1)), "every"), (dict(p=dict(start=-1)), "start"), (dict(p=dict(stop=-2)), "stop"),
    (dict(p=dict(max_moves=-1)), "max_moves"), (dict(p=dict(max_moves=0)), "max_moves"),
    (dict(p=dict(alpha_dead=NAN)), "finite"), (dict(p=dict(grad_min=INF)), "finite"),
    (dict(p=dict(split_log=-INF)), "finite"), (dict(p=dict(log_shrink=NAN)), "finite"),
    (dict(p=dict(split_offset=INF)), "finite"),
    (dict(p=dict(alpha_dead=-0.5)), "alpha_dead"), (dict(p=dict(alpha_dead=255.5)), "alpha_dead"),
    (dict(p=dict(grad_min=-1e-6)), "grad_min"), (dict(p=dict(log_shrink=-0.1)), "log_shrink"),
    (dict(B=0), "B="), (dict(B=-1), "B="), (dict(N=0), "N="), (dict(N=-4), "N="), (dict(B=65536), "limit"),
    (dict(B=65535, N=4096), "B*N"), (dict(H=0), "H="), (dict(W=0), "W="), (dict(n_acc=-1), "n_acc"),
    (dict(lo=1.0, hi=0.5), "interval"), (dict(lo=NAN), "interval"), (dict(hi=NAN), "interval"),
]


def _call(a):
    return _lib.lib.ggs_density_relocate(
        0, _FAKE if a["x"] else None, _FAKE if a["m"] else None, _FAKE if a["v"] else None,
        _FAKE if a["acc"] else None, a["n_acc"], a["B"], a["N"], a["H"], a["W"], a["lo"], a["hi"], _prm(a["p"]),
        _FAKE if a["xo"] else None, _FAKE if a["mo"] else None, _FAKE if a["vo"] else None,
        _IFAKE if a["pairs"] else None, _IFAKE if a["n_pairs"] else None, _IFAKE if a["is_split"] else None)


@pytest.mark.parametrize("over,word", BAD)
def test_relocate_reports_bad_arguments_without_a_device(over, word):
    a = dict(GOOD)
    a.update(over)
    assert _call(a) == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


def test_set_density_and_read_refuse_a_null_handle():
    assert _lib.lib.ggs_refine_set_density(None, _prm({})) == _lib.GGS_EINVAL and "null" in _lib.last_error()
    assert _lib.lib.ggs_refine_density_read(None, None, None, None, None, None, None) == _lib.GGS_EINVAL


def test_every_zero_is_the_identity_without_a_device():
    rng = np.random.default_rng(0)
    x, m, v = (rng.normal(0, 1, (2, 6, 9)).astype(np.float32) for _ in range(3))
    acc = rng.uniform(0, 1, (2, 6)).astype(np.float32)
    p = DensityParams(every=0)
    x2, m2, v2, pairs, n_pairs, is_split = api.density_relocate(x, m, v, acc, 3, 16, 24, p, -1.0, 3.0)
    assert x2.tobytes() == x.tobytes() and m2.tobytes() == m.tobytes() and v2.tobytes() == v.tobytes()
    assert pairs.shape == (2, 0, 2) and is_split.shape == (2, 0) and n_pairs.tolist() == [0, 0]
    # one splat: min(max_moves, N / 2) is zero, so nothing can move and no device is needed
    one = api.density_relocate(x[:, :1], m[:, :1], v[:, :1], acc[:, :1], 3, 16, 24, DensityParams(every=1), -1.0, 3.0)
    assert one[0].tobytes() == x[:, :1].tobytes() and one[4].tolist() == [0, 0]


PARAMS_BAD = [
    (dict(every=-1), "every"), (dict(start=-3), "start"), (dict(stop=-1), "stop"), (dict(max_moves=-2), "max_moves"),
    (dict(every=2.5), "every"), (dict(max_moves=0), "max_moves"), (dict(alpha_dead=NAN), "alpha_dead"),
    (dict(alpha_dead=-1.0), "alpha_dead"), (dict(alpha_dead=256.0), "alpha_dead"), (dict(grad_min=-0.1), "grad_min"),
    (dict(grad_min=INF), "grad_min"), (dict(split_log=NAN), "split_log"), (dict(shrink=0.9), "shrink"),
    (dict(shrink=0.0), "shrink"), (dict(shrink=INF), "shrink"), (dict(split_offset=NAN), "split_offset"),
    (dict(split_offset=1e39), "split_offset"),
]


@pytest.mark.parametrize("over,word", PARAMS_BAD)
def test_density_params_are_refused_in_python(over, word):
    p = DensityParams()._replace(**over)
    with pytest.raises(ggs.GGSInputError, match=word):
        density_params_c(p)
    x = np.zeros((1, 4, 9), np.float32)
    with pytest.raises(ggs.GGSInputError, match=word):
        api.density_relocate(x, x, x, np.zeros((1, 4), np.float32), 1, 8, 8, p, -1.0, 1.0)
    with pytest.raises(ggs.GGSInputError, match=word):
        relocate(x, x, x, np.zeros((1, 4), np.float32), 1, 8, 8, p, -1.0, 1.0)


def test_python_wrapper_reports_shape_errors():
    x = np.zeros((2, 4, 9), np.float32)
    p = DensityParams()
    with pytest.raises(ggs.GGSInputError, match="x, m, v"):
        api.density_relocate(x, x[:1], x, np.zeros((2, 4), np.float32), 1, 8, 8, p, -1.0, 1.0)
    with pytest.raises(ggs.GGSInputError, match="x, m, v"):
        api.density_relocate(x[0], x[0], x[0], np.zeros((4,), np.float32), 1, 8, 8, p, -1.0, 1.0)
    with pytest.raises(ggs.GGSInputError, match="acc must be"):
        api.density_relocate(x, x, x, np.zeros((2, 5), np.float32), 1, 8, 8, p, -1.0, 1.0)
    with pytest.raises(ggs.GGSInputError, match="interval"):
        api.density_relocate(x, x, x, np.zeros((2, 4), np.float32), 1, 8, 8, p, 2.0, 1.0)
