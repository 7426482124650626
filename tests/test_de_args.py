"""The ggs_de_* C ABI without a GPU: the exports exist, and every invalid argument
of ggs_de_create / ggs_de_set_params / ggs_de_run / ggs_de_read is GGS_EINVAL with
a message before the library looks for a device (the pattern of
tests/test_planset_args.py)."""
from __future__ import annotations

import ctypes as C

import pytest

from ggs import _lib
from ggs.ga_device import _config

_f32p = C.POINTER(C.c_float)
ZERO = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
# the pointers are never read: every call below fails its argument checks
_FAKE = C.cast(0x1000, _f32p)
EXPORTS = ("ggs_de_create", "ggs_de_set_params", "ggs_de_run", "ggs_de_read", "ggs_de_destroy")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert [f[0] for f in _lib.DeParams._fields_] == ["strategy", "crossover", "f_lo", "f_hi", "cr"]
    assert C.sizeof(_lib.DeParams) == 20


def _create(cfg_over=None, de_over=None, mask=True, target=True, pop=True, handle=True, cfg=True, de=True):
    """ggs_de_create on a valid argument set with some fields replaced."""
    kw = dict(P=8, N=3, H=16, W=24, tour_k=1, elite_k=0, cxpb=0.0, mutpb=0.0, k_sigma=3.0,
              min_scale_splats=0.5, max_scale_splats=0.5, boost_only=False, boost_beta=1.0,
              schedule="linear", mut_sigma_max=ZERO, mut_sigma_min=ZERO, seed=0, mask=True)
    kw.update(cfg_over or {})
    c = _config(**kw)
    dkw = dict(strategy=0, crossover=0, f_lo=0.5, f_hi=0.9, cr=0.3)
    dkw.update(de_over or {})
    d = _lib.DeParams(dkw["strategy"], dkw["crossover"], dkw["f_lo"], dkw["f_hi"], dkw["cr"])
    h = C.c_void_p()
    rc = _lib.lib.ggs_de_create(0, C.byref(c) if cfg else None, C.byref(d) if de else None,
                                _FAKE if target else None, _FAKE if mask else None, _FAKE if pop else None,
                                C.byref(h) if handle else None)
    assert rc != _lib.GGS_OK
    return rc, _lib.last_error()


@pytest.mark.parametrize("over,word", [
    (dict(cfg_over=dict(P=3)), "pop_size"),
    (dict(cfg_over=dict(P=0)), "pop_size"),
    (dict(cfg_over=dict(P=513)), "pop_size"),
    (dict(cfg_over=dict(N=0)), "n_splats"),
    (dict(cfg_over=dict(H=0)), "H="),
    (dict(de_over=dict(cr=-0.01)), "cr="),
    (dict(de_over=dict(cr=1.01)), "cr="),
    (dict(de_over=dict(cr=float("nan"))), "cr="),
    (dict(de_over=dict(f_lo=0.9, f_hi=0.5)), "f_lo"),
    (dict(de_over=dict(f_lo=float("nan"))), "finite"),
    (dict(de_over=dict(f_hi=float("inf"))), "finite"),
    (dict(de_over=dict(strategy=3)), "strategy"),
    (dict(de_over=dict(strategy=-1)), "strategy"),
    (dict(de_over=dict(crossover=2)), "crossover"),
    (dict(de_over=dict(crossover=-1)), "crossover"),
    (dict(cfg=False), "null"),
    (dict(de=False), "null"),
    (dict(target=False), "null"),
    (dict(pop=False), "null"),
    (dict(handle=False), "null"),
    (dict(mask=False), "mask"),                                  # weighted mode without a mask
    (dict(mask=False, cfg_over=dict(boost_only=True)), "mask"),
])
def test_de_create_invalid_arguments(over, word):
    rc, msg = _create(**over)
    assert rc == _lib.GGS_EINVAL, (rc, msg)
    assert word in msg, msg


def test_de_session_calls_reject_null_handles_and_bad_params():
    lib = _lib.lib
    ok = _lib.DeParams(0, 0, 0.5, 0.9, 0.3)
    assert lib.ggs_de_set_params(None, C.byref(ok)) == _lib.GGS_EINVAL and "handle" in _lib.last_error()
    # the parameters are checked before the handle is used
    bad = _lib.DeParams(0, 0, 0.5, 0.9, 2.0)
    assert lib.ggs_de_set_params(C.c_void_p(0x1000), C.byref(bad)) == _lib.GGS_EINVAL and "cr=" in _lib.last_error()
    assert lib.ggs_de_set_params(C.c_void_p(0x1000), None) == _lib.GGS_EINVAL and "null" in _lib.last_error()
    assert lib.ggs_de_run(None, 1, 1) == _lib.GGS_EINVAL
    assert lib.ggs_de_run(C.c_void_p(0x1000), 1, -1) == _lib.GGS_EINVAL
    assert lib.ggs_de_read(None, None, None, None, None, None, None, None, None) == _lib.GGS_EINVAL
    lib.ggs_de_destroy(None)


def test_python_names_are_checked():
    from ggs import de
    assert de.strategy_id("rand1") == 0 and de.strategy_id("best1") == 1 and de.strategy_id("current-to-best1") == 2
    assert de.crossover_id("gene") == 0 and de.crossover_id("splat") == 1
    assert de.f_range(0.7) == (0.7, 0.7) and de.f_range((0.5, 0.9)) == (0.5, 0.9)
    with pytest.raises(ValueError):
        de.strategy_id("rand2")
    with pytest.raises(ValueError):
        de.crossover_id("row")
