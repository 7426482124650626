"""Residual-driven placement's C ABI without a GPU: the exports exist, every refusal of
ggs_seed_sites_device, ggs_seed_sites and ggs_seed_genomes is GGS_EINVAL with a message
before the library looks for a device (the pattern of tests/test_density_args.py), a refused
call leaves its outputs alone, and ``SeedParams`` / the Python wrappers refuse the same
values themselves."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ggs
from ggs import _lib, api
from ggs import seed as S

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
# the pointers are never read: every call below fails its argument checks
_FAKE = C.cast(0x1000, _f32p)
_IFAKE = C.cast(0x1000, _i32p)
_VFAKE = C.c_void_p(0x1000)
NAN, INF = float("nan"), float("inf")
EXPORTS = ("ggs_seed_sites_device", "ggs_seed_sites", "ggs_seed_genomes")


def test_exports_are_declared_exported_and_bound():
    from test_capi import declared_functions
    for name in EXPORTS:
        assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(_lib.lib, name), name
    assert callable(ggs.seed_sites) and callable(ggs.seed_genomes) and ggs.SeedParams is S.SeedParams
    assert callable(ggs.seed_schedule) and callable(ggs.seeded_population) and ggs.SeedRound is S.SeedRound
    assert C.sizeof(_lib.SeedParamsC) == 24 and C.sizeof(_lib.SeedRoundC) == 16
    c = S.seed_params_c(S.SeedParams(8, 5, 2, 0.5, 1.25, 100.0))
    assert (c.cell, c.max_sites, c.first_row, c.err_min, c.log_sigma, c.alpha) == (8, 5, 2, 0.5, 1.25, 100.0)


def test_the_profiler_has_a_seed_slot():
    ms, n = api.profile_read("seed")             # nothing here has placed anything with the profiler on
    assert ms >= 0.0 and n >= 0
    with pytest.raises(ggs.GGSInputError, match="seed"):
        api.profile_read("no such slot")


def _prm(p):
    if p is None:
        return None
    base = dict(cell=8, max_sites=6, first_row=0, err_min=0.0, log_sigma=1.0, alpha=200.0)
    base.update(p)
    return C.byref(_lib.SeedParamsC(*[base[k] for k, _ in _lib.SeedParamsC._fields_]))


GOOD = dict(img=True, bg=None, tgt=True, w=True, B=4, K=2, group=2, H=33, W=47, p={}, rows=False, x=True, N=24,
            xo=True, sites=True, n=True, err=True)
BAD = [
    (dict(p=None), "null"), (dict(tgt=False), "null"), (dict(sites=False), "null"), (dict(n=False), "null"),
    (dict(p=dict(cell=0)), "cell"), (dict(p=dict(cell=3)), "cell"), (dict(p=dict(cell=128)), "cell"),
    (dict(p=dict(cell=-8)), "cell"), (dict(p=dict(cell=1)), "cell"),
    (dict(p=dict(max_sites=0)), "max_sites"), (dict(p=dict(max_sites=-1)), "max_sites"),
    (dict(p=dict(err_min=NAN)), "finite"), (dict(p=dict(err_min=INF)), "finite"),
    (dict(p=dict(log_sigma=NAN)), "finite"), (dict(p=dict(log_sigma=-INF)), "finite"),
    (dict(p=dict(alpha=NAN)), "finite"), (dict(p=dict(err_min=-1e-6)), "err_min"),
    (dict(p=dict(alpha=-0.5)), "alpha"), (dict(p=dict(alpha=255.5)), "alpha"),
    (dict(p=dict(first_row=-1)), "first_row"), (dict(p=dict(first_row=19)), "first_row"),
    (dict(p=dict(max_sites=25)), "first_row"),
    (dict(B=0), "B="), (dict(B=-2), "B="), (dict(B=65536, group=1, K=65536), "limit"),
    (dict(K=0), "K="), (dict(H=0), "H="), (dict(W=0), "W="), (dict(N=0), "N="), (dict(N=-3), "N="),
    (dict(group=0), "group"), (dict(group=3), "multiple"), (dict(group=1), "images wanted"),
    (dict(B=65535, K=65535, group=1, H=4096, W=4096, p=dict(cell=2)), "cells"),
    (dict(B=65535, K=65535, group=1, N=4096), "B*N"),
    (dict(bg=(NAN, 0.0, 0.0)), "background"),
]


def _common(a):
    bg = None if a["bg"] is None else (C.c_float * 3)(*a["bg"])
    return bg, _prm(a["p"])


def _call_host(a):
    bg, prm = _common(a)
    return _lib.lib.ggs_seed_sites(
        0, _FAKE if a["img"] else None, bg, _FAKE if a["tgt"] else None, _FAKE if a["w"] else None, a["B"], a["K"],
        a["group"], a["H"], a["W"], prm, _IFAKE if a["rows"] else None, _FAKE if a["x"] else None, a["N"],
        _FAKE if a["xo"] else None, _IFAKE if a["sites"] else None, _IFAKE if a["n"] else None,
        _FAKE if a["err"] else None)


def _call_device(a):
    bg, prm = _common(a)
    v = lambda on: _VFAKE if on else None  # noqa: E731
    return _lib.lib.ggs_seed_sites_device(
        0, None, v(a["img"]), bg, v(a["tgt"]), v(a["w"]), a["B"], a["K"], a["group"], a["H"], a["W"], prm,
        v(a["rows"]), v(a["x"]), a["N"], v(a["sites"]), v(a["n"]), v(a["err"]))


@pytest.mark.parametrize("call", [_call_host, _call_device])
@pytest.mark.parametrize("over,word", BAD)
def test_seed_sites_reports_bad_arguments_without_a_device(call, over, word):
    a = dict(GOOD)
    a.update(over)
    assert call(a) == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


def test_host_export_refuses_one_genome_array_alone_and_rows_outside_the_genome():
    a = dict(GOOD)
    for over in (dict(xo=False), dict(x=False)):
        b = dict(a)
        b.update(over)
        assert _call_host(b) == _lib.GGS_EINVAL and "alone" in _lib.last_error()
    B, M, N = 2, 3, 5
    for bad in (-1, N):
        rows = np.array([[0, 1, 2], [3, bad, 4]], np.int32)
        out = np.full((B, N, 9), 7.0, np.float32)
        sites = np.full((B, M), 9, np.int32)
        n = np.full((B,), 9, np.int32)
        err = np.full((B, 4), 7.0, np.float32)
        prm = _lib.SeedParamsC(8, M, 0, 0.0, 1.0, 200.0)
        rc = _lib.lib.ggs_seed_sites(0, None, None, _FAKE, None, B, 1, 2, 16, 16, C.byref(prm),
                                     rows.ctypes.data_as(_i32p), _FAKE, N, out.ctypes.data_as(_f32p),
                                     sites.ctypes.data_as(_i32p), n.ctypes.data_as(_i32p), err.ctypes.data_as(_f32p))
        assert rc == _lib.GGS_EINVAL and "row" in _lib.last_error()
        # a refused call leaves its outputs alone
        assert (out == 7.0).all() and (sites == 9).all() and (n == 9).all() and (err == 7.0).all()


def _rounds(rs):
    if rs is None:
        return None, 0
    arr = (_lib.SeedRoundC * max(len(rs), 1))(*[_lib.SeedRoundC(*r) for r in rs])
    return arr, len(rs)


G_GOOD = dict(tgt=True, w=True, K=2, H=33, W=47, N=24, rounds=[(16, 8, 1.5, 200.0), (8, 16, 1.1, 200.0)], err_min=0.0,
              lo=1.0986, k=3.0, bg=None, out=True, placed=True)
G_BAD = [
    (dict(tgt=False), "null"), (dict(rounds=None), "null"), (dict(out=False), "null"), (dict(rounds=[]), "n_rounds"),
    (dict(rounds=[(16, 8, 1.5, 200.0), (5, 16, 1.1, 200.0)]), "cell"),
    (dict(rounds=[(16, -1, 1.5, 200.0), (8, 25, 1.1, 200.0)]), "count"),
    (dict(rounds=[(16, 8, 1.5, 200.0), (8, 15, 1.1, 200.0)]), "sum"),
    (dict(rounds=[(16, 8, 1.5, 200.0), (8, 17, 1.1, 200.0)]), "sum"),
    (dict(rounds=[(16, 8, NAN, 200.0), (8, 16, 1.1, 200.0)]), "finite"),
    (dict(rounds=[(16, 8, 1.5, 256.0), (8, 16, 1.1, 200.0)]), "alpha"),
    (dict(rounds=[(16, 8, 1.5, -1.0), (8, 16, 1.1, 200.0)]), "alpha"),
    (dict(err_min=-0.1), "err_min"), (dict(err_min=NAN), "finite"), (dict(lo=INF), "finite"), (dict(k=NAN), "finite"),
    (dict(K=0), "B="), (dict(K=65536), "limit"), (dict(H=0), "H="), (dict(W=-1), "W="), (dict(N=0), "N="),
    (dict(N=2 ** 25, rounds=[(16, 2 ** 25, 1.5, 200.0)]), "exceeds"),
    (dict(bg=(0.0, INF, 0.0)), "background"),
]


@pytest.mark.parametrize("over,word", G_BAD)
def test_seed_genomes_reports_bad_arguments_without_a_device(over, word):
    a = dict(G_GOOD)
    a.update(over)
    arr, nr = _rounds(a["rounds"])
    bg = None if a["bg"] is None else (C.c_float * 3)(*a["bg"])
    rc = _lib.lib.ggs_seed_genomes(0, _FAKE if a["tgt"] else None, _FAKE if a["w"] else None, a["K"], a["H"], a["W"],
                                   a["N"], arr, nr, a["err_min"], a["lo"], a["k"], bg, _FAKE if a["out"] else None,
                                   _IFAKE if a["placed"] else None)
    assert rc == _lib.GGS_EINVAL and word in _lib.last_error(), _lib.last_error()


PARAMS_BAD = [
    (dict(cell=3), "cell"), (dict(cell=0), "cell"), (dict(cell=8.5), "cell"), (dict(max_sites=0), "max_sites"),
    (dict(max_sites=-2), "max_sites"), (dict(first_row=-1), "first_row"), (dict(err_min=-1.0), "err_min"),
    (dict(err_min=NAN), "err_min"), (dict(log_sigma=INF), "log_sigma"), (dict(log_sigma=1e39), "log_sigma"),
    (dict(alpha=NAN), "alpha"), (dict(alpha=-1.0), "alpha"), (dict(alpha=256.0), "alpha"),
]


@pytest.mark.parametrize("over,word", PARAMS_BAD)
def test_seed_params_are_refused_in_python(over, word):
    p = S.SeedParams()._replace(**over)
    with pytest.raises(ggs.GGSInputError, match=word):
        S.seed_params_c(p)
    tgt = np.zeros((1, 8, 8, 3), np.float32)
    x = np.zeros((1, 64, 9), np.float32)
    with pytest.raises(ggs.GGSInputError, match=word):
        api.seed_sites(x, None, tgt, p)
    with pytest.raises(ggs.GGSInputError, match=word):
        S.place_sites(x, None, tgt, p)


def test_python_wrappers_report_shape_and_round_errors():
    tgt = np.zeros((2, 8, 8, 3), np.float32)
    p = S.SeedParams(4, 2, 0, 0.0, 1.0, 200.0)
    with pytest.raises(ggs.GGSInputError, match="targets"):
        api.seed_sites(None, None, tgt[..., :2], p)
    with pytest.raises(ggs.GGSInputError, match="image"):
        api.seed_sites(None, np.zeros((2, 8, 9, 3), np.float32), tgt, p)
    with pytest.raises(ggs.GGSInputError, match="weights"):
        api.seed_sites(None, None, tgt, p, weights=np.zeros((2, 8, 7), np.float32))
    with pytest.raises(ggs.GGSInputError, match="genomes"):
        api.seed_sites(np.zeros((3, 4, 9), np.float32), None, tgt, p)
    with pytest.raises(ggs.GGSInputError, match="rows"):
        api.seed_sites(np.zeros((2, 4, 9), np.float32), None, tgt, p, rows=np.zeros((2, 3), np.int32))
    with pytest.raises(ggs.GGSInputError, match="row"):          # the C layer, before any device
        api.seed_sites(np.zeros((2, 4, 9), np.float32), None, tgt, p, rows=np.array([[0, 1], [2, 4]], np.int32))
    with pytest.raises(ggs.GGSInputError, match="first_row"):
        api.seed_sites(np.zeros((2, 4, 9), np.float32), None, tgt, p._replace(first_row=3))
    with pytest.raises(ggs.GGSInputError, match="multiple"):
        api.seed_sites(None, np.zeros((3, 8, 8, 3), np.float32), tgt, p, group=2)
    with pytest.raises(ggs.GGSInputError, match="sum"):
        S.seed_genomes(tgt, 10, [S.SeedRound(8, 4, 1.0, 200.0), S.SeedRound(4, 5, 1.0, 200.0)])
    with pytest.raises(ggs.GGSInputError, match="cell"):
        S.seed_genomes(tgt, 4, [S.SeedRound(6, 4, 1.0, 200.0)])
    with pytest.raises(ggs.GGSInputError, match="count"):
        S.seed_genomes(tgt, 4, [S.SeedRound(8, -1, 1.0, 200.0), S.SeedRound(8, 5, 1.0, 200.0)])
    with pytest.raises(ggs.GGSInputError, match="round"):
        S.seed_genomes(tgt, 4, [])
