"""Plan sets and island groups with a target per island, without a GPU:

* every invalid argument of ggs_planset_create, ggs_fitness_device_planset and
  ggs_ga_islands_create_targets is GGS_EINVAL with a message before the library
  looks for a device (the pattern of tests/test_ga_islands_host.py);
* ``ggs.ga.ring_migration(..., refit=...)``, the numpy statement the device's
  re-scoring migration is held to, on a hand-worked K = 3, P = 4, m = 1 case.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from ggs import _lib, ga
from ggs.ga_device import _config

_f32p = C.POINTER(C.c_float)
SIG = {"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0}
H, W, K, P, N = 16, 24, 2, 8, 3
# the pointers are never read: every call below fails its argument checks
_FAKE = 0x1000


def _planset_create(targets=_FAKE, masks=_FAKE, mode=_lib.GGS_FIT_WEIGHTED, H=H, W=W, K=K, out=True):
    h = C.c_void_p()
    rc = _lib.lib.ggs_planset_create(0, None, C.c_void_p(targets), C.c_void_p(masks), mode, 1.0, H, W, K,
                                     C.byref(h) if out else None)
    assert rc != _lib.GGS_OK
    return rc, _lib.last_error()


@pytest.mark.parametrize("over,word", [
    (dict(K=0), "K="),
    (dict(K=-2), "K="),
    (dict(targets=None), "null"),
    (dict(out=False), "null"),
    (dict(mode=3), "mode"),
    (dict(mode=-1), "mode"),
    (dict(masks=None, mode=_lib.GGS_FIT_WEIGHTED), "mask"),
    (dict(masks=None, mode=_lib.GGS_FIT_BOOST), "mask"),
    (dict(H=0), "H="),
    (dict(W=-1), "W="),
    (dict(H=4096, W=4096, K=1 << 20), "grid limit"),       # the set's strips are numbered in 32 bits
])
def test_planset_create_invalid_arguments(over, word):
    rc, msg = _planset_create(**over)
    assert rc == _lib.GGS_EINVAL, (rc, msg)
    assert word in msg, msg


@pytest.mark.parametrize("B,group,word", [
    (12, 0, "group"),
    (12, -4, "group"),
    (12, 5, "multiple"),          # B % group != 0
    (12, 4, "null plan set"),     # valid numbers: the missing set is the error
])
def test_fitness_device_planset_invalid_arguments(B, group, word):
    rc = _lib.lib.ggs_fitness_device_planset(None, None, C.c_void_p(_FAKE), B, N, 9, group, 3.0, C.c_void_p(_FAKE))
    assert rc == _lib.GGS_EINVAL, (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def test_planset_destroy_null_is_a_noop():
    _lib.lib.ggs_planset_destroy(None)


def _create_targets(cfg_over=None, isl_over=None, seeds=True, pops=True, mask=True, targets=True, handle=True):
    """ggs_ga_islands_create_targets on a valid argument set with some fields replaced."""
    kw = dict(P=P, N=N, H=H, W=W, tour_k=2, elite_k=2, cxpb=0.5, mutpb=0.1, k_sigma=3.0,
              min_scale_splats=3.0, max_scale_splats=0.1, boost_only=False, boost_beta=1.0,
              schedule="cosine", mut_sigma_max=SIG, mut_sigma_min=SIG, seed=0, mask=True)
    kw.update(cfg_over or {})
    cfg = _config(**kw)
    isl_kw = dict(n_islands=K, migrate_every=4, n_migrants=2, topology=0)
    isl_kw.update(isl_over or {})
    k_, h_, w_ = max(isl_kw["n_islands"], 1), max(kw["H"], 1), max(kw["W"], 1)
    small = k_ * h_ * w_ < 1 << 20          # (refused before anything is read: no gigabyte arrays)
    t = np.zeros((k_, h_, w_, 3) if small else 1, np.float32)
    m = np.ones((k_, h_, w_) if small else 1, np.float32)
    sd = np.arange(k_, dtype=np.uint64)
    isl = _lib.GaIslands(isl_kw["n_islands"], isl_kw["migrate_every"], isl_kw["n_migrants"],
                         isl_kw["topology"], sd.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds else None)
    shape = (k_, max(kw["P"], 1), max(kw["N"], 1), 9)
    init = np.zeros(shape if np.prod(shape) < 1 << 20 else 1, np.float32)
    h = C.c_void_p()
    rc = _lib.lib.ggs_ga_islands_create_targets(
        0, C.byref(cfg), C.byref(isl), t.ctypes.data_as(_f32p) if targets else None,
        m.ctypes.data_as(_f32p) if mask else None, init.ctypes.data_as(_f32p) if pops else None,
        C.byref(h) if handle else None)
    if rc == _lib.GGS_OK:                 # only where a GPU is present
        _lib.lib.ggs_ga_islands_destroy(h)
    return rc, _lib.last_error()


@pytest.mark.parametrize("over,word", [
    (dict(cfg_over=dict(P=0)), "pop_size"),
    (dict(cfg_over=dict(tour_k=0)), "tour_k"),
    (dict(cfg_over=dict(elite_k=P + 1)), "elite_k"),
    (dict(cfg_over=dict(H=0)), "H="),
    (dict(mask=False), "mask"),                                 # weighted mode without masks
    (dict(targets=False), "null"),
    (dict(handle=False), "null"),
    (dict(isl_over=dict(n_islands=0)), "n_islands"),
    (dict(cfg_over=dict(P=513), isl_over=dict(n_migrants=0)), "pop_size"),
    (dict(isl_over=dict(migrate_every=-1)), "migrate_every"),
    (dict(isl_over=dict(n_migrants=-1)), "n_migrants"),
    (dict(isl_over=dict(n_migrants=P // 2 + 1)), "n_migrants"),
    (dict(isl_over=dict(topology=1)), "topology"),
    (dict(seeds=False), "seeds"),
    (dict(pops=False), "init_pops"),
    (dict(cfg_over=dict(P=512, N=1, H=1024, W=1024), isl_over=dict(n_islands=8192)), "grid limit"),
])
def test_islands_create_targets_invalid_arguments(over, word):
    rc, msg = _create_targets(**over)
    assert rc == _lib.GGS_EINVAL, (rc, msg)
    assert word in msg, msg


def test_islands_create_targets_null_structs():
    h = C.c_void_p()
    rc = _lib.lib.ggs_ga_islands_create_targets(0, None, None, None, None, None, C.byref(h))
    assert rc == _lib.GGS_EINVAL and _lib.last_error()


def test_python_wrapper_reports_a_k_mismatch():
    from ggs.ga_device import DeviceGAIslands
    kw = dict(tour_k=2, elite_k=2, cxpb=0.5, mutpb=0.1, mut_sigma_max=SIG, mut_sigma_min=SIG,
              schedule="cosine", min_scale_splats=3.0, max_scale_splats=0.1)
    pops = np.zeros((K, P, N, 9), np.float32)
    t3 = np.zeros((K + 1, H, W, 3), np.float32)
    with pytest.raises(_lib.GGSInputError, match="per-island targets"):
        DeviceGAIslands(t3, np.ones((K + 1, H, W), np.float32), pops, [1, 2], 0, 0, **kw)
    with pytest.raises(_lib.GGSInputError, match="per-island masks"):
        DeviceGAIslands(t3[:K], np.ones((H, W), np.float32), pops, [1, 2], 0, 0, **kw)
    with pytest.raises(_lib.GGSInputError, match="target must be"):
        DeviceGAIslands(t3[0, 0], None, pops, [1, 2], 0, 0, **kw)


# ---- ring_migration(refit=...) -----------------------------------------------------
def _hand_case():
    # genome of island k, row r: every gene = 10 k + r
    pops = np.empty((3, 4, 2, 9), np.float32)
    for k in range(3):
        for r in range(4):
            pops[k, r] = 10 * k + r
    fits = np.asarray([[0.4, 0.1, 0.3, 0.2],       # best row 1, worst row 0
                       [0.5, 0.5, 0.2, 0.5],       # best row 2, worst: the tie 0, 1, 3 -> rank 3 is row 3
                       [0.9, 0.8, 0.7, 0.6]],      # best row 3, worst row 0
                      np.float32)
    return pops, fits


def test_ring_migration_refit_hand_example():
    pops, fits = _hand_case()
    calls = []

    def refit(k, genomes):
        calls.append((k, genomes.copy()))
        # "fitness on island k": a function of the island and the genome alone
        return np.asarray([100.0 * (k + 1) + genomes[0, 0, 0]], np.float32)

    new_p, new_f = ga.ring_migration(pops, fits, 1, refit=refit)
    want_p, want_f = pops.copy(), fits.copy()
    # island 0 <- island 2's best (row 3, genome 23) onto its worst row 0
    want_p[0, 0] = 23
    want_f[0, 0] = 100.0 + 23
    # island 1 <- island 0's best (row 1, genome 1) onto rank 3 of the tie: row 3
    want_p[1, 3] = 1
    want_f[1, 3] = 200.0 + 1
    # island 2 <- island 1's best (row 2, genome 12) onto its worst row 0
    want_p[2, 0] = 12
    want_f[2, 0] = 300.0 + 12
    np.testing.assert_array_equal(new_p, want_p)
    np.testing.assert_array_equal(new_f, want_f)
    assert new_f.dtype == np.float32
    assert [k for k, _ in calls] == [0, 1, 2]
    for (k, g), gene in zip(calls, (23, 1, 12)):
        assert g.shape == (1, 2, 9) and (g == gene).all(), (k, g)
    # the inputs are not modified
    p0, f0 = _hand_case()
    np.testing.assert_array_equal(pops, p0)
    np.testing.assert_array_equal(fits, f0)


def test_ring_migration_refit_none_is_the_plain_rule():
    pops, fits = _hand_case()
    a_p, a_f = ga.ring_migration(pops, fits, 1)
    b_p, b_f = ga.ring_migration(pops, fits, 1, refit=None)
    np.testing.assert_array_equal(a_p, b_p)
    np.testing.assert_array_equal(a_f, b_f)
    # ... which installs the source island's fitness
    want_f = fits.copy()
    want_f[0, 0], want_f[1, 3], want_f[2, 0] = fits[2, 3], fits[0, 1], fits[1, 2]
    np.testing.assert_array_equal(a_f, want_f)
    # and a refit that returns the source fitness changes nothing
    src_f = {0: fits[2, 3], 1: fits[0, 1], 2: fits[1, 2]}
    c_p, c_f = ga.ring_migration(pops, fits, 1, refit=lambda k, g: [src_f[k]])
    np.testing.assert_array_equal(c_p, a_p)
    np.testing.assert_array_equal(c_f, a_f)


def test_ring_migration_refit_two_migrants_order():
    """refit sees island k's immigrants in the order j = 0 .. m - 1 of the source's ranks."""
    pops, fits = _hand_case()
    seen = {}

    def refit(k, genomes):
        seen[k] = genomes[:, 0, 0].tolist()
        return np.zeros(len(genomes), np.float32)

    ga.ring_migration(pops[:2], fits[:2], 2, refit=refit)
    # island 0 <- island 1's ranks 0, 1: rows 2 (0.2), then 0 (first of the 0.5 tie)
    assert seen[0] == [12.0, 10.0]
    # island 1 <- island 0's ranks 0, 1: rows 1 (0.1), 3 (0.2)
    assert seen[1] == [1.0, 3.0]
