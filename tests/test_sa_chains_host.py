"""SA chain groups (ggs_sa_chains_*) without a GPU:

* every invalid argument of ggs_sa_chains_create / _create_targets / _run is
  GGS_EINVAL with a message before the library looks for a device (the pattern
  of tests/test_planset_args.py);
* ``ggs.annealing.replica_exchange``, the numpy statement the device's exchange
  kernel is held to, on synthetic energies;
* ``ggs_sa_exchange_uniform`` against an integer Philox restatement of its
  counter (it, k, 1, ACCEPT), written from DESIGN.md's table.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from ggs import _lib, annealing
from ggs.ga_device import _config

_f32p = C.POINTER(C.c_float)
_f64p = C.POINTER(C.c_double)
SIG = {"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0}
H, W, K, CAP, N = 16, 24, 3, 4, 3


def _create(multi, cfg_over=None, ch_over=None, seeds=True, inds=True, mask=True, target=True, handle=True,
            chains=True):
    """ggs_sa_chains_create[_targets] on a valid argument set with some fields replaced."""
    kw = dict(P=CAP, N=N, H=H, W=W, tour_k=1, elite_k=0, cxpb=0.0, mutpb=0.1, k_sigma=3.0,
              min_scale_splats=3.0, max_scale_splats=0.1, boost_only=False, boost_beta=1.0,
              schedule="cosine", mut_sigma_max=SIG, mut_sigma_min=SIG, seed=0, mask=True)
    kw.update(cfg_over or {})
    cfg = _config(**kw)
    ch_kw = dict(n_chains=K, exchange_every=0, exchange_seed=7)
    ch_kw.update(ch_over or {})
    k_, h_, w_ = max(min(ch_kw["n_chains"], 128), 1), max(kw["H"], 1), max(kw["W"], 1)
    small = k_ * h_ * w_ < 1 << 20          # (refused before anything is read: no gigabyte arrays)
    t = np.zeros(((k_, h_, w_, 3) if multi else (h_, w_, 3)) if small else 1, np.float32)
    m = np.ones(((k_, h_, w_) if multi else (h_, w_)) if small else 1, np.float32)
    sd = np.arange(k_, dtype=np.uint64)
    ch = _lib.SaChains(ch_kw["n_chains"], ch_kw["exchange_every"],
                       sd.ctypes.data_as(C.POINTER(C.c_uint64)) if seeds else None, ch_kw["exchange_seed"])
    init = np.zeros((k_, max(kw["N"], 1), 9), np.float32)
    h = C.c_void_p()
    fn = _lib.lib.ggs_sa_chains_create_targets if multi else _lib.lib.ggs_sa_chains_create
    rc = fn(0, C.byref(cfg), C.byref(ch) if chains else None, t.ctypes.data_as(_f32p) if target else None,
            m.ctypes.data_as(_f32p) if mask else None, init.ctypes.data_as(_f32p) if inds else None,
            C.byref(h) if handle else None, None)
    if rc == _lib.GGS_OK:                 # only where a GPU is present
        _lib.lib.ggs_sa_chains_destroy(h)
    return rc, _lib.last_error()


COMMON = [
    (dict(ch_over=dict(n_chains=0)), "n_chains"),
    (dict(ch_over=dict(n_chains=-3)), "n_chains"),
    (dict(ch_over=dict(n_chains=65)), "n_chains"),      # above GGS_SA_MAX_CHAINS = 64
    (dict(ch_over=dict(exchange_every=-1)), "exchange_every"),
    (dict(seeds=False), "seeds"),
    (dict(chains=False), "null"),
    (dict(target=False), "null"),
    (dict(inds=False), "null"),
    (dict(handle=False), "null"),
    (dict(mask=False), "mask"),                                     # weighted mode without a mask
    (dict(cfg_over=dict(P=0)), "pop_size"),
    (dict(cfg_over=dict(H=0)), "H="),
    (dict(cfg_over=dict(W=-1)), "W="),
]


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("over,word", COMMON)
def test_chains_create_invalid_arguments(multi, over, word):
    rc, msg = _create(multi, **over)
    assert rc == _lib.GGS_EINVAL, (rc, msg)
    assert word in msg, msg


def test_exchange_with_a_target_per_chain_is_refused():
    rc, msg = _create(True, ch_over=dict(exchange_every=4))
    assert rc == _lib.GGS_EINVAL, (rc, msg)
    assert "exchange" in msg and "target" in msg, msg


def test_chains_create_null_structs():
    h = C.c_void_p()
    for fn in (_lib.lib.ggs_sa_chains_create, _lib.lib.ggs_sa_chains_create_targets):
        rc = fn(0, None, None, None, None, None, C.byref(h), None)
        assert rc == _lib.GGS_EINVAL and _lib.last_error()


def test_null_handles():
    t = np.ones(4, np.float64)
    c = np.empty(8, np.float64)
    assert _lib.lib.ggs_sa_chains_run(None, 0, 1, 10, 1, t.ctypes.data_as(_f64p), 0,
                                      c.ctypes.data_as(_f64p)) == _lib.GGS_EINVAL
    assert "null" in _lib.last_error()
    assert _lib.lib.ggs_sa_chains_state(None, None, None, None, None, None, None, None) == _lib.GGS_EINVAL
    assert _lib.lib.ggs_sa_chains_read(None, None, None) == _lib.GGS_EINVAL
    _lib.lib.ggs_sa_chains_destroy(None)


def test_python_wrapper_reports_shape_mismatches():
    from ggs.ga_device import DeviceSAChains
    kw = dict(max_tries=CAP, mutpb=0.1, mut_sigma_max=SIG, mut_sigma_min=SIG, schedule="cosine",
              min_scale_splats=3.0, max_scale_splats=0.1)
    inds = np.zeros((K, N, 9), np.float32)
    t4 = np.zeros((K + 1, H, W, 3), np.float32)
    with pytest.raises(_lib.GGSInputError, match="per-chain targets"):
        DeviceSAChains(t4, np.ones((K + 1, H, W), np.float32), inds, [1, 2, 3], **kw)
    with pytest.raises(_lib.GGSInputError, match="per-chain masks"):
        DeviceSAChains(t4[:K], np.ones((H, W), np.float32), inds, [1, 2, 3], **kw)
    with pytest.raises(_lib.GGSInputError, match="target must be"):
        DeviceSAChains(t4[0, 0], None, inds, [1, 2, 3], **kw)
    with pytest.raises(_lib.GGSInputError, match="seeds"):
        DeviceSAChains(t4[0], np.ones((H, W), np.float32), inds, [1, 2], **kw)
    with pytest.raises(_lib.GGSInputError, match=r"\[K, N, 9\]"):
        DeviceSAChains(t4[0], np.ones((H, W), np.float32), inds[0], [1], **kw)
    # exchange between images: the library's own message, before any device
    with pytest.raises(_lib.GGSInputError, match="exchange"):
        DeviceSAChains(t4[:K], np.ones((K, H, W), np.float32), inds, [1, 2, 3], exchange_every=2, **kw)


# ---- the exchange uniform -------------------------------------------------------------
# Philox4x32-10 in Python integers, restated here (tests/_philox.py has no entry for
# the exchange counter): counter (it, k, 1, 8 = ACCEPT), key (seed low, seed high);
# u = ((x >> 5) 2^26 + (y >> 6)) 2^-53.
def _philox(c, k0, k1):
    c = list(c)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _uniform53(seed, it, k, what):
    x, y, _, _ = _philox((it, k, what, 8), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return ((x >> 5) * 67108864 + (y >> 6)) / 9007199254740992.0


def _xu(seed, it, k):
    u = C.c_double()
    assert _lib.lib.ggs_sa_exchange_uniform(seed, it, k, C.byref(u)) == _lib.GGS_OK, _lib.last_error()
    return u.value


def test_philox_restatement_is_philox():
    # Random123's known-answer vector for Philox4x32-10: counter and key all ones
    assert _philox((0xFFFFFFFF,) * 4, 0xFFFFFFFF, 0xFFFFFFFF) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


@pytest.mark.parametrize("seed", [0, 1, 0x0123456789ABCDEF, 2**64 - 1])
def test_exchange_uniform_is_the_documented_counter(seed):
    for it, k in [(0, 0), (3, 1), (255, 62), (2**31 - 1, 5), (17, 2**31 - 1)]:
        u = _xu(seed, it, k)
        assert u == _uniform53(seed, it, k, 1), (seed, it, k)
        assert 0.0 <= u < 1.0
        a = C.c_double()
        assert _lib.lib.ggs_sa_accept_uniform(seed, it, k, C.byref(a)) == _lib.GGS_OK
        assert a.value == _uniform53(seed, it, k, 0)
        assert a.value != u, "the exchange uniform must not be the acceptance uniform of (it, k)"


def test_exchange_uniform_invalid_arguments():
    u = C.c_double()
    assert _lib.lib.ggs_sa_exchange_uniform(1, 0, 0, None) == _lib.GGS_EINVAL
    assert _lib.lib.ggs_sa_exchange_uniform(1, -1, 0, C.byref(u)) == _lib.GGS_EINVAL
    assert _lib.lib.ggs_sa_exchange_uniform(1, 0, -1, C.byref(u)) == _lib.GGS_EINVAL


# ---- replica_exchange -----------------------------------------------------------------
def _state(K_, fits, bests=None):
    """Chain k's current genome is all k, its best all 100 + k."""
    cur = np.empty((K_, 2, 9), np.float32)
    best = np.empty((K_, 2, 9), np.float32)
    for k in range(K_):
        cur[k], best[k] = k, 100 + k
    f = np.asarray(fits, np.float64)
    b = np.asarray(bests if bests is not None else np.minimum(f, 0.0) - 1.0, np.float64)   # no best update
    return cur, f, best, b


def _ids(cur):
    return cur[:, 0, 0].astype(int).tolist()


SEED = 99


def test_forced_accept_and_forced_refuse():
    # pair (0, 1): chain 0 hotter and better: d = (E0 - E1)(1/T0 - 1/T1) = (-1)(-9) = 9 >= 0: swaps
    # pair (2, 3): chain 2 hotter and worse: d = (+1)(1/1 - 1/1e-6) ~ -1e6: exp(d) = 0: never
    cur, f, best, b = _state(4, [1.0, 2.0, 3.0, 2.0])
    T = [1.0, 0.1, 1.0, 1e-6]
    c, cf, bb, bf, tried, acc = annealing.replica_exchange(cur, f, best, b, T, 3, 4, SEED)   # e = 0: even pairs
    assert (tried, acc) == (2, 1)
    assert _ids(c) == [1, 0, 2, 3]
    assert cf.tolist() == [2.0, 1.0, 3.0, 2.0]
    np.testing.assert_array_equal(bb, best)
    np.testing.assert_array_equal(bf, b)
    # the inputs are not modified
    assert _ids(cur) == [0, 1, 2, 3] and f.tolist() == [1.0, 2.0, 3.0, 2.0]


def test_parities_and_the_unpaired_chain():
    cur, f, best, b = _state(5, [5.0, 4.0, 3.0, 2.0, 1.0])
    T = [1.0] * 5                                   # equal temperatures: d = 0, always swaps
    # e = 0 (it = 1, M = 2): pairs (0, 1), (2, 3); chain 4 unpaired
    c, cf, _, _, tried, acc = annealing.replica_exchange(cur, f, best, b, T, 1, 2, SEED)
    assert (tried, acc) == (2, 2) and _ids(c) == [1, 0, 3, 2, 4] and cf.tolist() == [4.0, 5.0, 2.0, 3.0, 1.0]
    # e = 1 (it = 3): pairs (1, 2), (3, 4); chain 0 unpaired
    c, cf, _, _, tried, acc = annealing.replica_exchange(cur, f, best, b, T, 3, 2, SEED)
    assert (tried, acc) == (2, 2) and _ids(c) == [0, 2, 1, 4, 3] and cf.tolist() == [5.0, 3.0, 4.0, 1.0, 2.0]
    # K = 2, odd exchange: no pair at all
    c, cf, _, _, tried, acc = annealing.replica_exchange(cur[:2], f[:2], best[:2], b[:2], T[:2], 3, 2, SEED)
    assert (tried, acc) == (0, 0) and _ids(c) == [0, 1]
    # K = 1
    c, cf, _, _, tried, acc = annealing.replica_exchange(cur[:1], f[:1], best[:1], b[:1], T[:1], 1, 2, SEED)
    assert (tried, acc) == (0, 0) and _ids(c) == [0]


def test_no_exchange_is_due_off_the_grid():
    cur, f, best, b = _state(2, [1.0, 2.0])
    with pytest.raises(ValueError, match="no exchange"):
        annealing.replica_exchange(cur, f, best, b, [1.0, 1.0], 2, 4, SEED)


def test_non_positive_temperature_is_skipped_and_not_counted():
    cur, f, best, b = _state(4, [1.0, 2.0, 3.0, 4.0])
    for T in ([0.0, 1.0, 1.0, 1.0], [1.0, -2.0, 1.0, 1.0]):
        c, cf, _, _, tried, acc = annealing.replica_exchange(cur, f, best, b, T, 0, 1, SEED)
        assert (tried, acc) == (1, 1) and _ids(c) == [0, 1, 3, 2], T


def test_the_metropolis_case_follows_the_exported_uniform():
    # d = (E0 - E1)(1/T0 - 1/T1) = (1)(1 - 2) = -1: swap iff u < exp(-1); both outcomes occur over its
    outcomes = set()
    for it in range(12):
        cur, f, best, b = _state(2, [2.0, 1.0])
        c, _, _, _, tried, acc = annealing.replica_exchange(cur, f, best, b, [1.0, 0.5], it, 1, SEED)
        if it % 2 == 1:                             # odd exchange number: K = 2 has no odd pair
            assert tried == 0
            continue
        want = _uniform53(SEED, it, 0, 1) < np.exp(-1.0)
        assert tried == 1 and acc == int(want) and _ids(c) == ([1, 0] if want else [0, 1]), it
        outcomes.add(bool(want))
    assert outcomes == {True, False}


def test_best_update_margin():
    # chain 1 receives energy 1.0.  best 1.0 + 5e-13: 1.0 + 1e-12 < best is false -> kept;
    # best 1.0 + 2e-12: true -> the received state becomes its best, genome and energy
    for best1, updated in ((1.0 + 5e-13, False), (1.0 + 2e-12, True)):
        cur, f, best, b = _state(2, [1.0, 3.0], bests=[0.5, best1])
        c, cf, bb, bf, tried, acc = annealing.replica_exchange(cur, f, best, b, [1.0, 1.0], 0, 1, SEED)
        assert acc == 1 and _ids(c) == [1, 0]
        assert bf[0] == 0.5 and (bb[0] == 100).all()        # chain 0 got the worse state
        if updated:
            assert bf[1] == 1.0 and (bb[1] == 0).all()
        else:
            assert bf[1] == best1 and (bb[1] == 101).all()


def test_all_pairs_are_decided_from_the_pre_exchange_state():
    # equal temperatures, K = 4, even exchange: both pairs swap; a sequential rule that
    # re-read chain 2 after pair (0, 1) would be the same here, so also check that an odd
    # exchange moves chain 1's PRE-exchange state to chain 2 and nothing travels two places
    cur, f, best, b = _state(4, [4.0, 3.0, 2.0, 1.0])
    c, cf, _, _, _, _ = annealing.replica_exchange(cur, f, best, b, [1.0] * 4, 1, 1, SEED)   # e = 1
    assert _ids(c) == [0, 2, 1, 3] and cf.tolist() == [4.0, 2.0, 3.0, 1.0]
    c, cf, _, _, _, _ = annealing.replica_exchange(cur, f, best, b, [1.0] * 4, 0, 1, SEED)   # e = 0
    assert _ids(c) == [1, 0, 3, 2] and cf.tolist() == [3.0, 4.0, 1.0, 2.0]
    # d of pair (2, 3) uses E_2 = 2.0 and E_3 = 1.0 whatever pair (0, 1) did: a hot/cold pair
    # that refuses on the pre-exchange energies (hot chain 2 worse) refuses
    T = [1.0, 1.0, 1.0, 1e-6]
    c, _, _, _, tried, acc = annealing.replica_exchange(cur, f, best, b, T, 0, 1, SEED)
    assert (tried, acc) == (2, 1) and _ids(c) == [1, 0, 2, 3]


def test_chain_seeds_keep_the_run_seed_for_chain_0():
    assert annealing.chain_seeds(5, 3) == [5, 6, 7]
    assert annealing.chain_seeds(2**64 - 1, 2) == [2**64 - 1, 0]


def test_simulated_annealing_chains_argument_rules():
    kw = dict(target_img_uint8=np.zeros((8, 8, 3), np.uint8), H=8, W=8, device=None, n_splats=2, mutpb=0.1,
              mut_sigma_max=SIG, mut_sigma_min=SIG, sigma_schedule="cosine", min_scale_splats=3.0,
              max_scale_splats=0.1, k_sigma=3.0, mask_strength=0.5, boost_only=False, iterations=1, temp0=1.0,
              temp_schedule="exp", progress=False)
    with pytest.raises(ValueError, match="chains must be"):
        annealing.simulated_annealing(**kw, chains=0)
    with pytest.raises(ValueError, match="device backend"):
        annealing.simulated_annealing(**kw, chains=2, backend="host")
    with pytest.raises(ValueError, match="temp_ladder"):
        annealing.simulated_annealing(**kw, chains=2, temp_ladder=[1.0], seed=1)
    with pytest.raises(ValueError, match="at least one image"):
        annealing.simulated_annealing_many([], 8, 8, None, 2, 0.1, SIG, SIG, "cosine", 3.0, 0.1, 3.0, 0.5, False,
                                           1, 1.0, "exp")
