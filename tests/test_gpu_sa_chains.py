"""SA chain groups on the GPU (ggs_sa_chains_*, ggs.ga_device.DeviceSAChains).

Every comparison is exact.  Every group is run in two ``run`` calls, so the
continuation of a chunk is covered everywhere.

1. A chain is a session: chain k of a group, shared target or a target per
   chain, equals ``DeviceSA(targets[k], masks[k], inits[k], seed=seeds[k])`` run
   with ``temps[k]`` — genomes, energies, curves, accepted count — with the chains
   pushed out of step (one hot, one so cold that only improvements pass).
2. The group's trajectory does not depend on the round width.
3. Replica exchange is ``ggs.annealing.replica_exchange`` applied between chunks.
4. ``simulated_annealing(chains=K)`` and ``simulated_annealing_many``.
"""
from __future__ import annotations

import numpy as np
import pytest

from ggs import annealing as A
from ggs import ga
from ggs.ga_device import DeviceSA, DeviceSAChains
from ggs.mask import compute_importance_mask, prepare_target

pytestmark = pytest.mark.gpu
SIG_MAX = {"xy": 0.1, "alog": 0.5, "blog": 0.5, "theta": 0.3, "rgb": 25.0, "alpha": 25.0}
SIG_MIN = {"xy": 0.01, "alog": 0.05, "blog": 0.05, "theta": 0.025, "rgb": 2.0, "alpha": 2.0}
MIN_S, MAX_S = 3.0, 0.1
KW = dict(mutpb=0.2, mut_sigma_max=SIG_MAX, mut_sigma_min=SIG_MIN, schedule="cosine",
          min_scale_splats=MIN_S, max_scale_splats=MAX_S)
TRIES, ITERS, CAP, SPLIT = 3, 12, 4, 5
HOT, COLD = 1.0, 1e-12          # accepts almost everything / only improvements pass


def _problem(H, W, K, seed):
    rng = np.random.default_rng(seed)
    targets = np.stack([prepare_target(rng.uniform(0, 255, (H + 9, W + 5, 3)).astype(np.float32), H, W)
                        for _ in range(K)])
    masks = np.stack([compute_importance_mask(t, H, W, smooth=3, strength=0.7) for t in targets])
    return targets, masks


def _inits(K, N, H, W, seed):
    return np.stack([ga.new_population(1, N, H, W, MIN_S, MAX_S, np.random.default_rng(seed + k))[0]
                     for k in range(K)])


def _temps(K, n=ITERS):
    """Chain 0 hot, chain 1 cold, the others on a cosine schedule between the two."""
    rows = [[HOT] * n, [COLD] * n] + [[A.temp_schedule("cosine", 2e-3 * k, i, n) for i in range(n)]
                                      for k in range(2, K)]
    return np.asarray(rows[:K], np.float64)


def _run2(sa, temps, width=0, first=0):
    """Iterations first .. first + n - 1 in two ``run`` calls."""
    t = np.atleast_2d(temps) if isinstance(sa, DeviceSAChains) else temps
    n = t.shape[-1]
    s = min(SPLIT, n - 1)
    a = sa.run(first, t[..., :s], ITERS, TRIES, width)
    b = sa.run(first + s, t[..., s:], ITERS, TRIES, width)
    return np.concatenate([a, b], axis=-2)


def _session(target, mask, init, seed, temps):
    sa = DeviceSA(target, mask, init, max_tries=CAP, seed=seed, **KW)
    try:
        curves = _run2(sa, temps)
        cur, best, _ = sa.read()
        return dict(curves=curves, cur=cur, best=best, st=sa.loop_state(), init_fit=sa.init_fit)
    finally:
        sa.close()


def _group(target, mask, inits, seeds, temps, width=0, **kw):
    sa = DeviceSAChains(target, mask, inits, seeds, max_tries=CAP, **KW, **kw)
    try:
        curves = _run2(sa, temps, width)
        cur, best = sa.read()
        return dict(curves=curves, cur=cur, best=best, st=sa.loop_state(), init_fits=sa.init_fits)
    finally:
        sa.close()


# (H, W, K, N): partial tile and odd K; the N < 2 swap exit; three 256-splat mutate blocks and the
# saturation raster instances; a single-chain group
SHAPES = [(40, 40, 3, 33), (24, 24, 2, 1), (40, 40, 2, 700), (24, 24, 1, 5)]


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "targets"])
@pytest.mark.parametrize("H,W,K,N", SHAPES)
def test_a_chain_is_a_session(H, W, K, N, per_chain):
    targets, masks = _problem(H, W, K, 11)
    inits, seeds, temps = _inits(K, N, H, W, 40), [7 + 1000 * k for k in range(K)], _temps(K)
    g = _group(targets if per_chain else targets[0], masks if per_chain else masks[0], inits, seeds, temps)
    for k in range(K):
        kt = k if per_chain else 0
        s = _session(targets[kt], masks[kt], inits[k], seeds[k], temps[k])
        np.testing.assert_array_equal(g["cur"][k], s["cur"], err_msg=f"chain {k}")
        np.testing.assert_array_equal(g["best"][k], s["best"], err_msg=f"chain {k}")
        np.testing.assert_array_equal(g["curves"][k], s["curves"], err_msg=f"chain {k}")
        assert g["init_fits"][k] == np.float32(s["init_fit"])
        assert g["st"]["best_fit"][k] == s["st"]["best_fit"]
        assert g["st"]["current_fit"][k] == s["st"]["current_fit"]
        assert int(g["st"]["accepted"][k]) == s["st"]["accepted"]
    st = g["st"]
    assert st["swaps_tried"] == 0 and st["swaps_accepted"] == 0
    if K >= 2:
        # out of step: the hot chain consumes one try per round, the cold one a whole width
        assert len(set(int(r) for r in st["rounds"][:2])) == 2, st["rounds"]


@pytest.mark.parametrize("per_chain", [False, True], ids=["shared", "targets"])
def test_width_invariance(per_chain):
    H, W, K, N = SHAPES[0]
    targets, masks = _problem(H, W, K, 11)
    inits, seeds, temps = _inits(K, N, H, W, 40), [7 + 1000 * k for k in range(K)], _temps(K)
    t, m = (targets, masks) if per_chain else (targets[0], masks[0])
    outs = [_group(t, m, inits, seeds, temps, width=w) for w in (1, 3, CAP, 0)]
    for o in outs[1:]:
        for key in ("cur", "best", "curves"):
            np.testing.assert_array_equal(o[key], outs[0][key])
        for key in ("best_fit", "current_fit", "accepted"):
            np.testing.assert_array_equal(o["st"][key], outs[0]["st"][key])
    # width 1: a round is one try of every unfinished chain
    np.testing.assert_array_equal(outs[0]["st"]["evaluated"], outs[0]["st"]["rounds"])
    assert (outs[0]["st"]["rounds"] == ITERS * TRIES).all()


# ---- replica exchange -------------------------------------------------------------------------
M = 4
XSEED = 2024
# Chains 0 and 1 share a temperature (their pair always swaps), chains 2 and 3 are a hot / cold pair
# (it refuses whenever the hot chain holds the worse state); all chains start from ONE individual, so
# after M iterations the cold chain, which only ever improved on it, is below the hot one, which
# accepted every mutation.  K = 3 keeps chains 0 .. 2: exchange 0 has the pair (0, 1), exchange 1
# the pair (1, 2) — cold-ish against hot.
# Seeds 300 + 17 k (target seed 3, init seed 5) were checked beforehand without a GPU: the host SA
# steps (ggs.ga.mutate_batch) on the oracle evaluator at 24 x 24, fed the Philox draws of these seeds
# restated in numpy (tests/_philox.py), M iterations per chain, end at the energies 0.4819, 0.4555,
# 0.5522, 0.4555: chain 0 has moved (the swap of pair (0, 1) is visible), and the hot chain 2 is 0.097
# above the cold chain 3, so d = -9.7e5 and exp(d) underflows to 0 whatever the uniform: K = 4 counts
# one swap and one refusal at its first exchange.
XTEMPS = [2e-2, 2e-2, HOT, 1e-7]
XSEEDS = [300, 317, 334, 351]
XH = XW = 24
XN = 12


def _xgroup(t, m, inits, K, exchange):
    return DeviceSAChains(t, m, inits, XSEEDS[:K], max_tries=CAP, exchange_every=M if exchange else 0,
                          exchange_seed=XSEED, **KW)


def _read(sa):
    cur, best = sa.read()
    st = sa.loop_state()
    return cur, st["current_fit"].copy(), best, st["best_fit"].copy(), st


XCOUNTS = {}


@pytest.mark.parametrize("K", [4, 3])
def test_exchange_is_the_numpy_statement(K):
    targets, masks = _problem(XH, XW, 1, 3)
    t, m = targets[0], masks[0]
    one = ga.new_population(1, XN, XH, XW, MIN_S, MAX_S, np.random.default_rng(5))[0]
    inits = np.repeat(one[None], K, axis=0)
    temps = np.repeat(np.asarray(XTEMPS[:K], np.float64)[:, None], 2 * M, axis=1)
    total = 2 * M

    def run(sa, first, tt):
        """[first, first + n) in two calls (the exchange falls at the end of the second)."""
        a = sa.run(first, tt[:, :2], total, TRIES)
        b = sa.run(first + 2, tt[:, 2:], total, TRIES)
        return np.concatenate([a, b], axis=1)

    x = _xgroup(t, m, inits, K, True)
    y = _xgroup(t, m, inits, K, False)
    try:
        # iterations 0 .. M - 1, then exchange 0 (even pairs)
        cvx1 = run(x, 0, temps[:, :M])
        cvy1 = run(y, 0, temps[:, :M])
        np.testing.assert_array_equal(cvx1, cvy1)         # curves already written are not touched
        x1 = _read(x)
        yc, ycf, yb, ybf, _ = _read(y)
        want = A.replica_exchange(yc, ycf, yb, ybf, temps[:, M - 1], M - 1, M, XSEED)
        for got, w in zip(x1[:4], want[:4]):
            np.testing.assert_array_equal(got, w)
        assert (x1[4]["swaps_tried"], x1[4]["swaps_accepted"]) == want[4:]
        assert want[5] >= 1, "the equal-temperature pair (0, 1) always swaps"
        assert not np.array_equal(x1[0][0], yc[0])
        # iterations M .. 2M - 1 from the exchanged state: a fresh group without exchange, started there
        cvx2 = run(x, M, temps[:, M:])
        z = DeviceSAChains(t, m, x1[0], XSEEDS[:K], max_tries=CAP, **KW)
        try:
            np.testing.assert_array_equal(z.init_fits.astype(np.float64), x1[1])
            cvz = run(z, M, temps[:, M:])
            zc, zcf, zb, zbf, _ = _read(z)
        finally:
            z.close()
        np.testing.assert_array_equal(cvx2[:, :, 1], cvz[:, :, 1])
        # exchange 1 (odd pairs) at the end.  The group's pre-exchange best is its best-energy curve's
        # last row; its genome is z's best where z reached that energy, else the best it had at M
        pre_bf = cvx2[:, -1, 0]
        pre_b = np.empty_like(zb)
        for k in range(K):
            if pre_bf[k] == zbf[k]:
                pre_b[k] = zb[k]
            else:
                assert pre_bf[k] == x1[3][k], (k, pre_bf[k], zbf[k], x1[3][k])
                pre_b[k] = x1[2][k]
        want2 = A.replica_exchange(zc, zcf, pre_b, pre_bf, temps[:, 2 * M - 1], 2 * M - 1, M, XSEED)
        x2 = _read(x)
        for got, w in zip(x2[:4], want2[:4]):
            np.testing.assert_array_equal(got, w)
        assert x2[4]["swaps_tried"] == want[4] + want2[4]
        assert x2[4]["swaps_accepted"] == want[5] + want2[5]
        XCOUNTS[K] = (x2[4]["swaps_tried"], x2[4]["swaps_accepted"])
    finally:
        x.close()
        y.close()
    if len(XCOUNTS) == 2:       # over the two cases: at least one swap and at least one refusal
        tried = sum(v[0] for v in XCOUNTS.values())
        acc = sum(v[1] for v in XCOUNTS.values())
        assert acc >= 1 and tried - acc >= 1, XCOUNTS


# ---- Python surface ---------------------------------------------------------------------------
def _sa_kw(**over):
    kw = dict(mutpb=0.2, mut_sigma_max=SIG_MAX, mut_sigma_min=SIG_MIN, sigma_schedule="cosine",
              min_scale_splats=MIN_S, max_scale_splats=MAX_S, k_sigma=3.0, mask_strength=0.7, boost_only=False,
              iterations=6, temp0=2e-3, temp_schedule="cosine", tries_per_iter=3, progress=False,
              return_state=True, speculate=4, chunk=4)
    kw.update(over)
    return kw


def test_simulated_annealing_chains():
    H = W = 24
    img = np.random.default_rng(2).uniform(0, 255, (30, 28, 3)).astype(np.float32)
    b3, f3, st3 = A.simulated_annealing(img, H, W, "cuda", 9, seed=50, chains=3, **_sa_kw())
    fits = [c["best_fit"] for c in st3["chains"]]
    assert f3 == min(fits) and st3["best_chain"] == int(np.argmin(fits))
    np.testing.assert_array_equal(b3, st3["chains"][st3["best_chain"]]["best"])
    # chain k is the lone run of seed 50 + k; chain 0 keeps the run's seed
    for k in range(3):
        b1, f1, st1 = A.simulated_annealing(img, H, W, "cuda", 9, seed=50 + k, **_sa_kw())
        c = st3["chains"][k]
        np.testing.assert_array_equal(c["best"], b1)
        np.testing.assert_array_equal(c["current"], st1["current"])
        assert c["best_fit"] == f1 and c["curves"] == st1["curves"]
        assert c["accepted"] == st1["stats"]["accepted"]
    # a ladder and exchange: runs, counts its exchanges, and returns the minimum
    b, f, st = A.simulated_annealing(img, H, W, "cuda", 9, seed=50, chains=3, temp_ladder=[1.0, 1.0, 50.0],
                                     exchange_every=2, **_sa_kw())
    assert f == min(c["best_fit"] for c in st["chains"])
    assert st["stats"]["swaps_tried"] == 3          # exchanges 0, 1, 2 of 6 iterations: one pair each


@pytest.mark.parametrize("prep", ["host", "device"])
def test_simulated_annealing_many(prep):
    H = W = 24
    rng = np.random.default_rng(4)
    images = [rng.uniform(0, 255, s).astype(np.float32) for s in ((30, 28, 3), (24, 24, 3), (41, 35, 3))]
    out = A.simulated_annealing_many(images, H, W, "cuda", 9, seed=70, prep=prep,
                                     **{k: v for k, v in _sa_kw().items()})
    assert len(out) == 3
    if prep == "device":        # targets within 2e-5 of the host's: another (valid) trajectory
        for best, f, st in out:
            assert best.shape == (9, 9) and np.isfinite(f) and f == st["curves"]["best"][-1]
        return
    for k, (best, f, st) in enumerate(out):
        b1, f1, st1 = A.simulated_annealing(images[k], H, W, "cuda", 9, seed=70 + k, **_sa_kw())
        np.testing.assert_array_equal(best, b1)
        np.testing.assert_array_equal(st["current"], st1["current"])
        assert f == f1 and st["curves"] == st1["curves"] and st["current_fit"] == st1["current_fit"]
