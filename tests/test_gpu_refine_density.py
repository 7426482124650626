"""Density control inside a refine session (ggs_refine_set_density) on an
MI355X: 12 steps with ``every = 4``, ``start = 4`` at 33 x 47 (height x width), N = 24, on each
of the three session kinds.  Three alphas per candidate are planted at 0 and ``alpha_dead`` is
16, so Adam's ``lr[8] = 2`` cannot revive them before step 4; ``max_moves = 1`` leaves dead splats
for the later events.  Even candidates start with every log-scale below ``split_log`` (their
first pair is a clone), odd ones above it (a split).

Each session is held, bit for bit after every step, to the host loop ``api.fitness_grad`` /
``api.loss_grad`` -> ``density_accumulate`` -> ``adam_step`` -> ``relocate``: genomes, fitness,
best, best_fits, last_grad and ``density_stats()``.  A run in which nothing relocates fails."""
from __future__ import annotations

import numpy as np
import pytest

import ggs
import ggs_oracle as oracle
from ggs import api, ga
from ggs.ga_device import DeviceRefine
from ggs.refine import DEFAULT_LR, AdamParams, DensityParams, adam_step, density_accumulate, density_moves, relocate

pytestmark = pytest.mark.gpu
H, W, N = 33, 47, 24
MIN_S, MAX_S = 0.5, 0.5
LOSS = ggs.LossParams(0.8, 0.0, 0.2)
BG = (0.9, 0.8, 0.7)
SPLIT_LOG = 1.5
DENSITY = DensityParams(every=4, start=4, stop=0, max_moves=1, alpha_dead=16.0, grad_min=0.0, split_log=SPLIT_LOG,
                        shrink=1.6, split_offset=0.5)
KEYS = ("genomes", "fitness", "best", "best_fits", "last_grad")


def _problem(B):
    G = np.ascontiguousarray(ga.clamp_genome(oracle.synthetic_population(B, N, H, W, seed=21), H, W, MIN_S, MAX_S))
    rng = np.random.default_rng(22)
    G[0::2, :, 2:4] = np.minimum(G[0::2, :, 2:4], np.float32(SPLIT_LOG - 0.5))    # clones first
    G[1::2, :, 2:4] = np.maximum(G[1::2, :, 2:4], np.float32(SPLIT_LOG + 0.5))    # splits first
    tg = np.stack([oracle.render(oracle.genome_to_renderer_batched(
        oracle.synthetic_population(1, 10, H, W, seed=30 + k)), H, W, k_sigma=3.0)[0] for k in range(2)])
    tg = np.clip(tg + rng.normal(0, 0.03, tg.shape), 0, 1).astype(np.float32)
    mask = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    for b in range(B):
        # A splat of alpha 0 has no gradient but alpha's.  Its colour is the far end from the
        # target under its centre (candidate b's image is b // group = b // 2; the one-target
        # session's is image 0 and has two candidates), so more of it raises the error, Adam
        # pushes alpha against the clamp at 0 and the splats not yet relocated stay dead for the
        # events at steps 8 and 12.
        for s in rng.permutation(N)[:N // 8]:
            px, py = int(round(float(G[b, s, 0]) * (W - 1))), int(round(float(G[b, s, 1]) * (H - 1)))
            G[b, s, 5:8] = np.where(tg[min(b // 2, 1), py, px] < 0.5, 255.0, 0.0)
            G[b, s, 8] = 0.0
    return G, tg, mask


def _kind(name):
    """→ genomes, the session's keyword arguments (target, mask, ...), the host gradient call."""
    if name == "single_weighted":
        G, tg, mask = _problem(2)
        return G, dict(target=tg[0], mask=mask), lambda x: api.fitness_grad(x, tg[0], H, W, 3.0, weight_mask=mask)
    if name == "targets":
        G, tg, _ = _problem(4)
        return G, dict(target=tg, mask=None, group=2), lambda x: api.fitness_grad(x, tg, H, W, 3.0, group=2)
    G, tg, _ = _problem(4)
    return (G, dict(target=tg, mask=None, group=2, loss=LOSS, background=BG),
            lambda x: api.loss_grad(x, tg, H, W, LOSS, k_sigma=3.0, background=BG, layout="axes", group=2))


def _session(G, target, mask, **kw):
    return DeviceRefine(target, mask, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S, **kw)


class HostLoop:
    """The numpy statement of a session with density control on from step ``on_from``."""

    def __init__(self, G, grad_fn, density, on_from=1):
        lo, hi = ga.scale_log_bounds(H, W, MIN_S, MAX_S)
        self.p = AdamParams(lr=DEFAULT_LR, log_lo=lo, log_hi=hi)
        self.grad_fn, self.d, self.on_from = grad_fn, density, on_from
        self.x, self.m, self.v = G.copy(), np.zeros_like(G), np.zeros_like(G)
        self.t = 0
        first, _ = grad_fn(G)
        self.best, self.best_x = first.astype(np.float64), G.copy()
        self.fit, self.grad = first, np.zeros_like(G)
        B = G.shape[0]
        M = density_moves(density, N)
        self.acc, self.n_acc = np.zeros((B, N), np.float32), 0
        self.moves, self.splits = np.zeros(B, np.int64), np.zeros(B, np.int64)
        self.last_pairs, self.last_n = np.full((B, M, 2), -1, np.int32), np.zeros(B, np.int32)
        self.events = []                                       # (t, pairs moved, of them splits)

    def step(self):
        self.t += 1
        t, d = self.t, self.d
        _, self.grad = self.grad_fn(self.x)
        on = t >= self.on_from and d.every > 0
        if on:
            self.acc = density_accumulate(self.acc, self.grad, H, W)
            self.n_acc += 1
        self.x, self.m, self.v = adam_step(self.x, self.grad, self.m, self.v, t, self.p)
        if on and t % d.every == 0 and t >= d.start and (d.stop == 0 or t <= d.stop):
            self.x, self.m, self.v, pairs, is_split = relocate(self.x, self.m, self.v, self.acc, self.n_acc, H, W, d,
                                                               self.p.log_lo, self.p.log_hi)
            self.last_pairs = pairs
            self.last_n = (pairs[:, :, 0] >= 0).sum(1).astype(np.int32)
            self.moves += self.last_n
            self.splits += is_split.sum(1)
            self.acc, self.n_acc = np.zeros_like(self.acc), 0
            self.events.append((t, int(self.last_n.sum()), int(is_split.sum())))
        self.fit, _ = self.grad_fn(self.x)
        better = self.fit.astype(np.float64) + 1e-10 < self.best
        self.best = np.where(better, self.fit.astype(np.float64), self.best)
        self.best_x[better] = self.x[better]

    def check(self, s, stats=True):
        r, t = s.read(), self.t
        want = dict(genomes=self.x, fitness=self.fit, best=self.best_x, best_fits=self.best.astype(np.float32),
                    last_grad=self.grad)
        for k in KEYS:
            assert r[k].tobytes() == want[k].tobytes(), (k, t)
        if stats:
            st = s.density_stats()
            assert st["acc"].tobytes() == self.acc.tobytes() and st["n_acc"] == self.n_acc, t
            assert st["moves"].tobytes() == self.moves.tobytes() and st["splits"].tobytes() == self.splits.tobytes(), t
            assert st["last_pairs"].tobytes() == self.last_pairs.tobytes(), t
            assert st["last_n"].tobytes() == self.last_n.tobytes(), t


@pytest.mark.parametrize("kind", ["single_weighted", "targets", "loss"])
def test_twelve_steps_are_the_host_loop_bit_for_bit(kind):
    G, kw, grad_fn = _kind(kind)
    s = _session(G, **kw)
    try:
        s.set_density(DENSITY)
        host = HostLoop(G, grad_fn, DENSITY)
        host.check(s)
        for _ in range(12):
            s.run(1)
            host.step()
            host.check(s)
        print(kind, "events (t, moved, splits):", host.events, "moves", host.moves.tolist(), "alpha of the planted:",
              np.sort(host.x[..., 8], axis=1)[:, :3].tolist())
        # a run in which nothing relocates must fail: every event moved something, both ways over the run
        assert [t for t, _, _ in host.events] == [4, 8, 12]
        assert all(n >= 1 for _, n, _ in host.events), host.events
        n_moved, n_split = sum(n for _, n, _ in host.events), sum(k for _, _, k in host.events)
        assert 0 < n_split < n_moved, host.events
    finally:
        s.close()


def test_stop_takes_exactly_one_event_and_set_density_applies_from_the_next_step():
    G, kw, grad_fn = _kind("single_weighted")
    one = DENSITY._replace(stop=4)
    late = DENSITY._replace(every=2, start=0)
    s, s2 = _session(G, **kw), _session(G, **kw)
    try:
        s.set_density(one)
        host = HostLoop(G, grad_fn, one)
        # the second session runs three plain steps first, then turns it on between two runs
        host2 = HostLoop(G, grad_fn, late, on_from=4)
        s2.run(3)
        for _ in range(3):
            host2.step()
        host2.check(s2, stats=False)
        with pytest.raises(ggs.GGSInputError, match="off"):
            s2.density_stats()
        s2.set_density(late)
        for _ in range(12):
            s.run(1)
            host.step()
            host.check(s)
        assert [t for t, _, _ in host.events] == [4] and host.events[0][1] >= 1
        for _ in range(5):
            s2.run(1)
            host2.step()
            host2.check(s2)
        assert [t for t, _, _ in host2.events] == [4, 6, 8] and host2.events[0][1] >= 1
        assert s2.density_stats()["moves"].sum() == sum(n for _, n, _ in host2.events)
    finally:
        s.close()
        s2.close()


@pytest.mark.parametrize("kind", ["single_weighted", "targets", "loss"])
def test_off_is_the_plain_session_bytewise(kind):
    G, kw, _ = _kind(kind)
    sessions = [_session(G, **kw) for _ in range(4)]
    try:
        plain, none, zero, toggled = sessions
        none.set_density(None)
        zero.set_density(DENSITY._replace(every=0))
        toggled.set_density(DENSITY)               # on, and off again before any step
        toggled.set_density(None)
        for n in (2, 4):                           # past step 4, where an event would have been due
            reads = []
            for s in sessions:
                s.run(n)
                reads.append(s.read())
            for r in reads[1:]:
                for k in KEYS:
                    assert r[k].tobytes() == reads[0][k].tobytes(), k
        # a bad setting is refused and leaves the session as it was
        with pytest.raises(ggs.GGSInputError, match="max_moves"):
            plain.set_density(DENSITY._replace(max_moves=0))
    finally:
        for s in sessions:
            s.close()
