"""What the six device-resident session types share (csrc/ggs_host.h ``Session``) on an
MI355X:

* a session of any kind, created through any of the nine create entry points, stepped
  once, read and destroyed, leaves the context's pool of per-stream workspaces as it
  found it (``ggs_workspace_count``; free device memory cannot serve on a shared GPU);
* a refine session created after a GA session on another target was destroyed scores
  its candidates against its own target: the two are the first sessions of their kinds
  in a fresh process, where their plan keys used to coincide, and the refiner's stream
  may get the handle of the GA's.
"""
from __future__ import annotations

import subprocess
import sys

import numpy as np
import pytest

import ggs
import ggs_oracle as oracle
from conftest import ORACLE, PKG
from ggs import _lib, api, ga
from ggs.ga_device import DeviceDE, DeviceGA, DeviceGAIslands, DeviceRefine, DeviceSA, DeviceSAChains
from ggs.refine import DEFAULT_LR

pytestmark = pytest.mark.gpu
H, W = 33, 47                   # no multiple of the tile in either direction
N, P, E, K, B = 5, 6, 2, 2, 3   # splats, population (DE needs >= 4), elites, islands / chains / targets, refine candidates
MIN_S, MAX_S = 0.5, 0.5
ZERO = dict.fromkeys(("xy", "alog", "blog", "theta", "rgb", "alpha"), 0.0)
SMAX = dict(xy=0.05, alog=0.2, blog=0.2, theta=0.3, rgb=20.0, alpha=20.0)
SCALE = dict(min_scale_splats=MIN_S, max_scale_splats=MAX_S)
MUT = dict(mutpb=0.3, mut_sigma_max=SMAX, mut_sigma_min=ZERO, schedule="linear", **SCALE)
GA = dict(tour_k=2, elite_k=E, cxpb=0.5, **MUT)


def _inputs():
    rng = np.random.default_rng(7)
    pops = ga.clamp_genome(oracle.synthetic_population(K * P, N, H, W, seed=7), H, W, MIN_S, MAX_S)
    targets = rng.uniform(0, 1, (K, H, W, 3)).astype(np.float32)
    masks = rng.uniform(0.2, 1.0, (K, H, W)).astype(np.float32)
    return pops.reshape(K, P, N, 9), targets, masks


def _ga(pops, t, m):
    s = DeviceGA(t[0], m[0], pops[0], seed=3, **GA)
    s.run(1, 1, 4)
    return s


def _islands(pops, t, m):
    s = DeviceGAIslands(t, m, pops, [3, 4], **GA)
    s.run(1, 1, 4)
    return s


def _sa(pops, t, m):
    s = DeviceSA(t[0], m[0], pops[0, 0], max_tries=P, seed=3, **MUT)
    s.run(0, [0.01], 4, 2)
    return s


def _chains(pops, t, m):
    s = DeviceSAChains(t, m, pops[:, 0], [3, 4], max_tries=P, **MUT)
    s.run(0, np.full((K, 1), 0.01), 4, 2)
    return s


def _de(pops, t, m):
    s = DeviceDE(t[0], m[0], pops[0], seed=3, **SCALE)
    s.run(1, 1)
    return s


def _refine(pops, t, m, **kw):
    s = DeviceRefine(t, m, pops[0, :B], lr=DEFAULT_LR, **SCALE, **kw)
    s.run(1)
    return s


CREATES = {
    "ggs_ga_create": _ga,
    "ggs_ga_islands_create": lambda p, t, m: _islands(p, t[0], m[0]),
    "ggs_ga_islands_create_targets": _islands,
    "ggs_sa_create": _sa,
    "ggs_sa_chains_create": lambda p, t, m: _chains(p, t[0], m[0]),
    "ggs_sa_chains_create_targets": _chains,
    "ggs_de_create": _de,
    "ggs_refine_create": lambda p, t, m: _refine(p, t[0], m[0]),
    "ggs_refine_create_targets": lambda p, t, m: _refine(p, t, m, group=B),
    "ggs_refine_create_loss": lambda p, t, m: _refine(p, t, None, group=B, loss=ggs.LossParams(0.8, 0.0, 0.2)),
}


def _count() -> int:
    n = _lib.lib.ggs_workspace_count(0)
    assert n >= 0, _lib.last_error()
    return n


@pytest.mark.parametrize("entry", sorted(CREATES))
def test_sessions_leave_no_workspace(entry):
    """At the parent of the session base this failed for ggs_ga_create alone: its
    initial evaluation made a workspace for the session's stream that no destroy released."""
    pops, targets, masks = _inputs()
    ggs.ensure_init()
    before = _count()
    s = CREATES[entry](pops, targets, masks)
    s.read()
    s.close()
    assert _count() == before, entry


_CHILD = r'''
import sys
sys.path[:0] = [{pkg!r}, {oracle!r}, {tests!r}]
import numpy as np
import test_gpu_sessions as T
from ggs import api
pops, targets, masks = T._inputs()
T.DeviceGA(targets[0], masks[0], pops[0], seed=3, **T.GA).close()      # target A, its plan in the stream's workspace
s = T.DeviceRefine(targets[1], masks[1], pops[0, :T.B], lr=T.DEFAULT_LR, **T.SCALE)   # target B, no step taken
got = s.read()["fitness"]
s.close()
want = api.fitness(pops[0, :T.B], targets[1], T.H, T.W, 3.0, weight_mask=masks[1])
print("GOT", got.tobytes().hex())
print("WANT", want.tobytes().hex())
'''


def test_refine_after_ga_scores_its_own_target():
    import os
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD.format(pkg=PKG, oracle=ORACLE, tests=tests)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict(l.split(" ", 1) for l in r.stdout.splitlines() if l.startswith(("GOT", "WANT")))
    # the lone session's comparison of test_gpu_refine.py: the host fitness, bit for bit
    assert out["GOT"] == out["WANT"]
