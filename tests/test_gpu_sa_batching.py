"""The SA round driver's batching does not show in the trajectory (csrc/ggs_sess_sa.cpp).

The rounds-per-sync cap (GGS_SA_MAX_ROUNDS_PER_SYNC) is read once per process, so
each setting runs in a fresh child: a lone ``DeviceSA`` and a three-chain
``DeviceSAChains`` at tests/test_gpu_sa_chains.py's shape and constants (24 x 24,
12 splats, capacity 4, 3 tries, 12 iterations, hot / cold / cosine temperatures,
adaptive width), each in two ``run`` calls.  The curves and the current and best
genomes must be the same bits at a sync after every round, after every second
round and at the default cap, and the lone session must be chain 0 of the group.
The ``rounds`` counters depend on the cadence and are not compared.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

import ggs

pytestmark = pytest.mark.gpu

_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_sa_chains as T
H = W = 24
K, N = 3, 12
targets, masks = T._problem(H, W, 1, 11)
inits, seeds, temps = T._inits(K, N, H, W, 40), [7 + 1000 * k for k in range(K)], T._temps(K)
sha = lambda a: hashlib.sha256(T.np.ascontiguousarray(a).tobytes()).hexdigest()
g = T._group(targets[0], masks[0], inits, seeds, temps)
s = T._session(targets[0], masks[0], inits[0], seeds[0], temps[0])
assert g["curves"].shape == (K, T.ITERS, 2) and s["curves"].shape == (T.ITERS, 2)
print(json.dumps({"group": {k: sha(g[k]) for k in ("curves", "cur", "best")},
                  "chain0": {k: sha(g[k][0]) for k in ("curves", "cur", "best")},
                  "lone": {k: sha(s[k]) for k in ("curves", "cur", "best")}}))
"""


def _child(cap):
    env = dict(os.environ)
    env.pop("GGS_SA_MAX_ROUNDS_PER_SYNC", None)
    if cap is not None:
        env["GGS_SA_MAX_ROUNDS_PER_SYNC"] = str(cap)
    pkg = os.path.dirname(os.path.dirname(ggs.__file__))
    r = subprocess.run([sys.executable, "-c", _CHILD, pkg, os.path.dirname(__file__)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_trajectory_does_not_depend_on_rounds_per_sync():
    outs = {cap: _child(cap) for cap in (1, 2, None)}
    for cap, o in outs.items():
        assert o["lone"] == o["chain0"], f"cap {cap}: the lone session is not chain 0"
    assert outs[1] == outs[None], "a sync after every round changed the trajectory"
    assert outs[2] == outs[None], "a sync after every second round changed the trajectory"
