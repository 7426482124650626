"""The Adam refiner over K images (ggs_refine_create_targets, DeviceRefine with a
4-D target) on an MI355X: 64 x 64, N = 16, K = 3, group = 2, B = 6, six steps run as
2 + 4.  Everything ``read`` returns for candidate b is bytes-equal to a
single-target ``DeviceRefine`` on (genome b, image b // 2)."""
from __future__ import annotations

import numpy as np
import pytest

import ggs_oracle as oracle
from ggs import ga
from ggs.ga_device import DeviceRefine
from ggs.refine import DEFAULT_LR

pytestmark = pytest.mark.gpu
H = W = 64
N, K, GROUP = 16, 3, 2
B = K * GROUP
MIN_S, MAX_S = 0.5, 0.5
KEYS = ("genomes", "fitness", "best", "best_fits", "last_grad")


def _run(target, mask, G, **kw):
    s = DeviceRefine(target, mask, G, lr=DEFAULT_LR, min_scale_splats=MIN_S, max_scale_splats=MAX_S, **kw)
    try:
        s.run(2)
        mid = s.read()
        s.run(4)
        return mid, s.read()
    finally:
        s.close()


@pytest.mark.parametrize("masked", [True, False], ids=["weighted", "none"])
def test_a_candidate_is_the_single_target_session_on_its_image(masked):
    rng = np.random.default_rng(11)
    G = ga.clamp_genome(oracle.synthetic_population(B, N, H, W, seed=4), H, W, MIN_S, MAX_S)
    targets = rng.uniform(0, 1, (K, H, W, 3)).astype(np.float32)
    masks = rng.uniform(0.2, 1.0, (K, H, W)).astype(np.float32) if masked else None
    mid, end = _run(targets, masks, G, group=GROUP)
    assert (end["best_fits"] <= mid["best_fits"]).all() and np.abs(end["last_grad"]).max() > 0
    for b in range(B):
        k = b // GROUP
        smid, send = _run(targets[k], None if masks is None else masks[k], G[b:b + 1])
        for key in KEYS:
            assert mid[key][b].tobytes() == smid[key][0].tobytes(), (b, key, "after 2 steps")
            assert end[key][b].tobytes() == send[key][0].tobytes(), (b, key, "after 6 steps")
    # the images differ: candidate 2 (image 1) against image 0 goes elsewhere
    _, other = _run(targets[0], None if masks is None else masks[0], G[2:3])
    assert other["fitness"][0] != end["fitness"][2]
