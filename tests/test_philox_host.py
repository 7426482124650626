"""The Philox restatement of tests/_philox.py and the new stage export's C
boundary, without a GPU.

* the restated generator gives Random123's Philox4x32-10 known-answer vectors
  and, on stream 8, ``ggs_sa_accept_uniform`` (host code of libggs);
* the counter map of one generation is injective: no Philox word feeds two
  different draws, apart from the two sharings the layout declares, and nothing
  but the acceptance uniform uses stream 8;
* the draw-source adapter hands the numpy GA exactly an exported dict;
* the two Box-Muller edge inputs (u1 = 1 and u1 = 2^-24) sit at the committed
  counters (found once by a search of 2^27 words, not at test time);
* ``ggs_ga_philox_draws`` rejects bad arguments before any device is touched.
"""
from __future__ import annotations

import numpy as np
import pytest

import _philox as X
import ggs
from ggs import _lib
from ggs.ga_device import MUTATION_KEYS, draws_from_host, philox_draws

# Random123 kat_vectors, philox4x32 10: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

# Box-Muller edge inputs: (seed, gen, o, s, pair index into _philox.NORMAL_PAIRS), found by
# searching the first words of all five pairs over gen = 0 .. 43690, o < 4, s < 64, streams
# 2-4 under seed 42 (2^27 words, searched once with _philox.block; the test only re-derives the
# two words).  tests/test_gpu_ga_philox.py runs the device at these counters.
EDGE_U1_ONE = (42, 9899, 0, 21, 1)       # a >> 8 == 0xFFFFFF: u1 = 1, r = 0 (4 such words in the range)
EDGE_U1_MIN = (42, 30542, 0, 40, 4)      # a >> 8 == 0: u1 = 2^-24, r = 5.768 (2 such words, both in pair 4)


def test_philox_known_answer_vectors():
    for ctr, key, want in KAT:
        got = X.philox4x32(*ctr, *key)
        assert tuple(int(v) for v in got) == want, (ctr, key)
    # vectorised over counters: the same blocks in one call
    c = np.array([k[0] for k in KAT[:1]] * 3, np.uint64).T
    got = X.philox4x32(c[0], c[1], c[2], c[3], 0, 0)
    assert all(int(got[i][j]) == KAT[0][2][i] for i in range(4) for j in range(3))


def test_restated_accept_uniform_is_the_librarys():
    from ggs.ga_device import PhiloxAcceptDraws
    for seed in (0, 42, 2**63 + 12345):
        d = PhiloxAcceptDraws(seed)
        for it in (0, 1, 7, 1000):
            for k in range(5):
                assert X.accept_uniform(seed, it, k) == d.accept_at(it, k), (seed, it, k)


def _word(seed, gen, w):
    stream, who, what, i = w
    return int(X.block(seed, gen, who, what, stream)[i])


@pytest.mark.parametrize("P,N,tour_k", [(7, 5, 3), (8, 1, 3)])
def test_counter_map_is_injective(P, N, tour_k):
    entries = list(X.layout(P, P, N, tour_k))
    assert all(w[0] in range(1, 8) for _, w in entries), "stream 8 is the acceptance uniform's alone"
    assert all(0 <= w[3] < 4 for _, w in entries)
    shared = {w: u for w, u in X.word_users(entries).items() if len(u) > 1}
    # the two deliberate sharings, and nothing else
    want = {}
    for pair in range(P // 2):                                    # pairs with two children
        for s in range(N):
            want[(X.S_CX, pair, s + 1, 0)] = [("cx_u", pair, s, "child", 2 * pair),
                                              ("cx_u", pair, s, "child", 2 * pair + 1)]
    if P % 2:                                                     # slot (2 * last + 1) mod P == 0
        last = P // 2
        for j in range(tour_k):
            want[(X.S_TOUR, 0, j, 0)] = [("tour", "pair", 0, "parent", 0, j),
                                         ("tour", "pair", last, "parent", 1, j)]
    assert shared == want
    # every draw of the export is fed: the layout names each slot the kernels consume
    fed = {d[0] for d, _ in entries}
    assert fed == {"u_xy", "u_ab", "u_t", "u_rgb", "u_a", "n_xy", "n_ab", "n_t", "n_rgba", "k_color", "k_xy",
                   "k_ab", "k_t", "swap_u", "cx", "cx_u", "tour"} | ({"swap_i"} if N >= 2 else set())


@pytest.mark.parametrize("P,N,tour_k,first", [(7, 5, 3, 0), (8, 1, 3, 0), (5, 4, 2, 3)])
def test_vectorised_draws_follow_the_layout(P, N, tour_k, first):
    """``draws`` (array arithmetic) against the layout walked word by word."""
    seed, gen, cxpb = 2**63 + 12345, 9, 0.5
    d = X.draws(seed, gen, P, P, N, tour_k, cxpb, first=first)
    done = set()
    for draw, w in X.layout(P, P, N, tour_k, first=first):
        f, x = draw[0], _word(seed, gen, w)
        u = np.float32((x >> 8) / 16777216.0)
        if f in ("u_xy", "u_ab", "u_t", "u_rgb", "u_a"):
            assert d[f][draw[1], draw[2], draw[3]] == u, draw
        elif f == "cx_u":
            assert d[f][draw[1], draw[2]] == u, draw
        elif f == "swap_u":
            assert d[f][draw[1]] == float(u), draw
        elif f in ("k_color", "k_xy", "k_ab"):
            assert d[f][draw[1]] == x % (2 * N), draw
        elif f == "k_t":
            assert d[f][draw[1]] == x % N, draw
        elif f == "swap_i":
            assert d[f][draw[1]] == x % (N - 1), draw
        elif f == "cx":
            assert d[f][draw[1]] == int(u < np.float32(cxpb)), draw
        elif f == "tour":
            assert d["tour_idx"][w[1], w[2]] == min(int(np.float32(u * np.float32(P))), P - 1), draw
        else:                                                     # a normal: its pair's two words
            o, s, pi = X._pair_of(draw)
            if (o, s, pi) in done:
                continue
            done.add((o, s, pi))
            st, ia, ib, d1, d2 = X.NORMAL_PAIRS[pi]
            a, b = _word(seed, gen, (st, first + o, s, ia)), _word(seed, gen, (st, first + o, s, ib))
            c, sn = X.box_muller(a, b)
            assert d[d1[0]][o, s, d1[1]] == c
            if d2 is not None:
                assert d[d2[0]][o, s, d2[1]] == sn
    assert np.array_equal(d["perm"], np.arange(P)) and (d["swap_pick"] == -1).all()
    if N < 2:
        assert (d["swap_i"] == 0).all()
    assert d["tour_idx"].min() >= 0 and d["tour_idx"].max() < P


def test_adapter_round_trip():
    """draws_from_host of what the adapter hands the numpy GA is the dict again."""
    P, N, k = 7, 5, 3
    rng = np.random.default_rng(0)
    n, np2 = P, (P + 1) // 2
    d = {"tour_idx": rng.integers(0, P, (P, k)).astype(np.int32), "perm": np.arange(P, dtype=np.int32),
         "cx": np.array([1, 0, 1, 1], np.int32), "cx_u": rng.random((np2, N), dtype=np.float32),
         "u_xy": rng.random((n, N, 2), dtype=np.float32), "u_ab": rng.random((n, N, 2), dtype=np.float32),
         "u_t": rng.random((n, N, 1), dtype=np.float32), "u_rgb": rng.random((n, N, 1), dtype=np.float32),
         "u_a": rng.random((n, N, 1), dtype=np.float32),
         "k_color": rng.integers(0, 2 * N, n).astype(np.int32), "k_xy": rng.integers(0, 2 * N, n).astype(np.int32),
         "k_ab": rng.integers(0, 2 * N, n).astype(np.int32), "k_t": rng.integers(0, N, n).astype(np.int32),
         "n_xy": rng.standard_normal((n, N, 2), dtype=np.float32),
         "n_ab": rng.standard_normal((n, N, 2), dtype=np.float32),
         "n_t": rng.standard_normal((n, N, 1), dtype=np.float32),
         "n_rgba": rng.standard_normal((n, N, 4), dtype=np.float32),
         "swap_i": rng.integers(0, N - 1, n).astype(np.int32), "swap_pick": np.full(n, -1, np.int32),
         "swap_u": rng.random(n)}
    d["cx_u"][d["cx"] == 0] = 1.0          # draws_from_host's filler for the pairs that do not cross
    a = X.ExportedDraws([d])
    tour = a.tournament(P, k)
    perm = a.shuffle(P)
    for cxpb in (0.5, 2.0 ** -10, 1.0):
        assert np.array_equal(a.uniform(np2) < cxpb, d["cx"] != 0)
    cx = a.uniform(np2) < 0.5
    cxu, mut = a.generation(cx, P, N, 0.25)
    assert cxu.shape == (int(cx.sum()), N, 1) and sorted(mut) == sorted(MUTATION_KEYS)
    back = draws_from_host(tour, perm, cx, cxu, mut, N)
    assert sorted(back) == sorted(d)
    for key in d:
        np.testing.assert_array_equal(np.asarray(back[key]).reshape(d[key].shape), d[key], err_msg=key)


@pytest.mark.parametrize("edge,top,u1,r", [(EDGE_U1_ONE, 0xFFFFFF, 1.0, 0.0),
                                           (EDGE_U1_MIN, 0, 2.0 ** -24, np.sqrt(48.0 * np.log(2.0)))])
def test_edge_words_are_where_the_search_found_them(edge, top, u1, r):
    seed, gen, o, s, pi = edge
    st, ia, ib, d1, _ = X.NORMAL_PAIRS[pi]
    w = X.block(seed, gen, o, s, st)
    assert int(w[ia]) >> 8 == top
    c, sn = X.box_muller(w[ia], w[ib])
    assert np.hypot(c, sn) == pytest.approx(r, abs=1e-12)          # r = sqrt(-2 ln u1); 5.768 at 2^-24
    d = X.draws(seed, gen, o + 1, 2, s + 1, 1, 0.5)
    assert d[d1[0]][o, s, d1[1]] == c


# ---- ggs_ga_philox_draws: the C boundary ------------------------------------------------
def test_export_is_declared_exported_bound_and_its_kernel_uses_no_scratch():
    from test_capi import declared_functions
    from test_kernel_resources import _tool
    name = "ggs_ga_philox_draws"
    assert name in declared_functions() and name in _lib.SIGNATURES and hasattr(ggs.lib, name)
    # ggs_ga_draws_out is ggs_ga_draws field for field: one ctypes structure serves both
    assert [f[0] for f in _lib.GaDraws._fields_] == [
        "tour_idx", "perm", "cx", "cx_u", "u_xy", "u_ab", "u_t", "u_rgb", "u_a", "k_color", "k_xy", "k_ab", "k_t",
        "n_xy", "n_ab", "n_t", "n_rgba", "swap_i", "swap_pick", "swap_u"]
    res = {n: r for n, r in _tool().kernel_resources(ggs.LIB_PATH).items() if "ga_philox_draws_kernel" in n}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r


# ---- ggs_ga_philox_draws: argument errors (no device is touched) ------------------------
def _export(n_off=2, P=3, N=4, tour_k=2, gen=1, first=0, null=None, no_struct=False):
    import ctypes as C
    keep, d = [], _lib.GaDraws()
    for name, typ in _lib.GaDraws._fields_:
        if name == null:
            continue
        a = np.zeros(4096, np.float64)
        keep.append(a)
        setattr(d, name, C.cast(a.ctypes.data, typ))
    rc = ggs.lib.ggs_ga_philox_draws(0, 7, gen, first, n_off, P, N, tour_k, 0.5, None if no_struct else C.byref(d))
    return rc, ggs.lib.ggs_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(n_off=0), "n_off=0"), (dict(n_off=-2), "n_off=-2"), (dict(P=0), "P=0"), (dict(N=0), "N=0"),
    (dict(tour_k=0), "tour_k=0"), (dict(gen=-1), "gen=-1"), (dict(first=-1), "first=-1"),
    (dict(no_struct=True), "null output"), (dict(null="tour_idx"), "null output"),
    (dict(null="n_rgba"), "null output"), (dict(null="swap_u"), "null output"),
    (dict(n_off=2**14, N=2**14), "exceed the limit"),
])
def test_philox_draws_bad_arguments_are_einval_before_any_device(kw, msg):
    rc, err = _export(**kw)
    assert rc == _lib.GGS_EINVAL, (rc, err)
    assert msg in err, err


def test_philox_draws_well_formed_call_reaches_the_device_layer():
    """A well-formed call gets past the argument checks: GGS_ENODEV without a GPU."""
    have_gpu = ggs.lib.ggs_init(0) > 0
    rc, err = _export()
    assert rc == (_lib.GGS_OK if have_gpu else _lib.GGS_ENODEV), (rc, err)
    if not have_gpu:
        with pytest.raises(AssertionError):
            philox_draws(1, 1, 2, 3, 4, 2, 0.5)
