"""Edges sampled by weight through the CPU twins (come_cpu_edge_cdf, come_cpu_edge_sample,
come_cpu_edge_pick), which compile the kernels' own arithmetic (csrc/come_edge_sample.h): the CDF
is the documented formula's word for word, every edge owns exactly the documented share of the 2^64
draws, sampled frequencies follow the weights, the stream composes over offsets, and CSRGraph
carries one weight per undirected edge."""
import numpy as np
import pytest

from come_amd import cpu
from come_amd.graph import CSRGraph
from edge_sample_common import (TWO64, check_frequencies, edge_cdf_formula, first_r64, g12_edges,
                                lognormal_weights, units)

BIG = 70_001


def weight_sets():
    g12 = g12_edges()[1]
    assert (g12 == 1000).sum() == 1 and g12[0] == 0 and (g12 == 0).sum() == 1
    assert ((g12[(g12 > 0) & (g12 < 1000)] >= 1) & (g12[(g12 > 0) & (g12 < 1000)] <= 5)).all()
    return {
        "one": np.array([0.37], np.float32),
        "g12": g12,
        "zeros": np.array([3, 0, 0, 1.5, 0, 7, 2, 0, 0], np.float32),  # middle and tail
        "wmax_twice": np.array([1, 9, 2, 9, 0.5], np.float32),
        "lognormal": lognormal_weights(BIG),
    }


@pytest.mark.parametrize("name", ["one", "g12", "zeros", "wmax_twice", "lognormal"])
def test_cdf_is_the_documented_formula(name):
    w = weight_sets()[name]
    ecdf, status = cpu.edge_cdf(w, threads=1, return_status=True)
    assert status == 0 and ecdf.dtype == np.uint64 and ecdf.shape == w.shape
    np.testing.assert_array_equal(ecdf, edge_cdf_formula(w))
    np.testing.assert_array_equal(cpu.edge_cdf(w, threads=3), ecdf)
    assert int(ecdf[-1]) < 2 ** 63 and int(units(w).max()) == 2 ** 32


@pytest.mark.parametrize("bad", [np.nan, np.inf, -1.0, None])
def test_invalid_weights_set_the_status_word(bad):
    w = np.array([1, 2, 3, 4], np.float32)
    if bad is None:
        w[:] = 0
    else:
        w[2] = bad
    assert cpu.edge_cdf(w, return_status=True)[1] == 1
    with pytest.raises(ValueError):
        cpu.edge_cdf(w)


@pytest.mark.parametrize("name", ["g12", "lognormal"])
def test_every_edge_owns_its_exact_share_of_the_draws(name):
    """Edge i is picked for r64 in [ceil(U_{i-1} 2^64 / U_E), ceil(U_i 2^64 / U_E)): checked at
    both ends of every interval, with Python integers, and the implied probability against
    w_i / W from the definition."""
    w = weight_sets()[name]
    ecdf = cpu.edge_cdf(w)
    u = units(w)
    first = first_r64(ecdf)
    assert first[0] == 0 and first[-1] == TWO64
    pos = np.flatnonzero(u > 0)
    lo = np.array([first[i] for i in pos], np.uint64)
    np.testing.assert_array_equal(cpu.edge_pick(ecdf, lo), pos)
    # one below an interval's first draw: the previous edge of positive mass
    below = np.array([first[i] - 1 for i in pos[1:]], np.uint64)
    np.testing.assert_array_equal(cpu.edge_pick(ecdf, below), pos[:-1])
    ends = cpu.edge_pick(ecdf, np.array([0, TWO64 - 1], np.uint64))
    assert ends[0] == pos[0] and ends[1] == pos[-1]
    E, UE = len(w), int(ecdf[-1])
    wd = w.astype(np.float64)
    p = wd / wd.sum()
    for i in range(E):
        mass = first[i + 1] - first[i]
        if u[i] == 0:
            assert mass == 0
        if wd[i] == 0:
            assert u[i] == 0
        bound = (0.5 + p[i] * E / 2) / UE + 2.0 ** -63
        assert abs(mass / TWO64 - p[i]) <= bound, (i, mass / TWO64, p[i], bound)


def test_sampled_frequencies_follow_the_weights():
    edges, w = g12_edges()
    ecdf = cpu.edge_cdf(w)
    rows, index = cpu.sample_edges(edges, ecdf, 1_000_000, seed=2024, return_index=True)
    assert check_frequencies(index, w) == 15  # every positive edge; the lightest has S p ~ 1,900
    assert not (index == 0).any()             # the zero-weight edge
    np.testing.assert_array_equal(rows, edges[index])


def test_stream_composes_over_offsets_and_depends_on_the_seed():
    w = lognormal_weights(BIG)
    edges = np.random.RandomState(5).randint(0, 1000, (BIG, 2)).astype(np.int32)
    ecdf = cpu.edge_cdf(w)
    whole, wi = cpu.sample_edges(edges, ecdf, 1000, seed=9, return_index=True)
    a, ai = cpu.sample_edges(edges, ecdf, 400, seed=9, offset=0, return_index=True)
    b, bi = cpu.sample_edges(edges, ecdf, 600, seed=9, offset=400, return_index=True)
    np.testing.assert_array_equal(whole, np.concatenate([a, b]))
    np.testing.assert_array_equal(wi, np.concatenate([ai, bi]))
    np.testing.assert_array_equal(whole, edges[wi])
    np.testing.assert_array_equal(cpu.sample_edges(edges, ecdf, 1000, seed=9, threads=1), whole)
    off = 2 ** 32 - 5  # the counter's low word wraps inside this piece
    cross = cpu.sample_edges(edges, ecdf, 10, seed=9, offset=off)
    halves = [cpu.sample_edges(edges, ecdf, 5, seed=9, offset=off),
              cpu.sample_edges(edges, ecdf, 5, seed=9, offset=2 ** 32)]
    np.testing.assert_array_equal(cross, np.concatenate(halves))
    assert not np.array_equal(cross[:5], cross[5:])
    other = cpu.sample_edges(edges, ecdf, 1000, seed=10, return_index=True)[1]
    assert (other != wi).mean() > 0.9
    assert cpu.sample_edges(edges, ecdf, 0, seed=9).shape == (0, 2)


def test_csrgraph_keeps_one_weight_per_undirected_edge():
    rows = [(0, 1), (2, 1), (3, 3), (1, 0), (4, 2), (0, 4), (2, 4)]
    w = [5.0, 2.0, 9.0, 7.0, 1.0, 3.0, 0.25]  # (0,1) and (2,4) listed twice; a weighted self-loop
    g = CSRGraph(5, rows, weights=w)
    assert g.edge_weights.dtype == np.float32 and g.edge_weights.shape == (len(g.edges),)
    want = {(0, 1): 7.0, (1, 2): 2.0, (2, 4): 0.25, (0, 4): 3.0}  # the last listing wins
    got = {tuple(e): float(x) for e, x in zip(g.edges.tolist(), g.edge_weights)}
    assert got == want
    np.testing.assert_array_equal(g.edge_ids(), g.edges + 1)
    s = (np.bincount(g.edges[:, 0], g.edge_weights.astype(np.float64), minlength=g.V)
         + np.bincount(g.edges[:, 1], g.edge_weights.astype(np.float64), minlength=g.V))
    np.testing.assert_array_equal(s, g.strength)
    assert CSRGraph(5, rows).edge_weights is None
