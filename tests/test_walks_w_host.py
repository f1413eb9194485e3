"""Edge-weighted walks through the CPU twins (come_cpu_walk_cdf, come_cpu_random_walks_w), which
compile the kernels' own arithmetic and step body (csrc/come_walk_pq.h): the thresholds are the
documented formula's, unit weights give the unweighted walkers' streams, the step frequencies are
the exact weighted node2vec probabilities, a zero-weight edge is never walked, walks do not depend
on the split over launches or threads, invalid arguments write nothing; and the Python graph
classes carry weights."""
import ctypes

import numpy as np
import pytest

from come_amd import _lib, cpu
from come_amd import graph_utils as gu
from come_amd.graph import CSRGraph, chung_lu
from walks_pq_common import SETTINGS, assert_steps_are_edges, sort_rows
from walks_w_common import (cdf_formula, check_distribution_w, count_zero_edge, g12w,
                            picked_mass)

DEGREES = (1, 2, 63, 64, 65, 5000)


def pattern_rows():
    """One CSR whose rows are every degree of DEGREES under every weight pattern."""
    rng = np.random.RandomState(7)
    rows = []
    for deg in DEGREES:
        equal = np.full(deg, 3.5)
        dominant = rng.randint(1, 4, deg).astype(np.float64)
        dominant[deg // 2] = 1e9
        spread = 2.0 ** rng.uniform(-30, 30, deg)
        spread[0], spread[-1] = 2.0 ** -30, 2.0 ** 30
        zeros = rng.randint(0, 3, deg).astype(np.float64)  # about a third are 0
        zeros[0] = 0.0
        zeros[deg // 2] = 2.0
        head = np.zeros(deg)
        head[-1] = 5.0  # every entry but the last is 0
        tail = np.zeros(deg)
        tail[0] = 5.0
        rows += [equal, dominant, spread, zeros, head, tail]
    rowptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=rowptr[1:])
    return rowptr, np.concatenate(rows).astype(np.float32)


def test_cdf_is_the_documented_formula():
    rowptr, w = pattern_rows()
    wcdf, status = cpu.walk_cdf(rowptr, w, threads=1, return_status=True)
    assert status == 0 and wcdf.dtype == np.uint32
    np.testing.assert_array_equal(wcdf, cdf_formula(rowptr, w))
    np.testing.assert_array_equal(cpu.walk_cdf(rowptr, w, threads=3), wcdf)
    m = picked_mass(rowptr, wcdf)
    for v in range(len(rowptr) - 1):
        lo, hi = rowptr[v], rowptr[v + 1]
        t = wcdf[lo:hi].astype(np.int64)
        assert t[-1] == 2 ** 32 - 1 and (np.diff(t) >= 0).all()
        # m_i = wcdf[i] - wcdf[i-1] from -1: the masses sum to 2^32, and so do the picked ones
        assert np.diff(np.concatenate([[-1], t])).sum() == 2 ** 32
        assert m[lo:hi].sum() == 2 ** 32
        wd = w[lo:hi].astype(np.float64)
        assert (m[lo:hi][wd == 0] == 0).all()  # weight 0: never picked, wherever it stands
        # come.h's bound on the mass: the rounding of each u_i, spread over the row
        pr = wd / wd.sum()
        bound = 3.0 + pr * (hi - lo) * wd.max() / (2.0 * wd.sum())
        assert (np.abs(m[lo:hi] - pr * 2.0 ** 32) <= bound).all(), v


@pytest.mark.parametrize("deg", [1, 2, 3, 7, 63, 64, 65, 1000, 5000, 99991])
def test_equal_weights_give_the_multiply_shift_pick(deg):
    rowptr = np.array([0, deg], np.int64)
    wcdf = cpu.walk_cdf(rowptr, np.full(deg, 0.7, np.float32)).astype(np.int64)
    # (r * deg) >> 32 == i exactly for r in [ceil(i 2^32 / deg), ceil((i + 1) 2^32 / deg))
    want = np.array([-((-(i + 1) * 2 ** 32) // deg) - 1 for i in range(deg)], np.int64)
    np.testing.assert_array_equal(wcdf, want)


def test_cdf_status():
    rowptr = np.array([0, 3, 3, 5, 6], np.int64)
    good = np.array([1, 0, 2, 0, 4, 1], np.float32)
    assert cpu.walk_cdf(rowptr, good, return_status=True)[1] == 0
    for at, val in ((1, np.nan), (4, -1.0), (5, np.inf), (0, -0.5)):
        w = good.copy()
        w[at] = val
        assert cpu.walk_cdf(rowptr, w, return_status=True)[1] == 1, (at, val)
        with pytest.raises(ValueError, match="edge weights"):
            cpu.walk_cdf(rowptr, w)
    w = good.copy()
    w[3:5] = 0.0  # a row of positive degree, all zeros
    assert cpu.walk_cdf(rowptr, w, return_status=True)[1] == 1
    w = good.copy()
    w[5] = -0.0  # a lone negative zero is a zero row too
    assert cpu.walk_cdf(rowptr, w, return_status=True)[1] == 1
    many = np.zeros(200 * 5, np.float32)  # enough rows for three threads to share
    many[::5] = 1.0
    rp = np.arange(0, 1001, 5, dtype=np.int64)
    assert cpu.walk_cdf(rp, many, threads=3, return_status=True)[1] == 0
    many[995] = 0.0
    assert cpu.walk_cdf(rp, many, threads=3, return_status=True)[1] == 1


@pytest.mark.parametrize("p,q", [(1.0, 1.0)] + SETTINGS[:3])
def test_unit_weights_are_the_unweighted_walks(p, q):
    g = chung_lu(2000, 8.0)
    assert (g.degree == 0).any()
    rng = np.random.RandomState(1)
    starts = rng.randint(0, g.V, 3000).astype(np.int32)
    starts[::13] = -1
    starts[5::17] = g.V
    starts[7::19] = np.flatnonzero(g.degree == 0)[0]
    emit = rng.permutation(g.V).astype(np.int32)
    cs = cpu.sorted_adjacency(g.rowptr, g.col)
    wcdf = cpu.walk_cdf(g.rowptr, np.full(len(cs), 2.5, np.float32))
    for alpha in (0.0, 0.3):
        for em in (None, emit):
            kw = dict(alpha=alpha, p=p, q=q, seed=2 ** 40 + 3, walk_offset=11, emit=em,
                      return_trials=True)
            ref, ref_trials = cpu.random_walks_pq(g.rowptr, cs, starts, 40, col_sorted=cs, **kw)
            got, trials = cpu.random_walks_w(g.rowptr, cs, wcdf, starts, 40, **kw)
            np.testing.assert_array_equal(got, ref)
            assert trials == ref_trials > 0


def g12w_walks(p, q, passes, L=20, seed=12, **kw):
    rowptr, col, w = g12w()
    starts = np.tile(np.arange(12, dtype=np.int32), passes)
    wcdf = cpu.walk_cdf(rowptr, w)
    return rowptr, col, w, cpu.random_walks_w(rowptr, col, wcdf, starts, L, alpha=0.0, p=p, q=q,
                                              seed=seed, **kw)


FREQ_SETTINGS = [(1.0, 1.0)] + SETTINGS + [(1.0 / 16, 1.0), (1.0 / 256, 4.0)]
FREQ_PASSES = 1500


@pytest.mark.parametrize("p,q", FREQ_SETTINGS)
def test_step_frequencies_are_the_exact_weighted_probabilities(p, q):
    rowptr, col, w, walks = g12w_walks(p, q, FREQ_PASSES)
    checked, first = check_distribution_w(walks, rowptr, col, w, p, q)
    print("p=%g q=%g: %d triples, %d first steps checked" % (p, q, checked, first))
    assert checked >= 20 and first >= 20, (checked, first)
    assert count_zero_edge(walks) == 0
    # the heavy edge is walked from both ends, so the outlier runs with prev's mass near 1
    assert ((walks[:, :-2] == 4) & (walks[:, 1:-1] == 5) & (walks[:, 2:] == 4)).sum() > 100


@pytest.mark.parametrize("p,q", [(1.0 / 256, 4.0), (1.0, 1.0), (256.0, 1.0 / 16)])
def test_every_step_is_an_edge_whatever_the_row_order(p, q):
    rowptr, col, w = g12w(scramble=np.random.RandomState(3))
    assert not np.array_equal(col, sort_rows(rowptr, col))
    wcdf = cpu.walk_cdf(rowptr, w)
    starts = np.tile(np.arange(-1, 13, dtype=np.int32), 200)
    walks = cpu.random_walks_w(rowptr, col, wcdf, starts, 30, p=p, q=q, seed=5)
    real = (starts >= 0) & (starts < 12)
    assert (walks[~real] == -1).all() and (walks[real] >= 0).all()
    assert np.array_equal(walks[real][:, 0], starts[real])
    assert_steps_are_edges(walks[real], rowptr, col)


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (1.0, 1.0), (1.0 / 16, 2.0)])
def test_shards_and_threads(p, q):
    g = chung_lu(2000, 8.0)
    rng = np.random.RandomState(2)
    starts = rng.randint(0, g.V, 1000).astype(np.int32)
    cs, ws = cpu.sort_weighted_adjacency(
        g.rowptr, g.col, rng.lognormal(0.0, 1.5, len(g.col)).astype(np.float32))
    wcdf = cpu.walk_cdf(g.rowptr, ws)
    kw = dict(alpha=0.1, p=p, q=q, seed=9, return_trials=True)
    whole, trials = cpu.random_walks_w(g.rowptr, cs, wcdf, starts, 25, walk_offset=7, threads=1,
                                       **kw)
    four = cpu.random_walks_w(g.rowptr, cs, wcdf, starts, 25, walk_offset=7, threads=4, **kw)
    assert np.array_equal(four[0], whole) and four[1] == trials
    parts = [cpu.random_walks_w(g.rowptr, cs, wcdf, np.ascontiguousarray(starts[lo:hi]), 25,
                                walk_offset=7 + lo, **kw)
             for lo, hi in ((0, 333), (333, 334), (334, 1000))]
    assert np.array_equal(np.concatenate([w for w, _ in parts]), whole)
    assert sum(t for _, t in parts) == trials
    other = cpu.random_walks_w(g.rowptr, cs, wcdf, starts, 25, walk_offset=8, **kw)[0]
    assert not np.array_equal(other, whole)
    unit = cpu.random_walks_w(g.rowptr, cs, cpu.walk_cdf(g.rowptr, np.ones_like(ws)), starts, 25,
                              walk_offset=7, **kw)[0]
    assert not np.array_equal(unit, whole)  # the weights matter


def test_invalid_arguments_write_nothing():
    rowptr, col, w = g12w()
    wcdf = cpu.walk_cdf(rowptr, w)
    starts = np.arange(12, dtype=np.int32)
    L = _lib.lib()
    f32 = np.float32

    def call(alpha, p, q, V=12, P=12, steps=9, offset=0, threads=2, col_=col, wcdf_=wcdf):
        out = np.full((12, 9), 0x5A5A5A5A, np.int32)
        trials = ctypes.c_uint64(77)
        rc = L.come_cpu_random_walks_w(
            _lib.ptr(rowptr), None if col_ is None else _lib.ptr(col_),
            None if wcdf_ is None else _lib.ptr(wcdf_), V, _lib.ptr(starts), P, steps, alpha, p,
            q, 3, offset, None, _lib.ptr(out), ctypes.byref(trials), threads)
        return rc, bool((out == 0x5A5A5A5A).all()) and trials.value == 77

    up = lambda x: float(np.nextafter(f32(x), f32(np.inf)))  # noqa: E731
    down = lambda x: float(np.nextafter(f32(x), f32(0)))  # noqa: E731
    bad = [(0.0, up(256), 1.0), (0.0, down(1 / 256), 1.0), (0.0, 1.0, up(16)),
           (0.0, 1.0, down(1 / 16)), (0.0, float("nan"), 1.0), (0.0, 1.0, float("nan")),
           (0.0, 0.0, 1.0), (0.0, -1.0, 1.0), (0.0, float("inf"), 1.0),
           (-0.01, 2.0, 2.0), (1.01, 2.0, 2.0), (float("nan"), 2.0, 2.0)]
    for alpha, p, q in bad:
        assert call(alpha, p, q) == (-1, True), (alpha, p, q)
    assert call(0.0, 1.0, 1.0, V=0) == (-1, True)
    assert call(0.0, 1.0, 1.0, P=-1) == (-1, True)
    assert call(0.0, 1.0, 1.0, steps=-1) == (-1, True)
    assert call(0.0, 1.0, 1.0, offset=-1) == (-1, True)
    assert call(0.0, 1.0, 1.0, threads=0) == (-1, True)
    for p, q in ((1.0, 1.0), (2.0, 1.0), (0.5, 2.0)):  # never NULL here, whatever (p, q)
        assert call(0.0, p, q, col_=None) == (-1, True)
        assert call(0.0, p, q, wcdf_=None) == (-1, True)
    assert b"null pointer" in L.come_last_error()
    assert call(0.0, 1.0, 1.0, P=0) == (0, True) and call(0.0, 1.0, 1.0, steps=0) == (0, True)
    for alpha, p, q in ((0.0, 256.0, 16.0), (1.0, 1 / 256, 1 / 16), (0.0, 1.0, 1.0)):
        assert call(alpha, p, q) == (0, False), (alpha, p, q)
    status = ctypes.c_int32(55)
    out = np.full(len(w), 0x5A5A5A5A, np.uint32)
    for args in ((None, _lib.ptr(w), 12), (_lib.ptr(rowptr), None, 12),
                 (_lib.ptr(rowptr), _lib.ptr(w), 0)):
        assert L.come_cpu_walk_cdf(*args, _lib.ptr(out), ctypes.byref(status), 1) == -1
    assert status.value == 55 and (out == 0x5A5A5A5A).all()
    with pytest.raises(_lib.ComeError, match="p must be"):
        cpu.random_walks_w(rowptr, col, wcdf, starts, 9, p=300.0)


def test_sort_weighted_adjacency_keeps_weights_with_their_entries():
    rowptr, col, w = g12w()
    rp2, scrambled, w2 = g12w(scramble=np.random.RandomState(8))
    cs, ws = cpu.sort_weighted_adjacency(rp2, scrambled, w2)
    np.testing.assert_array_equal(cs, col)
    np.testing.assert_array_equal(ws, w)


def test_csrgraph_weights():
    edges = [(0, 1), (1, 2), (2, 1), (3, 3), (0, 3), (1, 0), (4, 2)]
    g = CSRGraph(5, edges, weights=[1, 2, 3, 9, 4, 5, 0.5])
    plain = CSRGraph(5, edges)
    np.testing.assert_array_equal(g.col, plain.col)
    np.testing.assert_array_equal(g.rowptr, plain.rowptr)
    np.testing.assert_array_equal(g.edges, plain.edges)
    assert g.weights.dtype == np.float32 and g.strength.dtype == np.float64
    dense = np.zeros((5, 5))
    row = np.repeat(np.arange(5), g.degree)
    dense[row, g.col] = g.weights
    want = np.zeros((5, 5))
    for (a, b), w in (((0, 1), 5), ((1, 2), 3), ((0, 3), 4), ((2, 4), 0.5)):  # last listing wins
        want[a, b] = want[b, a] = w
    np.testing.assert_array_equal(dense, want)  # symmetric, and the self-loop is dropped
    np.testing.assert_array_equal(g.strength, want.sum(1))
    ids, s = g.degree_by_id(weighted=True)
    np.testing.assert_array_equal(s, want.sum(1))
    np.testing.assert_array_equal(g.degree_by_id()[1], plain.degree_by_id()[1])
    np.testing.assert_array_equal(ids, plain.degree_by_id()[0])
    # a graph without weights is today's
    assert plain.weights is None
    np.testing.assert_array_equal(plain.strength, plain.degree)
    old = chung_lu(500, 6.0)
    assert old.weights is None
    a = np.minimum(old.edges[:, 0], old.edges[:, 1])
    again = CSRGraph(500, old.edges, weights=np.ones(len(a)))
    np.testing.assert_array_equal(again.col, old.col)
    np.testing.assert_array_equal(again.rowptr, old.rowptr)
    assert (again.weights == 1).all()
    with pytest.raises(ValueError):
        CSRGraph(5, edges, weights=[1, 2])


def test_weighted_edgelist_round_trip(tmp_path):
    f = tmp_path / "g.wel"
    f.write_text("# u v w\n10 20 1.5\n20 30 2\n\n30 10 0.25  # trailing comment\n"
                 "20 10 4e0\n40 30 0\n")
    G = gu.load_weighted_edgelist(str(f))
    plain = gu.Graph.from_edges([(10, 20), (20, 30), (30, 10), (20, 10), (40, 30)])
    np.testing.assert_array_equal(G.node_ids, plain.node_ids)
    np.testing.assert_array_equal(G.rowptr, plain.rowptr)
    np.testing.assert_array_equal(G.col, plain.col)
    assert plain.weights is None and G.weights.dtype == np.float32
    got = {}
    for u in range(len(G.node_ids)):
        for k in range(G.rowptr[u], G.rowptr[u + 1]):
            got[(int(G.node_ids[u]), int(G.node_ids[G.col[k]]))] = float(G.weights[k])
    want = {(10, 20): 4.0, (20, 30): 2.0, (10, 30): 0.25, (30, 40): 0.0}
    assert got == {**want, **{(b, a): w for (a, b), w in want.items()}}
    ids, s = G.degree_by_id(weighted=True)
    assert dict(zip(ids.tolist(), s.tolist())) == {10: 4.25, 20: 6.0, 30: 2.25, 40: 0.0}
    U = G.to_undirected()
    back = {}
    for u in range(len(U.node_ids)):
        for k in range(U.rowptr[u], U.rowptr[u + 1]):
            back[(int(U.node_ids[u]), int(U.node_ids[U.col[k]]))] = float(U.weights[k])
    assert back == got
    # written back out and read again: the same graph
    f2 = tmp_path / "g2.wel"
    f2.write_text("".join("%d %d %r\n" % (a, b, w) for (a, b), w in want.items()))
    G2 = gu.load_weighted_edgelist(str(f2))
    np.testing.assert_array_equal(G2.strength, G.strength)
    with pytest.raises(ValueError, match="expected 'u v w'"):
        f2.write_text("1 2\n")
        gu.load_weighted_edgelist(str(f2))
