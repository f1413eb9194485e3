"""node2vec (p, q) second-order walks through the CPU twin (come_cpu_random_walks_pq), which
compiles the kernel's own step body (csrc/come_walk_pq.h): the stream at p = q = 1 is the
first-order walker's, the step frequencies are the exact node2vec probabilities, the expected
trials per step are bounded, every step is an edge, walks do not depend on the split over launches
or threads, and invalid arguments write nothing."""
import ctypes

import numpy as np
import pytest

from come_amd import _lib, cpu
from come_amd.graph import chung_lu
from oracle import oracle as orc
from walks_pq_common import (SETTINGS, assert_steps_are_edges, check_distribution,
                             directed_cycle, g12, sort_rows)


def g12_walks(p, q, passes=400, L=20, seed=12, **kw):
    rowptr, col = g12()
    starts = np.tile(np.arange(12, dtype=np.int32), passes)
    return rowptr, col, starts, cpu.random_walks_pq(rowptr, col, starts, L, alpha=0.0, p=p, q=q,
                                                    seed=seed, **kw)


def test_p1_unit_bias_is_the_first_order_stream():
    g = chung_lu(2000, 8.0)
    assert (g.degree == 0).any()  # dead ends
    rng = np.random.RandomState(1)
    starts = rng.randint(0, g.V, 3000).astype(np.int32)
    starts[::13] = -1
    starts[5::17] = g.V
    starts[7::19] = np.flatnonzero(g.degree == 0)[0]
    emit = rng.permutation(g.V).astype(np.int32)
    cs = cpu.sorted_adjacency(g.rowptr, g.col)
    for alpha in (0.0, 0.3):
        for L in (1, 17, 40):
            for off in (0, 2 ** 33 + 5):
                for em in (None, emit):
                    ref = orc.philox_walks(g.rowptr, g.col, starts, L, alpha, seed=2 ** 40 + 3,
                                           walk_offset=off, emit=em)
                    got = cpu.random_walks_pq(g.rowptr, g.col, starts, L, alpha=alpha,
                                              seed=2 ** 40 + 3, walk_offset=off, emit=em)
                    np.testing.assert_array_equal(got, ref)
                    # a col_sorted that is not needed changes nothing
                    got = cpu.random_walks_pq(g.rowptr, g.col, starts, L, alpha=alpha,
                                              seed=2 ** 40 + 3, walk_offset=off, emit=em,
                                              col_sorted=cs, threads=3)
                    np.testing.assert_array_equal(got, ref)
    empty = (starts < 0) | (starts >= g.V)
    assert empty.sum() > 300 and (got[empty] == -1).all() and (got[~empty, 0] >= 0).all()


@pytest.mark.parametrize("p,q", SETTINGS)
def test_step_frequencies_are_the_exact_node2vec_probabilities(p, q):
    rowptr, col, _, w = g12_walks(p, q)
    assert w.shape == (4800, 20)
    seen, checked = check_distribution(w, rowptr, col, p, q)
    assert seen == 32 and checked >= 50, (seen, checked)


@pytest.mark.parametrize("p,q", SETTINGS)
def test_expected_trials_per_step_are_bounded(p, q):
    rowptr, col, starts, (w, trials) = g12_walks(p, q, return_trials=True)
    deg = np.diff(rowptr)
    second = deg[w[:, 1:-1]] >= 2  # steps t >= 2 that run the trial loop (alpha = 0, no dead end)
    direct = w[:, 1:].size - int(second.sum())  # first steps and leaves: one block, no trial
    mean = (trials - direct) / second.sum()
    print("p=%g q=%g: %.3f trials per second-order step" % (p, q, mean))
    assert 1.0 <= mean <= 2.0 * max(q, 1.0 / q), mean
    again = cpu.random_walks_pq(rowptr, col, starts, 20, p=p, q=q, seed=12, return_trials=True,
                                threads=3)
    assert again[1] == trials and np.array_equal(again[0], w)


@pytest.mark.parametrize("graph", [g12, directed_cycle])
@pytest.mark.parametrize("p,q", [(1.0 / 256, 4.0), (1.0 / 256, 1.0), (256.0, 1.0 / 16)])
def test_p3_every_step_is_an_edge(graph, p, q):
    rowptr, col = graph()
    V = len(rowptr) - 1
    starts = np.tile(np.arange(-1, V + 1, dtype=np.int32), 200)
    for cs in (sort_rows(rowptr, col), sort_rows(rowptr, col, reverse=True)):
        w = cpu.random_walks_pq(rowptr, col, starts, 30, p=p, q=q, seed=5, col_sorted=cs)
        real = (starts >= 0) & (starts < V)
        assert (w[~real] == -1).all() and (w[real] >= 0).all()
        assert np.array_equal(w[real][:, 0], starts[real])
        assert_steps_are_edges(w[real], rowptr, col)


def test_p3_a_leaf_returns_along_its_edge():
    _, _, _, w = g12_walks(256.0, 1.0, passes=100)
    at_leaf = w[:, 1:-1] == 11
    assert at_leaf.sum() > 50
    assert (w[:, 2:][at_leaf] == 10).all() and (w[:, :-2][at_leaf] == 10).all()


@pytest.mark.parametrize("p,q", [(0.25, 4.0), (0.5, 1.0), (2.0, 1.0)])
def test_p2_p4_shards_and_threads(p, q):
    g = chung_lu(2000, 8.0)
    starts = np.random.RandomState(2).randint(0, g.V, 1000).astype(np.int32)
    kw = dict(alpha=0.1, p=p, q=q, seed=9)
    whole, trials = cpu.random_walks_pq(g.rowptr, g.col, starts, 25, walk_offset=7,
                                        return_trials=True, threads=1, **kw)
    four = cpu.random_walks_pq(g.rowptr, g.col, starts, 25, walk_offset=7, return_trials=True,
                               threads=4, **kw)
    assert np.array_equal(four[0], whole) and four[1] == trials
    parts = [cpu.random_walks_pq(g.rowptr, g.col, np.ascontiguousarray(starts[lo:hi]), 25,
                                 walk_offset=7 + lo, return_trials=True, **kw)
             for lo, hi in ((0, 333), (333, 334), (334, 1000))]
    assert np.array_equal(np.concatenate([w for w, _ in parts]), whole)
    assert sum(t for _, t in parts) == trials
    other = cpu.random_walks_pq(g.rowptr, g.col, starts, 25, walk_offset=8, **kw)
    assert not np.array_equal(other, whole)


def test_invalid_arguments_write_nothing():
    rowptr, col = g12()
    cs = sort_rows(rowptr, col)
    starts = np.arange(12, dtype=np.int32)
    L = _lib.lib()
    f32 = np.float32

    def call(alpha, p, q, sorted_col=cs):
        out = np.full((12, 9), 0x5A5A5A5A, np.int32)
        trials = ctypes.c_uint64(77)
        rc = L.come_cpu_random_walks_pq(
            _lib.ptr(rowptr), _lib.ptr(col), None if sorted_col is None else _lib.ptr(sorted_col),
            12, _lib.ptr(starts), 12, 9, alpha, p, q, 3, 0, None, _lib.ptr(out),
            ctypes.byref(trials), 2)
        return rc, bool((out == 0x5A5A5A5A).all()) and trials.value == 77

    up = lambda x: float(np.nextafter(f32(x), f32(np.inf)))  # noqa: E731
    down = lambda x: float(np.nextafter(f32(x), f32(0)))  # noqa: E731
    bad = [(0.0, up(256), 1.0), (0.0, down(1 / 256), 1.0), (0.0, 1.0, up(16)),
           (0.0, 1.0, down(1 / 16)), (0.0, float("nan"), 1.0), (0.0, 1.0, float("nan")),
           (0.0, 0.0, 1.0), (0.0, -1.0, 1.0), (0.0, float("inf"), 1.0),
           (-0.01, 2.0, 2.0), (1.01, 2.0, 2.0), (float("nan"), 2.0, 2.0)]
    for alpha, p, q in bad:
        assert call(alpha, p, q) == (-1, True), (alpha, p, q)
    for p, q in ((1.0, 2.0), (1.0, down(1.0)), (0.5, 1.0)):  # these search: NULL is refused
        assert call(0.0, p, q, sorted_col=None) == (-1, True), (p, q)
    assert b"col_sorted" in L.come_last_error()
    # the range's ends, and NULL where nothing is searched, are accepted
    for alpha, p, q, s in ((0.0, 256.0, 16.0, cs), (1.0, 1 / 256, 1 / 16, cs),
                           (0.0, 2.0, 1.0, None), (0.0, 1.0, 1.0, None)):
        assert call(alpha, p, q, sorted_col=s) == (0, False), (alpha, p, q)
    with pytest.raises(_lib.ComeError, match="p must be"):
        cpu.random_walks_pq(rowptr, col, starts, 9, p=300.0)


def test_sorted_adjacency_sorts_each_row():
    g = chung_lu(2000, 8.0)
    rng = np.random.RandomState(3)
    col = g.col.copy()
    for v in range(g.V):  # shuffle the rows
        rng.shuffle(col[g.rowptr[v]:g.rowptr[v + 1]])
    np.testing.assert_array_equal(cpu.sorted_adjacency(g.rowptr, col),
                                  sort_rows(g.rowptr, g.col))
    rowptr, c12 = g12()
    assert not np.array_equal(c12, sort_rows(rowptr, c12))
    np.testing.assert_array_equal(cpu.sorted_adjacency(rowptr, c12), sort_rows(rowptr, c12))
