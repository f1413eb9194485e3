"""Shared by tests/test_walks_pq_host.py and tests/test_gpu_walks_pq.py: the 12-node test graph,
the exact node2vec (p, q) step probabilities and the frequency check against them."""
import numpy as np

# a 4-clique, triangles, a leaf (11), a path and a degree-6 node (5)
G12_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 4), (4, 5), (5, 6), (5, 7),
             (5, 8), (8, 9), (5, 9), (9, 10), (10, 11), (2, 6)]
SETTINGS = [(0.25, 4.0), (4.0, 0.25), (1.0, 0.5), (1.0 / 16, 16.0), (16.0, 1.0 / 16), (2.0, 1.0)]


def csr_of(V, directed_edges):
    """(rowptr int64, col int32) with each row in the order the edges are listed."""
    e = np.asarray(directed_edges, np.int64)
    order = np.argsort(e[:, 0], kind="stable")
    rowptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=V), out=rowptr[1:])
    return rowptr, np.ascontiguousarray(e[order, 1].astype(np.int32))


def g12():
    """G12, rows deliberately not ascending (reverse listing order), so col != col_sorted."""
    und = G12_EDGES + [(b, a) for a, b in G12_EDGES]
    return csr_of(12, und[::-1])


def directed_cycle():
    """An asymmetric CSR: the directed 8-cycle with three chords; prev is mostly not in N(cur)."""
    return csr_of(8, [(i, (i + 1) % 8) for i in range(8)] + [(0, 4), (2, 6), (5, 1)])


def sort_rows(rowptr, col, reverse=False):
    out = col.copy()
    for v in range(len(rowptr) - 1):
        r = np.sort(col[rowptr[v]:rowptr[v + 1]])
        out[rowptr[v]:rowptr[v + 1]] = r[::-1] if reverse else r
    return out


def neighbours(rowptr, col):
    return [col[rowptr[v]:rowptr[v + 1]].tolist() for v in range(len(rowptr) - 1)]


def exact_step_probs(rowptr, col, p, q):
    """{(prev, cur): {x: probability}} of the node2vec step, from the adjacency."""
    nb = neighbours(rowptr, col)
    probs = {}
    for prev in range(len(nb)):
        for cur in nb[prev]:
            w = {x: (1.0 / p if x == prev else 1.0 if x in nb[prev] else 1.0 / q)
                 for x in nb[cur]}
            tot = sum(w.values())
            probs[(prev, cur)] = {x: v / tot for x, v in w.items()}
    return probs


def assert_steps_are_edges(walks, rowptr, col):
    nb = [set(r) for r in neighbours(rowptr, col)]
    for row in walks:
        for a, b in zip(row[:-1], row[1:]):
            assert int(b) in nb[int(a)], (row, a, b)


def check_distribution(walks, rowptr, col, p, q, min_expected=100.0, sigmas=5.0):
    """Second-order frequencies of alpha = 0 walks against the exact probabilities: for every
    (c_{t-2}, c_{t-1}, c_t) whose expected count N * P is at least min_expected,
    |n - N P| <= sigmas * sqrt(N P (1 - P)); the first steps against the uniform choice by the
    same rule.  Returns (contexts seen, triples checked)."""
    assert (walks >= 0).all()
    V = len(rowptr) - 1
    probs = exact_step_probs(rowptr, col, p, q)
    a, b, c = walks[:, :-2].ravel(), walks[:, 1:-1].ravel(), walks[:, 2:].ravel()
    cnt = np.zeros((V, V, V), np.int64)
    np.add.at(cnt, (a, b, c), 1)
    ctx = cnt.sum(2)
    seen = checked = 0
    for (prev, cur), row in probs.items():
        N = int(ctx[prev, cur])
        seen += N > 0
        assert cnt[prev, cur].sum() == sum(cnt[prev, cur, x] for x in row)  # edges only
        for x, P in row.items():
            if N * P >= min_expected:
                n = int(cnt[prev, cur, x])
                assert abs(n - N * P) <= sigmas * np.sqrt(N * P * (1 - P)), (
                    (p, q), (prev, cur, x), n, N * P)
                checked += 1
    assert ctx.sum() == sum(int(ctx[k]) for k in probs)  # no context off the graph
    first = np.zeros((V, V), np.int64)
    np.add.at(first, (walks[:, 0], walks[:, 1]), 1)
    deg = np.diff(rowptr)
    first_checked = 0
    for v in range(V):
        N, P = int(first[v].sum()), 1.0 / deg[v]
        for x in col[rowptr[v]:rowptr[v + 1]]:
            if N * P >= min_expected:
                assert abs(first[v, x] - N * P) <= sigmas * np.sqrt(N * P * (1 - P)), (v, x)
                first_checked += 1
    assert first_checked > 0
    return seen, checked
