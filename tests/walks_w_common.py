"""Shared by tests/test_walks_w_host.py and tests/test_gpu_walks_w.py: G12 with edge weights, the
numpy restatement of come_walk_cdf's formula, the exact weighted node2vec step probabilities and
the frequency check against them."""
import numpy as np

from walks_pq_common import G12_EDGES, csr_of, neighbours

HEAVY = (4, 5)   # weight 1000: from 4 or 5, prev = the other end holds almost the whole row
ZERO = (0, 1)    # weight 0: still an adjacency, never stepped along; first in both its rows


def g12_weight(a, b):
    a, b = min(a, b), max(a, b)
    if (a, b) == HEAVY:
        return 1000.0
    if (a, b) == ZERO:
        return 0.0
    return float(1 + (7 * a + 3 * b) % 5)


def g12w(scramble=None):
    """(rowptr, col, weights) of the weighted G12, each row ascending -- or, with a RandomState,
    each row in a random order (weights aligned)."""
    und = sorted(G12_EDGES + [(b, a) for a, b in G12_EDGES])
    rowptr, col = csr_of(12, und)
    if scramble is not None:
        for v in range(12):
            scramble.shuffle(col[rowptr[v]:rowptr[v + 1]])
    row = np.repeat(np.arange(12), np.diff(rowptr))
    w = np.array([g12_weight(a, b) for a, b in zip(row, col)], np.float32)
    return rowptr, col, w


def cdf_formula(rowptr, weights):
    """include/come.h's come_walk_cdf, restated: u = rint(w / wmax * 2^32), exact prefix sums,
    T = min(2^32, ceil(U / U_last * 2^32)), T_last = 2^32, stored T - 1 (0 where T = 0)."""
    out = np.zeros(len(weights), np.uint32)
    two32 = 4294967296.0
    for v in range(len(rowptr) - 1):
        w = weights[rowptr[v]:rowptr[v + 1]].astype(np.float64)
        if not len(w):
            continue
        u = np.rint(w / w.max() * two32).astype(np.uint64)
        U = np.cumsum(u, dtype=np.uint64)
        T = np.minimum(two32, np.ceil(U.astype(np.float64) / np.float64(U[-1]) * two32))
        T[-1] = two32
        T = T.astype(np.uint64)
        out[rowptr[v]:rowptr[v + 1]] = (np.maximum(T, 1) - 1).astype(np.uint32)
    return out


def picked_mass(rowptr, wcdf):
    """Per entry, how many of the 2^32 values of r the walker's search (the first i with
    max(r, 1) <= wcdf[i]) sends to it: int64, aligned with wcdf."""
    m = np.zeros(len(wcdf), np.int64)
    for v in range(len(rowptr) - 1):
        t = wcdf[rowptr[v]:rowptr[v + 1]].astype(np.int64) + 1
        if not len(t):
            continue
        H = np.maximum(t, 1)
        L = np.maximum(np.concatenate([[0], t[:-1]]), 1)
        m[rowptr[v]:rowptr[v + 1]] = H - L + ((L == 1) & (H >= 2))
    return m


def exact_step_probs_w(rowptr, col, weights, p, q):
    """({(prev, cur): {x: probability}}, {cur: {x: probability}}): the second-order step
    (w(cur, x) * beta, beta = 1/p, 1, 1/q) for every directed adjacency (prev, cur), and the first
    step (w / sum w).  float64, straight from the definition."""
    nb = neighbours(rowptr, col)
    wt = [dict(zip(nb[v], weights[rowptr[v]:rowptr[v + 1]].astype(np.float64).tolist()))
          for v in range(len(nb))]
    second, first = {}, {}
    for cur in range(len(nb)):
        tot = sum(wt[cur].values())
        first[cur] = {x: wt[cur][x] / tot for x in nb[cur]}
    for prev in range(len(nb)):
        for cur in nb[prev]:
            if len(nb[cur]) == 1:
                second[(prev, cur)] = dict(first[cur])
                continue
            w = {x: wt[cur][x] * (1.0 / p if x == prev else 1.0 if x in nb[prev] else 1.0 / q)
                 for x in nb[cur]}
            tot = sum(w.values())
            second[(prev, cur)] = {x: v / tot for x, v in w.items()}
    return second, first


def check_distribution_w(walks, rowptr, col, weights, p, q, min_expected=100.0, sigmas=5.0):
    """walks_pq_common.check_distribution's rule on alpha = 0 walks over weights: every
    (c_{t-2}, c_{t-1}, c_t) with expected count N P >= min_expected has |n - N P| <= sigmas *
    sqrt(N P (1 - P)), first steps likewise against w / sum w, and a step of probability 0 (a
    zero-weight entry) never occurs.  Returns (triples checked, first steps checked)."""
    assert (walks >= 0).all()
    V = len(rowptr) - 1
    second, first = exact_step_probs_w(rowptr, col, weights, p, q)
    a, b, c = walks[:, :-2].ravel(), walks[:, 1:-1].ravel(), walks[:, 2:].ravel()
    cnt = np.zeros((V, V, V), np.int64)
    np.add.at(cnt, (a, b, c), 1)
    ctx = cnt.sum(2)
    checked = 0
    for (prev, cur), row in second.items():
        N = int(ctx[prev, cur])
        assert cnt[prev, cur].sum() == sum(cnt[prev, cur, x] for x in row)  # edges only
        for x, P in row.items():
            n = int(cnt[prev, cur, x])
            if P == 0.0:
                assert n == 0, ((p, q), (prev, cur, x), n)
            if N * P >= min_expected:
                assert abs(n - N * P) <= sigmas * np.sqrt(N * P * (1 - P)), (
                    (p, q), (prev, cur, x), n, N * P)
                checked += 1
    assert ctx.sum() == sum(int(ctx[k]) for k in second)  # no context off the graph
    f = np.zeros((V, V), np.int64)
    np.add.at(f, (walks[:, 0], walks[:, 1]), 1)
    first_checked = 0
    for v in range(V):
        N = int(f[v].sum())
        assert N == sum(f[v, x] for x in first[v])
        for x, P in first[v].items():
            if P == 0.0:
                assert f[v, x] == 0, (v, x)
            if N * P >= min_expected:
                assert abs(f[v, x] - N * P) <= sigmas * np.sqrt(N * P * (1 - P)), (v, x)
                first_checked += 1
    assert checked > 0 and first_checked > 0
    return checked, first_checked


def count_zero_edge(walks):
    """Steps along ZERO, either direction."""
    a, b = walks[:, :-1].ravel(), walks[:, 1:].ravel()
    return int((((a == ZERO[0]) & (b == ZERO[1])) | ((a == ZERO[1]) & (b == ZERO[0]))).sum())
