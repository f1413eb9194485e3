"""The CPU twins of the hot-path entry points (include/come.h ``come_cpu_*``):
the same computations on host numpy arrays with ``threads`` worker threads, in libcome.so's
plain C++ (csrc/come_cpu.cpp).  For callers without a GPU; the GPU entry points never fall back
to them.

    sgns_o2(node, ctx, walks, seeds, window, negative, table, lr, alpha, mode, threads) -> pairs
    sgns_o1(node, edges, seeds, negative, table, lr, mode, threads)                   -> pairs
    community_grad(x, pi, mu, inv_cov, beta, lr, iters, threads)    (community_embeddings.py:61-78)
    gmm_estep(x, prec_chol, mu_prec, log_norm, threads) -> (resp, lse)  (predict_proba, :37)
    community_loss(x, pi, prec_chol, mu_prec, log_norm, threads) -> total   (what :40-59 means)
    sgns_o2_loss(node, ctx, walks, seeds, window, negative, table) -> (total, pairs[, per walk])
    sgns_pairs_loss(inp, out, rows_in, rows_pos, rows_neg)         -> (total, counted[, per pair])
    random_walks_pq(rowptr, col, starts, path_length, alpha, p, q, seed, ...) -> walks[, trials]
    walk_cdf(rowptr, weights)                                      -> wcdf (edge-weighted walks)
    random_walks_w(rowptr, col, wcdf, starts, path_length, alpha, p, q, seed, ...) -> walks[, trials]
    edge_cdf(weights)                                              -> ecdf (edges sampled by weight)
    sample_edges(edges, ecdf, S, seed, offset)                     -> rows[, indices]
    topk(queries, base, k, metric, exclude, base_sq, threads)      -> (idx, score) (neighbour search)

Tables are updated in place (float32, C-contiguous, as the reference's numpy arrays).  ``mode``:
MODE_HOGWILD = ``threads`` workers taking jobs of 150 walks / edges with lock-free updates, as the
reference's worker threads (context_embeddings.py:72-102, node_embeddings.py:58-95);
MODE_SEQUENTIAL = walks in order on the calling thread, bit-identical to the GPU's sequential mode.
"""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import MODE_HOGWILD, MODE_SEQUENTIAL, check, ptr  # noqa: F401


def default_threads():
    """CPUs this process may use (affinity mask)."""
    try:
        return max(1, len(os.sched_getaffinity(0)))
    except AttributeError:
        return os.cpu_count() or 1


def _threads(threads):
    return default_threads() if threads is None else int(threads)


def _arr(a, dtype, name, writable=False):
    if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags.c_contiguous:
        raise TypeError("%s must be a C-contiguous numpy %s array" % (name, np.dtype(dtype).name))
    if writable and not a.flags.writeable:
        raise ValueError("%s must be writable (updated in place)" % name)
    return a


def sgns_o2(node, ctx, walks, seeds, window, negative, table, lr, alpha=1.0,
            mode=MODE_HOGWILD, threads=None):
    """train_o2 (pyx:454-509) over walk rows [P, L] int32 (-1 = None) with per-walk seeds
    (uint64 [P]); returns the pair updates performed."""
    _arr(node, np.float32, "node", True)
    _arr(ctx, np.float32, "ctx", True)
    _arr(walks, np.int32, "walks")
    _arr(seeds, np.uint64, "seeds")
    _arr(table, np.uint32, "table")
    assert node.shape == ctx.shape and walks.ndim == 2 and seeds.shape == (walks.shape[0],)
    pairs = ctypes.c_int64(0)
    check(_lib.lib().come_cpu_sgns_o2(
        ptr(node), ptr(ctx), node.shape[0], node.shape[1], ptr(walks), walks.shape[0],
        walks.shape[1], ptr(seeds), int(window), int(negative), ptr(table), len(table),
        float(lr), float(alpha), int(mode), _threads(threads),
        ctypes.byref(pairs)), "come_cpu_sgns_o2")
    return pairs.value


def sgns_o1(node, edges, seeds, negative, table, lr, mode=MODE_HOGWILD, threads=None):
    """train_o1 (pyx:407-450) over edge rows [E, 2] int32 with per-edge seeds (uint64 [E]);
    returns the pair updates performed."""
    _arr(node, np.float32, "node", True)
    _arr(edges, np.int32, "edges")
    _arr(seeds, np.uint64, "seeds")
    _arr(table, np.uint32, "table")
    assert edges.ndim == 2 and edges.shape[1] == 2 and seeds.shape == (edges.shape[0],)
    pairs = ctypes.c_int64(0)
    check(_lib.lib().come_cpu_sgns_o1(
        ptr(node), node.shape[0], node.shape[1], ptr(edges), edges.shape[0], ptr(seeds),
        int(negative), ptr(table), len(table), float(lr), int(mode),
        _threads(threads), ctypes.byref(pairs)), "come_cpu_sgns_o1")
    return pairs.value


def community_grad(x, pi, mu, inv_cov, beta, lr, iters=1, threads=None):
    """Community2Vec.train's update on all rows of x [V, d] in place (community_embeddings.py:
    61-78): x -= lr * clip((beta / K) * sum_k pi[:, k] inv_cov[k] (x - mu[k]), -5, 5), `iters`
    times."""
    _arr(x, np.float32, "x", True)
    for a, n in ((pi, "pi"), (mu, "mu"), (inv_cov, "inv_cov")):
        _arr(a, np.float32, n)
    V, d = x.shape
    K = mu.shape[0]
    assert pi.shape == (V, K) and mu.shape == (K, d) and inv_cov.shape == (K, d, d)
    check(_lib.lib().come_cpu_community_grad(ptr(x), V, d, ptr(pi), ptr(mu), ptr(inv_cov), K,
                                             float(beta), float(lr), int(iters),
                                             _threads(threads)),
          "come_cpu_community_grad")
    return x


def gmm_estep(x, prec_chol, mu_prec, log_norm, threads=None):
    """Responsibilities [V, K] and per-row log-sum-exp [V] of a full-covariance GMM given its
    precision Cholesky factors (as come_gmm_estep: mu_prec[k] = mu_k @ prec_chol[k], log_norm[k] =
    log w_k + log det(prec_chol[k]) - d/2 log(2 pi))."""
    for a, n in ((x, "x"), (prec_chol, "prec_chol"), (mu_prec, "mu_prec"),
                 (log_norm, "log_norm")):
        _arr(a, np.float32, n)
    V, d = x.shape
    K = log_norm.shape[0]
    assert prec_chol.shape == (K, d, d) and mu_prec.shape == (K, d)
    resp = np.empty((V, K), np.float32)
    lse = np.empty(V, np.float32)
    check(_lib.lib().come_cpu_gmm_estep(ptr(x), V, d, ptr(prec_chol), ptr(mu_prec),
                                        ptr(log_norm), K, ptr(resp), ptr(lse),
                                        _threads(threads)), "come_cpu_gmm_estep")
    return resp, lse


def community_loss(x, pi, prec_chol, mu_prec, log_norm, return_rows=False, threads=None):
    """sum_i sum_k pi[i, k] (log_norm[k] - |x_i prec_chol[k] - mu_prec[k]|^2 / 2) in float64 (as
    come_community_loss: prec_chol the UPPER precision Cholesky factors, mu_prec[k] = mu_k @
    prec_chol[k], log_norm[k] = log det(prec_chol[k]) - d/2 log(2 pi), no mixture weight).  Returns
    the signed total as a Python float, or (total, rows [V] float32) with ``return_rows``."""
    for a, n in ((x, "x"), (pi, "pi"), (prec_chol, "prec_chol"), (mu_prec, "mu_prec"),
                 (log_norm, "log_norm")):
        _arr(a, np.float32, n)
    V, d = x.shape
    K = log_norm.shape[0]
    assert pi.shape == (V, K) and prec_chol.shape == (K, d, d) and mu_prec.shape == (K, d)
    rows = np.zeros(V, np.float32) if return_rows else None
    total = ctypes.c_double(0.0)
    check(_lib.lib().come_cpu_community_loss(ptr(x), V, d, ptr(pi), ptr(prec_chol), ptr(mu_prec),
                                             ptr(log_norm), K,
                                             ptr(rows) if return_rows else None,
                                             ctypes.byref(total), _threads(threads)),
          "come_cpu_community_loss")
    return (total.value, rows) if return_rows else total.value


def sgns_o2_loss(node, ctx, walks, seeds, window, negative, table, return_walks=False,
                 threads=None):
    """come_cpu_sgns_o2_loss: the SGNS objective of the batch ``sgns_o2`` would train on with these
    walk rows [P, L] int32 and seeds (uint64 [P]) -- the trainer's pairs, LCG negatives and fp32
    dot, a float64 softplus, nothing written.  ``table``: uint32 [T] (None with negative = 0).
    Returns ``(total, pairs)``, or ``(total, pairs, per_walk float64 [P])`` with
    ``return_walks``; per_walk does not depend on ``threads``."""
    _arr(node, np.float32, "node")
    _arr(ctx, np.float32, "ctx")
    _arr(walks, np.int32, "walks")
    _arr(seeds, np.uint64, "seeds")
    if table is not None:
        _arr(table, np.uint32, "table")
    assert node.shape == ctx.shape and walks.ndim == 2 and seeds.shape == (walks.shape[0],)
    P = walks.shape[0]
    per_walk = np.zeros(P, np.float64) if return_walks else None
    total, pairs = ctypes.c_double(0.0), ctypes.c_int64(0)
    check(_lib.lib().come_cpu_sgns_o2_loss(
        ptr(node), ptr(ctx), node.shape[0], node.shape[1], ptr(walks), P, walks.shape[1],
        ptr(seeds), int(window), int(negative), None if table is None else ptr(table),
        0 if table is None else len(table), ptr(per_walk) if return_walks else None,
        ctypes.byref(total), ctypes.byref(pairs), _threads(threads)), "come_cpu_sgns_o2_loss")
    return (total.value, pairs.value, per_walk) if return_walks else (total.value, pairs.value)


def sgns_pairs_loss(inp, out, rows_in, rows_pos, rows_neg=None, return_pairs=False, threads=None):
    """come_cpu_sgns_pairs_loss: the SGNS objective of explicit lists -- input rows ``rows_in`` [M]
    of ``inp``, positive rows ``rows_pos`` [M] and negative rows ``rows_neg`` [M, n] (or None) of
    ``out``, int32.  Returns ``(total, counted)``, or ``(total, counted, per_pair float64 [M])``
    with ``return_pairs``."""
    _arr(inp, np.float32, "inp")
    _arr(out, np.float32, "out")
    _arr(rows_in, np.int32, "rows_in")
    _arr(rows_pos, np.int32, "rows_pos")
    M = rows_in.shape[0]
    n = 0
    if rows_neg is not None:
        _arr(rows_neg, np.int32, "rows_neg")
        assert rows_neg.ndim == 2 and rows_neg.shape[0] == M
        n = rows_neg.shape[1]
    assert inp.shape == out.shape and rows_in.ndim == 1 and rows_pos.shape == (M,)
    per_pair = np.zeros(M, np.float64) if return_pairs else None
    total, counted = ctypes.c_double(0.0), ctypes.c_int64(0)
    check(_lib.lib().come_cpu_sgns_pairs_loss(
        ptr(inp), ptr(out), inp.shape[0], inp.shape[1], ptr(rows_in), ptr(rows_pos),
        ptr(rows_neg) if n else None, M, n, ptr(per_pair) if return_pairs else None,
        ctypes.byref(total), ctypes.byref(counted), _threads(threads)),
          "come_cpu_sgns_pairs_loss")
    return (total.value, counted.value, per_pair) if return_pairs else (total.value,
                                                                         counted.value)


def sorted_adjacency(rowptr, col):
    """``col`` with each row ascending (numpy form of graph_utils.sorted_adjacency): one sort of
    the (row << 32) | col keys."""
    _arr(rowptr, np.int64, "rowptr")
    _arr(col, np.int32, "col")
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    key = np.sort((row << 32) | col.astype(np.int64))
    return (key & 0xFFFFFFFF).astype(np.int32)


def random_walks_pq(rowptr, col, starts, path_length, alpha=0.0, p=1.0, q=1.0, seed=0,
                    walk_offset=0, emit=None, col_sorted=None, out=None, return_trials=False,
                    threads=None):
    """come_cpu_random_walks_pq: node2vec (p, q) second-order walks, the device walker's
    (graph_utils.device_walks(..., p, q)) bit for bit.  rowptr int64 [V+1], col int32 (positions,
    non-negative), starts int32 [P]; ``col_sorted`` (each row of col ascending) is built when it is
    needed and not given.  Returns int32 [P, path_length] (-1 after a walk ends), or
    ``(walks, trials)`` with ``return_trials``: the Philox blocks drawn, one per step taken plus
    one per rejected trial; it does not depend on ``threads``."""
    _arr(rowptr, np.int64, "rowptr")
    _arr(col, np.int32, "col")
    _arr(starts, np.int32, "starts")
    V, P = len(rowptr) - 1, len(starts)
    if emit is not None:
        _arr(emit, np.int32, "emit")
        assert emit.shape == (V,)
    if col_sorted is None and not (float(q) == 1.0 and float(p) >= 1.0):
        col_sorted = sorted_adjacency(rowptr, col)
    if col_sorted is not None:
        _arr(col_sorted, np.int32, "col_sorted")
        assert col_sorted.shape == col.shape
    if out is None:
        out = np.empty((P, int(path_length)), np.int32)
    else:
        _arr(out, np.int32, "out", True)
        assert out.shape == (P, int(path_length))
    trials = ctypes.c_uint64(0)
    check(_lib.lib().come_cpu_random_walks_pq(
        ptr(rowptr), ptr(col), None if col_sorted is None else ptr(col_sorted), V, ptr(starts), P,
        int(path_length), float(alpha), float(p), float(q), int(seed) & (2 ** 64 - 1),
        int(walk_offset), None if emit is None else ptr(emit), ptr(out), ctypes.byref(trials),
        _threads(threads)), "come_cpu_random_walks_pq")
    return (out, trials.value) if return_trials else out


def sort_weighted_adjacency(rowptr, col, weights):
    """(col, weights) with each row ascending by neighbour (numpy form of the sort inside
    graph_utils.weighted_adjacency): one sort of the (row << 32) | col keys, the weights riding
    along through the sort indices."""
    _arr(rowptr, np.int64, "rowptr")
    _arr(col, np.int32, "col")
    _arr(weights, np.float32, "weights")
    assert weights.shape == col.shape
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    key = (row << 32) | col.astype(np.int64)
    order = np.argsort(key, kind="stable")
    return (key[order] & 0xFFFFFFFF).astype(np.int32), np.ascontiguousarray(weights[order])


def walk_cdf(rowptr, weights, threads=None, return_status=False):
    """come_cpu_walk_cdf: the weighted walker's per-entry thresholds (uint32, aligned with
    ``weights``: fp32, one per CSR entry), come_walk_cdf's bit for bit.  Raises ValueError when the
    weights cannot be used (NaN, infinite, negative, or a row with only zeros); with
    ``return_status`` returns ``(wcdf, status)`` instead of raising."""
    _arr(rowptr, np.int64, "rowptr")
    _arr(weights, np.float32, "weights")
    assert weights.shape == (int(rowptr[-1]),)
    wcdf = np.zeros(len(weights), np.uint32)
    status = ctypes.c_int32(0)
    check(_lib.lib().come_cpu_walk_cdf(ptr(rowptr), ptr(weights), len(rowptr) - 1, ptr(wcdf),
                                       ctypes.byref(status), _threads(threads)),
          "come_cpu_walk_cdf")
    if return_status:
        return wcdf, status.value
    if status.value:
        raise ValueError("edge weights must be finite and >= 0, with a positive weight in every "
                         "row that has entries")
    return wcdf


def random_walks_w(rowptr, col, wcdf, starts, path_length, alpha=0.0, p=1.0, q=1.0, seed=0,
                   walk_offset=0, emit=None, out=None, return_trials=False, threads=None):
    """come_cpu_random_walks_w: edge-weighted node2vec (p, q) walks, the device walker's
    (graph_utils.device_walks(..., weights=)) bit for bit.  ``col``: each row ascending; ``wcdf``:
    walk_cdf of the weights in that order (sort_weighted_adjacency gives both from any order).
    Returns and ``return_trials`` as random_walks_pq."""
    _arr(rowptr, np.int64, "rowptr")
    _arr(col, np.int32, "col")
    _arr(wcdf, np.uint32, "wcdf")
    _arr(starts, np.int32, "starts")
    assert wcdf.shape == col.shape
    V, P = len(rowptr) - 1, len(starts)
    if emit is not None:
        _arr(emit, np.int32, "emit")
        assert emit.shape == (V,)
    if out is None:
        out = np.empty((P, int(path_length)), np.int32)
    else:
        _arr(out, np.int32, "out", True)
        assert out.shape == (P, int(path_length))
    trials = ctypes.c_uint64(0)
    check(_lib.lib().come_cpu_random_walks_w(
        ptr(rowptr), ptr(col), ptr(wcdf), V, ptr(starts), P, int(path_length), float(alpha),
        float(p), float(q), int(seed) & (2 ** 64 - 1), int(walk_offset),
        None if emit is None else ptr(emit), ptr(out), ctypes.byref(trials), _threads(threads)),
        "come_cpu_random_walks_w")
    return (out, trials.value) if return_trials else out


def edge_cdf(weights, threads=None, return_status=False):
    """come_cpu_edge_cdf: the exact uint64 prefix sums of the weights' 2^-32 units (fp32 [E], one
    weight per edge), come_edge_cdf's bit for bit.  Raises ValueError when the weights cannot be
    used (NaN, infinite, negative, or all zero); with ``return_status`` returns ``(ecdf, status)``
    instead of raising."""
    _arr(weights, np.float32, "weights")
    assert weights.ndim == 1
    ecdf = np.zeros(len(weights), np.uint64)
    status = ctypes.c_int32(0)
    check(_lib.lib().come_cpu_edge_cdf(ptr(weights), len(weights), ptr(ecdf),
                                       ctypes.byref(status), _threads(threads)),
          "come_cpu_edge_cdf")
    if return_status:
        return ecdf, status.value
    if status.value:
        raise ValueError("edge weights must be finite and >= 0, with at least one positive")
    return ecdf


def sample_edges(edges, ecdf, S, seed, offset=0, return_index=False, threads=None):
    """come_cpu_edge_sample: ``S`` rows of ``edges`` (int32 [E, 2]) drawn with replacement by
    ``ecdf`` = edge_cdf(weights), the device sampler's (training_sdg_inner.sample_edges) bit for
    bit; sample s is global sample ``offset + s`` of the stream ``seed``.  Returns int32 [S, 2],
    or ``(rows, indices)`` with the int64 [S] positions in ``edges`` when ``return_index``."""
    _arr(edges, np.int32, "edges")
    _arr(ecdf, np.uint64, "ecdf")
    assert edges.ndim == 2 and edges.shape[1] == 2 and ecdf.shape == (edges.shape[0],)
    S = int(S)
    out = np.empty((S, 2), np.int32)
    index = np.empty(S, np.int64) if return_index else None
    check(_lib.lib().come_cpu_edge_sample(
        ptr(edges), ptr(ecdf), len(ecdf), S, int(seed) & (2 ** 64 - 1), int(offset), ptr(out),
        ptr(index) if return_index else None, _threads(threads)), "come_cpu_edge_sample")
    return (out, index) if return_index else out


def edge_pick(ecdf, r64):
    """come_cpu_edge_pick (test support): the sampler's pick for each 64-bit uniform of ``r64``
    (uint64 [n]) in place of a Philox draw; int64 [n]."""
    _arr(ecdf, np.uint64, "ecdf")
    _arr(r64, np.uint64, "r64")
    idx = np.empty(len(r64), np.int64)
    check(_lib.lib().come_cpu_edge_pick(ptr(ecdf), len(ecdf), ptr(r64), len(r64), ptr(idx)),
          "come_cpu_edge_pick")
    return idx


def topk(queries, base, k, metric='cosine', exclude=None, base_sq=None, threads=None):
    """come_amd.neighbors.topk on host arrays (come_cpu_topk): the k best rows of base [V, d] for
    every row of queries [Q, d] under 'dot', 'cosine' or 'l2': (idx int64 [Q, k], score fp32
    [Q, k]), best first, equal scores in ascending index, the tail idx -1 / score -inf (+inf for
    'l2') where fewer than k candidates exist.  exclude: optional int32 [Q] (-1: none); base_sq:
    optional fp32 [V] squared base norms."""
    _arr(queries, np.float32, "queries")
    _arr(base, np.float32, "base")
    if queries.ndim != 2 or base.ndim != 2 or queries.shape[1] != base.shape[1]:
        raise ValueError("queries [Q, d] and base [V, d] must share d")
    if metric not in _lib.TOPK_METRICS:
        raise ValueError("metric must be one of %s (got %r)" % (sorted(_lib.TOPK_METRICS), metric))
    Q, d = queries.shape
    V = base.shape[0]
    if exclude is not None:
        _arr(exclude, np.int32, "exclude")
        assert exclude.shape == (Q,)
    if base_sq is not None:
        _arr(base_sq, np.float32, "base_sq")
        assert base_sq.shape == (V,)
    idx = np.empty((Q, int(k)), np.int32)
    score = np.empty((Q, int(k)), np.float32)
    check(_lib.lib().come_cpu_topk(ptr(queries), Q, ptr(base), V, d, int(k),
                                   _lib.TOPK_METRICS[metric],
                                   None if exclude is None else ptr(exclude),
                                   None if base_sq is None else ptr(base_sq), ptr(idx), ptr(score),
                                   _threads(threads)), "come_cpu_topk")
    return idx.astype(np.int64), score
