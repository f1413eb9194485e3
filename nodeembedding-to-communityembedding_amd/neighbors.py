"""Exact top-k neighbour search over embedding tables on the GPU: what a user of the trained
``node_embedding`` runs first (most similar nodes, a k-nearest-neighbour graph, retrieval for link
prediction), and the same over ``centroid`` for "which nodes sit nearest community k".

One search is come_topk (csrc/come_topk.hip): query tiles x base chunks, a k-entry list per query
and chunk, then a merge.  No [Q, V] score matrix exists -- the scratch is chunks * Q * k * 8 bytes
(plus 4 V for the base norms when none are cached) -- and no float atomics run, so a result is
bit-identical from run to run.

    topk(queries, base, k, metric)            -> (idx int64 [Q, k], score fp32 [Q, k]), best first
    Index(base, metric).search(queries, k)    the same with the base norms computed once
    knn_graph(X, k, metric, batch)            every row's k neighbours, the row itself excluded
    cpu_topk(...)                             the CPU twin on numpy arrays (come_amd.cpu.topk)

Metrics: 'dot' (larger is better), 'cosine' (a zero row scores 0), 'l2' (squared distance, smaller
is better).  Equal scores come in ascending index; a NaN score is never returned; where fewer than
k candidates exist the tail is idx -1 with score -inf (+inf for 'l2').  k <= 64, fp32 tables.
"""
import ctypes

from . import _lib
from ._lib import TOPK_METRICS, check, ptr, stream_handle
from .cpu import topk as cpu_topk  # noqa: F401

DEFAULT_BATCH = 16384  # knn_graph's queries per search


def _metric(metric):
    if metric not in TOPK_METRICS:
        raise ValueError("metric must be one of %s (got %r)" % (sorted(TOPK_METRICS), metric))
    return TOPK_METRICS[metric]


def plan(Q, V, d, k, cus=0):
    """(chunks, rows_per_chunk) of come_topk for Q queries against V rows on a device with `cus`
    compute units (come_topk_scratch): chunks <= 64, rows_per_chunk a multiple of the 32-row base
    tile."""
    chunks, rows = ctypes.c_int(0), ctypes.c_int64(0)
    check(_lib.lib().come_topk_scratch(int(Q), int(V), int(d), int(k), int(cus),
                                       ctypes.byref(chunks), ctypes.byref(rows)),
          "come_topk_scratch")
    return chunks.value, rows.value


def scratch_bytes(Q, V, k, chunks, have_base_sq):
    """Bytes of come_topk's scratch: the chunks' lists, and the base norms when none are passed."""
    return chunks * int(Q) * int(k) * 8 + (0 if have_base_sq else 4 * int(V))


def _table(t, name):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError("%s must be a CUDA fp32 tensor [rows, d]" % name)
    return t if t.is_contiguous() else t.contiguous()


def row_sqnorms(X):
    """|x_r|^2 per row of a device fp32 table [V, d] (come_row_sqnorms): fp32 [V]."""
    import torch
    X = _table(X, "X")
    out = torch.empty((X.shape[0],), dtype=torch.float32, device=X.device)
    check(_lib.lib().come_row_sqnorms(ptr(X), X.shape[0], X.shape[1], ptr(out),
                                      stream_handle(X.device)), "come_row_sqnorms")
    return out


def topk(queries, base, k, metric='cosine', exclude=None, base_sq=None, chunks=None):
    """The k best rows of `base` [V, d] for every row of `queries` [Q, d] (device fp32 tensors):
    (idx int64 [Q, k], score fp32 [Q, k]), best first.  exclude: optional device integer tensor
    [Q], the base row each query must not return (-1: none).  base_sq: row_sqnorms(base), for a
    table searched more than once.  chunks: the number of base chunks (default: the plan's)."""
    import torch
    queries, base = _table(queries, "queries"), _table(base, "base")
    Q, d = queries.shape
    V = base.shape[0]
    if base.shape[1] != d or base.device != queries.device:
        raise ValueError("queries [Q, d] and base [V, d] must share d and the device")
    if Q < 1:
        raise ValueError("topk needs at least one query")
    m = _metric(metric)
    dev = queries.device
    if chunks is None:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        chunks, _ = plan(Q, V, d, k, cus)
    if exclude is not None:
        if exclude.shape != (Q,) or exclude.device != dev:
            raise ValueError("exclude must be a device tensor [Q]")
        exclude = exclude.to(torch.int32).contiguous()
    if base_sq is not None:
        if base_sq.shape != (V,) or base_sq.dtype != torch.float32 or base_sq.device != dev:
            raise ValueError("base_sq must be a device fp32 tensor [V]")
        base_sq = base_sq.contiguous()
    nbytes = scratch_bytes(Q, V, k, int(chunks), base_sq is not None)
    scratch = torch.empty((max(1, nbytes // 4),), dtype=torch.int32, device=dev)
    idx = torch.empty((Q, int(k)), dtype=torch.int32, device=dev)
    score = torch.empty((Q, int(k)), dtype=torch.float32, device=dev)
    check(_lib.lib().come_topk(ptr(queries), Q, ptr(base), V, d, int(k), m,
                               None if exclude is None else ptr(exclude),
                               None if base_sq is None else ptr(base_sq), int(chunks),
                               ptr(scratch), ptr(idx), ptr(score), stream_handle(dev)),
          "come_topk")
    return idx.long(), score


class Index(object):
    """A table searched many times: the base rows' squared norms are computed once."""

    def __init__(self, base, metric='cosine'):
        _metric(metric)
        self.base = _table(base, "base")
        self.metric = metric
        self.base_sq = None if metric == 'dot' else row_sqnorms(self.base)

    def search(self, queries, k, exclude=None):
        return topk(queries, self.base, k, metric=self.metric, exclude=exclude,
                    base_sq=self.base_sq)


def knn_graph(X, k, metric='cosine', batch=None):
    """Every row's k nearest other rows of the device table X [V, d]: (idx int64 [V, k], score fp32
    [V, k]).  The queries go `batch` rows at a time (default 16,384), so the scratch stays at
    chunks * batch * k * 8 bytes whatever V is."""
    import torch
    index = Index(X, metric)
    V = index.base.shape[0]
    batch = DEFAULT_BATCH if batch is None else int(batch)
    if batch < 1:
        raise ValueError("batch must be >= 1")
    idx = torch.empty((V, int(k)), dtype=torch.int64, device=index.base.device)
    score = torch.empty((V, int(k)), dtype=torch.float32, device=index.base.device)
    for r0 in range(0, V, batch):
        r1 = min(V, r0 + batch)
        own = torch.arange(r0, r1, dtype=torch.int32, device=index.base.device)
        idx[r0:r1], score[r0:r1] = index.search(index.base[r0:r1], k, exclude=own)
    return idx, score
