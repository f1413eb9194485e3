"""k-means on the GPU: the initialisation of come_amd.gmm.GaussianMixture
(``kmeans_backend='native'``) and an estimator of its own for clustering embeddings (what the
reference's users run sklearn.cluster.KMeans for).

One Lloyd iteration is three launches of libcome.so: come_kmeans_lloyd (labels, and the cluster
sums / counts / inertia as per-chunk partials reduced in a fixed order into float64 -- X is read
once, no [V, K] matrix, no float atomics, bit-identical from run to run), and come_kmeans_update
(centres in place, the squared shift into a device double).  The host reads that shift only every
``check_every`` iterations.

The greedy k-means++ seeding in front of them is a chain of torch ops (``kmeans_plusplus``, the
default) or, with ``seeding='native'``, three more entry points per step
(``kmeans_plusplus_native``: come_kmeans_pp_sample, come_kmeans_pp_step, come_kmeans_pp_pick; one
read of X per step, nothing read back to the host; the same distribution, another random stream).

``KMeans`` keeps sklearn's surface for what is used here: ``n_clusters``, ``init`` ('k-means++' or
an array [K, d]), ``n_init``, ``max_iter``, ``tol`` (scaled by the mean feature variance, sklearn's
_tolerance), ``random_state``; ``fit`` / ``fit_predict`` / ``predict``; ``cluster_centers_``,
``labels_``, ``inertia_``, ``n_iter_``.  Two rules differ from sklearn's and follow
GaussianMixture._kmeans_labels: a cluster that loses all its rows keeps its centre (no
relocation), and the seeding draws from a device generator.

``distributed=True``: every rank passes its shard of the rows; seeding runs on rank 0's shard and
the centres are broadcast; the variance statistics, and each iteration's counts, sums and inertia,
are all-reduced, so every rank holds the same centres after every iteration.
"""
import math

import numpy as np

from . import _lib
from ._lib import check, ptr, stream_handle
from .distributed import all_reduce_sum, world_of


def scratch_plan(V, d, K, cus=0):
    """(chunks, rows_per_chunk) of come_kmeans_lloyd for V rows on a device with `cus` compute
    units: the partial sums take chunks * K * d * 4 bytes (<= 128 MB), and at most rows_per_chunk
    rows are summed in fp32 before the float64 reduction."""
    import ctypes
    chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.lib().come_kmeans_scratch(int(V), int(d), int(K), int(cus), ctypes.byref(chunks),
                                         ctypes.byref(rows)), "come_kmeans_scratch")
    return chunks.value, rows.value


def _cus(device):
    import torch
    return torch.cuda.get_device_properties(device).multi_processor_count


def assign(X, C):
    """(labels int64 [V], mindist fp32 [V]) of device fp32 rows X [V, d] for centres C [K, d]."""
    import torch
    V, d = X.shape
    K = C.shape[0]
    labels = torch.empty((V,), dtype=torch.int32, device=X.device)
    mind = torch.empty((V,), dtype=torch.float32, device=X.device)
    check(_lib.lib().come_kmeans_assign(ptr(X), V, d, ptr(C), K, ptr(labels), ptr(mind),
                                        stream_handle(X.device)), "come_kmeans_assign")
    return labels.long(), mind


def accumulate(X, C, return_mindist=False):
    """One assignment pass with its sufficient statistics: (labels int32 [V], sums float64 [K, d],
    counts int64 [K], inertia float64 scalar), all on the device (plus mindist fp32 [V] when
    asked)."""
    import torch
    V, d = X.shape
    K = C.shape[0]
    dev = X.device
    chunks, _ = scratch_plan(V, d, K, _cus(dev))
    scratch = torch.empty((chunks * (2 + K * d + K),), dtype=torch.int32, device=dev)
    labels = torch.empty((V,), dtype=torch.int32, device=dev)
    mind = torch.empty((V,), dtype=torch.float32, device=dev) if return_mindist else None
    sums = torch.empty((K, d), dtype=torch.float64, device=dev)
    counts = torch.empty((K,), dtype=torch.int64, device=dev)
    inertia = torch.empty((), dtype=torch.float64, device=dev)
    check(_lib.lib().come_kmeans_lloyd(ptr(X), V, d, ptr(C), K, chunks, ptr(scratch), ptr(labels),
                                       ptr(mind) if return_mindist else None, ptr(sums),
                                       ptr(counts), ptr(inertia), stream_handle(dev)),
          "come_kmeans_lloyd")
    if return_mindist:
        return labels, sums, counts, inertia, mind
    return labels, sums, counts, inertia


def update(C, sums, counts):
    """C[k] = sums[k] / counts[k] in place (a cluster with count 0 keeps its centre); returns the
    squared shift sum (new - old)^2 as a device float64 scalar -- no host read."""
    import torch
    K, d = C.shape
    stats = torch.zeros((2,), dtype=torch.float64, device=C.device)
    check(_lib.lib().come_kmeans_update(ptr(C), ptr(sums), ptr(counts), K, d, ptr(stats),
                                        stream_handle(C.device)), "come_kmeans_update")
    return stats[0]


def kmeans_plusplus(X, xx, K, gen):
    """sklearn's greedy k-means++ seeding (2 + log K local trials) on the rows X: [K, d] centres.
    The arithmetic and the generator draws of GaussianMixture._kmeans_plusplus, in the same order;
    the best candidate of a step is chosen on the device (argmin, index_select), so no step reads
    anything back to the host."""
    import torch
    V, d = X.shape
    if V < K:
        raise ValueError("k-means++ seeding needs >= n_clusters rows on rank 0")
    trials = 2 + int(math.log(K))
    first = torch.randint(0, V, (1,), generator=gen, device=X.device)
    c0 = X.index_select(0, first)[0]
    centers = [c0]
    closest = (xx - 2 * X @ c0 + c0.dot(c0)).clamp_min(0)
    pot = closest.sum()
    for _ in range(1, K):
        r = torch.rand(trials, generator=gen, device=X.device, dtype=torch.float64) * pot
        cand = torch.searchsorted(torch.cumsum(closest.double(), 0), r).clamp_max(V - 1)
        C = X.index_select(0, cand)
        dist = (xx[:, None] - 2 * X @ C.t() + (C * C).sum(1)[None]).clamp_min(0)
        dist = torch.minimum(dist, closest[:, None])
        pots = dist.sum(0)
        best = torch.argmin(pots).reshape(1)
        closest = dist.index_select(1, best)[:, 0].contiguous()
        pot = pots.index_select(0, best)[0]
        centers.append(C.index_select(0, best)[0])
    return torch.stack(centers)


def pp_plan(V, d, T, cus=0):
    """(chunks, rows_per_chunk) of the native seeding's pass over V rows with T candidates on a
    device with `cus` compute units (come_kmeans_pp_scratch): chunks * T * 8 bytes <= 2 MB."""
    import ctypes
    chunks, rows = ctypes.c_int(0), ctypes.c_int(0)
    check(_lib.lib().come_kmeans_pp_scratch(int(V), int(d), int(T), int(cus), ctypes.byref(chunks),
                                            ctypes.byref(rows)), "come_kmeans_pp_scratch")
    return chunks.value, rows.value


def pp_step(X, closest, cand, chunks, out=None):
    """The seeding's one pass over X for the candidates `cand` (device int32 [T], rows of X):
    (dist fp32 [V, T] = min(closest, squared distance to each candidate), ppot float64 [chunks, T]
    its per-chunk column sums, pots float64 [T] their totals).  closest: device fp32 [V] or None
    (+inf).  `out` = (dist, ppot, pots) to write into."""
    import torch
    V, d = X.shape
    T = cand.shape[0]
    if out is None:
        out = (torch.empty((V, T), dtype=torch.float32, device=X.device),
               torch.empty((chunks, T), dtype=torch.float64, device=X.device),
               torch.empty((T,), dtype=torch.float64, device=X.device))
    dist, ppot, pots = out
    check(_lib.lib().come_kmeans_pp_step(ptr(X), V, d, None if closest is None else ptr(closest),
                                         ptr(cand), T, chunks, ptr(dist), ptr(ppot), ptr(pots),
                                         stream_handle(X.device)), "come_kmeans_pp_step")
    return dist, ppot, pots


def pp_pick(dist, ppot, pots, out=None):
    """The best candidate of a step: (closest fp32 [V] = its column of dist, cpot float64 [chunks]
    = its column of ppot, best int32 [1] = argmin pots with ties to the lowest index, pot float64
    [1] = pots[best]), all on the device.  `out` = (closest, cpot, best, pot) to write into."""
    import torch
    V, T = dist.shape
    chunks = ppot.shape[0]
    if out is None:
        out = (torch.empty((V,), dtype=torch.float32, device=dist.device),
               torch.empty((chunks,), dtype=torch.float64, device=dist.device),
               torch.empty((1,), dtype=torch.int32, device=dist.device),
               torch.empty((1,), dtype=torch.float64, device=dist.device))
    closest, cpot, best, pot = out
    check(_lib.lib().come_kmeans_pp_pick(ptr(dist), V, T, ptr(ppot), ptr(pots), chunks,
                                         ptr(closest), ptr(cpot), ptr(best), ptr(pot),
                                         stream_handle(dist.device)), "come_kmeans_pp_pick")
    return closest, cpot, best, pot


def pp_sample(closest, cpot, rows_per_chunk, u, out=None):
    """Rows drawn with probability proportional to `closest`: for each u[t] (device float64 in
    [0, 1)) the first row whose float64 cumulative sum of closest reaches u[t] * its total; device
    int32 [T].  cpot / rows_per_chunk: the chunk sums of closest (pp_step, pp_pick) and pp_plan's
    rows per chunk.  A row with closest == 0 is never returned for u > 0 unless all are 0."""
    import torch
    V = closest.shape[0]
    T = u.shape[0]
    if out is None:
        out = torch.empty((T,), dtype=torch.int32, device=closest.device)
    check(_lib.lib().come_kmeans_pp_sample(ptr(closest), V, ptr(cpot), cpot.shape[0],
                                           int(rows_per_chunk), ptr(u), T, ptr(out),
                                           stream_handle(closest.device)), "come_kmeans_pp_sample")
    return out


def kmeans_plusplus_native(X, K, gen, first=None, u=None, return_trace=False):
    """sklearn's greedy k-means++ seeding (2 + log K local trials) on the kernels of libcome.so:
    [K, d] centres, rows of X.  Each of the K - 1 steps is one read of X (come_kmeans_pp_step: the
    candidates' distances summed from squared differences, no [V, d] x [d, trials] product), the
    choice of the candidate of lowest potential (come_kmeans_pp_pick) and the draw of the next
    candidates from the float64 cumulative sum (come_kmeans_pp_sample); nothing is read back to the
    host and all scratch is allocated before the loop.

    The distribution is that of ``kmeans_plusplus``; the random stream is not: the first centre is
    one ``torch.randint`` draw from `gen` (or `first`, device int64 [1]) and all uniforms are one
    ``torch.rand`` [K - 1, trials] float64 from `gen` (or `u`), drawn up front, not once per step,
    and the distances carry another fp32 rounding.  The same seed therefore gives other centres
    than the torch seeding.

    return_trace=True: (centres, chosen int64 [K], candidates int32 [K - 1, trials], potentials
    float64 [K - 1, trials], best int32 [K - 1]), all on the device."""
    import torch
    V, d = X.shape
    if V < K:
        raise ValueError("k-means++ seeding needs >= n_clusters rows on rank 0")
    if X.dtype != torch.float32 or not X.is_contiguous():
        raise ValueError("X must be a contiguous float32 array")
    dev = X.device
    trials = 2 + int(math.log(K))
    if first is None:
        first = torch.randint(0, V, (1,), generator=gen, device=dev)
    if u is None:
        u = torch.rand((K - 1, trials), generator=gen, device=dev, dtype=torch.float64)
    if tuple(u.shape) != (K - 1, trials) or u.dtype != torch.float64 or not u.is_contiguous():
        raise ValueError("u must be a contiguous float64 array [%d, %d]" % (K - 1, trials))
    chunks, rows = pp_plan(V, d, trials, _cus(dev))
    closest = torch.empty((V,), dtype=torch.float32, device=dev)
    cpot = torch.empty((chunks,), dtype=torch.float64, device=dev)
    pot = torch.empty((1,), dtype=torch.float64, device=dev)
    step_out = (torch.empty((V, trials), dtype=torch.float32, device=dev),
                torch.empty((chunks, trials), dtype=torch.float64, device=dev))
    cands = torch.empty((max(K - 1, 1), trials), dtype=torch.int32, device=dev)
    pots = torch.empty((max(K - 1, 1), trials), dtype=torch.float64, device=dev)
    best = torch.empty((max(K - 1, 1),), dtype=torch.int32, device=dev)
    # the first centre: one candidate against +inf writes closest and its chunk sums directly
    pp_step(X, None, first.to(torch.int32), chunks, out=(closest.view(V, 1), cpot.view(chunks, 1),
                                                         pot))
    # pp_sample, pp_step and pp_pick on raw addresses: K - 1 rounds of three calls, with no tensor
    # view or stream lookup between them (the host's share of a round would otherwise exceed the
    # kernels')
    L, stream = _lib.lib(), stream_handle(dev)
    a_x, a_closest, a_cpot, a_pot, a_dist, a_ppot, a_u, a_cands, a_pots, a_best = (
        t.data_ptr() for t in (X, closest, cpot, pot, step_out[0], step_out[1], u, cands, pots,
                               best))
    for k in range(K - 1):
        a_c, a_p = a_cands + 4 * trials * k, a_pots + 8 * trials * k
        rc = L.come_kmeans_pp_sample(a_closest, V, a_cpot, chunks, rows, a_u + 8 * trials * k,
                                     trials, a_c, stream)
        rc = rc or L.come_kmeans_pp_step(a_x, V, d, a_closest, a_c, trials, chunks, a_dist,
                                         a_ppot, a_p, stream)
        rc = rc or L.come_kmeans_pp_pick(a_dist, V, trials, a_ppot, a_p, chunks, a_closest,
                                         a_cpot, a_best + 4 * k, a_pot, stream)
        check(rc, "come_kmeans_pp_sample / _step / _pick")
    cands, pots, best = cands[:K - 1], pots[:K - 1], best[:K - 1]
    chosen = torch.cat([first.long(), cands.long().gather(1, best.long()[:, None])[:, 0]])
    centers = X.index_select(0, chosen)
    if return_trace:
        return centers, chosen, cands, pots, best
    return centers


class KMeans(object):
    def __init__(self, n_clusters=8, init='k-means++', n_init=1, max_iter=300, tol=1e-4,
                 random_state=None, check_every=4, device=None, distributed=False, group=None,
                 seeding='torch'):
        if isinstance(init, str) and init != 'k-means++':
            raise ValueError("init must be 'k-means++' or an array [n_clusters, d]")
        if seeding not in ('torch', 'native'):
            raise ValueError("seeding must be 'torch' or 'native'")
        self.seeding = seeding
        if int(check_every) < 1:
            raise ValueError("check_every must be >= 1")
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.random_state = random_state
        self.check_every = int(check_every)
        self.device = device
        self.distributed = bool(distributed)
        self.group = group

    def _rank_world(self):
        return world_of(self.group) if self.distributed else (0, 1)

    def _prepare_x(self, X):
        from .gmm import _as_device_x
        return _as_device_x(X, self.device)

    def _generator(self, device):
        import torch
        g = torch.Generator(device=device)
        rs = self.random_state
        if rs is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        elif isinstance(rs, (int, np.integer)):
            seed = int(rs)
        else:
            seed = int(rs.randint(0, 2 ** 31 - 1))
        if self._rank_world()[1] > 1:  # one stream for the job: rank 0's seed
            import torch.distributed as dist
            t = torch.tensor([seed], dtype=torch.int64, device=device)
            dist.broadcast(t, 0, group=self.group)
            seed = int(t[0])
        g.manual_seed(seed)
        return g

    def _tolerance(self, X):
        """tol * the mean feature variance (np.var, ddof 0) over all ranks' rows."""
        import torch
        if self._rank_world()[1] == 1:
            return self.tol * float(X.var(0, unbiased=False).mean())
        s1 = X.sum(0, dtype=torch.float64)
        s2 = (X.double() ** 2).sum(0)
        n = torch.tensor([float(X.shape[0])], dtype=torch.float64, device=X.device)
        all_reduce_sum([s1, s2, n], self.group)
        n = float(n[0])
        return self.tol * float(((s2 - s1 * s1 / n) / n).mean())

    def _seed(self, X, xx, gen):
        import torch
        K, d = self.n_clusters, X.shape[1]
        if not isinstance(self.init, str):
            C = torch.as_tensor(np.asarray(self.init, np.float32)).to(X.device)
            if tuple(C.shape) != (K, d):
                raise ValueError("init must have shape (%d, %d)" % (K, d))
            return C.contiguous().clone()
        rank, world = self._rank_world()
        if rank == 0 and self.seeding == 'native':
            C = kmeans_plusplus_native(X, K, gen).contiguous()
        elif rank == 0:
            C = kmeans_plusplus(X, xx, K, gen).contiguous()
        else:
            C = torch.empty((K, d), dtype=torch.float32, device=X.device)
        if world > 1:
            import torch.distributed as dist
            dist.broadcast(C, 0, group=self.group)
        return C

    def _fit_device(self, X, gen):
        """Lloyd from n_init seedings on device rows X; keeps the run of lowest inertia.  Sets
        _centers (device fp32 [K, d]), _labels (device int64 [V]) and the fitted scalars."""
        import torch
        V, d = X.shape
        K = self.n_clusters
        if d > 512 or K > (4096 if d in (64, 128) or d > 128 else 64) or K < 1:
            raise ValueError("GPU KMeans supports d <= 512 and 1 <= n_clusters <= 64 (<= 4096 for "
                             "d = 64, 128 and d > 128)")
        world = self._rank_world()[1]
        tol = self._tolerance(X)
        xx = (X * X).sum(1) if isinstance(self.init, str) and self.seeding == 'torch' else None
        best = None
        for _ in range(self.n_init if isinstance(self.init, str) else 1):
            C = self._seed(X, xx, gen)
            history, shifts, n_iter = [], [], 0
            while n_iter < self.max_iter:
                _, sums, counts, inertia = accumulate(X, C)
                if world > 1:
                    all_reduce_sum([counts, sums, inertia], self.group)
                shift2 = update(C, sums, counts)
                history.append(inertia)
                shifts.append(shift2)
                n_iter += 1
                # the only host read of the loop, every check_every iterations
                if (n_iter % self.check_every == 0 or n_iter == self.max_iter) \
                        and float(shift2) <= tol:
                    break
            labels, mind = assign(X, C)
            total = mind.sum(dtype=torch.float64)
            if world > 1:
                all_reduce_sum([total], self.group)
            total = float(total)
            if best is None or total < best[0]:
                best = (total, C, labels, n_iter, history, shifts)
        self.inertia_, self._centers, self._labels, self.n_iter_, history, shifts = best
        self.tol_ = tol
        if history:
            both = torch.stack([torch.stack(history), torch.stack(shifts)]).cpu().numpy()
            self.inertia_history_, self.shift2_history_ = both[0], both[1]
        else:
            self.inertia_history_ = self.shift2_history_ = np.zeros(0)
        return self

    def fit(self, X, y=None):
        X = self._prepare_x(X)
        self._fit_device(X, self._generator(X.device))
        self.cluster_centers_ = self._centers.cpu().numpy()
        self.labels_ = self._labels.cpu().numpy()
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        X = self._prepare_x(X)
        return assign(X, self._centers)[0].cpu().numpy()
