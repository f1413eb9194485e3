"""O1 (first-order, edges) trainer -- reference: ADSCModel/node_embeddings.py.

``Node2Vec(lr, workers, negative).train(model, edges, chunksize, iter)`` keeps the reference
signature (:19-106): the edge list is repeated ``iter`` times (RepeatCorpusNTimes, :47), every
edge draws its own next_random from the global numpy RNG in edge order (pyx:427), and each edge
trains the pairs (edge[0] -> edge[1]) then (edge[1] -> edge[0]) on node_embedding only
(pyx:444-448).  One launch per pass over the edges (passes stay ordered), one wavefront per edge
(Hogwild across edges) or, with ``deterministic=True``, one wavefront in edge order (== the
reference with workers=1).  ``loss`` reproduces :26-31 (-sum log sigma(u.v) over the edges;
``backend='native'`` evaluates it in one kernel launch).

Edge weights (``train(..., weights=)``, ``loss(..., weights=)``): the weighted first-order
objective sum_e w_e log sigma(x_u . x_v) is trained by edge sampling -- each pass draws edges with
probability w_e / W on the device (training_sdg_inner.edge_cdf / sample_edges) and trains the
draws with the same launch and the plain step.  Without weights nothing changes.

Multi-GPU (``distributed=True``): every rank is handed the same edge list, draws
every edge's seed per pass (the global numpy RNG advances as in one process), trains its
contiguous shard of each pass and exchanges its node_embedding progress with the other ranks
after every ``sync_edges`` of its edges and at the end of each pass (DeltaAllReduce over RCCL,
combine rule touched_mean as Context2Vec's; blocking: an O1 pass is ~1 ms at C2).
"""
import logging as log
import time

import numpy as np

from . import training_sdg_inner as tsi


class _SeedUpload(object):
    """Every edge's seed for one pass (training_sdg_inner.draw_seeds: the global numpy RNG, pyx:427)
    drawn straight into one of two pinned host buffers and copied to the device asynchronously, so
    the host draws pass p + 1's seeds while pass p trains (a pageable copy would wait for the
    launch before it).  A buffer is rewritten only after its previous copy has completed."""

    def __init__(self, dev):
        self.dev = dev
        self.bufs = [None, None]
        self.events = [None, None]
        self.k = 0

    def __call__(self, n):
        import torch
        if self.dev.type != "cuda":
            return torch.from_numpy(tsi.draw_seeds(n).view(np.int64))
        i = self.k % 2
        self.k += 1
        if self.bufs[i] is None or self.bufs[i].numel() != n:
            self.bufs[i] = torch.empty(n, dtype=torch.int64, pin_memory=True)
            self.events[i] = None
        if self.events[i] is not None:
            self.events[i].synchronize()
        tsi.draw_seeds(n, out=self.bufs[i].numpy().view(np.uint64))
        d = self.bufs[i].to(self.dev, non_blocking=True)
        self.events[i] = torch.cuda.Event()
        self.events[i].record(torch.cuda.current_stream(self.dev))
        return d


class Node2Vec(object):
    def __init__(self, lr=0.2, workers=1, negative=0, deterministic=False, distributed=False,
                 sync_edges=None, group=None, combine="touched_mean"):
        self.workers = workers
        self.lr = float(lr)
        self.negative = negative
        self.window_size = 1
        self.deterministic = deterministic
        self.distributed = bool(distributed)
        self.sync_edges = None if sync_edges is None else int(sync_edges)
        self.group = group
        self.combine = combine  # as Context2Vec's
        self._exchanges = {}
        if self.distributed and self.deterministic:
            raise ValueError("distributed=True trains Hogwild shards; deterministic=True is the "
                             "one-wavefront parity mode")

    def exchange(self, model):
        """Delta exchange of model.node_embedding (cached), based on the table as it is now."""
        from .distributed import DeltaAllReduce
        key = id(model.node_embedding)
        ex = self._exchanges.get(key)
        if ex is None:
            self._exchanges = {key: DeltaAllReduce([model.node_embedding], group=self.group,
                                                   combine=self.combine)}
            return self._exchanges[key]
        ex.reset()
        return ex

    def _edge_rows(self, model, edges):
        """Edges -> [E, 2] int32 rows as prepare_sentences would pass them to train_o1: OOV
        endpoints dropped and, with down-sampling, each endpoint kept by the reference's draw
        (embedding.py:126-136; the draws are consumed edge by edge, endpoint by endpoint).  An
        edge left with fewer than two endpoints makes the reference read an uninitialised index
        (pyx:433-440, undefined behaviour): such edges are skipped (-1)."""
        e = np.asarray(edges, np.int64).reshape(-1, 2)
        rows = model.rows_of(e.reshape(-1)).reshape(-1, 2)
        if model.down_sampling:
            from .embedding import downsample_rows
            kept = downsample_rows(model, [r[r >= 0] for r in rows])
            rows = np.array([k if len(k) == 2 else (-1, -1) for k in kept],
                            np.int64).reshape(-1, 2)
        bad = (rows < 0).any(axis=1)
        rows[bad] = -1
        return rows.astype(np.int32)

    def loss(self, model, edges, backend='torch', weights=None):
        """-sum log sigma(x_v . x_u) over the valid edges (:26-31).  backend 'torch' (default): a
        gather-multiply-sum chain with two [E x d] temporaries; 'native': one
        training_sdg_inner.sgns_pairs_loss launch (no negatives, no temporaries; the trainer's
        fp32 dot order, float64 softplus).  ``weights`` (one per row of ``edges``): the weighted
        first-order objective -sum_e w_e log sigma(x_u . x_v) instead -- the per-edge terms of the
        same launch / chain times the weights, summed in float64 on the device."""
        import torch
        dev = model.node_embedding.device
        if weights is not None:
            w = np.ascontiguousarray(weights, np.float64).reshape(-1)
            if len(w) != len(np.asarray(edges).reshape(-1, 2)):
                raise ValueError("weights must hold one value per row of edges")
            w = torch.from_numpy(w).to(dev)
        if backend == 'native':
            rows = torch.from_numpy(self._edge_rows(model, edges)).to(dev)
            x = model.node_embedding
            r0, r1 = rows[:, 0].contiguous(), rows[:, 1].contiguous()
            if weights is None:
                return tsi.sgns_pairs_loss(x, x, r0, r1)[0]
            per = tsi.sgns_pairs_loss(x, x, r0, r1, return_pairs=True)[2]
            return float((per * w)[rows[:, 0] >= 0].sum())
        if backend != 'torch':
            raise ValueError("backend must be 'torch' or 'native'")
        rows = torch.from_numpy(self._edge_rows(model, edges)).to(dev)
        ok = (rows >= 0).all(dim=1)
        rows = rows[ok].long()
        x = model.node_embedding
        dots = (x[rows[:, 1]] * x[rows[:, 0]]).sum(dim=1).double()
        if weights is None:
            return float(-torch.nn.functional.logsigmoid(dots).sum())
        return float(-(torch.nn.functional.logsigmoid(dots) * w[ok]).sum())

    def _weighted_cdf(self, rows, weights, dev):
        """(ecdf, positive rows) of one pass: the weights of skipped rows (-1: an OOV or
        down-sampled endpoint) set to 0, then training_sdg_inner.edge_cdf on the device."""
        import torch
        w = np.array(weights, np.float32).reshape(-1)
        if len(w) != rows.shape[0]:
            raise ValueError("weights must hold one value per row of edges")
        w[rows[:, 0] < 0] = 0.0
        return tsi.edge_cdf(torch.from_numpy(w).to(dev)), int((w > 0).sum())

    def train(self, model, edges, chunksize=150, iter=1, weights=None, samples=None, seed=None):
        """One pass over ``edges`` per ``iter``, every edge once (see the module docstring).

        ``weights`` (one value >= 0 per row of ``edges``): edge sampling for the weighted
        first-order objective sum_e w_e log sigma(x_u . x_v) + negatives.  Each pass draws
        ``samples`` edges (default: the number of rows with positive weight) with probability
        w_e / W, with replacement, on the device (training_sdg_inner.edge_cdf once per call --
        once per pass with down-sampling -- then sample_edges) and trains the draws with the plain
        step, per-sample seeds from draw_seeds exactly as a pass over ``samples`` edges.  Rows
        with an OOV or down-sampled endpoint get weight 0.  The draws of pass k come from the
        Philox stream ``seed + k``; ``seed=None`` takes one 64-bit value per pass from the global
        numpy RNG (``np.random.randint(0, 2 ** 64, dtype=np.uint64)``), before that pass's
        draw_seeds.  ``deterministic=True`` trains the same draws in order on one wavefront.
        ``distributed=True`` needs no new exchange: every rank draws the identical sample list
        (as every rank draws every edge's seed) and trains its contiguous shard of it.  Build the
        model's counts from strengths (CSRGraph.degree_by_id(weighted=True)): the endpoints of
        sampled edges appear in proportion to strength.  Without ``weights`` nothing changes, the
        global numpy RNG's draws included.  Returns the pairs trained."""
        import torch
        assert model.node_embedding.dtype == torch.float32
        if weights is None and (samples is not None or seed is not None):
            raise ValueError("samples and seed belong to edge sampling: pass weights")
        start = time.time()
        rows = self._edge_rows(model, edges)
        dev = model.node_embedding.device
        ed = torch.from_numpy(rows).to(dev)
        mode = tsi.MODE_SEQUENTIAL if self.deterministic else tsi.MODE_HOGWILD
        hot = None if self.deterministic else model.hot_rows()
        from .distributed import shard_range, world_of
        rank, world = world_of(self.group) if self.distributed else (0, 1)
        ex = self.exchange(model) if world > 1 else None
        pairs = 0
        n_valid = None
        seeds_to = _SeedUpload(dev)
        ecdf = None
        for it in range(int(iter)):
            if it > 0 and model.down_sampling:  # every pass draws its own sample (:47)
                rows = self._edge_rows(model, edges)
                ed = torch.from_numpy(rows).to(dev)
                n_valid = None
                ecdf = None
            if weights is None:
                batch, n = ed, rows.shape[0]
            else:  # this pass's corpus: n draws by weight, every one a valid edge
                if ecdf is None:
                    ecdf, positive = self._weighted_cdf(rows, weights, dev)
                n = positive if samples is None else int(samples)
                s64 = (int(np.random.randint(0, 2 ** 64, dtype=np.uint64)) if seed is None
                       else int(seed) + it)
                batch = tsi.sample_edges(ed, ecdf, n, s64)
            lo, hi = shard_range(n, rank, world)
            if weights is not None:
                n_valid = 2 * (hi - lo)
            elif n_valid is None:
                n_valid = 2 * int((rows[lo:hi] >= 0).all(axis=1).sum())
            pairs += n_valid
            sd = seeds_to(n)
            if ex is None:
                tsi.sgns_o1(model.node_embedding, batch, sd, self.negative,
                            model.negative_table(), self.lr, mode, hot=hot)
                continue
            # every rank makes the same number of exchanges per pass (rank 0's shard is largest)
            per = self.sync_edges or max(1, shard_range(n, 0, world)[1])
            for b in range(max(1, -(-shard_range(n, 0, world)[1] // per))):
                s, e = min(hi, lo + b * per), min(hi, lo + (b + 1) * per)
                if e > s:
                    tsi.sgns_o1(model.node_embedding, batch[s:e], sd[s:e], self.negative,
                                model.negative_table(), self.lr, mode, hot=hot)
                ex.sync()
        if model.node_embedding.is_cuda:
            torch.cuda.synchronize(dev)
        elapsed = time.time() - start
        log.info("O1 training: %i pair updates took %.2fs, %.0f pairs/s", pairs, elapsed,
                 pairs / elapsed if elapsed else 0.0)
        return pairs
