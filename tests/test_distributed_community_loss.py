"""Community2Vec.loss with distributed=True over two processes (gloo, CPU): every rank evaluates
its shard_range block of the listed rows and the float64 totals are all-reduced.  The HIP kernel
needs a GPU, so the workers swap come_amd.community_embeddings.community_loss for a float64 torch
stand-in of the same sum (as tests/test_distributed_c4.py does for the other kernels); what is
under test is the sharding and the exchange.  The kernel itself: tests/test_gpu_community_loss.py."""
import json
import math
import os
import socket
import types

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from come_amd import community_embeddings as ce

V, D, K = 203, 4, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cpu_community_loss(x, pi, mu, cov, return_rows=False):
    """sum_i sum_k pi_ik log N(x_i; mu_k, cov_k) in float64."""
    x, pi, mu, cov = x.double(), pi.double(), mu.double(), cov.double()
    chol = torch.linalg.cholesky(cov)
    diff = (x[:, None, :] - mu[None]).permute(1, 2, 0)               # [K, d, V]
    y = torch.linalg.solve_triangular(chol, diff, upper=False)        # L^-1 (x - mu)
    log_det = torch.log(torch.diagonal(chol, dim1=-2, dim2=-1)).sum(-1)
    lp = -0.5 * (y ** 2).sum(1) - log_det[:, None] - 0.5 * x.shape[1] * math.log(2 * math.pi)
    rows = (pi * lp.t()).sum(1)
    total = float(rows.sum())
    return (total, rows.float()) if return_rows else total


def _model():
    rng = np.random.RandomState(5)
    m = types.SimpleNamespace()
    m.k, m.vocab_size = K, V
    m.node_embedding = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32))
    m.pi = torch.from_numpy(rng.dirichlet(np.ones(K), V).astype(np.float32))
    m.centroid = torch.from_numpy(rng.standard_normal((K, D)).astype(np.float32))
    A = rng.standard_normal((K, D, D)).astype(np.float32)
    m.covariance_mat = torch.from_numpy(
        (np.einsum("kij,klj->kil", A, A) + np.eye(D, dtype=np.float32)).astype(np.float32))
    m.rows_of = lambda ids: np.asarray(ids, np.int64) - 1  # node id i -> row i-1
    return m


def _run(distributed):
    m = _model()
    c2v = ce.Community2Vec.__new__(ce.Community2Vec)
    c2v.lr, c2v.gmm_backend, c2v.distributed, c2v.group = 0.1, "gpu", distributed, None
    ids = np.concatenate([np.arange(1, V + 1, 3)[::-1], [7, 7, 10]])  # shuffled, with repeats
    return {"full": c2v.loss(np.arange(1, V + 1), m, beta=0.5),
            "sub": c2v.loss(ids, m, beta=0.5, chunksize=11)}


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ce.community_loss = _cpu_community_loss
    with open(os.path.join(out_dir, "r%d.json" % rank), "w") as f:
        json.dump(_run(True), f)
    dist.destroy_process_group()


def test_loss_row_sharded_world2(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    monkeypatch.setattr(ce, "community_loss", _cpu_community_loss)  # undone after the test
    single = _run(False)
    r0, r1 = (json.load(open(os.path.join(str(tmp_path), "r%d.json" % r))) for r in range(world))
    assert r0 == r1  # both ranks return the same value
    for key in ("full", "sub"):
        assert single[key] > 0
        assert abs(r0[key] - single[key]) <= 1e-9 * abs(single[key]), key
    # the stand-in is the documented sum: scipy's logpdf weighted by pi
    from scipy.stats import multivariate_normal
    m = _model()
    x, pi = m.node_embedding.numpy().astype(np.float64), m.pi.numpy().astype(np.float64)
    ref = sum((pi[:, k] * multivariate_normal(m.centroid[k].numpy().astype(np.float64),
                                              m.covariance_mat[k].numpy().astype(np.float64))
               .logpdf(x)).sum() for k in range(K))
    assert abs(single["full"] - abs(ref) * 0.5 / K) <= 1e-9 * abs(ref)
