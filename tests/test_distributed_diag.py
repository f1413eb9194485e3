"""covariance_type='diag' with distributed=True over two processes (gloo, CPU): the EM all-reduces
nk and resp^T X, then the K d scatter sums; Community2Vec shards loss / train by rows.  The HIP
kernels need a GPU, so the workers swap the come_amd wrappers for float64 torch stand-ins of the
same sums (the tests/test_distributed_community_loss.py pattern); what is under test is the
sharding and the exchange.  The kernels themselves: tests/test_gpu_diag.py."""
import math
import os
import socket
import types

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from come_amd import community_embeddings as ce
from come_amd import gmm
from come_amd.distributed import shard_range

V, D, K = 203, 4, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- float64 stand-ins for the HIP entry points ------------------------------------------------
def _logp(X, ps, mp_, ln):
    y = X.double()[:, None, :] * ps.double()[None] - mp_.double()[None]
    return ln.double()[None] - 0.5 * (y * y).sum(-1)


def _cpu_estep_diag(X, ps, mp_, ln, want_resp=True):
    logp = _logp(X, ps, mp_, ln)
    lse = torch.logsumexp(logp, 1)
    return (torch.exp(logp - lse[:, None]).float() if want_resp else None), lse.float()


def _cpu_moments(X, resp, chunks=None):
    return resp.double().sum(0), resp.double().t() @ X.double()


def _cpu_scatter(X, resp, means, chunks=None):
    diff = X.double()[:, None, :] - means.float().double()[None]
    return (resp.double()[:, :, None] * diff * diff).sum(0)


def _cpu_grad_diag(x, pi, mu, iv, beta, lr, iters):
    coef = float(np.float32(beta / mu.shape[0]))
    y = x.double()
    for _ in range(iters):
        g = (pi.double()[:, :, None] * (iv.double()[None] * (y[:, None, :] - mu.double()[None])))
        y = y - torch.clamp(g.sum(1) * coef, -5, 5) * float(np.float32(lr))
    x.copy_(y.float())


def _cpu_loss_diag(x, pi, mu, var, return_rows=False):
    ps = 1.0 / torch.sqrt(var.double())
    ln = torch.log(ps).sum(-1) - 0.5 * x.shape[1] * math.log(2 * math.pi)
    rows = (pi.double() * _logp(x, ps, mu.double() * ps, ln)).sum(1)
    total = float(rows.sum())
    return (total, rows.float()) if return_rows else total


def _patch(setattr_=setattr):
    setattr_(gmm, "estep_diag", _cpu_estep_diag)
    setattr_(gmm, "diag_moments", _cpu_moments)
    setattr_(gmm, "diag_scatter", _cpu_scatter)
    setattr_(gmm.GaussianMixture, "_prepare_x",
             lambda self, X: torch.as_tensor(X, dtype=torch.float32).contiguous())
    setattr_(ce, "community_grad_diag", _cpu_grad_diag)
    setattr_(ce, "community_loss_diag", _cpu_loss_diag)


def _data():
    rng = np.random.RandomState(7)
    centres = np.array([[4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 4, 1]], np.float32)
    lab = rng.randint(0, K, V)
    X = (centres[lab] + rng.standard_normal((V, D)) * 0.7).astype(np.float32)
    return X, np.full(K, 1.0 / K), centres.astype(np.float64) + 0.3, np.full((K, D), 2.0)


def _model(X):
    rng = np.random.RandomState(3)
    m = types.SimpleNamespace()
    m.k, m.vocab_size = K, V
    m.node_embedding = torch.from_numpy(X.copy())
    m.pi = torch.from_numpy(rng.dirichlet(np.ones(K), V).astype(np.float32))
    m.centroid = torch.from_numpy(rng.standard_normal((K, D)).astype(np.float32))
    m.covariance_mat = torch.from_numpy(rng.uniform(0.5, 1.5, (K, D)).astype(np.float32))
    m.inv_covariance_mat = 1.0 / m.covariance_mat
    m.rows_of = lambda ids: np.asarray(ids, np.int64) - 1  # node id i -> row i-1
    return m


def _run(rank, world, out_dir, distributed):
    X, w0, mu0, prec0 = _data()
    lo, hi = shard_range(V, rank, world) if distributed else (0, V)
    g = gmm.GaussianMixture(K, covariance_type="diag", reg_covar=1e-5, max_iter=12, tol=0.0,
                            weights_init=w0, means_init=mu0, precisions_init=prec0,
                            distributed=distributed)
    g.fit(X[lo:hi])
    res = dict(weights=g.weights_, means=g.means_, cov=g.covariances_, lb=g.lower_bound_,
               n_iter=g.n_iter_, score=g.score(X[lo:hi]))
    m = _model(X)
    c2v = ce.Community2Vec.__new__(ce.Community2Vec)
    c2v.lr, c2v.gmm_backend, c2v.distributed, c2v.group = 0.1, "gpu", distributed, None
    c2v.covariance_type = "diag"
    ids = np.concatenate([np.arange(1, V + 1, 3)[::-1], [7, 7, 10]])  # shuffled, with repeats
    res["loss_full"] = c2v.loss(np.arange(1, V + 1), m, beta=0.5)
    res["loss_sub"] = c2v.loss(ids, m, beta=0.5, chunksize=11)
    c2v.train(np.arange(1, V + 1), m, beta=0.5, iter=3)
    res["x_full"] = m.node_embedding.numpy().copy()
    c2v.train(ids, m, beta=0.5, chunksize=11, iter=2)
    res["x_sub"] = m.node_embedding.numpy().copy()
    c2v.g_mixture = g
    res["pi"] = c2v.responsibilities(m).numpy()
    np.savez(os.path.join(out_dir, "res_%s_r%d.npz" % ("dist" if distributed else "single",
                                                     rank)), **res)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _patch()
    _run(rank, world, out_dir, True)
    dist.destroy_process_group()


def test_diag_row_sharded_world2(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    _patch(monkeypatch.setattr)  # undone after the test
    _run(0, 1, str(tmp_path), False)
    single = np.load(os.path.join(str(tmp_path), "res_single_r0.npz"))
    r0 = np.load(os.path.join(str(tmp_path), "res_dist_r0.npz"))
    r1 = np.load(os.path.join(str(tmp_path), "res_dist_r1.npz"))
    for key in r0.files:  # both ranks end with the same parameters and replicas, bit for bit
        np.testing.assert_array_equal(r0[key], r1[key], err_msg=key)
    assert single["cov"].shape == (K, D) and int(r0["n_iter"]) == int(single["n_iter"]) == 12
    for key in ("weights", "means", "cov", "lb", "score"):
        np.testing.assert_allclose(r0[key], single[key], rtol=1e-9, err_msg=key)
    for key in ("loss_full", "loss_sub"):
        assert float(single[key]) > 0
        np.testing.assert_allclose(r0[key], single[key], rtol=1e-9, err_msg=key)
    # rows are independent: the sharded step equals the single-process one
    np.testing.assert_array_equal(r0["x_full"], single["x_full"])
    np.testing.assert_array_equal(r0["x_sub"], single["x_sub"])
    np.testing.assert_allclose(r0["pi"], single["pi"], rtol=1e-6, atol=1e-9)
    # the mixture the EM found is the data's: three blobs of equal weight and variance 0.49
    np.testing.assert_allclose(single["weights"], np.bincount(_lab(), minlength=K) / V, atol=0.02)
    np.testing.assert_allclose(single["cov"], 0.49, atol=0.2)


def _lab():
    return np.random.RandomState(7).randint(0, K, V)
