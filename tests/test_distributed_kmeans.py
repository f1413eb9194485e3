"""World size 2 (gloo, CPU) test of the row-sharded k-means (come_amd.kmeans.KMeans
distributed=True): seeding on rank 0 with the centres broadcast, all-reduced variance statistics
and, per iteration, all-reduced counts / sums / inertia between accumulate and update.  The HIP
kernels need a GPU, so the workers swap kmeans.assign / accumulate / update for float64 torch
stand-ins of the same operations; what is under test is the host-side protocol.  The kernels
themselves are covered by tests/test_gpu_kmeans.py."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from come_amd import gmm, kmeans
from come_amd.distributed import all_gather_rows, shard_range

V, D, K = 203, 4, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _data():  # the data of tests/test_distributed_c4.py
    rng = np.random.RandomState(7)
    centres = np.array([[4, 0, 0, 0], [0, 4, 0, 0], [0, 0, 4, 1]], np.float32)
    lab = rng.randint(0, K, V)
    X = (centres[lab] + rng.standard_normal((V, D)) * 0.5).astype(np.float32)
    return X, lab


# ---- float64 stand-ins for the HIP entry points --------------------------------------------------
def _dist2(X, C):
    return ((X.double()[:, None, :] - C.double()[None]) ** 2).sum(-1)


def _cpu_assign(X, C):
    d2 = _dist2(X, C)
    lab = torch.argmin(d2, 1)
    return lab, d2.gather(1, lab[:, None])[:, 0].float()


def _cpu_accumulate(X, C, return_mindist=False):
    lab, md = _cpu_assign(X, C)
    k = C.shape[0]
    sums = torch.zeros((k, X.shape[1]), dtype=torch.float64).index_add_(0, lab, X.double())
    counts = torch.bincount(lab, minlength=k)
    return lab.int(), sums, counts, md.double().sum()


def _cpu_update(C, sums, counts):
    new = torch.where(counts[:, None] > 0, (sums / counts.clamp_min(1)[:, None]).float(), C)
    shift2 = ((new.double() - C.double()) ** 2).sum()
    C.copy_(new)
    return shift2


def _cpu_estep(X, prec_chol, mu_prec, log_norm):
    Y = torch.einsum("vd,kde->vke", X.double(), prec_chol.double()) - mu_prec.double()[None]
    logp = -0.5 * (Y ** 2).sum(-1) + log_norm.double()[None]
    lse = torch.logsumexp(logp, 1)
    return torch.exp(logp - lse[:, None]).float(), lse.float()


def _cpu_scatter(X, resp, means, chunks=None):
    Xc = X.double()[:, None, :] - means.double()[None]
    return torch.einsum("vk,vkd,vke->kde", resp.double(), Xc, Xc).float()


def _cpu_params(S, nk, means, weights, reg):
    import math
    d = S.shape[-1]
    cov = S / nk[:, None, None] + reg * torch.eye(d, dtype=torch.float64)
    chol, info = torch.linalg.cholesky_ex(cov)
    eye = torch.eye(d, dtype=torch.float64).expand_as(cov)
    pc = torch.linalg.solve_triangular(chol, eye, upper=False).transpose(-1, -2).contiguous()
    log_det = torch.log(torch.diagonal(pc, dim1=-2, dim2=-1)).sum(-1)
    e_mp = torch.einsum("kd,kde->ke", means, pc).float()
    e_ln = (torch.log(weights) + log_det - 0.5 * d * math.log(2 * math.pi)).float()
    return cov, pc, pc.float(), e_mp, e_ln, info.int()


def _patch(setattr_=setattr):
    as_cpu = lambda self, X: torch.as_tensor(X, dtype=torch.float32).contiguous()  # noqa: E731
    setattr_(kmeans, "assign", _cpu_assign)
    setattr_(kmeans, "accumulate", _cpu_accumulate)
    setattr_(kmeans, "update", _cpu_update)
    setattr_(kmeans.KMeans, "_prepare_x", as_cpu)
    setattr_(gmm, "estep", _cpu_estep)
    setattr_(gmm, "scatter", _cpu_scatter)
    setattr_(gmm, "params", _cpu_params)
    setattr_(gmm.GaussianMixture, "_prepare_x", as_cpu)


def _run(rank, world, out_dir, distributed):
    X, _ = _data()
    lo, hi = shard_range(V, rank, world) if distributed else (0, V)
    res = {}
    for name, check_every in (("c1", 1), ("c4", 4)):
        km = kmeans.KMeans(K, n_init=2, random_state=0, check_every=check_every,
                           distributed=distributed).fit(X[lo:hi])
        full = torch.zeros(V, dtype=torch.int64)
        full[lo:hi] = torch.as_tensor(km.labels_)
        if distributed:
            all_gather_rows(full)
        res[name + "_centers"] = km.cluster_centers_
        res[name + "_labels"] = full.numpy()
        res[name + "_inertia"] = km.inertia_
        res[name + "_n_iter"] = km.n_iter_
    g = gmm.GaussianMixture(K, reg_covar=1e-5, n_init=2, random_state=0, distributed=distributed,
                            kmeans_backend='native')
    lab_local = g.fit_predict(X[lo:hi])
    full = torch.zeros(V, dtype=torch.int64)
    full[lo:hi] = lab_local
    if distributed:
        all_gather_rows(full)
    res["gmm_labels"] = full.numpy()
    res["gmm_means"] = g.means_
    np.savez(os.path.join(out_dir, "res_%s_r%d.npz" % ("dist" if distributed else "single",
                                                     rank)), **res)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _patch()
    _run(rank, world, out_dir, True)
    dist.destroy_process_group()


def test_kmeans_row_sharded_world2(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    _patch(monkeypatch.setattr)  # undone after the test
    _run(0, 1, str(tmp_path), False)
    single = np.load(os.path.join(str(tmp_path), "res_single_r0.npz"))
    r0 = np.load(os.path.join(str(tmp_path), "res_dist_r0.npz"))
    r1 = np.load(os.path.join(str(tmp_path), "res_dist_r1.npz"))
    for key in r0.files:  # both ranks end with the same centres, labels and mixture, bit for bit
        np.testing.assert_array_equal(r0[key], r1[key], err_msg=key)
    _, lab = _data()
    for name in ("c1", "c4"):
        # the sharded run seeds from rank 0's rows only, so it may start elsewhere; on these
        # separated blobs both reach the same optimum
        c_d = r0[name + "_centers"]
        c_s = single[name + "_centers"]
        order = [int(np.argmin(((c_d - c) ** 2).sum(1))) for c in c_s]
        assert sorted(order) == list(range(K)), order
        np.testing.assert_allclose(c_d[order], c_s, rtol=1e-6, atol=1e-6, err_msg=name)
        np.testing.assert_allclose(float(r0[name + "_inertia"]), float(single[name + "_inertia"]),
                                   rtol=1e-6)
        for labels in (r0[name + "_labels"], single[name + "_labels"]):
            pairs = set(zip(lab.tolist(), labels.tolist()))
            assert len(pairs) == K, pairs
    for labels in (r0["gmm_labels"], single["gmm_labels"]):
        pairs = set(zip(lab.tolist(), labels.tolist()))
        assert len(pairs) == K, pairs
