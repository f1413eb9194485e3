"""Community embedding trainer -- reference: ADSCModel/community_embeddings.py.

``Community2Vec(model, lr, reg_covar, gmm_backend="gpu", kmeans_backend='torch',
kmeans_seeding='torch', covariance_type='full')`` (``covariance_type='diag'``: diagonal
covariances for both backends -- covariance_mat and inv_covariance_mat are then [K, d], and
``train``, ``loss`` and ``responsibilities`` run the diagonal kernels, come_community_grad_diag,
come_community_loss_diag and come_gmm_estep_diag, dispatching on the stored matrices' dim();
``kmeans_backend='native'``: the mixture's k-means initialisation on
come_amd.kmeans; ``kmeans_seeding='native'``: its k-means++ seeding in libcome.so too):
  * ``fit(model)`` (:20-37): fits a GaussianMixture(n_components=k, covariance_type='full',
    n_init=10, reg_covar) -- by default the GPU EM of come_amd.gmm (MFMA E-step and M-step
    kernels, k-means init; unseeded like the reference's: the init draws its seed from the global
    numpy RNG), or with ``gmm_backend="sklearn"`` sklearn's own estimator on the host exactly as
    the reference does -- then stores centroid / covariance_mat (fp32 casts) and
    inv_covariance_mat (the inverse of the fp32 covariances, :36) on the GPU, and computes the
    responsibilities pi (:37, predict_proba) on the GPU with come_gmm_resp.
  * ``train(nodes, model, beta, chunksize, iter)`` (:61-78): the full-batch community gradient
    x -= lr * clip((beta/K) sum_k pi_ik inv_cov_k (x_i - mu_k), +-5), ``iter`` times, on the GPU
    (come_community_grad).  Every row's gradient depends only on that row (:65 snapshot), so rows
    outside ``nodes`` are left untouched by gathering/scattering the selected rows.
  * ``loss(nodes, model, beta, chunksize)`` (:40-59): the objective ``train`` descends,
    (beta / K) |sum_i sum_k pi_ik log N(x_i; mu_k, Sigma_k)| over the listed nodes, on the GPU
    (come_community_loss; ``community_loss`` is the signed total for tensors).
  * ``responsibilities(model)``: predict_proba of the fitted mixture on the current embedding.

Multi-GPU (``distributed=True``): every rank holds a full replica of
node_embedding (as after the SGNS phase) and owns the contiguous row block
``shard_range(V, rank, N)``.  ``fit`` runs the GMM EM over the ranks' blocks with all-reduced
sufficient statistics (come_amd.gmm, distributed=True) and all-gathers the responsibilities;
``train`` applies the community gradient to the rank's block only (rows are independent, :65) and
all-gathers the updated rows once per call (after all ``iter`` steps), so the replicas agree
bit for bit with a single-GPU run.  ``loss`` evaluates the rank's block and all-reduces the float64
totals (as GaussianMixture.score).  No other exchange is needed.
"""
import logging as log

import numpy as np

from . import _lib
from ._lib import check, ptr, stream_handle
from .distributed import all_gather_rows, all_reduce_sum, shard_range, world_of


def gmm_resp(x, prec_chol, mu_prec, log_norm):
    """Responsibilities [V, K] of a full-covariance GMM for rows x [V, d] (CUDA fp32)."""
    import torch
    V, d = x.shape
    K = prec_chol.shape[0]
    out = torch.empty((V, K), dtype=torch.float32, device=x.device)
    rc = _lib.lib().come_gmm_resp(ptr(x), V, d, ptr(prec_chol), ptr(mu_prec), ptr(log_norm), K,
                                  ptr(out), stream_handle(x.device))
    check(rc, "come_gmm_resp")
    return out


def gmm_resp_params(weights, means, precisions_cholesky, device):
    """Host precomputation (float64, then fp32) of what come_gmm_resp consumes: prec_chol,
    mu_k @ prec_chol_k and log w_k + log det(prec_chol_k) - d/2 log(2 pi)."""
    import torch
    pc = np.asarray(precisions_cholesky, np.float64)
    mu = np.asarray(means, np.float64)
    K, d = mu.shape
    mu_prec = np.einsum("kd,kde->ke", mu, pc)
    log_det = np.array([np.sum(np.log(np.diag(pc[k]))) for k in range(K)])
    log_norm = np.log(np.asarray(weights, np.float64)) + log_det - 0.5 * d * np.log(2 * np.pi)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)  # noqa: E731
    return t(pc), t(mu_prec), t(log_norm)


def community_grad(x, pi, mu, inv_cov, beta, lr, iters):
    """In-place community gradient steps on all rows of x (CUDA fp32 [V, d])."""
    V, d = x.shape
    K = pi.shape[1]
    rc = _lib.lib().come_community_grad(ptr(x), V, d, ptr(pi), ptr(mu), ptr(inv_cov), K,
                                        float(beta), float(lr), int(iters),
                                        stream_handle(x.device))
    check(rc, "come_community_grad")


def gmm_resp_params_diag(weights, means, precisions_cholesky, device):
    """gmm_resp_params for covariance_type='diag' (precisions_cholesky [K, d] = 1 / sqrt(var)):
    what come_gmm_estep_diag consumes, derived in float64 and handed over as fp32."""
    import math

    import torch
    pc = torch.from_numpy(np.asarray(precisions_cholesky, np.float64))
    mu = torch.from_numpy(np.asarray(means, np.float64))
    w = torch.from_numpy(np.asarray(weights, np.float64))
    ln = torch.log(w) + torch.log(pc).sum(-1) - 0.5 * mu.shape[1] * math.log(2 * math.pi)
    return tuple(a.float().contiguous().to(device) for a in (pc, mu * pc, ln))


def community_grad_diag(x, pi, mu, inv_var, beta, lr, iters):
    """In-place community gradient steps on all rows of x (CUDA fp32 [V, d]) for diagonal
    covariances: inv_var [K, d]."""
    V, d = x.shape
    K = pi.shape[1]
    rc = _lib.lib().come_community_grad_diag(ptr(x), V, d, ptr(pi), ptr(mu), ptr(inv_var), K,
                                             float(beta), float(lr), int(iters),
                                             stream_handle(x.device))
    check(rc, "come_community_grad_diag")


def community_loss_diag(x, pi, mu, var, return_rows=False):
    """community_loss for diagonal covariances var [K, d]: the signed total sum_i sum_k pi[i, k]
    log N(x_i; mu[k], diag(var[k])) as a Python float, or ``(total, rows)``.  The operands are
    derived in float64 on the device; a variance that is not positive raises ValueError."""
    import math

    import torch
    V, d = x.shape
    K = mu.shape[0]
    rows = torch.zeros((V,), dtype=torch.float32, device=x.device) if return_rows else None
    if V == 0:
        return (0.0, rows) if return_rows else 0.0
    var64 = var.double()
    if bool((~(var64 > 0)).any()):
        raise ValueError("community_loss_diag: variance of component %d is not positive"
                         % int(torch.nonzero((~(var64 > 0)).any(1))[0]))
    pc = 1.0 / torch.sqrt(var64)
    mp = (mu.double() * pc).float().contiguous()
    ln = (torch.log(pc).sum(-1) - 0.5 * d * math.log(2 * math.pi)).float().contiguous()
    pc = pc.float().contiguous()
    x, pi = x.contiguous(), pi.contiguous()
    total = torch.zeros((1,), dtype=torch.float64, device=x.device)
    rc = _lib.lib().come_community_loss_diag(ptr(x), V, d, ptr(pi), ptr(pc), ptr(mp), ptr(ln), K,
                                             ptr(rows) if return_rows else None, ptr(total),
                                             stream_handle(x.device))
    check(rc, "come_community_loss_diag")
    total = float(total.item())
    return (total, rows) if return_rows else total


def community_loss_params(mu, cov):
    """What come_community_loss consumes, derived in float64 on the device and handed over as
    fp32: (prec_chol, mu_prec, log_norm) with prec_chol[k] = P_k, the upper precision Cholesky
    factor of cov[k].double() (zeros below the diagonal), mu_prec[k] = mu_k P_k and log_norm[k] =
    c_k = sum(log diag P_k) - d/2 log(2 pi) (no mixture weight).  A covariance that is not positive
    definite raises ValueError, as scipy's multivariate_normal does."""
    import math

    import torch
    K, d = mu.shape
    mu64, cov64 = mu.double().contiguous(), cov.double().contiguous()
    if d <= 128:
        # come_gmm_params with unit nk and weights and no regularisation: one launch
        from . import gmm
        one = torch.ones(K, dtype=torch.float64, device=mu.device)
        _, _, e_pc, e_mp, e_ln, info = gmm.params(cov64, one, mu64, one, 0.0)
    else:  # the torch path of GaussianMixture._set_params
        chol, info = torch.linalg.cholesky_ex(cov64)
        chol = torch.where(info.view(K, 1, 1) != 0, torch.eye(d, dtype=torch.float64,
                                                                device=mu.device), chol)
        eye = torch.eye(d, dtype=torch.float64, device=mu.device).expand_as(chol)
        pc = torch.triu(torch.linalg.solve_triangular(chol, eye, upper=False).transpose(-1, -2))
        log_det = torch.log(torch.diagonal(pc, dim1=-2, dim2=-1)).sum(-1)
        e_pc = pc.float().contiguous()
        e_mp = torch.einsum("kd,kde->ke", mu64, pc).float().contiguous()
        e_ln = (log_det - 0.5 * d * math.log(2 * math.pi)).float().contiguous()
    if bool((info != 0).any()):
        raise ValueError("community_loss: covariance of component %d is not positive definite"
                         % int(torch.nonzero(info)[0]))
    return e_pc, e_mp, e_ln


def community_loss(x, pi, mu, cov, return_rows=False):
    """The signed community objective sum_i sum_k pi[i, k] log N(x_i; mu[k], cov[k]) for device
    fp32 x [V, d], pi [V, K] (used as given: rows need not sum to 1), mu [K, d], cov [K, d, d], as
    a Python float (the rows summed in float64); ``(total, rows)`` with rows a device fp32 [V]
    tensor when ``return_rows``.  No rows: 0.0."""
    import torch
    V, d = x.shape
    K = mu.shape[0]
    rows = torch.zeros((V,), dtype=torch.float32, device=x.device) if return_rows else None
    if V == 0:
        return (0.0, rows) if return_rows else 0.0
    pc, mp, ln = community_loss_params(mu, cov)
    x, pi = x.contiguous(), pi.contiguous()
    total = torch.zeros((1,), dtype=torch.float64, device=x.device)
    rc = _lib.lib().come_community_loss(ptr(x), V, d, ptr(pi), ptr(pc), ptr(mp), ptr(ln), K,
                                        ptr(rows) if return_rows else None, ptr(total),
                                        stream_handle(x.device))
    check(rc, "come_community_loss")
    total = float(total.item())
    return (total, rows) if return_rows else total


class Community2Vec(object):
    def __init__(self, model, lr, reg_covar=0, gmm_backend="gpu", distributed=False,
                 group=None, kmeans_backend='torch', kmeans_seeding='torch',
                 covariance_type='full'):
        if covariance_type not in ('full', 'diag'):
            raise NotImplementedError("covariance_type must be 'full' or 'diag'")
        self.covariance_type = covariance_type
        self.lr = lr
        self.gmm_backend = gmm_backend
        self.distributed = bool(distributed)
        self.group = group
        if gmm_backend == "gpu":
            from .gmm import GaussianMixture
            self.g_mixture = GaussianMixture(n_components=model.k, reg_covar=reg_covar,
                                             covariance_type=covariance_type, n_init=10,
                                             distributed=distributed, group=group,
                                             kmeans_backend=kmeans_backend,
                                             kmeans_seeding=kmeans_seeding)
        elif gmm_backend == "sklearn":
            if distributed:
                raise ValueError("distributed=True needs gmm_backend='gpu'")
            from sklearn import mixture
            self.g_mixture = mixture.GaussianMixture(n_components=model.k, reg_covar=reg_covar,
                                                     covariance_type=covariance_type,
                                                     n_init=10)
        else:
            raise ValueError("gmm_backend must be 'gpu' or 'sklearn'")

    def _shard(self, V):
        """(lo, hi) rows this rank owns ((0, V) on one process)."""
        rank, world = world_of(self.group) if self.distributed else (0, 1)
        return shard_range(V, rank, world)

    def fit(self, model):
        import torch
        log.info("Fitting: {} communities".format(model.k))
        dev = model.node_embedding.device
        if self.gmm_backend == "gpu":
            lo, hi = self._shard(model.node_embedding.shape[0])
            self.g_mixture.fit(model.node_embedding[lo:hi])
        else:
            self.g_mixture.fit(model.node_embedding.detach().cpu().numpy())
        cov32 = torch.from_numpy(self.g_mixture.covariances_.astype(np.float32)).to(dev)
        model.centroid = torch.from_numpy(self.g_mixture.means_.astype(np.float32)).to(dev)
        model.covariance_mat = cov32
        if cov32.dim() == 2:  # 'diag': [K, d]
            model.inv_covariance_mat = (1.0 / cov32).contiguous()
        else:
            model.inv_covariance_mat = torch.linalg.inv(cov32).contiguous()  # :36, fp32 inverse
        model.pi = self.responsibilities(model)

    def responsibilities(self, model):
        import torch
        g = self.g_mixture
        x = model.node_embedding
        if np.ndim(g.precisions_cholesky_) == 2:  # 'diag'
            from .gmm import estep_diag
            pc, mp, ln = gmm_resp_params_diag(g.weights_, g.means_, g.precisions_cholesky_,
                                              x.device)
            resp_of = lambda rows: estep_diag(rows.contiguous(), pc, mp, ln)[0]  # noqa: E731
        else:
            pc, mp, ln = gmm_resp_params(g.weights_, g.means_, g.precisions_cholesky_, x.device)
            resp_of = lambda rows: gmm_resp(rows, pc, mp, ln)  # noqa: E731
        if not self.distributed:
            return resp_of(x)
        V = x.shape[0]
        lo, hi = self._shard(V)
        pi = torch.empty((V, pc.shape[0]), dtype=torch.float32, device=x.device)
        pi[lo:hi] = resp_of(x[lo:hi])
        return all_gather_rows(pi, self.group)

    def loss(self, nodes, model, beta, chunksize=150):
        """community_embeddings.py:40-59 as it is meant: O3 = (beta / K) |sum_i sum_k pi_ik
        log N(x_i; mu_k, Sigma_k)| over the listed nodes (each listing of a node counts once, so
        a node listed twice counts twice), the objective ``train`` descends.  Departs from two
        defects of the reference, which cannot run as written: :48 calls ``model.vocab(x)`` (a
        dict; ``train`` indexes it), and :57 overwrites its accumulator with each component's
        term where it should add it.  ``chunksize`` is accepted for the reference's signature and
        has no effect (the sum does not depend on the chunking).  Reads model.centroid,
        model.covariance_mat, model.pi and model.node_embedding only.  Ids outside the vocabulary
        raise KeyError, as in ``train``."""
        import torch
        ids = np.fromiter((int(n) for n in nodes), np.int64)
        rows = model.rows_of(ids)
        if (rows < 0).any():
            raise KeyError(int(ids[np.argmax(rows < 0)]))
        x, pi = model.node_embedding, model.pi
        if not (len(rows) == model.vocab_size and (rows == np.arange(len(rows))).all()):
            idx = torch.from_numpy(np.ascontiguousarray(rows, np.int64)).to(x.device)
            x, pi = x.index_select(0, idx), pi.index_select(0, idx)
        lo, hi = self._shard(len(rows))
        total = 0.0
        if hi > lo:  # a row block of a C-contiguous table is itself contiguous
            loss_of = community_loss_diag if model.covariance_mat.dim() == 2 else community_loss
            total = loss_of(x[lo:hi], pi[lo:hi], model.centroid, model.covariance_mat)
        if self.distributed and world_of(self.group)[1] > 1:
            t = torch.tensor([total], dtype=torch.float64, device=x.device)
            all_reduce_sum([t], self.group)
            total = float(t[0])
        return abs(total) * beta / model.k

    def train(self, nodes, model, beta, chunksize=150, iter=1):
        """community_embeddings.py:61-78.  The reference walks `nodes` in chunks of `chunksize`
        and adds each chunk's gradient with grad_input[node_index] += batch (numpy fancy-index
        add: a node listed twice in ONE chunk counts once, a node in m different chunks m
        times), then updates every row.  So row r moves by clip(m_r * coef * G_r) with m_r the
        number of chunks that list it; here m_r scales pi's row (G is linear in it).  Ids outside
        the vocabulary raise KeyError, as model.vocab[x] does."""
        import torch
        ids = np.fromiter((int(n) for n in nodes), np.int64)
        rows = model.rows_of(ids)
        if (rows < 0).any():
            raise KeyError(int(ids[np.argmax(rows < 0)]))
        x = model.node_embedding
        # ([K, d] inverse variances: fit's covariance_type='diag'; train reads no covariance_mat)
        grad = community_grad_diag if model.inv_covariance_mat.dim() == 2 else community_grad
        chunksize = max(1, int(chunksize))
        if len(rows) == model.vocab_size and (np.sort(rows) == np.arange(len(rows))).all():
            lo, hi = self._shard(x.shape[0])
            if hi > lo:  # a row block of a C-contiguous table is itself contiguous
                grad(x[lo:hi], model.pi[lo:hi], model.centroid, model.inv_covariance_mat, beta,
                     self.lr, iter)
            if self.distributed:
                all_gather_rows(x, self.group)
            return
        # multiplicity: the number of chunks that list the row
        chunk = np.arange(len(rows)) // chunksize
        pairs = np.unique(chunk * np.int64(model.vocab_size) + rows)
        uniq, mult = np.unique(pairs % model.vocab_size, return_counts=True)
        idx = torch.from_numpy(uniq).to(x.device)
        sub = x.index_select(0, idx).contiguous()
        pi = model.pi.index_select(0, idx)
        if (mult > 1).any():
            pi = pi * torch.from_numpy(mult.astype(np.float32)).to(x.device)[:, None]
        pi = pi.contiguous()
        lo, hi = self._shard(len(uniq))
        if hi > lo:
            grad(sub[lo:hi], pi[lo:hi], model.centroid, model.inv_covariance_mat, beta, self.lr,
                 iter)
        if self.distributed:
            all_gather_rows(sub, self.group)
        x.index_copy_(0, idx, sub)
