"""The community loss on the GPU (come_community_loss, come_amd.community_embeddings.community_loss,
Community2Vec.loss) against float64 scipy.

Inputs: tests/test_gpu_gmm.py:problem with pi from a Dirichlet (test_community_loss_host.problem);
mu and cov are rounded to fp32 first, so the float64 reference sees the Sigma_k the entry sees.
Tolerances (the E-step's, tests/test_gpu_gmm.py: lse at rtol 2e-5, atol 2e-3, through the
pi-weighted sum): per row 2e-3 sum_k |pi_ik| + 2e-5 sum_k |pi_ik lp_ik|, the total the sum of them.
"""
import functools

import numpy as np
import pytest

from come_amd import _lib
from come_amd import community_embeddings as ce
from test_community_loss_host import problem, reference

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def t(a):
    return torch.as_tensor(np.array(a, np.float32), device=dev())  # a copy: the cases are frozen


@functools.lru_cache(maxsize=None)
def case(V, K, d):
    """(X, pi, mu, cov) in fp32 and the float64 reference of them, computed once per shape."""
    dev()
    X, pi, mu, cov = problem(V, K, d, V + d)
    mu, cov = mu.astype(np.float32), cov.astype(np.float32)
    ref = reference(X, pi, mu.astype(np.float64), cov.astype(np.float64))
    for a in (X, pi, mu, cov) + ref[:1] + ref[2:3]:
        a.setflags(write=False)
    return X, pi, mu, cov, ref


def check(total, rows, ref, what):
    rows_ref, total_ref, row_tol, total_tol = ref
    rows = rows.cpu().numpy() if hasattr(rows, "cpu") else rows
    nz = row_tol > 0  # a row of zero weights has tolerance 0: it must be exactly 0
    print("%s: total %.4f ref %.4f |diff| %.3g tol %.3g; rows max |diff|/tol %.3g"
          % (what, total, total_ref, abs(total - total_ref), total_tol,
             np.max(np.abs(rows - rows_ref)[nz] / row_tol[nz])))
    assert np.isfinite(rows).all()
    assert (np.abs(rows - rows_ref) <= row_tol).all()
    assert abs(total - total_ref) <= total_tol


def raw_loss(x, pi, pc, mp, ln, with_rows=True):
    """come_community_loss on given factors (the tensors are passed as they are, views included)."""
    V, d = x.shape
    rows = torch.zeros(V, dtype=torch.float32, device=x.device) if with_rows else None
    total = torch.zeros(1, dtype=torch.float64, device=x.device)
    _lib.check(_lib.lib().come_community_loss(
        _lib.ptr(x), V, d, _lib.ptr(pi), _lib.ptr(pc), _lib.ptr(mp), _lib.ptr(ln), pc.shape[0],
        _lib.ptr(rows) if with_rows else None, _lib.ptr(total), _lib.stream_handle(x.device)),
        "come_community_loss")
    return float(total.item()), rows


# MFMA with V not a multiple of 128; a one-row last workgroup and K = 1; VALU; the wide form, K > 64
SHAPES = [(2500, 5, 128), (3000, 6, 64), (129, 2, 64), (1, 1, 128), (777, 3, 100), (900, 4, 256),
          (300, 70, 200)]


@pytest.mark.parametrize("V,K,d", SHAPES)
def test_rows_and_total_vs_float64(V, K, d):
    X, pi, mu, cov, ref = case(V, K, d)
    total, rows = ce.community_loss(t(X), t(pi), t(mu), t(cov), return_rows=True)
    assert isinstance(total, float) and rows.shape == (V,)
    check(total, rows, ref, "(%d, %d, %d)" % (V, K, d))


@pytest.mark.parametrize("V,K,d", [(129, 2, 64), (2500, 5, 128)])
def test_unaligned_factors_take_the_valu_kernel(V, K, d):
    """prec_chol and mu_prec as contiguous views at element offset 1 of larger buffers: not 16-byte
    aligned, so the call runs k_comm_loss_valu at d = 64 / 128 and meets the same bounds."""
    X, pi, mu, cov, ref = case(V, K, d)

    def off1(a):
        v = torch.empty(a.numel() + 1, dtype=torch.float32, device=a.device)[1:].view(a.shape)
        v.copy_(a)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    pc, mp, ln = ce.community_loss_params(t(mu), t(cov))
    total, rows = raw_loss(t(X), t(pi), off1(pc), off1(mp), ln)
    check(total, rows, ref, "unaligned (%d, %d, %d)" % (V, K, d))


@pytest.mark.parametrize("V,K,d", [(3000, 6, 64), (777, 3, 100)])
def test_pi_is_used_as_given(V, K, d):
    """Rows of pi scaled by 0, 2 and 3 (train scales them by a multiplicity): a zero row gives
    exactly 0.0, the others scale with it."""
    X, pi, mu, cov, _ = case(V, K, d)
    scale = np.array([0.0, 2.0, 3.0], np.float32)[np.arange(V) % 3]
    pis = pi * scale[:, None]
    ref = reference(X, pis, mu.astype(np.float64), cov.astype(np.float64))
    total, rows = ce.community_loss(t(X), t(pis), t(mu), t(cov), return_rows=True)
    check(total, rows, ref, "scaled pi (%d, %d, %d)" % (V, K, d))
    rows = rows.cpu().numpy()
    assert (rows[scale == 0] == 0.0).all()
    assert (rows[scale != 0] != 0.0).all()


@pytest.mark.parametrize("V,K,d", [(2500, 5, 128), (777, 3, 100), (900, 4, 256)])
def test_bit_identical_from_run_to_run(V, K, d):
    X, pi, mu, cov, _ = case(V, K, d)
    x, p = t(X), t(pi)
    pc, mp, ln = ce.community_loss_params(t(mu), t(cov))
    total_a, rows_a = raw_loss(x, p, pc, mp, ln)
    total_b, rows_b = raw_loss(x, p, pc, mp, ln)
    total_c, _ = raw_loss(x, p, pc, mp, ln, with_rows=False)  # row_out = NULL
    assert total_a == total_b == total_c
    assert torch.equal(rows_a, rows_b)


@pytest.mark.parametrize("V,K,d", [(2500, 5, 128), (3000, 6, 64)])
def test_community_step_ascends_the_signed_total(V, K, d):
    """One come_community_grad step (beta = 1, lr = 0.1) is a descent step on the objective the
    loss evaluates: in float64 the signed total rises by 9.86e4 at (2500, 5, 128) and 5.38e4 at
    (3000, 6, 64) with no coordinate clipped, against total tolerances of 71 and 49.  The GPU's
    rise (kernel loss before and after the kernel step) equals the float64 rise (float64 loss
    before and after the float64 step) within twice the total's tolerance."""
    X, pi, mu, cov, ref = case(V, K, d)
    beta, lr = 1.0, 0.1
    inv = np.linalg.inv(cov.astype(np.float64)).astype(np.float32)
    x64, p64 = X.astype(np.float64), pi.astype(np.float64)
    G = np.zeros_like(x64)
    for k in range(K):
        G += p64[:, k, None] * ((x64 - mu[k].astype(np.float64)) @ inv[k].astype(np.float64).T)
    g = beta / K * G
    assert np.abs(g).max() < 5.0  # no coordinate clipped
    after = reference((x64 - lr * g), pi, mu.astype(np.float64), cov.astype(np.float64))
    rise_ref = after[1] - ref[1]
    x, p, m, c = t(X), t(pi), t(mu), t(cov)
    before_gpu = ce.community_loss(x, p, m, c)
    ce.community_grad(x, p, m, t(inv), beta, lr, 1)
    rise_gpu = ce.community_loss(x, p, m, c) - before_gpu
    print("(%d, %d, %d): rise float64 %.6g, GPU %.6g, total tolerance %.3g"
          % (V, K, d, rise_ref, rise_gpu, ref[3]))
    assert rise_ref > 100 * ref[3]
    assert abs(rise_gpu - rise_ref) <= 2 * ref[3]


@functools.lru_cache(maxsize=None)
def fitted(backend="gpu"):
    """A small fitted model (V = 600, K = 3, d = 64) and the float64 rows of its buffers."""
    from come_amd.model import Model
    V, K, d = 600, 3, 64
    X = problem(V, K, d, 11, sep=4.0)[0]
    np.random.seed(0)
    m = Model((np.arange(1, V + 1), np.ones(V)), size=d, table_size=1000, k=K, device=dev())
    m.node_embedding = torch.as_tensor(X, device=dev())
    cm = ce.Community2Vec(m, lr=0.1, reg_covar=1e-5, gmm_backend=backend)
    cm.g_mixture.n_init = 1
    cm.fit(m)
    ref = reference(X, m.pi.cpu().numpy(), m.centroid.cpu().numpy().astype(np.float64),
                    m.covariance_mat.cpu().numpy().astype(np.float64))
    return m, cm, ref


def test_community2vec_loss_on_a_fitted_model():
    m, cm, (rows_ref, total_ref, row_tol, total_tol) = fitted()
    V, beta = m.vocab_size, 0.7
    full = cm.loss(range(1, V + 1), m, beta)
    assert abs(full - abs(total_ref) * beta / m.k) <= total_tol * beta / m.k
    assert cm.loss(range(1, V + 1), m, beta, chunksize=7) == full  # no effect
    # a node listed twice counts twice
    twice = cm.loss(list(range(1, V + 1)) + [5], m, beta)
    assert abs(twice - abs(total_ref + rows_ref[4]) * beta / m.k) <= \
        (total_tol + row_tol[4]) * beta / m.k
    assert twice != full
    # a subset in shuffled order is the sum of its rows
    ids = np.random.RandomState(3).permutation(V)[:217] + 1
    sub = cm.loss(ids, m, beta)
    assert abs(sub - abs(rows_ref[ids - 1].sum()) * beta / m.k) <= \
        row_tol[ids - 1].sum() * beta / m.k
    with pytest.raises(KeyError):
        cm.loss([1, V + 1], m, beta)
    # distributed=True on one process: the shard is every row and no collective runs
    cd = ce.Community2Vec(m, lr=0.1, reg_covar=1e-5, distributed=True)
    assert cd.loss(range(1, V + 1), m, beta) == full
    assert cd.loss(ids, m, beta) == sub


def test_sklearn_backend_model_and_bad_covariance():
    """The loss reads only model.centroid / covariance_mat / pi / node_embedding, so a model
    fitted by gmm_backend='sklearn' works; a covariance with a negative eigenvalue raises."""
    import types
    m, cm, (_, total_ref, _, total_tol) = fitted("sklearn")
    assert abs(cm.loss(range(1, m.vocab_size + 1), m, 1.0) - abs(total_ref) / m.k) <= \
        total_tol / m.k
    bad = types.SimpleNamespace(**{k: getattr(m, k) for k in
                                   ("k", "vocab_size", "node_embedding", "pi", "centroid",
                                    "rows_of")})
    cov = m.covariance_mat.clone()
    cov[1, 0, 0] = -1.0
    bad.covariance_mat = cov
    with pytest.raises(ValueError):
        cm.loss(range(1, m.vocab_size + 1), bad, 1.0)
    mu = torch.zeros((2, 200), device=dev())
    cov = torch.eye(200, device=dev()).repeat(2, 1, 1)
    cov[0, 3, 3] = -2.0  # the torch path (d > 128)
    with pytest.raises(ValueError):
        ce.community_loss(torch.zeros((4, 200), device=dev()),
                          torch.ones((4, 2), device=dev()), mu, cov)
