"""The diagonal-covariance path without a GPU: the M-step planner's invariants
(come_gmm_diag_scratch, a host function), the Python parameter derivation against sklearn's own
'diag' helpers, and the covariance types that stay unimplemented."""
import numpy as np
import pytest
import torch

import diag_cases as dc
from come_amd import _lib, gmm
from come_amd import community_embeddings as ce

PARTIAL_CAP = 128 << 20


def test_symbols_and_abi():
    L = _lib.lib()
    for name in ("come_gmm_estep_diag", "come_gmm_diag_scratch", "come_gmm_diag_moments",
                 "come_gmm_diag_scatter", "come_community_grad_diag", "come_community_loss_diag"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.come_abi_version() == _lib.ABI_VERSION == 5


@pytest.mark.parametrize("d,K", [(1, 1), (8, 4), (64, 6), (128, 50), (200, 70), (256, 50),
                                 (512, 4096), (32, 300)])
@pytest.mark.parametrize("cus", [256, 64, 0])
def test_planner_invariants(d, K, cus):
    prev = 0
    for V in (1, 2, 63, 64, 65, 1000, 4097, 100_000, 1_000_000, 10_000_000, (1 << 31) - 1):
        chunks, rows = gmm.diag_plan(V, d, K, cus)
        assert chunks >= 1 and rows >= 1
        assert chunks * (K * d + K) * 4 <= PARTIAL_CAP or chunks == 1
        assert chunks * rows >= V and rows == -(-V // chunks)
        assert chunks <= max(1, -(-V // 64))  # a chunk has 64 rows or more (or is the only one)
        assert chunks >= prev  # monotone in V
        prev = chunks
    assert gmm.diag_plan(1_000_000, d, K, 0) == gmm.diag_plan(1_000_000, d, K, 256)


def test_planner_rejects_bad_arguments():
    for V, d, K in ((10, 0, 3), (10, 513, 3), (10, 8, 0), (10, 8, 4097), (-1, 8, 3)):
        with pytest.raises(_lib.ComeError, match="need V>=0"):
            gmm.diag_plan(V, d, K, 256)


def test_parameter_derivation_matches_sklearn():
    from sklearn.mixture._gaussian_mixture import (_compute_precision_cholesky,
                                                   _estimate_log_gaussian_prob)
    X, _, w, mu, var = dc.problem(200, 4, 24, 3)
    pc, mp, ln = (a.numpy() for a in gmm.diag_estep_params(*(torch.from_numpy(a)
                                                             for a in (w, mu, var))))
    sk_pc = _compute_precision_cholesky(var, "diag")
    np.testing.assert_allclose(pc, sk_pc, rtol=1e-12)
    np.testing.assert_allclose(mp, mu * sk_pc, rtol=1e-12)
    ps, mp_ref, ln_ref = dc.operands(w, mu, var)
    np.testing.assert_allclose(ln, ln_ref, rtol=1e-12)
    # the kernels' form with these operands is sklearn's weighted log-density
    x64 = X.astype(np.float64)
    sk_lp = _estimate_log_gaussian_prob(x64, mu, sk_pc, "diag") + np.log(w)
    np.testing.assert_allclose(dc.log_prob(X, pc, mp, ln), sk_lp, rtol=1e-12, atol=1e-9)
    # what Community2Vec.responsibilities hands the E-step: the same, as fp32
    e_pc, e_mp, e_ln = ce.gmm_resp_params_diag(w, mu, sk_pc, "cpu")
    for got, ref in ((e_pc, pc), (e_mp, mp), (e_ln, ln)):
        assert got.dtype == torch.float32
        assert np.array_equal(got.numpy(), ref.astype(np.float32))


def test_estimator_attributes_for_diag():
    """The parameter step of the estimator on CPU tensors: sklearn's 'diag' attribute shapes and
    values from given statistics."""
    K, d = 3, 5
    rng = np.random.RandomState(0)
    g = gmm.GaussianMixture(K, covariance_type="diag")
    w = torch.from_numpy(rng.dirichlet(np.ones(K)))
    mu = torch.from_numpy(rng.normal(size=(K, d)))
    cov = torch.from_numpy(rng.uniform(0.5, 2.0, size=(K, d)))
    g._set_params(w, mu, cov)
    g._export()
    np.testing.assert_allclose(g.precisions_cholesky_, 1 / np.sqrt(cov.numpy()), rtol=1e-15)
    np.testing.assert_allclose(g.precisions_, 1 / cov.numpy(), rtol=1e-14)
    assert g.covariances_.shape == (K, d)
    g._set_params_from_precisions(w, mu, 1.0 / cov)
    np.testing.assert_allclose(g._pc.numpy(), 1 / np.sqrt(cov.numpy()), rtol=1e-14)
    np.testing.assert_allclose(g._cov.numpy(), cov.numpy(), rtol=1e-14)
    cov[1, 2] = 0.0
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        g._set_params(w, mu, cov)


def test_other_covariance_types_still_raise():
    for kind in ("tied", "spherical"):
        with pytest.raises(NotImplementedError):
            gmm.GaussianMixture(2, covariance_type=kind)
        with pytest.raises(NotImplementedError):
            ce.Community2Vec(None, 0.1, covariance_type=kind)
    assert gmm.GaussianMixture(2).covariance_type == "full"
    assert gmm.GaussianMixture(2, covariance_type="diag").covariance_type == "diag"
