"""The community loss without a GPU: the two C-ABI symbols, argument validation before any device
work, and the CPU twin (come_cpu_community_loss) against float64 scipy.

Tolerances: the E-step's own (tests/test_gpu_gmm.py holds its per-row log-sum-exp to rtol 2e-5,
atol 2e-3), carried through the pi-weighted sum of the same log-densities:
    per row   2e-3 * sum_k |pi_ik| + 2e-5 * sum_k |pi_ik * lp_ik|
    total     the sum of the row tolerances
"""
import ctypes

import numpy as np
import pytest

from come_amd import _lib, cpu
from oracle import oracle as orc


def problem(V, K, d, seed, sep=3.0):
    """tests/test_gpu_gmm.py:problem (same draws), with pi drawn from a Dirichlet so that every
    component contributes to every row."""
    rng = np.random.RandomState(seed)
    mu = rng.normal(size=(K, d)) * sep
    A = rng.normal(size=(K, d, d)) / np.sqrt(d)
    cov = np.einsum("kij,klj->kil", A, A) * 0.5 + np.eye(d)[None] * 0.5
    w = rng.dirichlet(np.ones(K) * 3)
    lab = rng.choice(K, V, p=w)
    X = np.empty((V, d))
    for k in range(K):
        m = lab == k
        X[m] = rng.multivariate_normal(mu[k], cov[k], m.sum())
    pi = rng.dirichlet(np.ones(K), V).astype(np.float32)
    return X.astype(np.float32), pi, mu, cov


def reference(X, pi, mu, cov):
    """(rows, total, row tolerances, total tolerance) in float64 from scipy's logpdf."""
    from scipy.stats import multivariate_normal
    lp = np.stack([multivariate_normal(mu[k], cov[k]).logpdf(X.astype(np.float64)).reshape(-1)
                   for k in range(len(mu))], 1)
    p = pi.astype(np.float64)
    rows = (p * lp).sum(1)
    tol = 2e-3 * np.abs(p).sum(1) + 2e-5 * np.abs(p * lp).sum(1)
    return rows, rows.sum(), tol, tol.sum()


def factors(mu, cov):
    """The entry's fp32 operands from float64: upper precision Cholesky factors, mu_k P_k, c_k."""
    pc = orc.precision_cholesky(cov)
    d = mu.shape[1]
    mp = np.einsum("kd,kde->ke", mu, pc)
    ln = np.log(np.diagonal(pc, axis1=1, axis2=2)).sum(1) - 0.5 * d * np.log(2 * np.pi)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return f(pc), f(mp), f(ln)


def test_symbols_and_abi():
    L = _lib.lib()
    for name in ("come_community_loss", "come_cpu_community_loss"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    assert L.come_abi_version() == _lib.ABI_VERSION == 5


@pytest.mark.parametrize("V,d,K,null_out", [(-1, 8, 2, False), (10, 0, 2, False),
                                             (10, 513, 2, False), (10, 8, 0, False),
                                             (10, 8, 2, True)])
def test_invalid_arguments_fail_before_device_work(V, d, K, null_out):
    L = _lib.lib()
    p = ctypes.c_void_p(16)
    out = ctypes.c_void_p(0) if null_out else p
    rc = L.come_community_loss(p, V, d, p, p, p, p, K, None, out, None)
    assert rc == -1 and b"community_loss" in L.come_last_error()
    rc = L.come_cpu_community_loss(p, V, d, p, p, p, p, K, None, out, 1)
    assert rc == -1 and b"community_loss" in L.come_last_error()


def test_empty_input_is_a_no_op():
    L = _lib.lib()
    p = ctypes.c_void_p(0)
    assert L.come_community_loss(p, 0, 8, p, p, p, p, 2, p, p, p) == 0
    assert L.come_cpu_community_loss(p, 0, 8, p, p, p, p, 2, p, p, 1) == 0
    z = np.zeros((0, 8), np.float32)
    pc, mp, ln = factors(np.zeros((2, 8)), np.stack([np.eye(8)] * 2))
    assert cpu.community_loss(z, np.zeros((0, 2), np.float32), pc, mp, ln) == 0.0


@pytest.mark.parametrize("V,K,d", [(300, 3, 8), (257, 4, 64), (130, 2, 128)])
def test_cpu_twin_vs_scipy(V, K, d):
    X, pi, mu, cov = problem(V, K, d, V + d)
    rows_ref, total_ref, row_tol, total_tol = reference(X, pi, mu, cov)
    pc, mp, ln = factors(mu, cov)
    total, rows = cpu.community_loss(X, pi, pc, mp, ln, return_rows=True, threads=1)
    print("V=%d K=%d d=%d total %.6f ref %.6f |diff| %.3g tol %.3g; rows max |diff|/tol %.3g"
          % (V, K, d, total, total_ref, abs(total - total_ref), total_tol,
             np.max(np.abs(rows - rows_ref) / row_tol)))
    assert (np.abs(rows - rows_ref) <= row_tol).all()
    assert abs(total - total_ref) <= total_tol
    assert cpu.community_loss(X, pi, pc, mp, ln, threads=1) == total  # rows or not: same total
    total4 = cpu.community_loss(X, pi, pc, mp, ln, threads=4)
    assert abs(total4 - total) <= total_tol and abs(total4 - total_ref) <= total_tol
