"""The mixture kernels past K = 64, at the limits of their narrow forms, with components of weight
zero, with library scratch that regrows and on non-default streams -- against float64 numpy.

V = 130 rows everywhere: one full 128-row workgroup and a ragged tile of two rows.  What only runs
at large K:
  * resp_normalize's second pass (K > 64) in k_gmm_resp_b16;
  * a second trip through the grid-stride loops of k_comm_split16 (K > 512 at d = 128, > 2048 at
    d = 64) and k_pack_upper_b16 (K >= 820 at d = 128, >= 2731 at d = 64): K = 900 and K = 4096;
  * k_gmm_resp's LP[kTR][64] buffer full (K = 64, d other than 64 / 128) and the rejection at 65;
  * k_comm_loss_b16's weight prefetch with K % 4 = 0, 1, 3.
Inputs follow the existing tests: rows standard normal, factors triu(randn / sqrt(d)) + 2 I
(test_gpu_gmm.py::test_estep_default_and_fallback_agree), inv_cov as
test_gpu_parity.py::_community_vs_oracle, pi and resp from a Dirichlet.  The float64 references take
the fp32-rounded operands the kernels see and walk the components in blocks (no V x K x d array).
Tolerances are each kernel's own: test_gpu_gmm.py::test_estep_vs_numpy (resp atol 2e-4, lse rtol
2e-5 / atol 2e-3, row sums within 1e-4 as test_estep_default_and_fallback_agree),
test_gpu_parity.py::test_community_grad_vs_oracle (2e-5), test_gpu_community_loss.py (per row and
total), test_gpu_gmm.py::test_scatter_vs_numpy, test_gpu_kmeans.py (check_labels, sums, counts,
inertia).
"""
import functools
import warnings

import numpy as np
import pytest

from come_amd import _lib, gmm, kmeans
from come_amd import community_embeddings as ce
from come_amd._lib import options, ptr, stream_handle
from test_gpu_community_loss import check as check_loss
from test_gpu_community_loss import raw_loss
from test_gpu_kmeans import U, check_labels

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

V = 130
K128 = [63, 64, 65, 67, 128, 900]   # 900 > 512 (k_comm_split16) and >= 820 (k_pack_upper_b16)
K64 = [64, 65, 67, 4096]            # 4096 > 2048 and >= 2731; the documented maximum
SWEEP = [(K, 128) for K in K128] + [(K, 64) for K in K64]
SWEEP_FULL = [(K, d) for K, d in SWEEP if K <= 128]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def t(a):
    return torch.as_tensor(np.array(a, np.float32), device=dev())  # a copy: the cases are frozen


def off1(a):
    v = torch.empty(a.numel() + 1, dtype=torch.float32, device=a.device)[1:].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- inputs and float64 references, built once per shape ---------------------------------------
@functools.lru_cache(maxsize=None)
def mixture(rows, K, d, lower=False):
    """fp32 (X, P, mp, ln): standard-normal rows, upper factors triu(randn / sqrt(d)) + 2 I (with
    `lower`, component K // 2 transposed: a lower factor, so the launch runs k_gmm_resp16_full),
    mp = mu P with mu = 0.3 randn, ln = log of Dirichlet weights."""
    dev()
    rng = np.random.RandomState(1000 * d + 7 * K + rows)
    X = rng.standard_normal((rows, d)).astype(np.float32)
    P = np.triu(rng.standard_normal((K, d, d)) / np.sqrt(d)) + 2 * np.eye(d)
    if lower:
        P[K // 2] = P[K // 2].T.copy()
    mu = rng.standard_normal((K, d)) * 0.3
    mp = np.matmul(mu[:, None, :], P)[:, 0, :]
    ln = np.log(rng.dirichlet(np.ones(K)))
    return freeze(X, P.astype(np.float32), mp.astype(np.float32), ln.astype(np.float32))


def log_prob64(X, P, mp, ln, block=64):
    """float64 [V, K]: ln_k - |x P_k - mp_k|^2 / 2 from the fp32 operands, `block` components at a
    time as one GEMM."""
    rows, d = X.shape
    K = P.shape[0]
    X64 = X.astype(np.float64)
    lp = np.empty((rows, K))
    for k0 in range(0, K, block):
        Pb = P[k0:k0 + block].astype(np.float64)
        b = Pb.shape[0]
        Y = (X64 @ Pb.transpose(1, 0, 2).reshape(d, b * d)).reshape(rows, b, d)
        Y -= mp[k0:k0 + b].astype(np.float64)[None]
        lp[:, k0:k0 + b] = ln[k0:k0 + b].astype(np.float64)[None] - 0.5 * (Y * Y).sum(-1)
    return lp


def resp64(lp):
    """(responsibilities, per-row log-sum-exp) of float64 log-probabilities; -inf columns give 0."""
    from scipy.special import logsumexp
    lse = logsumexp(lp, 1)
    return np.exp(lp - lse[:, None]), lse


@functools.lru_cache(maxsize=None)
def estep_case(rows, K, d, lower=False):
    ops = mixture(rows, K, d, lower)
    return ops + freeze(*resp64(log_prob64(*ops)))


def check_estep(resp, lse, ref_resp, ref_lse, what):
    resp, lse = resp.cpu().numpy(), lse.cpu().numpy()
    print("%s: max |resp - ref| %.3g, max |lse - ref| %.3g, max |row sum - 1| %.3g" % (
        what, np.abs(resp - ref_resp).max(), np.abs(lse - ref_lse).max(),
        np.abs(resp.sum(1, dtype=np.float64) - 1).max()))
    assert np.isfinite(resp).all() and np.isfinite(lse).all()
    np.testing.assert_allclose(resp, ref_resp, atol=2e-4)
    np.testing.assert_allclose(lse, ref_lse, rtol=2e-5, atol=2e-3)
    assert np.abs(resp.sum(1, dtype=np.float64) - 1).max() < 1e-4


@functools.lru_cache(maxsize=None)
def community_case(K, d):
    """(x0, pi, mu, inv) of test_gpu_parity.py::_community_vs_oracle (A A^T as a batched matmul)."""
    dev()
    rng = np.random.RandomState(d + V + K)
    x0 = rng.normal(size=(V, d)).astype(np.float32)
    A = rng.normal(size=(K, d, d)) / np.sqrt(d)
    cov = A @ A.transpose(0, 2, 1) + np.eye(d)[None] * 0.5
    inv = np.linalg.inv(cov.astype(np.float32)).astype(np.float32)
    mu = rng.normal(size=(K, d)).astype(np.float32)
    pi = rng.dirichlet(np.ones(K), V).astype(np.float32)
    return freeze(x0, pi, mu, inv)


ITERS, LR, BETAS = 2, 0.1, (0.05, 40.0)


def betas(K):
    """_community_vs_oracle's two betas, and one that grows with K: the step is beta / K times an
    average over the components, so at K >= 63 beta = 40 no longer reaches the clip at +-5; beta =
    8 K clips about a quarter of the coordinates."""
    return BETAS + (8.0 * K,)


@functools.lru_cache(maxsize=None)
def community64(K, d, beta, block=64):
    """oracle.community_train restated in float64 (its K matmuls per chunk take seconds at
    K = 4096): x -= lr clip(beta / K sum_k pi_ik inv_k (x_i - mu_k), -5, 5), ITERS times."""
    x0, pi, mu, inv = community_case(K, d)
    x, p64, mu64 = x0.astype(np.float64), pi.astype(np.float64), mu.astype(np.float64)
    for _ in range(ITERS):
        G = np.zeros_like(x)
        for k0 in range(0, K, block):
            b = min(block, K - k0)
            D = (x[:, None, :] - mu64[None, k0:k0 + b]) * p64[:, k0:k0 + b, None]
            M = inv[k0:k0 + b].astype(np.float64).transpose(0, 2, 1).reshape(b * d, d)
            G += D.reshape(V, b * d) @ M  # G[i, c] += sum_k sum_j pi_ik (x_i - mu_k)_j inv_k[c, j]
        x = x - np.clip(G * (beta / K), -5, 5) * LR
    return freeze(x)[0]


def check_community(x, K, d, beta, what):
    ref = community64(K, d, beta)
    x = x.cpu().numpy()
    print("%s beta %g: max |x - ref| %.3g" % (what, beta, np.abs(x - ref).max()))
    np.testing.assert_allclose(x, ref, rtol=2e-5, atol=2e-5)


def run_community(K, d, beta):
    x0, pi, mu, inv = community_case(K, d)
    x = t(x0)
    ce.community_grad(x, t(pi), t(mu), t(inv), beta, LR, ITERS)
    return x


# ---- scratch that regrows, and non-default streams (first: before anything grew the scratch) ----
@pytest.mark.parametrize("r16", [3, 2])
def test_estep_scratch_regrows_on_one_stream(r16):
    """K = 3, then 900, then 3 on one fresh stream (its library scratch starts empty, grows for
    the second call and is reused by the third): every result against its own reference."""
    s = torch.cuda.Stream(device=dev())
    outs = []
    torch.cuda.synchronize()
    with torch.cuda.stream(s), options(gmm_resp16=r16):
        for K in (3, 900, 3):
            X, P, mp, ln = estep_case(V, K, 128)[:4]
            outs.append((K, gmm.estep(t(X), t(P), t(mp), t(ln))))
    torch.cuda.synchronize()
    for K, (resp, lse) in outs:
        check_estep(resp, lse, *estep_case(V, K, 128)[4:], what="K=%d r16=%d" % (K, r16))


@pytest.mark.parametrize("kern", [3, 2])
def test_community_scratch_regrows_on_one_stream(kern):
    s = torch.cuda.Stream(device=dev())
    outs = []
    torch.cuda.synchronize()
    with torch.cuda.stream(s), options(community_async=kern):
        for K in (3, 900, 3):
            outs.append((K, run_community(K, 128, BETAS[0])))
    torch.cuda.synchronize()
    for K, x in outs:
        check_community(x, K, 128, BETAS[0], "K=%d kern=%d" % (K, kern))


def test_two_streams_run_different_component_counts():
    """E-step and community step issued from one thread on two non-default streams, K = 3 on one
    and K = 900 on the other (d = 128): on each stream the rows come out of a torch op (2 x halved:
    exact) and the result goes into one; both are checked after one synchronize."""
    streams = [torch.cuda.Stream(device=dev()) for _ in range(2)]
    Ks = (3, 900)
    doubled = [t(2 * estep_case(V, K, 128)[0]) for K in Ks]
    doubled_x0 = [t(2 * community_case(K, 128)[0]) for K in Ks]
    ops = [[t(a) for a in estep_case(V, K, 128)[1:4]] for K in Ks]
    cops = [[t(a) for a in community_case(K, 128)[1:]] for K in Ks]
    torch.cuda.synchronize()
    outs = []
    for rep in range(2):  # the second round meets scratch the first one grew
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                resp, lse = gmm.estep(doubled[i] * 0.5, *ops[i])
                x = doubled_x0[i] * 0.5
                ce.community_grad(x, *cops[i], BETAS[0], LR, ITERS)
                outs.append((Ks[i], resp + 0.0, lse + 0.0, x + 0.0))
    torch.cuda.synchronize()
    for K, resp, lse, x in outs:
        check_estep(resp, lse, *estep_case(V, K, 128)[4:], what="stream K=%d" % K)
        check_community(x, K, 128, BETAS[0], "stream K=%d" % K)


# ---- A. the K sweep ------------------------------------------------------------------------------
@pytest.mark.parametrize("r16", [3, 2])
@pytest.mark.parametrize("K,d", SWEEP)
def test_estep_sweep(K, d, r16):
    X, P, mp, ln, ref_resp, ref_lse = estep_case(V, K, d)
    with options(gmm_resp16=r16):
        resp, lse = gmm.estep(t(X), t(P), t(mp), t(ln))
    check_estep(resp, lse, ref_resp, ref_lse, "K=%d d=%d r16=%d" % (K, d, r16))


@pytest.mark.parametrize("r16", [3, 2])
@pytest.mark.parametrize("K,d", SWEEP_FULL)
def test_estep_full_body_sweep(K, d, r16):
    """One lower factor in the launch: every component runs k_gmm_resp16_full."""
    X, P, mp, ln, ref_resp, ref_lse = estep_case(V, K, d, True)
    assert np.tril(P[K // 2], -1).any()
    with options(gmm_resp16=r16):
        resp, lse = gmm.estep(t(X), t(P), t(mp), t(ln))
    check_estep(resp, lse, ref_resp, ref_lse, "full K=%d d=%d r16=%d" % (K, d, r16))


@pytest.mark.parametrize("kern", [3, 2])
@pytest.mark.parametrize("K,d", SWEEP)
def test_community_grad_sweep(K, d, kern):
    with options(community_async=kern):
        for beta in betas(K):
            check_community(run_community(K, d, beta), K, d, beta,
                            "K=%d d=%d kern=%d" % (K, d, kern))


@functools.lru_cache(maxsize=None)
def loss_case(K, d):
    """The E-step's rows and factors with log_norm = sum log diag P - d/2 log(2 pi) (no weight) and
    pi from a Dirichlet; the reference tuple of test_community_loss_host.reference."""
    X, P, mp, _ = mixture(V, K, d)
    ln = (np.log(np.diagonal(P, axis1=1, axis2=2).astype(np.float64)).sum(1)
          - 0.5 * d * np.log(2 * np.pi)).astype(np.float32)
    pi = np.random.RandomState(K + d).dirichlet(np.ones(K), V).astype(np.float32)
    p = pi.astype(np.float64)
    lp = log_prob64(X, P, mp, ln)
    rows = (p * lp).sum(1)
    tol = 2e-3 * np.abs(p).sum(1) + 2e-5 * np.abs(p * lp).sum(1)
    freeze(ln, pi, rows, tol)
    return X, P, mp, ln, pi, (rows, rows.sum(), tol, tol.sum())


@pytest.mark.parametrize("K,d", SWEEP)
def test_community_loss_sweep(K, d):
    X, P, mp, ln, pi, ref = loss_case(K, d)
    total, rows = raw_loss(t(X), t(pi), t(P), t(mp), t(ln))
    check_loss(total, rows, ref, "K=%d d=%d" % (K, d))


@functools.lru_cache(maxsize=None)
def scatter_case(K, d):
    dev()
    rng = np.random.RandomState(V + K + d)
    X = rng.normal(size=(V, d)).astype(np.float32)
    R = rng.dirichlet(np.ones(K), V).astype(np.float32)
    M = rng.normal(size=(K, d)).astype(np.float32)
    X64 = X.astype(np.float64)
    ref = np.empty((K, d, d))
    for k in range(K):
        D = X64 - M[k]
        ref[k] = (R[:, k, None] * D).T @ D
    return freeze(X, R, M, ref)


@pytest.mark.parametrize("cov", [3, 4, 5])
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("K", [65, 67])
def test_scatter_past_64_components(K, d, cov):
    """No K loop in the scatter: the grid is K / (components per workgroup), ragged at 65 and 67."""
    X, R, M, ref = scatter_case(K, d)
    with options(gmm_cov_async=cov):
        S = gmm.scatter(t(X), t(R), t(M), chunks=2).cpu().numpy()
    for k in range(K):
        np.testing.assert_allclose(S[k], ref[k], rtol=1e-4, atol=1e-4 * np.abs(ref[k]).max())


@functools.lru_cache(maxsize=None)
def kmeans_case(rows, K, d):
    """Standard-normal rows; centres = rows drawn with replacement + 0.3 N(0, 1) (K may be > V)."""
    rng = np.random.RandomState(rows + K + d)
    X = rng.standard_normal((rows, d)).astype(np.float32)
    C = X[rng.randint(0, rows, K)] + 0.3 * rng.standard_normal((K, d))
    return torch.as_tensor(X, device=dev()), torch.as_tensor(C.astype(np.float32), device=dev())


def check_kmeans(rows, K, d):
    """test_gpu_kmeans.py's checks: optimal labels within fp32 rounding (assign and lloyd agree),
    counts exact, sums within R u sum |x|, inertia the float64 sum of mindist."""
    X, C = kmeans_case(rows, K, d)
    labels, mind = kmeans.assign(X, C)
    check_labels(X, C, labels, mind)
    lab2, sums, counts, inertia, mind2 = kmeans.accumulate(X, C, return_mindist=True)
    assert torch.equal(lab2.long(), labels) and torch.equal(mind2, mind)
    _, R = kmeans.scratch_plan(rows, d, K,
                               torch.cuda.get_device_properties(X.device).multi_processor_count)
    assert torch.equal(counts, torch.bincount(labels, minlength=K))
    S64 = torch.zeros((K, d), dtype=torch.float64, device=X.device).index_add_(0, labels,
                                                                             X.double())
    A = torch.zeros((K, d), dtype=torch.float64, device=X.device).index_add_(0, labels,
                                                                             X.double().abs())
    assert bool(((sums - S64).abs() <= R * U * A).all())
    ref = mind.double().sum()
    assert abs(float(inertia) - float(ref)) <= rows * 2.0 ** -53 * float(ref)


@pytest.mark.parametrize("rows,K,d", [(V, 65, 128), (V, 4096, 64)])
def test_kmeans_past_64_components(rows, K, d):
    """K > 64 at d = 64, 128: the VALU kernel."""
    check_kmeans(rows, K, d)


# ---- the limits of the narrow forms ------------------------------------------------------------
NARROW = [(V, 64, 100), (V, 64, 8), (63, 64, 1)]


@pytest.mark.parametrize("rows,K,d", NARROW)
def test_estep_at_the_valu_kernels_last_component_count(rows, K, d):
    """K = 64 fills k_gmm_resp's LP[kTR][64]."""
    X, P, mp, ln, ref_resp, ref_lse = estep_case(rows, K, d)
    resp, lse = gmm.estep(t(X), t(P), t(mp), t(ln))
    check_estep(resp, lse, ref_resp, ref_lse, "V=%d K=%d d=%d" % (rows, K, d))


@pytest.mark.parametrize("rows,K,d", NARROW)
def test_kmeans_at_the_narrow_limit(rows, K, d):
    check_kmeans(rows, K, d)


@pytest.mark.parametrize("d,unaligned", [(100, False), (128, True)])
def test_estep_rejects_65_components_and_writes_nothing(d, unaligned):
    """K = 65 at d = 100, and at d = 128 when prec_chol is not 16-byte aligned (the VALU kernel's
    route): COME_E_INVALID, resp_out and lse_out bit for bit as they were."""
    K = 65
    X, P, mp, ln = (t(a) for a in mixture(V, K, d))
    if unaligned:
        P = off1(P)
    resp = torch.randint(-2 ** 31, 2 ** 31 - 1, (V, K), dtype=torch.int32, device=dev())
    lse = torch.randint(-2 ** 31, 2 ** 31 - 1, (V,), dtype=torch.int32, device=dev())
    resp0, lse0 = resp.clone(), lse.clone()
    rc = _lib.lib().come_gmm_estep(ptr(X), V, d, ptr(P), ptr(mp), ptr(ln), K, ptr(resp), ptr(lse),
                                   stream_handle(X.device))
    assert rc == -1  # COME_E_INVALID
    with pytest.raises(_lib.ComeError, match="gmm_resp"):
        _lib.check(rc, "come_gmm_estep")
    torch.cuda.synchronize()
    assert torch.equal(resp, resp0) and torch.equal(lse, lse0)


# ---- B. components of weight zero ----------------------------------------------------------------
ZERO_FORMS = [("b16", 64), ("b16", 128), ("16t", 64), ("16t", 128), ("full", 64), ("full", 128),
              ("valu", 100), ("wide", 200), ("unaligned", 128)]


@pytest.mark.parametrize("zero", [(0,), (0, 1), (2,), (5,)])
@pytest.mark.parametrize("form,d", ZERO_FORMS)
def test_estep_zero_weight_components(form, d, zero):
    """log_norm = -inf (log of a weight 0, GaussianMixture(weights_init=[0, ...])) on some of K = 6
    components: those columns are exactly 0.0, the others and lse are the mixture of the remaining
    components, nothing is NaN.  (All of them -inf is NaN in sklearn too: not asserted.)"""
    K = 6
    X, P, mp, ln = mixture(V, K, d, form == "full")
    ln = ln.copy()
    ln[list(zero)] = -np.inf
    with np.errstate(invalid="ignore"):
        ref_resp, ref_lse = resp64(log_prob64(X, P, mp, ln))
    keep = [k for k in range(K) if k not in zero]
    kept = resp64(log_prob64(X, P[keep], mp[keep], ln[keep]))  # the float64 mixture without them
    np.testing.assert_allclose(ref_resp[:, keep], kept[0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref_lse, kept[1], rtol=1e-12, atol=0)
    assert (ref_resp[:, list(zero)] == 0).all()
    Pt = off1(t(P)) if form == "unaligned" else t(P)
    with options(gmm_resp16=2 if form == "16t" else 3):
        resp, lse = gmm.estep(t(X), Pt, t(mp), t(ln))
    got = resp.cpu().numpy()
    assert not np.isnan(got).any() and not np.isnan(lse.cpu().numpy()).any()
    assert (got[:, list(zero)] == 0.0).all()
    check_estep(resp, lse, ref_resp, ref_lse, "%s d=%d zero=%s" % (form, d, zero))


def test_gaussian_mixture_with_a_zero_initial_weight_matches_sklearn():
    """weights_init = [0, .5, .5] at d = 64, one EM iteration from fixed means and precisions,
    against sklearn with the same init (test_gpu_gmm.py::test_em_iterations_match_sklearn's
    tolerances)."""
    from sklearn.exceptions import ConvergenceWarning
    from sklearn.mixture import GaussianMixture as SkGMM
    from test_gpu_gmm import problem
    rows, K, d = 1500, 3, 64
    X, w, mu, cov = problem(rows, K, d, 7 * rows + d, sep=1.5)
    rng = np.random.RandomState(1)
    mu0 = mu + rng.normal(size=mu.shape) * 0.5
    prec0 = np.stack([np.linalg.inv(c + np.eye(d) * 0.3) for c in cov])
    kw = dict(n_components=K, covariance_type="full", tol=0.0, reg_covar=1e-5, max_iter=1,
              weights_init=np.array([0.0, 0.5, 0.5]), means_init=mu0, precisions_init=prec0)
    sk = SkGMM(random_state=0, **kw)
    with warnings.catch_warnings(), np.errstate(divide="ignore"):
        warnings.simplefilter("ignore", ConvergenceWarning)
        warnings.simplefilter("ignore", RuntimeWarning)  # log(0) of the zero weight
        sk.fit(X.astype(np.float64))
    g = gmm.GaussianMixture(random_state=0, **kw).fit(torch.as_tensor(X, device=dev()))
    assert g.n_iter_ == sk.n_iter_ == 1
    for a in (g.weights_, g.means_, g.covariances_):
        assert np.isfinite(a).all()
    assert np.isfinite(g.lower_bound_)
    np.testing.assert_allclose(g.weights_, sk.weights_, rtol=2e-3, atol=1e-5)
    np.testing.assert_allclose(g.means_, sk.means_, rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(g.covariances_, sk.covariances_, rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(g.lower_bound_, sk.lower_bound_, rtol=1e-4)
    pp = g.predict_proba(X).cpu().numpy()
    np.testing.assert_allclose(pp, sk.predict_proba(X.astype(np.float64)), atol=5e-3)
