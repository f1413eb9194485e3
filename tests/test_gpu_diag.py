"""The diagonal-covariance entries on the GPU against float64 numpy (tests/diag_cases.py):
come_gmm_estep_diag, come_gmm_diag_moments, come_gmm_diag_scatter, come_community_grad_diag and
come_community_loss_diag, through their come_amd wrappers.

Tolerances are the project's own for the full-covariance kernels: E-step resp atol 2e-4, lse rtol
2e-5 / atol 2e-3 (tests/test_gpu_gmm.py); M-step sums rtol 1e-4, atol 1e-4 max|ref| per component
and, at production chunk lengths, RMS <= 2x and max <= 3x the error of a plain fp32 running sum of
the same terms in the same chunks (tests/test_gpu_scatter_accuracy.py); community step rtol / atol
2e-5 and RMS <= 2x an fp32 numpy evaluation; loss per row 2e-3 sum|pi| + 2e-5 sum|pi lp|
(tests/test_gpu_community_loss.py)."""
import ctypes
import functools

import numpy as np
import pytest

import diag_cases as dc
from come_amd import _lib, gmm
from come_amd import community_embeddings as ce

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# V no multiple of any tile; a one-row launch; K = 1; K above the register batch and the M-step's
# component group; both ends of d
SHAPES = [(2500, 5, 128), (3000, 6, 64), (129, 2, 64), (1, 1, 128), (1000, 4, 8), (777, 3, 100),
          (900, 4, 256), (300, 70, 200), (257, 300, 32), (65, 3, 512), (500, 2, 1)]
THREE = [(3000, 6, 64), (777, 3, 100), (900, 4, 256)]


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


@functools.lru_cache(maxsize=None)
def case(V, K, d):
    """Inputs and fp32 operands, built once per shape and never modified."""
    X, pi, w, mu, var = dc.problem(V, K, d, V + d)
    ops = dc.f32(*dc.operands(w, mu, var))
    for a in (X, pi, w, mu, var) + ops:
        a.setflags(write=False)
    return X, pi, w, mu, var, ops


@functools.lru_cache(maxsize=None)
def estep_case(V, K, d):
    X, _, _, _, _, ops = case(V, K, d)
    return dc.estep_ref(X, *ops)


def check_estep(resp, lse, ref):
    np.testing.assert_allclose(resp.cpu().numpy(), ref[0], atol=2e-4)
    np.testing.assert_allclose(lse.cpu().numpy(), ref[1], rtol=2e-5, atol=2e-3)


# ---- E-step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,d", SHAPES)
def test_estep_vs_float64(V, K, d):
    X, _, _, _, _, (ps, mp, ln) = case(V, K, d)
    x = t(X)
    resp, lse = gmm.estep_diag(x, t(ps), t(mp), t(ln))
    assert resp.shape == (V, K) and lse.shape == (V,)
    check_estep(resp, lse, estep_case(V, K, d))
    none, lse2 = gmm.estep_diag(x, t(ps), t(mp), t(ln), want_resp=False)  # resp_out = NULL
    assert none is None and torch.equal(lse, lse2)


def test_estep_zero_weight_components():
    """Two components with log_norm = -inf: responsibility exactly 0, the lse that of the rest."""
    V, K, d = 777, 5, 100
    X, _, _, _, _, (ps, mp, ln) = case(V, K, d)
    ln = ln.copy()
    ln[[1, 3]] = -np.inf
    resp, lse = gmm.estep_diag(t(X), t(ps), t(mp), t(ln))
    resp, lse = resp.cpu().numpy(), lse.cpu().numpy()
    assert (resp[:, [1, 3]] == 0.0).all() and np.isfinite(resp).all() and np.isfinite(lse).all()
    keep = [0, 2, 4]
    ref = dc.estep_ref(X, ps[keep], mp[keep], ln[keep])
    np.testing.assert_allclose(resp[:, keep], ref[0], atol=2e-4)
    np.testing.assert_allclose(lse, ref[1], rtol=2e-5, atol=2e-3)


@pytest.mark.parametrize("V,K,d", [(129, 2, 64), (2500, 5, 128)])
def test_estep_operands_at_element_offset_1(V, K, d):
    X, _, _, _, _, (ps, mp, ln) = case(V, K, d)
    resp, lse = gmm.estep_diag(off1(t(X)), off1(t(ps)), off1(t(mp)), off1(t(ln)))
    check_estep(resp, lse, estep_case(V, K, d))


@pytest.mark.parametrize("V,K,d", [(3000, 6, 64), (777, 3, 100)])
def test_estep_agrees_with_the_full_covariance_estep(V, K, d):
    """come_gmm_estep fed diag(prec_sqrt[k]) as prec_chol: both results within the bounds."""
    X, _, _, _, _, (ps, mp, ln) = case(V, K, d)
    pc = np.zeros((K, d, d), np.float32)
    pc[:, np.arange(d), np.arange(d)] = ps
    x = t(X)
    resp, lse = gmm.estep_diag(x, t(ps), t(mp), t(ln))
    resp_f, lse_f = gmm.estep(x, t(pc), t(mp), t(ln))
    check_estep(resp, lse, (resp_f.cpu().numpy().astype(np.float64),
                            lse_f.cpu().numpy().astype(np.float64)))
    check_estep(resp_f, lse_f, estep_case(V, K, d))


# ---- M-step ----------------------------------------------------------------------------------
def check_sums(got, ref, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == ref.shape
    for k in range(len(ref)):
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-4 * np.abs(ref[k]).max(),
                                   err_msg="%s component %d" % (what, k))


def planned_chunks(V, K, d):
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    return gmm.diag_plan(V, d, K, cus)[0]


@pytest.mark.parametrize("V,K,d", SHAPES)
def test_moments_and_scatter_vs_float64(V, K, d):
    X, pi, _, mu, _, _ = case(V, K, d)
    means = mu.astype(np.float32)
    nk_ref, sx_ref = dc.moments_ref(X, pi)
    ssq_ref = dc.scatter_ref(X, pi, means)
    x, r, m = t(X), t(pi), t(means)
    ragged = 7 if V >= 7 and V % 7 else 4  # V % chunks != 0 wherever V allows it
    for chunks in (None, 1, 3, ragged):
        if chunks is not None and chunks > V:
            continue
        c = planned_chunks(V, K, d) if chunks is None else chunks
        nk, sx = gmm.diag_moments(x, r, chunks=c)
        np.testing.assert_allclose(nk.cpu().numpy(), nk_ref, rtol=1e-4)
        check_sums(sx, sx_ref, "sx chunks=%d" % c)
        check_sums(gmm.diag_scatter(x, r, m, chunks=c), ssq_ref, "ssq chunks=%d" % c)


@pytest.mark.parametrize("V,K,d", [(2500, 5, 128), (300, 70, 200), (777, 3, 100)])
def test_m_step_operands_at_element_offset_1(V, K, d):
    """X, resp and means 4 bytes off a 16-byte boundary: the moments take their 4-byte loads of x
    (16-byte loads need an aligned x and d % 4 == 0), under the same bounds."""
    X, pi, _, mu, _, _ = case(V, K, d)
    means = mu.astype(np.float32)
    x, r, m = off1(t(X)), off1(t(pi)), off1(t(means))
    nk, sx = gmm.diag_moments(x, r, chunks=3)
    np.testing.assert_allclose(nk.cpu().numpy(), dc.moments_ref(X, pi)[0], rtol=1e-4)
    check_sums(sx, dc.moments_ref(X, pi)[1], "sx")
    check_sums(gmm.diag_scatter(x, r, m, chunks=3), dc.scatter_ref(X, pi, means), "ssq")
    assert torch.equal(sx, gmm.diag_moments(t(X), t(pi), chunks=3)[1])  # the same sums, bit for bit


def test_m_step_with_one_chunk_needs_no_scratch():
    V, K, d = 777, 3, 100
    X, pi, _, mu, _, _ = case(V, K, d)
    x, r, m = t(X), t(pi), t(mu.astype(np.float32))
    L, P = _lib.lib(), _lib.ptr
    nk = torch.empty(K, dtype=torch.float64, device=dev())
    sx = torch.empty((K, d), dtype=torch.float64, device=dev())
    ssq = torch.empty((K, d), dtype=torch.float64, device=dev())
    s = _lib.stream_handle(x.device)
    _lib.check(L.come_gmm_diag_moments(P(x), V, d, P(r), K, 1, None, P(nk), P(sx), s), "moments")
    _lib.check(L.come_gmm_diag_scatter(P(x), V, d, P(r), P(m), K, 1, None, P(ssq), s), "scatter")
    check_sums(sx, dc.moments_ref(X, pi)[1], "sx")
    check_sums(ssq, dc.scatter_ref(X, pi, mu.astype(np.float32)), "ssq")


@pytest.mark.parametrize("V,K,d", [(3000, 6, 64), (300, 70, 200)])
def test_one_hot_resp_with_an_empty_component(V, K, d):
    X, _, _, mu, _, _ = case(V, K, d)
    rng = np.random.RandomState(V)
    lab = rng.randint(0, K - 1, V)
    lab[lab >= 2] += 1  # component 2 gets no row
    resp = np.zeros((V, K), np.float32)
    resp[np.arange(V), lab] = 1.0
    means = mu.astype(np.float32)
    x, r, m = t(X), t(resp), t(means)
    nk, sx = gmm.diag_moments(x, r, chunks=3)
    ssq = gmm.diag_scatter(x, r, m, chunks=3)
    assert (nk.cpu().numpy() == np.bincount(lab, minlength=K)).all()
    assert nk[2] == 0 and (sx[2] == 0).all() and (ssq[2] == 0).all()
    check_sums(sx, dc.moments_ref(X, resp)[1], "sx")
    check_sums(ssq, dc.scatter_ref(X, resp, means), "ssq")


@functools.lru_cache(maxsize=None)
def chunk_length_case(R, d):
    """Two chunks of R rows, K = 2: inputs, float64 references and the fp32 running-sum model's
    error (tests/test_gpu_scatter_accuracy.py's construction)."""
    V, K = 2 * R, 2
    rng = np.random.RandomState(R + d)
    means = (rng.normal(size=(K, d)) * 2).astype(np.float32)
    lab = rng.randint(0, K, V)
    X = (means[lab] + rng.normal(size=(V, d))).astype(np.float32)
    resp = rng.dirichlet(np.ones(K), V).astype(np.float32)
    sx_ref = dc.moments_ref(X, resp)[1]
    ssq_ref = dc.scatter_ref(X, resp, means)
    sx_terms = resp[:, :, None] * X[:, None, :]
    diff = X[:, None, :] - means[None]
    ssq_terms = resp[:, :, None] * (diff * diff)
    assert sx_terms.dtype == ssq_terms.dtype == np.float32
    model = (dc.err_stats(dc.running_sum_f32(sx_terms, 2), sx_ref),
             dc.err_stats(dc.running_sum_f32(ssq_terms, 2), ssq_ref))
    return X, resp, means, sx_ref, ssq_ref, model


@pytest.mark.parametrize("V,d", [(1_000_000, 128), (10_000_000, 256)])
def test_fp32_error_at_production_chunk_length(V, d):
    cus = torch.cuda.get_device_properties(dev()).multi_processor_count
    R = gmm.diag_plan(V, d, 50, cus)[1]
    X, resp, means, sx_ref, ssq_ref, model = chunk_length_case(R, d)
    x, r, m = t(X), t(resp), t(means)
    _, sx = gmm.diag_moments(x, r, chunks=2)
    ssq = gmm.diag_scatter(x, r, m, chunks=2)
    for name, got, ref, mod in (("sx", sx, sx_ref, model[0]), ("ssq", ssq, ssq_ref, model[1])):
        st = dc.err_stats(got.cpu().numpy(), ref)
        print("\n%s rows/chunk %d d %d: rms %.3g max %.3g | running sum: rms %.3g max %.3g | "
              "ratio %.2f %.2f" % (name, R, d, st[0], st[1], mod[0], mod[1], st[0] / mod[0],
                                   st[1] / mod[1]))
        assert st[0] <= 2 * mod[0] and st[1] <= 3 * mod[1], (name, st, mod)


# ---- community step --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_case(V, K, d, iters):
    """beta and lr for which some elements clip at +-5 and most do not: beta / K puts the 95th
    percentile of the first step's |gradient| at the clip."""
    X, pi, _, mu, var, _ = case(V, K, d)
    mu32, iv = mu.astype(np.float32), (1.0 / var).astype(np.float32)
    _, g1 = dc.grad_ref(X, pi, mu32, iv, float(K), 0.01, 1)  # beta / K = 1: the plain sum
    beta, lr = float(K) * 5.0 / float(np.percentile(np.abs(g1), 95)), 0.01
    ref, g0 = dc.grad_ref(X, pi, mu32, iv, beta, lr, iters)
    ref32, _ = dc.grad_ref(X, pi, mu32, iv, beta, lr, iters, dtype=np.float32)
    return X, pi, mu32, iv, beta, lr, ref, g0, ref32


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("V,K,d", SHAPES)
def test_community_grad_vs_float64(V, K, d, iters):
    X, pi, mu32, iv, beta, lr, ref, g0, ref32 = grad_case(V, K, d, iters)
    clipped = (np.abs(g0) > 5).mean()
    assert 0 < clipped < 0.5, clipped  # both kinds exist
    x = t(X)
    ce.community_grad_diag(x, t(pi), t(mu32), t(iv), beta, lr, iters)
    got = x.cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5)
    rms, rms32 = dc.err_stats(got, ref)[0], dc.err_stats(ref32, ref)[0]
    print("\ngrad (%d, %d, %d) iters %d: rms %.3g, fp32 numpy %.3g" % (V, K, d, iters, rms, rms32))
    assert rms <= 2 * rms32


def test_community_grad_agrees_with_the_full_covariance_step():
    V, K, d = 3000, 6, 64
    X, pi, mu32, iv, beta, lr, ref, _, _ = grad_case(V, K, d, 3)
    inv = np.zeros((K, d, d), np.float32)
    inv[:, np.arange(d), np.arange(d)] = iv
    xa, xb = t(X), t(X)
    ce.community_grad_diag(xa, t(pi), t(mu32), t(iv), beta, lr, 3)
    ce.community_grad(xb, t(pi), t(mu32), t(inv), beta, lr, 3)
    np.testing.assert_allclose(xa.cpu().numpy(), xb.cpu().numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(xb.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


# ---- loss ------------------------------------------------------------------------------------
def check_loss(total, rows, ref):
    rows_ref, total_ref, row_tol, total_tol = ref
    rows = rows.cpu().numpy()
    assert np.isfinite(rows).all()
    assert (np.abs(rows - rows_ref) <= row_tol).all()
    assert abs(total - total_ref) <= total_tol


@pytest.mark.parametrize("V,K,d", SHAPES)
def test_loss_rows_and_total_vs_float64(V, K, d):
    X, pi, _, mu, var, _ = case(V, K, d)
    total, rows = ce.community_loss_diag(t(X), t(pi), t(mu), t(var), return_rows=True)
    assert isinstance(total, float) and rows.shape == (V,)
    check_loss(total, rows, dc.loss_ref(X, pi, mu, var))
    assert ce.community_loss_diag(t(X), t(pi), t(mu), t(var)) == total  # row_out = NULL


@pytest.mark.parametrize("V,K,d", [(3000, 6, 64), (777, 3, 100)])
def test_loss_uses_pi_as_given(V, K, d):
    X, pi, _, mu, var, _ = case(V, K, d)
    scale = np.array([0.0, 2.0, 3.0], np.float32)[np.arange(V) % 3]
    pis = pi * scale[:, None]
    total, rows = ce.community_loss_diag(t(X), t(pis), t(mu), t(var), return_rows=True)
    check_loss(total, rows, dc.loss_ref(X, pis, mu, var))
    rows = rows.cpu().numpy()
    assert (rows[scale == 0] == 0.0).all() and (rows[scale != 0] != 0.0).all()
    _, base = ce.community_loss_diag(t(X), t(pi), t(mu), t(var), return_rows=True)
    assert (rows[scale == 2] == 2 * base.cpu().numpy()[scale == 2]).all()  # exact in fp32


@pytest.mark.parametrize("V,K,d", [(2500, 5, 128), (3000, 6, 64)])
def test_gradient_step_raises_the_signed_total(V, K, d):
    """One step (beta = 1, lr = 0.1) raises the signed total, in float64 and on the GPU alike."""
    X, pi, _, mu, var, _ = case(V, K, d)
    mu32, iv = mu.astype(np.float32), (1.0 / var).astype(np.float32)
    ref = dc.loss_ref(X, pi, mu, var)
    after, g0 = dc.grad_ref(X, pi, mu32, iv, 1.0, 0.1, 1)
    assert np.abs(g0).max() < 5.0  # no coordinate clipped
    rise_ref = dc.loss_ref(after, pi, mu, var)[1] - ref[1]
    assert rise_ref > 100 * ref[3]
    x, p, m, v = t(X), t(pi), t(mu), t(var)
    before = ce.community_loss_diag(x, p, m, v)
    ce.community_grad_diag(x, p, t(mu32), t(iv), 1.0, 0.1, 1)
    rise = ce.community_loss_diag(x, p, m, v) - before
    print("\n(%d, %d, %d): rise float64 %.6g, GPU %.6g, tolerance %.3g" % (V, K, d, rise_ref, rise,
                                                                          ref[3]))
    assert rise > 0 and abs(rise - rise_ref) <= 2 * ref[3]


# ---- determinism -----------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,d", THREE)
def test_every_entry_is_bit_identical_from_run_to_run(V, K, d):
    X, pi, _, mu, var, (ps, mp, ln) = case(V, K, d)
    mu32, iv = mu.astype(np.float32), (1.0 / var).astype(np.float32)
    x, p = t(X), t(pi)

    def run():
        resp, lse = gmm.estep_diag(x, t(ps), t(mp), t(ln))
        nk, sx = gmm.diag_moments(x, p, chunks=3)
        ssq = gmm.diag_scatter(x, p, t(mu32), chunks=3)
        y = x.clone()
        ce.community_grad_diag(y, p, t(mu32), t(iv), 4.0 * K, 0.01, 2)
        total, rows = ce.community_loss_diag(x, p, t(mu), t(var), return_rows=True)
        return (resp, lse, nk, sx, ssq, y, rows), total

    (a, ta), (b, tb) = run(), run()
    assert ta == tb == ce.community_loss_diag(x, p, t(mu), t(var))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- argument checks -------------------------------------------------------------------------
def test_invalid_arguments():
    L = _lib.lib()
    p, n = ctypes.c_void_p(256), ctypes.c_void_p(0)
    ci = ctypes.c_int(0)
    calls = {
        "estep": lambda d, K, q: L.come_gmm_estep_diag(q, 10, d, p, p, p, K, p, p, n),
        "scratch": lambda d, K, q: L.come_gmm_diag_scratch(
            10, d, K, 256, ctypes.byref(ci) if q.value else None, ctypes.byref(ci)),
        "moments": lambda d, K, q: L.come_gmm_diag_moments(q, 10, d, p, K, 1, p, p, p, n),
        "scatter": lambda d, K, q: L.come_gmm_diag_scatter(q, 10, d, p, p, K, 1, p, p, n),
        "grad": lambda d, K, q: L.come_community_grad_diag(q, 10, d, p, p, p, K, 1.0, 0.1, 1, n),
        "loss": lambda d, K, q: L.come_community_loss_diag(q, 10, d, p, p, p, p, K, p, p, n),
    }
    for name, call in calls.items():
        for d, K, q in ((0, 3, p), (513, 3, p), (8, 0, p), (8, 4097, p), (8, 3, n)):
            assert call(d, K, q) == -1, (name, d, K)
            assert len(L.come_last_error()) > 0
