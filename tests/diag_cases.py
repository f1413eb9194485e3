"""Shared inputs and float64 numpy references for the diagonal-covariance entries
(come_gmm_estep_diag, come_gmm_diag_moments, come_gmm_diag_scatter, come_community_grad_diag,
come_community_loss_diag): used by tests/test_gpu_diag.py, tests/test_gpu_diag_fit.py and
tests/test_diag_host.py.  Not a test module.

mu and var are rounded to fp32 before any reference sees them (as test_gpu_community_loss.case
does), so the float64 reference evaluates the very parameters the entry is given."""
import numpy as np

LOG2PI = np.log(2 * np.pi)


def problem(V, K, d, seed, sep=3.0):
    """Blobs with per-feature variances in [0.5, 1.5]: X [V, d] fp32, pi [V, K] fp32 (Dirichlet),
    weights [K], mu [K, d] and var [K, d] float64 holding fp32 values."""
    rng = np.random.RandomState(seed)
    mu = (rng.normal(size=(K, d)) * sep).astype(np.float32).astype(np.float64)
    var = rng.uniform(0.5, 1.5, size=(K, d)).astype(np.float32).astype(np.float64)
    w = rng.dirichlet(np.ones(K) * 3)
    lab = rng.choice(K, V, p=w)
    X = (mu[lab] + rng.normal(size=(V, d)) * np.sqrt(var[lab])).astype(np.float32)
    pi = rng.dirichlet(np.ones(K), V).astype(np.float32)
    return X, pi, w, mu, var


def operands(w, mu, var):
    """(prec_sqrt, mu_prec, log_norm) in float64; w = None: no mixture weight (the loss)."""
    ps = 1.0 / np.sqrt(var)
    ln = np.log(ps).sum(1) - 0.5 * mu.shape[1] * LOG2PI
    if w is not None:
        with np.errstate(divide="ignore"):
            ln = ln + np.log(w)
    return ps, mu * ps, ln


def f32(*a):
    return tuple(np.ascontiguousarray(v, np.float32) for v in a)


def log_prob(X, ps, mp, ln):
    """[V, K] float64: ln[k] - 1/2 sum_j (x_ij ps_kj - mp_kj)^2 of the operands as given."""
    X = X.astype(np.float64)
    out = np.empty((len(X), len(ps)))
    for k in range(len(ps)):
        y = X * ps[k].astype(np.float64) - mp[k].astype(np.float64)
        out[:, k] = float(ln[k]) - 0.5 * (y * y).sum(1)
    return out


def estep_ref(X, ps, mp, ln):
    """(resp, lse) float64; a component with ln = -inf has responsibility exactly 0."""
    lp = log_prob(X, ps, mp, ln)
    m = lp.max(1, keepdims=True)
    e = np.exp(lp - m)
    s = e.sum(1, keepdims=True)
    return e / s, (m + np.log(s))[:, 0]


def moments_ref(X, resp):
    r, x = resp.astype(np.float64), X.astype(np.float64)
    return r.sum(0), r.T @ x


def scatter_ref(X, resp, means):
    r, x, m = resp.astype(np.float64), X.astype(np.float64), means.astype(np.float64)
    return np.stack([(r[:, k, None] * (x - m[k]) ** 2).sum(0) for k in range(r.shape[1])])


def grad_ref(X, pi, mu, inv_var, beta, lr, iters, dtype=np.float64):
    """x -= lr * clip((beta / K) sum_k pi_ik inv_var_kj (x_ij - mu_kj), +-5), `iters` times, in
    the reference's order ((x - mu) first, components added in order); also the unclipped
    gradient of the first step.  dtype = float32: the same formula in fp32 arithmetic."""
    K = mu.shape[0]
    x = X.astype(dtype).copy()
    p, m, v = pi.astype(dtype), mu.astype(dtype), inv_var.astype(dtype)
    coef = dtype(np.float32(beta / K))
    lr = dtype(np.float32(lr))
    g0 = None
    for _ in range(iters):
        G = np.zeros_like(x)
        for k in range(K):
            G += p[:, k, None] * (v[k] * (x - m[k]))
        g = G * coef
        if g0 is None:
            g0 = g.copy()
        x = x - np.clip(g, -5, 5) * lr
    return x, g0


def loss_ref(X, pi, mu, var):
    """(rows, total, row tolerances, total tolerance): test_gpu_community_loss.py's bound, per
    row 2e-3 sum_k |pi| + 2e-5 sum_k |pi lp|, the total the sum of them."""
    lp = log_prob(X, *operands(None, mu, var))
    p = pi.astype(np.float64)
    rows = (p * lp).sum(1)
    tol = 2e-3 * np.abs(p).sum(1) + 2e-5 * np.abs(p * lp).sum(1)
    return rows, rows.sum(), tol, tol.sum()


def chunk_bounds(V, chunks):
    """The row ranges the M-step entries sum in fp32: ceil(V / chunks) rows each."""
    per = -(-V // chunks)
    return [(lo, min(V, lo + per)) for lo in range(0, V, per)]


def running_sum_f32(terms, chunks):
    """A plain fp32 running sum of terms [V, ...] (fp32) over each chunk's rows in row order, the
    chunks added in float64: the model the M-step's fp32 error is measured against."""
    total = np.zeros(terms.shape[1:], np.float64)
    for lo, hi in chunk_bounds(len(terms), chunks):
        acc = np.zeros(terms.shape[1:], np.float32)
        for i in range(lo, hi):
            acc += terms[i]
        total += acc
    return total


def err_stats(got, ref):
    e = np.asarray(got, np.float64) - ref
    return float(np.sqrt((e * e).mean())), float(np.abs(e).max())
