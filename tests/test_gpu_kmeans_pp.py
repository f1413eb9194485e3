"""The native k-means++ seeding (come_kmeans_pp_step / _pick / _sample of libcome.so,
come_amd.kmeans.kmeans_plusplus_native and the estimators' seeding='native') on the GPU, against
float64 references.

Error bounds (u = 2^-24, the fp32 unit roundoff):
  * a distance is an fp32 sum of d squared differences: each difference carries one rounding (its
    square two), the fmaf chain and the lane butterfly at most d more: |dist - D64| <= (d + 3) u D64.
    A candidate's own row has all differences 0: exactly 0.
  * a potential is a float64 sum of V fp32 values in a fixed order: against another float64
    summation order of the same values, |difference| <= V 2^-52 times the sum.
  * a sampled row i answers r = u * pot when cum[i - 1] < r <= cum[i]; against numpy's cumsum of
    the same fp32 values both sides move by at most V 2^-52 pot.
"""
import math
import warnings

import numpy as np
import pytest
import torch

from come_amd import gmm, kmeans

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EPS = 2.0 ** -52


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def problem(V, K, d, seed, sep=3.0):
    """tests/test_gpu_kmeans.py's generator (same draws)."""
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
    return X.astype(np.float32), lab


def off1(a):
    v = torch.empty(a.numel() + 1, dtype=torch.float32, device=a.device)[1:].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


SHAPES = [(4099, 128), (1031, 64), (777, 100), (300, 200), (63, 1), (1, 128), (17, 64)]
TS = [1, 3, 5, 10, 16]
_cache = {}


def rows(V, d):
    """(X on the device, X in float64 on the device): built once per shape, never modified."""
    if (V, d) not in _cache:
        X, _ = problem(V, 3, d, V + d, sep=0.5)
        X = torch.as_tensor(X, device=dev())
        _cache[(V, d)] = (X, X.double())
    return _cache[(V, d)]


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def candidates(V, T, seed):
    """T rows of [0, V): a repeated index (T >= 3) and row V - 1 among them."""
    c = np.random.RandomState(seed).randint(0, V, T)
    c[-1] = V - 1
    if T >= 3:
        c[1] = c[0]
    return torch.as_tensor(c.astype(np.int32), device=dev())


def d64(X64, cand):
    """float64 squared distances [V, T] of every row to the rows `cand`, from differences."""
    return torch.stack([((X64 - X64[int(c)][None]) ** 2).sum(1) for c in cand.tolist()], 1)


def check_step(X, X64, closest, cand):
    V, d = X.shape
    T = cand.shape[0]
    chunks, per = kmeans.pp_plan(V, d, T, cus())
    dist, ppot, pots = kmeans.pp_step(X, closest, cand, chunks)
    assert dist.shape == (V, T) and ppot.shape == (chunks, T) and pots.shape == (T,)
    assert dist.dtype == torch.float32 and ppot.dtype == pots.dtype == torch.float64
    D = d64(X64, cand)
    if closest is not None:
        D = torch.minimum(D, closest.double()[:, None])
    err = (dist.double() - D).abs()
    print("V %d d %d T %d: max |dist - D64| / ((d + 3) u D64) = %.3g" % (
        V, d, T, float((err / ((d + 3) * U * D).clamp_min(1e-300)).max())))
    assert bool((err <= (d + 3) * U * D).all())
    own = dist[cand.long(), torch.arange(T, device=X.device)]
    assert bool((own == 0).all())  # a candidate's own row: exactly 0
    sums = dist.double().sum(0)
    assert bool(((pots - sums).abs() <= V * EPS * sums).all())
    assert bool(((ppot.sum(0) - pots).abs() <= V * EPS * pots).all())
    for c in range(chunks):  # each chunk's rows
        s = dist[c * per:(c + 1) * per].double().sum(0)
        assert bool(((ppot[c] - s).abs() <= per * EPS * s).all()), c
    again = kmeans.pp_step(X, closest, cand, chunks)
    for a, b in zip((dist, ppot, pots), again):
        assert torch.equal(a, b)
    return dist, ppot, pots


def some_closest(X, seed):
    """fp32 squared distances to one row: a `closest` that is lower than the candidates' distances
    for some rows and higher for others."""
    V, d = X.shape
    c = torch.as_tensor([seed % V], dtype=torch.int32, device=X.device)
    return kmeans.pp_step(X, None, c, kmeans.pp_plan(V, d, 1, cus())[0])[0][:, 0].contiguous()


# ---- 1. the pass over X ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("V,d", SHAPES)
def test_step_distances_and_potentials(V, d, T):
    X, X64 = rows(V, d)
    cand = candidates(V, T, V + T)
    check_step(X, X64, None, cand)
    check_step(X, X64, some_closest(X, 5 * T + 1), cand)


@pytest.mark.parametrize("T", [1, 5, 16])
def test_step_on_rows_that_are_not_16_byte_aligned(T):
    X, X64 = rows(1031, 64)
    Xo = off1(X)
    cand = candidates(1031, T, T)
    dist, _, pots = check_step(Xo, X64, None, cand)
    check_step(Xo, X64, some_closest(Xo, 3), cand)
    # the aligned rows take the vector loads: another summation order, the same bound
    dist2, _, pots2 = check_step(X, X64, None, cand)
    assert bool(((pots - pots2).abs() <= 2 * (64 + 3) * U * pots).all())


@pytest.mark.parametrize("V,d", [(4099, 128), (63, 1), (300, 200)])
def test_step_out_of_range_candidates_give_inf_columns(V, d):
    X, X64 = rows(V, d)
    cand = candidates(V, 5, 1)
    good = cand.clone()
    cand[1], cand[3] = -1, V
    chunks, _ = kmeans.pp_plan(V, d, 5, cus())
    for closest in (None, some_closest(X, 2)):
        dist, ppot, pots = kmeans.pp_step(X, closest, cand, chunks)
        ref = kmeans.pp_step(X, closest, good, chunks)
        for t in (1, 3):
            assert bool(torch.isinf(dist[:, t]).all()) and bool((dist[:, t] > 0).all())
            assert bool(torch.isinf(ppot[:, t]).all()) and math.isinf(float(pots[t]))
        for t in (0, 2, 4):
            assert torch.equal(dist[:, t], ref[0][:, t]) and torch.equal(ppot[:, t], ref[1][:, t])
            assert torch.equal(pots[t], ref[2][t])
        best = kmeans.pp_pick(dist, ppot, pots)[2]
        assert int(best[0]) in (0, 2, 4)


# ---- 2. the best candidate ------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 5, 10, 16])
@pytest.mark.parametrize("V,d", [(4099, 128), (1031, 64), (777, 100), (1, 128)])
def test_pick_is_the_argmin_with_ties_to_the_lowest_index(V, d, T):
    X, _ = rows(V, d)
    cand = candidates(V, T, 3 * T)
    if T == 2:
        cand[1] = cand[0]  # two identical candidates: identical columns, a tie
    chunks, _ = kmeans.pp_plan(V, d, T, cus())
    for closest in (None, some_closest(X, 7)):
        dist, ppot, pots = kmeans.pp_step(X, closest, cand, chunks)
        closest_out, cpot, best, pot = kmeans.pp_pick(dist, ppot, pots)
        assert best.dtype == torch.int32 and best.shape == (1,)
        want = int((pots == pots.min()).nonzero()[0])
        assert int(best[0]) == want
        if T == 2:
            assert torch.equal(pots[0], pots[1]) and want == 0
        assert torch.equal(closest_out, dist[:, want].contiguous())
        assert torch.equal(cpot, ppot[:, want].contiguous())
        assert torch.equal(pot[0], pots[want])
    # the minimum in the last place, and a tie between two later places
    p = torch.arange(T, 0, -1, dtype=torch.float64, device=X.device)
    assert int(kmeans.pp_pick(dist, ppot, p)[2][0]) == T - 1
    if T >= 3:
        p[T - 2] = p[T - 1]
        assert int(kmeans.pp_pick(dist, ppot, p)[2][0]) == T - 2


# ---- 3. the draw of the next candidates -------------------------------------------------------------
def masked_closest(X, seed):
    """(closest, cpot, rows_per_chunk): distances to one row with half the rows set to 0, and
    every third chunk as a whole (the first one too, where there is more than one), and the chunk
    sums a step gives for them."""
    V, d = X.shape
    chunks, per = kmeans.pp_plan(V, d, 1, cus())
    rng = np.random.RandomState(seed)
    keep = rng.rand(V) < 0.5
    if chunks > 1:
        keep &= (np.arange(V) // per) % 3 != 0
    c = torch.as_tensor([seed % V], dtype=torch.int32, device=X.device)
    full = kmeans.pp_step(X, None, c, chunks)[0][:, 0]
    closest = (full * torch.as_tensor(keep, device=X.device)).contiguous()
    dist, ppot, _ = kmeans.pp_step(X, closest, c, chunks)  # min(closest, full) = closest
    assert torch.equal(dist[:, 0], closest)
    return closest, ppot[:, 0].contiguous(), per


def draws(T, seed):
    u = np.random.RandomState(seed).rand(T)
    u[:5] = [0.0, np.nextafter(1.0, 0.0), 1.0 - 1e-9, 1e-300, 1e-12][:T]
    return u


@pytest.mark.parametrize("V,d", [s for s in SHAPES if s[0] > 1])
def test_sample_is_the_searchsorted_of_the_float64_cumsum(V, d):
    X, _ = rows(V, d)
    closest, cpot, per = masked_closest(X, V)
    h = closest.cpu().numpy()
    cum = np.cumsum(h.astype(np.float64))
    pot = cum[-1]
    assert pot > 0 and (h == 0).sum() >= V // 4
    tol = V * EPS * pot
    for T in (16, 1, 5):
        u = draws(T, T + V)
        got = kmeans.pp_sample(closest, cpot, per, torch.as_tensor(u, device=X.device))
        assert got.dtype == torch.int32 and got.shape == (T,)
        got = got.cpu().numpy()
        for t in range(T):
            i, r = int(got[t]), u[t] * pot
            assert 0 <= i < V
            lo = cum[i - 1] if i > 0 else 0.0
            assert lo - tol <= r <= cum[i] + tol, (t, i, u[t])
            if u[t] > 0:
                assert h[i] > 0, (t, i, u[t])  # a row without mass is never drawn
            else:
                assert i == 0
        again = kmeans.pp_sample(closest, cpot, per, torch.as_tensor(u, device=X.device))
        assert np.array_equal(again.cpu().numpy(), got)


@pytest.mark.parametrize("V,d", [(4099, 128), (1, 128), (63, 1)])
def test_sample_without_mass_returns_row_0(V, d):
    chunks, per = kmeans.pp_plan(V, d, 1, cus())
    closest = torch.zeros((V,), dtype=torch.float32, device=dev())
    cpot = torch.zeros((chunks,), dtype=torch.float64, device=dev())
    got = kmeans.pp_sample(closest, cpot, per, torch.as_tensor(draws(16, 0), device=dev()))
    assert int(got.abs().max()) == 0


# ---- 4. the whole seeding, replayed in float64 --------------------------------------------------------
def _trace(X, K, seed):
    V = X.shape[0]
    gen = torch.Generator(device=X.device)
    gen.manual_seed(seed)
    trials = 2 + int(math.log(K))
    first = torch.randint(0, V, (1,), generator=gen, device=X.device)
    u = torch.rand((K - 1, trials), generator=gen, device=X.device, dtype=torch.float64)
    return first, u, kmeans.kmeans_plusplus_native(X, K, gen, first=first, u=u, return_trace=True)


@pytest.mark.parametrize("V,K,d", [(4099, 50, 128), (1031, 7, 64)])
def test_seeding_replays_in_float64(V, K, d):
    X, _ = rows(V, d)
    first, u, trace = _trace(X, K, V)
    C, chosen, cands, pots, best = trace
    trials = 2 + int(math.log(K))
    assert C.shape == (K, d) and chosen.shape == (K,) and chosen.dtype == torch.int64
    assert cands.shape == pots.shape == (K - 1, trials) and best.shape == (K - 1,)
    assert torch.equal(C, X[chosen])
    X64 = X.cpu().numpy().astype(np.float64)
    chosen, cands, pots, best, u = (a.cpu().numpy() for a in (chosen, cands, pots, best, u))
    assert chosen[0] == int(first[0])
    assert len(set(chosen.tolist())) == K and chosen.min() >= 0 and chosen.max() < V
    bound = (d + 3) * U
    closest = ((X64 - X64[chosen[0]]) ** 2).sum(1)
    worst_pot, near_ties = 0.0, 0
    for k in range(K - 1):
        cum = np.cumsum(closest)
        pot = cum[-1]
        tol = (bound + V * EPS) * pot
        p64 = np.empty(trials)
        for t in range(trials):
            i = int(cands[k, t])
            assert 0 <= i < V
            r = u[k, t] * pot
            assert (cum[i - 1] if i > 0 else 0.0) - tol <= r <= cum[i] + tol, (k, t, i)
            p64[t] = np.minimum(closest, ((X64 - X64[i]) ** 2).sum(1)).sum()
        assert (np.abs(pots[k] - p64) <= bound * p64).all(), (k, pots[k], p64)
        worst_pot = max(worst_pot, float((np.abs(pots[k] - p64) / p64).max()))
        order = np.sort(p64)
        if order[1] - order[0] >= bound * order[1]:
            assert best[k] == int(np.argmin(p64)), (k, p64)
        else:  # (a candidate drawn twice, or two within the rounding of each other)
            near_ties += 1
            assert p64[best[k]] - order[0] <= bound * order[1]
        assert chosen[k + 1] == cands[k, best[k]]
        closest = np.minimum(closest, ((X64 - X64[chosen[k + 1]]) ** 2).sum(1))
    print("max |pot - pot64| / pot64 = %.3g (bound %.3g); steps whose two lowest potentials are "
          "within the bound: %d of %d" % (worst_pot, bound, near_ties, K - 1))
    _, _, again = _trace(X, K, V)
    for a, b in zip(trace, again):
        assert torch.equal(a, b)


# ---- 5. duplicated rows ---------------------------------------------------------------------------
def test_duplicated_rows_are_not_chosen_twice():
    base = np.random.RandomState(0).standard_normal((8, 64)).astype(np.float32)
    X = torch.as_tensor(np.tile(base, (4, 1)), device=dev())  # row i == row i % 8
    for seed in range(3):
        _, _, (C, chosen, _, pots, best) = _trace(X, 8, seed)
        assert sorted((chosen % 8).tolist()) == list(range(8))
        assert float(pots[-1, int(best[-1])]) == 0.0  # every row is a centre: exactly 0
        _, _, (C, chosen, cands, pots, best) = _trace(X, 12, seed)
        assert C.shape == (12, 64) and bool(torch.isfinite(C).all())
        assert sorted((chosen[:8] % 8).tolist()) == list(range(8))
        assert int(chosen.min()) >= 0 and int(chosen.max()) < 32
        assert bool((pots[7:] == 0).all())


# ---- 6. no host reads -----------------------------------------------------------------------------
def _sync_warnings(fn):
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, [w for w in rec if "synchroniz" in str(w.message)]


def test_seeding_reads_nothing_back():
    X, _ = rows(4099, 128)
    _, rec = _sync_warnings(lambda: X.sum().item())
    if not rec:
        pytest.skip("this torch build does not warn on a synchronizing .item()")
    gen = torch.Generator(device=X.device)
    gen.manual_seed(0)
    kmeans.kmeans_plusplus_native(X, 50, gen)  # warm-up
    C, rec = _sync_warnings(lambda: kmeans.kmeans_plusplus_native(X, 50, gen))
    assert C.shape == (50, 128) and len(rec) == 0, [str(w.message) for w in rec]


# ---- 7. the estimators ----------------------------------------------------------------------------
def _agreement(a, b, K):
    conf = np.zeros((K, K), np.int64)
    np.add.at(conf, (a, b), 1)
    return conf.max(1).sum() / len(a)


def test_estimator_recovers_blobs_from_the_native_seeding():
    X, lab = problem(20000, 5, 64, 3, sep=4.0)
    km = kmeans.KMeans(5, n_init=2, random_state=0, seeding='native').fit(X)
    assert km.cluster_centers_.shape == (5, 64) and km.labels_.shape == (20000,)
    assert _agreement(km.labels_, lab, 5) > 0.999
    assert np.array_equal(kmeans.KMeans(5, n_init=2, random_state=0,
                                        seeding='native').fit_predict(X), km.labels_)


def test_gaussian_mixture_native_seeding_reaches_sklearn_optimum():
    from sklearn.mixture import GaussianMixture as SkGMM
    X, lab = problem(20000, 5, 64, 3, sep=4.0)
    g = gmm.GaussianMixture(5, reg_covar=1e-5, n_init=2, random_state=0, kmeans_backend='native',
                            kmeans_seeding='native').fit(X)
    sk = SkGMM(5, covariance_type="full", reg_covar=1e-5, n_init=2, random_state=0).fit(X)
    assert g.converged_
    np.testing.assert_allclose(g.lower_bound_, sk.lower_bound_, rtol=1e-3)
    assert _agreement(g.predict(X).cpu().numpy(), sk.predict(X), 5) > 0.999
