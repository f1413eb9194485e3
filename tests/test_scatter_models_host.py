"""CPU checks of tests/scatter_models.py: the 'hard' responsibilities are what they claim to be,
the error bar that tests/test_gpu_scatter_accuracy.py holds the scatter kernels to admits every
valid fp32 order of the sum that the kernels use, and it rejects a truncating accumulator."""
import functools

import numpy as np
import pytest

import scatter_models as sm

K, D = 3, 32
LENGTHS = [614, 6135]  # rows per chunk: the suite's largest whole-matrix case, the 1M-row bench
KINDS = ["dirichlet", "hard"]


@functools.lru_cache(maxsize=None)
def case(R, kind):
    X, resp, means = sm.inputs(R, 1, K, D, kind, seed=R)
    ref = sm.ref64(X, resp, means)
    model = sm.stats(sm.fp32_running_sum(X, resp, means), ref)
    return X, resp, means, ref, model


def test_chunking_matches_the_library_entry():
    """come_gmm_scatter: ceil(V / chunks) rounded up to 64 rows, and only the chunks that hold
    rows are launched."""
    assert sm.rows_per_chunk(100_000, 163) == 640 and sm.used_chunks(100_000, 163) == 157
    assert sm.rows_per_chunk(5, 4) == 64 and sm.used_chunks(5, 4) == 1
    for R in (614, 3175, 6098, 6135, 14926, 61350):
        assert sm.used_chunks(3 * R - 5, 3) == 3 and sm.used_chunks(R - 5, 1) == 1


def test_inputs_shapes_and_features():
    X, resp, means = sm.inputs(614, 3, K, 128, "dirichlet", 0)
    assert X.shape == (3 * 614 - 5, 128) and resp.shape == (len(X), K) and means.shape == (K, 128)
    assert X.dtype == resp.dtype == means.dtype == np.float32
    np.testing.assert_allclose(resp.sum(1), 1.0, atol=1e-6)
    assert sm.model_features(32).tolist() == list(range(32))
    for d, hi in ((64, 32), (100, 64), (128, 64), (200, 64)):
        f = sm.model_features(d)
        assert f.tolist() == list(range(16)) + list(range(hi, hi + 16)) and f.max() < d
        # a diagonal 32-wide (and 64-wide) output tile's entries and an off-diagonal one's
        assert f[0] // 32 == f[15] // 32 and f[0] // 32 != f[16] // 32
        if d > 64:
            assert f[0] // 64 != f[16] // 64


@pytest.mark.parametrize("R", LENGTHS + [61350])
def test_hard_family_is_what_it_says(R):
    _, resp, _ = sm.inputs(R, 1, K, D, "hard", seed=R)
    n = resp.size
    assert (resp == 0).sum() == int(round(sm.HARD_ZERO_SHARE * n))
    tiny = np.finfo(np.float32).tiny
    assert ((resp > 0) & (resp < tiny)).sum() == 8  # fp32 denormals
    assert (resp == 1.0).sum() >= 8
    assert (resp >= 0).all() and (resp <= 1).all()
    assert (resp.astype(np.float64).sum(0) > 50).all()  # every component keeps nk > 50
    # late-EM shape: most of the remaining mass sits on one component per row
    assert np.median(resp.max(1)) > 0.9


def test_rounding_helpers():
    v = np.array([1.0 + 2.0 ** -24 + 2.0 ** -40, -(1.0 + 2.0 ** -24 + 2.0 ** -40), 3.0, 1e-300])
    assert sm._round32(v, "nearest").tolist() == [1.0 + 2.0 ** -23, -(1.0 + 2.0 ** -23), 3.0, 0.0]
    assert sm._round32(v, "zero").tolist() == [1.0, -1.0, 3.0, 0.0]
    x = np.random.RandomState(0).standard_normal(1000).astype(np.float32)
    p1, p2, p3 = sm._bf16_parts(x)
    for p in (p1, p2, p3):
        assert (p.view(np.uint32) & 0xFFFF == 0).all()
    assert np.abs(p1.astype(np.float64) - x).max() <= 2.0 ** -8 * np.abs(x).max()
    rest = x.astype(np.float64) - p1 - p2 - p3
    assert (np.abs(rest) <= 2.0 ** -24 * np.abs(x)).all()
    assert sm._bf16(np.array([1.0 + 2.0 ** -8], np.float32))[0] == 1.0  # ties to even


def test_running_sum_is_float32_numpy():
    """One rounding per row in row order is what float32 numpy does with the same terms (the
    terms rounded to fp32 first there, so equal only to a few ulps of the sum)."""
    X, resp, means, ref, _ = case(614, "dirichlet")
    S = sm.fp32_running_sum(X, resp, means)
    D0 = X - means[0]
    acc = np.zeros((D, D), np.float32)
    for i in range(len(X)):
        acc += (resp[i, 0] * D0[i])[:, None] * D0[i][None]
    np.testing.assert_allclose(S[0], acc, rtol=0, atol=4e-6 * np.abs(acc).max())
    # and chunks are summed separately, then in order
    S3 = sm.fp32_running_sum(X, resp, means, chunks=3)
    assert sm.used_chunks(len(X), 3) == 3 and not np.array_equal(S3, S)
    np.testing.assert_allclose(S3, ref, rtol=0, atol=4e-6 * np.abs(ref).max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", LENGTHS)
def test_valid_orders_stay_within_the_bar(R, kind):
    X, resp, means, ref, model = case(R, kind)
    perm = np.random.RandomState(R + 1).permutation(len(X))
    orders = {
        "one rounding per 4 rows": sm.blocked_sum(X, resp, means, group=4),
        "one rounding per 16 rows": sm.blocked_sum(X, resp, means, group=16),
        "six bf16 part products per 16 rows": sm.blocked_sum(X, resp, means, group=16, parts=True),
        "rows permuted": sm.fp32_running_sum(X[perm], resp[perm], means),
    }
    print("running sum: rms %.3g max %.3g diagonal bias %.3g" % model)
    for name, S in orders.items():
        st = sm.stats(S, ref)
        print("%s: rms %.3g (%.2fx) max %.3g (%.2fx) diagonal bias %.3g"
              % (name, st[0], st[0] / model[0], st[1], st[1] / model[1], st[2]))
        assert sm.within_bar(st, model), (name, st, model)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R", LENGTHS)
def test_truncating_accumulator_breaks_the_bar(R, kind):
    """Round toward zero, one rounding per 16 rows: the RMS bound alone rejects it."""
    X, resp, means, ref, model = case(R, kind)
    st = sm.stats(sm.blocked_sum(X, resp, means, group=16, mode="zero"), ref)
    print("truncating: rms %.3g (%.2fx) max %.3g (%.2fx) diagonal bias %.3g"
          % (st[0], st[0] / model[0], st[1], st[1] / model[1], st[2]))
    assert not sm.within_bar(st, model)
    assert st[0] > sm.RMS_BAR * model[0]


@pytest.mark.parametrize("kind", KINDS)
def test_row_sums_model(kind):
    """The per-row fp32 running sums behind the bars on gmm.resp_sum and gmm.resp_t_x: close to
    float64, and not equal to it."""
    X, resp, _ = sm.inputs(3906, 2, 8, D, kind, seed=5)
    nk, sx = sm.row_sums_model(resp, X, 2)
    rnk, rsx = sm.row_sums_ref64(resp, X)
    for got, ref in ((nk, rnk), (sx, rsx)):
        rms, mx = sm.flat_stats(got, ref)
        assert 0 < rms < 1e-5 and 0 < mx < 1e-5
