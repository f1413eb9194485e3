"""The fp32 error of the GMM M-step's sums over rows at the chunk lengths production runs.

come_gmm_scatter's workgroups each add all the rows of one chunk into one set of fp32 (MFMA or
VALU) accumulators, and gmm.scatter_chunks caps the chunk count, so the rows per chunk grow with V:
614 in the suite's largest whole-matrix test (100k rows), 6 135 at the benchmarked 1M x 128 and
61 350 at 10M.  The error depends on the rows per chunk, not on V, so K = 3 and one or three
chunks of those lengths reproduce the accumulation in a few thousand rows: every scatter kernel,
Dirichlet responsibilities and the hard ones of late EM iterations (exact zeros and ones,
denormals), against float64, with the error held to a multiple of what a plain fp32 running sum
of the same operands in the same chunks commits (tests/scatter_models.py: RMS <= 2x, max <= 3x,
margins that admit every valid summation order and reject a truncating accumulator;
tests/test_scatter_models_host.py).  K = 3 leaves k_gmm_cov_fb3 / k_gmm_cov16<128> a workgroup with
one live component and the four-component workgroups of d = 64 a partly filled one.

Also: the whole matrix at the tolerance of the other scatter tests (a layout or tiling error
fails that one), symmetry, bit-identical repeats, and the same budget for the M-step's other two
fp32 sums over rows, gmm.resp_sum and gmm.resp_t_x (torch sum / bmm over V / 256 rows per block)."""
import functools

import numpy as np
import pytest
import torch

import scatter_models as sm
from come_amd import gmm
from come_amd._lib import options

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K = 3

# name: (d, gmm_cov_async or None where the width decides, X at element offset 1)
KERNELS = {
    "cov16_d128": (128, 3, False),      # k_gmm_cov16<128>, fp32 16x16x4 MFMA
    "fb3_d128": (128, 4, False),        # k_gmm_cov_fb3<128>, bf16 parts, the default
    "bf3_d128": (128, 5, False),        # k_gmm_cov_bf3<128>
    "cov16_d64": (64, 3, False),        # k_gmm_cov16<64>
    "bf3_d64": (64, 4, False),          # k_gmm_cov_bf3<64>, the d = 64 default
    "valu_d100": (100, None, False),    # k_gmm_cov_valu
    "valu_d128_off1": (128, None, True),  # k_gmm_cov_valu: X not 16-byte aligned
    "wide_d200": (200, None, False),    # k_gmm_cov_wide
}


def t(a):
    return torch.from_numpy(np.array(a, np.float32)).to(DEV)  # (a copy: the cases are read-only)


def off1(a):
    v = torch.empty(a.numel() + 1, dtype=torch.float32, device=a.device)[1:].view(a.shape)
    v.copy_(a)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def rows_per_chunk(length, d):
    """Rows per chunk of production's own chunking at 1M (the bench) / 10M rows, K = 50; '100k'
    is the suite's largest whole-matrix scatter (614 at every width, for one scale)."""
    if length == "100k":
        return 614
    V = {"1M": 1_000_000, "10M": 10_000_000}[length]
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    return -(-V // gmm.scatter_chunks(V, 50, d, cus))


@functools.lru_cache(maxsize=None)
def case(R, chunks, d, kind):
    """Inputs, the float64 reference (whole matrices) and the running-sum model's error on the
    modelled features: built once per shape and kind, shared by the kernels, never modified."""
    X, resp, means = sm.inputs(R, chunks, K, d, kind, seed=7 * R + 3 * chunks + d)
    assert sm.used_chunks(len(X), chunks) == chunks
    ref = sm.ref64(X, resp, means)
    feats = sm.model_features(d)
    sub = np.ix_(range(K), feats, feats)
    model = sm.stats(sm.fp32_running_sum(X, resp, means, chunks, feats), ref[sub])
    for a in (X, resp, means, ref):
        a.setflags(write=False)
    return X, resp, means, ref, sub, model


def run_case(kernel, length, chunks, kind):
    d, cov, shifted = KERNELS[kernel]
    R = rows_per_chunk(length, d)
    X, resp, means, ref, sub, model = case(R, chunks, d, kind)
    xd, rd, md = t(X), t(resp), t(means)
    if shifted:
        xd = off1(xd)
    with options(**({} if cov is None else {"gmm_cov_async": cov})):
        S1 = gmm.scatter(xd, rd, md, chunks=chunks)
        S2 = gmm.scatter(xd, rd, md, chunks=chunks)
    assert torch.equal(S1, S2), "two runs of the same call differ"
    S = S1.cpu().numpy()
    st = sm.stats(S[sub], ref[sub])
    print("\nscatter %s %s rows/chunk %d chunks %d %s: rms %.3g max %.3g diag-bias %.3g | "
          "running sum: rms %.3g max %.3g | ratio %.2f %.2f"
          % (kernel, length, R, chunks, kind, st[0], st[1], st[2], model[0], model[1],
             st[0] / model[0], st[1] / model[1]))
    for k in range(K):
        np.testing.assert_allclose(S[k], ref[k], rtol=1e-4, atol=1e-4 * np.abs(ref[k]).max(),
                                   err_msg="component %d" % k)
    np.testing.assert_allclose(S, np.swapaxes(S, 1, 2), rtol=0, atol=1e-6 * np.abs(S).max())
    assert st[0] <= sm.RMS_BAR * model[0], ("rms", st, model)
    assert st[1] <= sm.MAX_BAR * model[1], ("max", st, model)


@pytest.mark.parametrize("kind", ["dirichlet", "hard"])
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("length", ["100k", "1M"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_scatter_error_within_running_sum_budget(kernel, length, chunks, kind):
    run_case(kernel, length, chunks, kind)


@pytest.mark.parametrize("kind", ["dirichlet", "hard"])
@pytest.mark.parametrize("kernel", ["cov16_d128", "fb3_d128", "bf3_d128", "valu_d128_off1"])
def test_scatter_error_at_10m_rows_chunk_length(kernel, kind):
    """61 350 rows in one chunk: scatter_chunks(10M, 50, 128)."""
    run_case(kernel, "10M", 1, kind)


@functools.lru_cache(maxsize=None)
def row_sums_case(R, kind):
    X, resp, _ = sm.inputs(R, 2, 8, 128, kind, seed=R)
    ref = sm.row_sums_ref64(resp, X)
    model = sm.row_sums_model(resp, X, 2)
    return X, resp, ref, [sm.flat_stats(m, r) for m, r in zip(model, ref)]


@pytest.mark.parametrize("kind", ["dirichlet", "hard"])
@pytest.mark.parametrize("V", [1_000_000, 10_000_000])
def test_row_sums_error_within_running_sum_budget(V, kind):
    """gmm.resp_sum and gmm.resp_t_x sum V / 256 rows per block in fp32 (torch sum and bmm) and
    the blocks in float64: two blocks of that length, against float64, within the budget of a
    per-row fp32 running sum per block."""
    R = V // 256
    X, resp, ref, model = row_sums_case(R, kind)
    got = (gmm.resp_sum(t(resp), chunks=2).cpu().numpy(),
           gmm.resp_t_x(t(resp), t(X), chunks=2).cpu().numpy())
    for name, g, r, m in zip(("resp_sum", "resp_t_x"), got, ref, model):
        assert g.dtype == np.float64 and g.shape == r.shape
        st = sm.flat_stats(g, r)
        print("\n%s rows/block %d %s: rms %.3g max %.3g | running sum: rms %.3g max %.3g"
              % (name, R, kind, st[0], st[1], m[0], m[1]))
        assert st[0] <= sm.RMS_BAR * m[0] and st[1] <= sm.MAX_BAR * m[1], (name, st, m)
