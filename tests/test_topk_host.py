"""Top-k neighbour search without a GPU: the symbols are bound, every validation error of
come_topk / come_topk_scratch / come_row_sqnorms returns its status before any device call, the
chunk plan keeps its bounds (and the scratch has no term in Q * V), and the CPU twin come_cpu_topk
meets the contract of tests/topk_common.py and the exact-data tests with 1 and 4 threads."""
import ctypes

import numpy as np
import pytest

import topk_common as tc
from come_amd import _lib, cpu, neighbors

P16 = ctypes.c_void_p(16)  # a non-null pointer that is never dereferenced
NULL = ctypes.c_void_p(0)


def test_symbols_are_bound():
    L = _lib.lib()
    for name in ("come_topk_scratch", "come_row_sqnorms", "come_topk", "come_cpu_topk"):
        assert name in _lib.SYMBOLS and getattr(L, name).argtypes is not None, name
    assert _lib.TOPK_METRICS == {"dot": 0, "cosine": 1, "l2": 2}


def _topk(Q=4, V=100, d=64, k=10, metric=1, chunks=1, q=P16, base=P16, scratch=P16, idx=P16,
          score=P16):
    return _lib.lib().come_topk(q, Q, base, V, d, k, metric, None, None, chunks, scratch, idx,
                                score, None)


@pytest.mark.parametrize("kw, msg", [
    (dict(k=0), b"k must be"), (dict(k=65), b"k must be"), (dict(d=0), b"d must be"),
    (dict(d=513), b"d must be"), (dict(Q=0), b"Q must be"), (dict(V=0), b"V must be"),
    (dict(V=2 ** 31), b"V must be"), (dict(metric=3), b"metric"), (dict(metric=-1), b"metric"),
    (dict(chunks=0), b"chunks must be"), (dict(chunks=65), b"chunks must be"),
    (dict(q=NULL), b"null pointer"), (dict(base=NULL), b"null pointer"),
    (dict(scratch=NULL), b"null pointer"), (dict(idx=NULL), b"null pointer"),
    (dict(score=NULL), b"null pointer")])
def test_topk_validation_returns_status_without_a_device(kw, msg):
    L = _lib.lib()
    assert _topk(**kw) == -1 and msg in L.come_last_error(), L.come_last_error()


def test_scratch_and_sqnorms_validation():
    L = _lib.lib()
    c, r = ctypes.c_int(0), ctypes.c_int64(0)
    for Q, V, d, k, msg in ((0, 10, 64, 1, b"Q must be"), (1, 0, 64, 1, b"V must be"),
                            (1, 10, 0, 1, b"d must be"), (1, 10, 513, 1, b"d must be"),
                            (1, 10, 64, 0, b"k must be"), (1, 10, 64, 65, b"k must be")):
        assert L.come_topk_scratch(Q, V, d, k, 256, ctypes.byref(c), ctypes.byref(r)) == -1
        assert msg in L.come_last_error()
    assert L.come_topk_scratch(1, 10, 64, 1, 256, None, ctypes.byref(r)) == -1
    assert L.come_topk_scratch(1, 10, 64, 1, 256, ctypes.byref(c), None) == -1
    assert L.come_row_sqnorms(P16, 0, 64, P16, None) == -1 and b"V must be" in L.come_last_error()
    assert L.come_row_sqnorms(P16, 10, 0, P16, None) == -1 and b"d must be" in L.come_last_error()
    assert L.come_row_sqnorms(NULL, 10, 64, P16, None) == -1
    assert L.come_row_sqnorms(P16, 10, 64, NULL, None) == -1
    # the twin: the same argument rules, and its thread count
    a = np.zeros((4, 8), np.float32)
    i, s = np.zeros((4, 2), np.int32), np.zeros((4, 2), np.float32)
    for kw, msg in ((dict(k=0), b"k must be"), (dict(k=65), b"k must be"), (dict(d=0), b"d must be"),
                    (dict(Q=0), b"Q >= 1"), (dict(V=0), b"V in"), (dict(metric=5), b"metric"),
                    (dict(threads=0), b"threads")):
        arg = dict(Q=4, V=4, d=8, k=2, metric=0, threads=1)
        arg.update(kw)
        rc = L.come_cpu_topk(_lib.ptr(a), arg["Q"], _lib.ptr(a), arg["V"], arg["d"], arg["k"],
                             arg["metric"], None, None, _lib.ptr(i), _lib.ptr(s), arg["threads"])
        assert rc == -1 and msg in L.come_last_error(), (kw, L.come_last_error())
    assert L.come_cpu_topk(None, 4, _lib.ptr(a), 4, 8, 2, 0, None, None, _lib.ptr(i), _lib.ptr(s),
                           1) == -1


@pytest.mark.parametrize("Q", [1, 33, 129, 2048, 16384, 1000000])
@pytest.mark.parametrize("V", [1, 5, 1000, 4099, 20000, 1000000, 2 ** 31 - 1])
@pytest.mark.parametrize("d, k", [(64, 1), (128, 10), (100, 64), (512, 64)])
def test_plan_bounds(Q, V, d, k):
    for cus in (0, 1, 256, 304):
        chunks, rows = neighbors.plan(Q, V, d, k, cus)
        assert 1 <= chunks <= 64
        assert rows >= 32 and rows % 32 == 0
        assert chunks * rows >= V > (chunks - 1) * rows  # covers V, no empty chunk
        # the scratch: the chunks' lists (+ the base norms): nothing in Q * V
        assert neighbors.scratch_bytes(Q, V, k, chunks, True) == chunks * Q * k * 8
        assert neighbors.scratch_bytes(Q, V, k, chunks, False) == chunks * Q * k * 8 + 4 * V


def test_plan_fills_the_chip_about_twice_over():
    # MFMA shapes: 128-query tiles x chunks ~ 2 x cus workgroups while the chunk bound allows
    for Q, want in ((16384, 4), (2048, 32), (1, 64)):
        chunks, _ = neighbors.plan(Q, 1000000, 128, 10, 256)
        assert chunks == want, (Q, chunks)


# the twin has one path whatever the alignment; the V = 20,000 shapes run with 4 threads only
TWIN_CASES = [(c, t) for c in tc.real_cases() if not c[2] for t in (1, 4)
              if not (c[4] == 20000 and t == 1)]


@pytest.mark.parametrize("case, threads", TWIN_CASES,
                         ids=["%s-t%d" % (tc.case_id(c), t) for c, t in TWIN_CASES])
def test_cpu_twin_meets_the_contract(case, threads):
    metric, d, off, Q, V, k, chunks, ex = case
    q, b, exclude = tc.real_data(case)
    idx, score = cpu.topk(q, b, k, metric=metric, exclude=exclude, threads=threads)
    tc.check_contract(q, b, k, metric, idx, score, exclude, who="cpu_topk")
    if metric != "dot":  # the caller's own norms
        bsq = (b.astype(np.float64) ** 2).sum(1).astype(np.float32)
        idx, score = cpu.topk(q, b, k, metric=metric, exclude=exclude, base_sq=bsq,
                              threads=threads)
        tc.check_contract(q, b, k, metric, idx, score, exclude, who="cpu_topk base_sq")


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("metric, d", [("dot", 64), ("dot", 128), ("l2", 64), ("l2", 128),
                                       ("cosine", 64)])
def test_cpu_twin_exact_data_bit_for_bit(metric, d, k, threads):
    q, b = tc.exact_data(metric, d, 129, 1000)
    exclude = np.arange(129, dtype=np.int32) * 7 % 1000
    exclude[::3] = -1
    for ex in (None, exclude):
        got = cpu.topk(q, b, k, metric=metric, exclude=ex, threads=threads)
        tc.assert_same_bits(got, tc.exact_reference(q, b, k, metric, ex), "cpu_topk")


def test_cpu_twin_edge_cases():
    """Cosine: a zero base row scores 0 and ranks among the zeros by index, a zero query returns
    the lowest indices; a NaN row is never returned; V < k pads the tail."""
    q, b, want_zero = tc.cosine_zero_data()
    idx, score = cpu.topk(q, b, len(want_zero), metric="cosine", threads=1)
    assert idx[0].tolist() == want_zero and (score[0] == 0).all()
    assert idx[1].tolist() == list(range(len(want_zero))) and (score[1] == 0).all()
    tc.assert_same_bits((idx, score), tc.exact_reference(q, b, len(want_zero), "cosine"), "zero")
    rng = np.random.RandomState(5)
    b = rng.randn(300, 100).astype(np.float32)
    q = rng.randn(70, 100).astype(np.float32)
    b[17, 3] = np.nan
    for metric in tc.METRICS:
        idx, score = cpu.topk(q, b, 64, metric=metric, threads=4)
        assert not (idx == 17).any() and not np.isnan(score).any()
        tc.check_contract(q, b, 64, metric, idx, score, who="cpu_topk nan")
        idx, score = cpu.topk(q, b[:5], 8, metric=metric, threads=1)
        assert (idx[:, 5:] == -1).all() and (idx[:, :5] >= 0).all()
        assert (score[:, 5:] == (np.inf if metric == "l2" else -np.inf)).all()
