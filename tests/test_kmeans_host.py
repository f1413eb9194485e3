"""The k-means entry points of libcome.so without a GPU: argument validation returns
COME_E_INVALID with a message before any device work, and come_kmeans_scratch (host only) keeps
the chunk partials within 128 MB."""
import ctypes

import pytest

from come_amd import _lib, kmeans

P0 = ctypes.c_void_p(0)


def _lloyd(L, V, d, K, chunks=1):
    return L.come_kmeans_lloyd(P0, V, d, P0, K, chunks, P0, P0, P0, P0, P0, P0, P0)


def _assign(L, V, d, K):
    return L.come_kmeans_assign(P0, V, d, P0, K, P0, P0, P0)


def _scratch(L, V, d, K):
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    return L.come_kmeans_scratch(V, d, K, 256, ctypes.byref(c), ctypes.byref(r))


def test_symbols_are_bound():
    L = _lib.lib()
    for name in ("come_kmeans_scratch", "come_kmeans_lloyd", "come_kmeans_assign",
                 "come_kmeans_update"):
        assert name in _lib.SYMBOLS and hasattr(L, name)


@pytest.mark.parametrize("call", [_lloyd, _assign, _scratch])
def test_invalid_shapes_are_refused_before_device_work(call):
    L = _lib.lib()
    assert call(L, -1, 128, 50) == -1 and b"V must be" in L.come_last_error()
    for d in (0, -3, 513):
        assert call(L, 100, d, 50) == -1 and b"d must be" in L.come_last_error()
    for d, K in ((128, 0), (128, 4097), (100, 65), (1, 65), (512, 4097), (64, -1)):
        assert call(L, 100, d, K) == -1 and b"K must be" in L.come_last_error(), (d, K)
    # the limits GaussianMixture.fit_predict enforces are accepted as shapes: the calls then stop
    # at the null pointers (still no device work)
    for d, K in ((128, 4096), (100, 64), (512, 4096), (1, 1)):
        if call is _scratch:
            assert call(L, 100, d, K) == 0
        elif call is _lloyd:
            assert call(L, 100, d, K) == -1 and b"null pointer" in L.come_last_error()


def test_empty_batch():
    """V = 0: come_kmeans_assign has nothing to write and returns 0 without touching the device;
    come_kmeans_lloyd (its sums, counts and inertia would still have to be written) and
    come_kmeans_scratch ask for V >= 1, as include/come.h says."""
    L = _lib.lib()
    assert _assign(L, 0, 128, 50) == 0
    assert _lloyd(L, 0, 128, 50) == -1 and b"V must be" in L.come_last_error()
    assert _scratch(L, 0, 128, 50) == -1 and b"V must be" in L.come_last_error()


def test_lloyd_refuses_bad_chunk_counts():
    L = _lib.lib()
    for chunks in (0, -2):
        assert _lloyd(L, 100, 128, 50, chunks) == -1 and b"chunks must be" in L.come_last_error()
    # more partials than 128 MB
    assert _lloyd(L, 100, 128, 4096, 65) == -1 and b"chunks must be" in L.come_last_error()


def test_update_validates():
    L = _lib.lib()
    assert L.come_kmeans_update(P0, P0, P0, 50, 0, P0, P0) == -1
    assert b"d must be" in L.come_last_error()
    assert L.come_kmeans_update(P0, P0, P0, 0, 128, P0, P0) == -1
    assert b"K must be" in L.come_last_error()
    assert L.come_kmeans_update(P0, P0, P0, 50, 128, P0, P0) == -1
    assert b"null pointer" in L.come_last_error()


@pytest.mark.parametrize("V,K,d", [(1_000_000, 50, 128), (1, 1, 1), (10_000_000, 4096, 128),
                                   (300, 70, 512)])
def test_scratch_is_bounded(V, K, d):
    for cus in (256, 0, 1, 304):
        chunks, rows = kmeans.scratch_plan(V, d, K, cus)
        assert chunks >= 1
        assert chunks * K * d * 4 <= 128 << 20
        assert rows >= 1 and rows % 16 == 0
        assert chunks * rows >= V > (chunks - 1) * rows  # the chunks tile the rows
