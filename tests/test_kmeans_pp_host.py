"""The k-means++ seeding entry points of libcome.so without a GPU: the symbols are bound, bad
arguments return COME_E_INVALID with a message before any device work, the planner
(come_kmeans_pp_scratch, host only) tiles the rows within its 2 MB of partials, and the estimators
refuse an unknown seeding."""
import ctypes

import pytest

from come_amd import _lib, gmm, kmeans

P0 = ctypes.c_void_p(0)
P1 = ctypes.c_void_p(64)  # non-null, never dereferenced: the calls stop at the bad argument


def _scratch(L, V=100, d=128, T=5, chunks=1, p=P1):
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    both = (ctypes.byref(c), ctypes.byref(r)) if p is P1 else (P0, P0)
    return L.come_kmeans_pp_scratch(V, d, T, 256, *both)


def _step(L, V=100, d=128, T=5, chunks=1, p=P1):
    return L.come_kmeans_pp_step(p, V, d, p, p, T, chunks, p, p, p, P0)


def _pick(L, V=100, d=128, T=5, chunks=1, p=P1):
    return L.come_kmeans_pp_pick(p, V, T, p, p, chunks, p, p, p, p, P0)


def _sample(L, V=100, d=128, T=5, chunks=1, p=P1, rows=128):
    return L.come_kmeans_pp_sample(p, V, p, chunks, rows, p, T, p, P0)


NAMES = ("come_kmeans_pp_scratch", "come_kmeans_pp_step", "come_kmeans_pp_pick",
         "come_kmeans_pp_sample")


def test_symbols_are_bound():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None


@pytest.mark.parametrize("call", [_scratch, _step, _pick, _sample])
def test_invalid_arguments_are_refused_before_device_work(call):
    L = _lib.lib()
    for V in (0, -1):
        assert call(L, V=V) == -1 and b"V must be" in L.come_last_error()
    for T in (0, 17, -2):
        assert call(L, T=T) == -1 and b"T must be" in L.come_last_error()
    if call in (_scratch, _step):  # (pick and sample never see the rows of X)
        for d in (0, 513):
            assert call(L, d=d) == -1 and b"d must be" in L.come_last_error()
    if call is not _scratch:
        for chunks in (0, -3):
            assert call(L, chunks=chunks) == -1 and b"chunks must be" in L.come_last_error()
    assert call(L, p=P0) == -1 and b"null pointer" in L.come_last_error()
    # the limits themselves are shapes: the calls then stop at the null pointers
    for d, T in ((1, 1), (512, 16)):
        assert call(L, d=d, T=T, p=P0) == -1 and b"null pointer" in L.come_last_error()
        if call is _scratch:
            assert call(L, d=d, T=T) == 0


def test_chunk_counts_beyond_the_partials_or_short_of_the_rows():
    L = _lib.lib()
    # chunks * T * 8 bytes > 2 MB
    assert _step(L, T=16, chunks=16385) == -1 and b"chunks must be" in L.come_last_error()
    assert _pick(L, T=16, chunks=16385) == -1 and b"chunks must be" in L.come_last_error()
    assert _step(L, T=16, chunks=16384, p=P0) == -1 and b"null pointer" in L.come_last_error()
    # chunks * rows_per_chunk < V
    assert _sample(L, V=1000, chunks=7, rows=128) == -1
    assert b"chunks must be" in L.come_last_error()
    assert _sample(L, V=1000, chunks=8, rows=0) == -1 and b"chunks must be" in L.come_last_error()
    assert _sample(L, V=1000, chunks=8, rows=128, p=P0) == -1
    assert b"null pointer" in L.come_last_error()


@pytest.mark.parametrize("V,d,T", [(1, 1, 1), (1_000_000, 128, 5), (10_000_000, 128, 10),
                                   (300, 512, 16)])
def test_plan_tiles_the_rows(V, d, T):
    for cus in (0, 1, 256, 304):
        chunks, rows = kmeans.pp_plan(V, d, T, cus)
        assert chunks >= 1 and rows >= 1
        assert chunks * rows >= V > (chunks - 1) * rows
        assert chunks * T * 8 <= 2 << 20
        # come_kmeans_pp_step derives its rows per chunk from the chunk count alone
        assert rows == -(-(-(-V // chunks)) // 32) * 32
    with pytest.raises(_lib.ComeError, match="T must be"):
        kmeans.pp_plan(V, d, 17)


def test_estimators_refuse_an_unknown_seeding():
    with pytest.raises(ValueError, match="seeding"):
        kmeans.KMeans(5, seeding='bogus')
    assert kmeans.KMeans(5).seeding == 'torch'
    assert kmeans.KMeans(5, seeding='native').seeding == 'native'
    with pytest.raises(ValueError, match="kmeans_seeding"):
        gmm.GaussianMixture(5, kmeans_backend='native', kmeans_seeding='bogus')
    with pytest.raises(ValueError, match="kmeans_seeding"):
        gmm.GaussianMixture(5, kmeans_backend='torch', kmeans_seeding='native')
    g = gmm.GaussianMixture(5, kmeans_backend='native', kmeans_seeding='native')
    assert g.kmeans_seeding == 'native'
    assert gmm.GaussianMixture(5).kmeans_seeding == 'torch'
