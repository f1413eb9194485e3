"""Shared by tests/test_edge_sample_host.py and tests/test_gpu_edge_sample.py: the weighted G12's
edge list, the numpy restatement of come_edge_cdf's formula, the exact masses of the sampler's pick
in Python integers, the weight sets of the CDF tests and the frequency check."""
import numpy as np

from walks_pq_common import G12_EDGES
from walks_w_common import g12_weight

TWO32, TWO64 = 2 ** 32, 2 ** 64
# the device scan's tile (csrc/come_edge_sample.hip: EDGE_TILE) and one round of its middle phase
# (256 tiles): sizes one below, at and one above each are where its carries change hands
TILE, ROUND = 2048, 256 * 2048
CDF_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, TILE - 1, TILE, TILE + 1, 4097,
             70_001, 300_007, ROUND - 1, ROUND, ROUND + 1)


def g12_edges():
    """(edges int32 [16, 2], weights float32 [16]) of walks_w_common's weighted G12 in G12_EDGES
    order: one weight 1000, one weight 0 at the head, fourteen small integers."""
    e = np.array(G12_EDGES, np.int32)
    return e, np.array([g12_weight(a, b) for a, b in G12_EDGES], np.float32)


def lognormal_weights(E, seed=11):
    return np.random.RandomState(seed).lognormal(0.0, 1.0, E).astype(np.float32)


def spread_weights(E, seed=12):
    """log-normal(0, 1) times 10^U(-6, 6): the prefix sums pass 2^32 within a few entries."""
    rng = np.random.RandomState(seed)
    return (rng.lognormal(0.0, 1.0, E) * 10.0 ** rng.uniform(-6, 6, E)).astype(np.float32)


def units(w):
    """u_i = rint(w_i / wmax * 2^32) as uint64 (include/come.h, come_edge_cdf)."""
    w = np.asarray(w, np.float32).astype(np.float64)
    return np.rint(w / w.max() * float(TWO32)).astype(np.uint64)


def edge_cdf_formula(w):
    return np.cumsum(units(w), dtype=np.uint64)


def first_r64(ecdf):
    """Per edge, ceil(U_{i-1} 2^64 / U_E) in Python integers -- the smallest r64 whose
    x = floor(r64 U_E / 2^64) reaches U_{i-1} -- followed by 2^64: a list of E + 1 ints.  Edge i
    owns [r[i], r[i + 1])."""
    U = [0] + [int(x) for x in ecdf]
    UE = U[-1]
    return [-((-u * TWO64) // UE) for u in U]


def check_frequencies(index, w, min_expected=100.0, sigmas=5.0):
    """walks_w_common.check_distribution_w's rule on sampled edge indices: every edge with
    S p >= min_expected has |n - S p| <= sigmas sqrt(S p (1 - p)), p = w / W in float64; a
    zero-weight edge is never drawn.  Returns how many edges were checked."""
    w = np.asarray(w, np.float64)
    S = len(index)
    n = np.bincount(index, minlength=len(w))
    assert len(n) == len(w)
    p = w / w.sum()
    assert (n[w == 0] == 0).all()
    checked = 0
    for i in range(len(w)):
        if S * p[i] >= min_expected:
            assert abs(n[i] - S * p[i]) <= sigmas * np.sqrt(S * p[i] * (1 - p[i])), (i, n[i],
                                                                                   S * p[i])
            checked += 1
    return checked
