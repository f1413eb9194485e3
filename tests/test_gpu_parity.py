"""GPU parity through the C-ABI (libcome.so on cuda:0).

Bars (written per test):
  * COME_MODE_SEQUENTIAL vs the oracle in its WAVE64 dot order: BIT-EXACT (same arithmetic in the
    same order).
  * vs the reference's golden vectors (tests/golden, produced by the Cython module itself):
    tier A <= 1e-6 abs for clean cases, tier B <= 1e-3 abs where a dot product lies within 1e-4
    bucket units of a sigmoid-table edge (OpenBLAS summation order can flip a bucket).
  * COME_MODE_HOGWILD (many walks in flight, races like the reference's threads): statistical --
    rows never touched stay bit-identical, per-row updates point where the sequential run's do
    (cosine > 0.985 node / 0.965 ctx) at low contention, bit-identical when walks share no row;
    held-out loss within 1% of the sequential oracle (tests/test_gpu_tierc.py).
  * community gradient / GMM responsibilities (fp32 contractions in a different summation
    order): rtol 1e-5 / atol 1e-5 vs the reference's numpy/sklearn outputs.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import oracle as orc

import come_amd.training_sdg_inner as tsi
from come_amd import community_embeddings as ce
from come_amd._lib import options

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
KAT_O2 = load_golden("kat_o2")
KAT_O1 = np.load(os.path.join(GOLDEN, "kat_o1.npz"))


def dev(a, dtype=None):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def run_o2(node0, ctx0, walks, seeds, w, neg, table, lr, alpha, mode=tsi.MODE_SEQUENTIAL,
           hot_share=None, opts=None):
    node, ctx = dev(node0.copy()), dev(ctx0.copy())
    tab = dev(table)
    hot = None if hot_share is None else tsi.hot_rows(tab, node0.shape[0],
                                                       max(1, int(hot_share * len(table))))
    tsi.sgns_o2(node, ctx, dev(walks.astype(np.int32)), dev(seeds.astype(np.uint64)), w, neg,
                tab, lr, alpha, mode, hot=hot, opts=opts)
    torch.cuda.synchronize()
    return node.cpu().numpy(), ctx.cpu().numpy()


def run_o1(node0, edges, seeds, neg, table, lr, mode=tsi.MODE_SEQUENTIAL):
    node = dev(node0.copy())
    tsi.sgns_o1(node, dev(edges.astype(np.int32)), dev(seeds.astype(np.uint64)), neg, dev(table),
                lr, mode)
    torch.cuda.synchronize()
    return node.cpu().numpy()


def tol_for(margin):
    return 1e-6 if margin >= 1e-4 else 1e-3


# ---- O2 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(KAT_O2["names"]))
def test_o2_kat_bit_exact_vs_oracle_and_golden(name):
    z, pre = KAT_O2, "o2_%s_" % name
    d, neg, w, V, L, P = [int(x) for x in z[pre + "params"]]
    lr, alpha = [float(x) for x in z[pre + "lr_alpha"]]
    node, ctx = run_o2(z[pre + "node0"], z[pre + "ctx0"], z[pre + "walks"], z[pre + "seeds"], w,
                       neg, z[pre + "table"], lr, alpha)
    n_ref, c_ref = z[pre + "node0"].copy(), z[pre + "ctx0"].copy()
    orc.sgns_o2(n_ref, c_ref, z[pre + "walks"], z[pre + "seeds"], w, neg, z[pre + "table"], lr,
                alpha, dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node, n_ref)
    np.testing.assert_array_equal(ctx, c_ref)
    tol = tol_for(float(z[pre + "margin"]))
    np.testing.assert_allclose(node, z[pre + "node1"], rtol=0, atol=tol)
    np.testing.assert_allclose(ctx, z[pre + "ctx1"], rtol=0, atol=tol)


@pytest.mark.parametrize("d,neg,w,V,L,P,T", [
    (128, 5, 5, 2000, 80, 24, 100000),   # the headline shape
    (128, 10, 5, 40, 30, 8, 3000),       # small V: many repeated negatives / positive hits
    (256, 10, 5, 500, 40, 6, 20000),
    (512, 3, 2, 300, 20, 4, 5000),
    (512, 3, 10, 300, 30, 3, 5000),      # ring would exceed 40 KB/wave: direct kernel
    (128, 5, 40, 300, 100, 3, 5000),     # 2w+1 > 64 slots: direct kernel
    (64, 5, 3, 100, 25, 10, 4000),
    (96, 7, 4, 100, 25, 6, 4000),        # masked layout, MAXN = 10
    (2, 4, 3, 34, 20, 20, 5000),         # Karate shape
    (33, 15, 6, 80, 30, 5, 3000),        # MAXN = 20
    (128, 0, 5, 100, 20, 5, 100),        # no negatives
    (128, 5, 0, 100, 20, 5, 1000),       # window 0: no pairs, tables untouched
    (128, 20, 1, 3, 10, 3, 100),         # V = 3: nearly every draw repeats
])
def test_o2_random_bit_exact_vs_oracle(d, neg, w, V, L, P, T):
    check_o2_random_vs_oracle(d, neg, w, V, L, P, T)


@pytest.mark.parametrize("d,neg,w,V,L,P,T", [
    (64, 5, 3, 100, 25, 10, 4000),
    (96, 7, 4, 100, 25, 6, 4000),        # masked layout, MAXN = 10
    (128, 10, 5, 40, 30, 8, 3000),       # small V: many repeated negatives / positive hits
    (256, 10, 5, 500, 40, 6, 20000),
    (33, 15, 6, 80, 30, 5, 3000),        # MAXN = 20
    (128, 20, 1, 3, 10, 3, 100),         # V = 3: nearly every draw repeats
])
def test_o2_direct_kernel_bit_exact_vs_oracle(d, neg, w, V, L, P, T):
    """The direct kernel (o2_kernel=1) on shapes the sequential mode gives to the ring kernel:
    both layouts, the three MAXN buckets, and vocabularies small enough that nearly every pair
    repeats a negative or draws its positive."""
    check_o2_random_vs_oracle(d, neg, w, V, L, P, T, opts={"o2_kernel": 1})


def check_o2_random_vs_oracle(d, neg, w, V, L, P, T, opts=None):
    rng = np.random.RandomState(d * 1000 + neg * 10 + V)
    counts = rng.randint(1, 100, V)
    table = orc.make_table(counts, T)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.2, 0.2, (V, d)).astype(np.float32)
    walks = rng.randint(0, V, (P, L)).astype(np.int32)
    walks[rng.uniform(size=walks.shape) < 0.05] = -1
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    node, ctx = run_o2(node0, ctx0, walks, seeds, w, neg, table, 0.05, 0.9, opts=opts)
    n_ref, c_ref = node0.copy(), ctx0.copy()
    orc.sgns_o2(n_ref, c_ref, walks, seeds, w, neg, table, 0.05, 0.9, dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node, n_ref)
    np.testing.assert_array_equal(ctx, c_ref)
    if w == 0:
        np.testing.assert_array_equal(node, node0)


@pytest.mark.parametrize("w,L", [(1, 30), (2, 40), (5, 80), (5, 300), (3, 129), (12, 200),
                                 (31, 150)])
def test_o2_ring_revisit_patterns_bit_exact(w, L):
    """Walks that revisit nodes at every distance 1 .. 2w+3 (the LDS ring's alias, leave-and-
    re-enter and same-slot cases), walks longer than the 128-position index window, None
    entries, and the widest ring (w = 31 -> 63 slots)."""
    rng = np.random.RandomState(w * 100 + L)
    V, d, neg = 12, 128, 5
    table = orc.make_table(rng.randint(1, 9, V), 3000)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.2, 0.2, (V, d)).astype(np.float32)
    walks = []
    for period in range(1, 2 * w + 4):
        base = rng.randint(0, V, period)
        walks.append(np.resize(base, L))
    walks = np.array(walks, np.int32)
    walks[rng.uniform(size=walks.shape) < 0.03] = -1
    seeds = rng.randint(0, 2 ** 48, len(walks), dtype=np.int64).astype(np.uint64)
    node, ctx = run_o2(node0, ctx0, walks, seeds, w, neg, table, 0.02, 1.0)
    n_ref, c_ref = node0.copy(), ctx0.copy()
    orc.sgns_o2(n_ref, c_ref, walks, seeds, w, neg, table, 0.02, 1.0, dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node, n_ref)
    np.testing.assert_array_equal(ctx, c_ref)


def test_o2_out_of_range_rows_are_none():
    """Walk entries >= V behave as None (never read/written); table values >= V are skipped."""
    rng = np.random.RandomState(3)
    V, d = 50, 128
    table = orc.make_table(rng.randint(1, 9, V), 1000)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.1, 0.1, (V, d)).astype(np.float32)
    walks = rng.randint(0, V, (4, 20)).astype(np.int32)
    seeds = rng.randint(0, 2 ** 40, 4).astype(np.uint64)
    bad = walks.copy()
    bad[:, 5] = V + 7
    ref_walks = walks.copy()
    ref_walks[:, 5] = -1
    a = run_o2(node0, ctx0, bad, seeds, 3, 5, table, 0.1, 1.0)
    b = run_o2(node0, ctx0, ref_walks, seeds, 3, 5, table, 0.1, 1.0)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    bad_table = table.copy()
    bad_table[::7] = V + 100  # never in range: those draws must be skipped, not read
    run_o2(node0, ctx0, walks, seeds, 3, 5, bad_table, 0.1, 1.0)


def test_o2_long_walk_truncated_at_max_sentence_len():
    rng = np.random.RandomState(4)
    V, d = 200, 64
    table = orc.make_table(rng.randint(1, 9, V), 1000)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    walks = rng.randint(0, V, (1, 10050)).astype(np.int32)
    seeds = np.array([123456789], np.uint64)
    a = run_o2(node0, np.zeros_like(node0), walks, seeds, 2, 2, table, 0.01, 1.0)
    b = run_o2(node0, np.zeros_like(node0), walks[:, :10000].copy(), seeds, 2, 2, table, 0.01,
               1.0)
    np.testing.assert_array_equal(a[0], b[0])


@pytest.mark.parametrize("hot_share", [None, tsi.DEFAULT_HOT_P])
def test_o2_hogwild_statistics(hot_share):
    """Many walks in flight, low row contention (the regime of the 1M-node benchmark): rows never
    touched stay bit-identical and the tables move as in the sequential (workers=1) run.  At
    lr=0.005 the updates are nearly order-independent (the oracle run in reversed walk order
    agrees with the forward run to cosine 0.998 on node rows, 0.99994 on context rows).  What
    is left is Hogwild itself: a row read-modify-written by two wavefronts at once keeps one
    update, and a store sits in one XCD's (non-coherent) L2 for microseconds before another XCD
    sees it.  Measured on MI355X (streaming kernel, 3 runs each, with and without the hot-row
    bitmap): cosine 0.9911-0.9913 (node) / 0.9725-0.9729 (ctx), run-to-run spread < 5e-4; bars
    0.985 / 0.965 (round 1: 0.98 / 0.95)."""
    rng = np.random.RandomState(5)
    V, d, L, P, w, neg = 500000, 128, 40, 1000, 5, 5
    table = orc.make_table(rng.randint(1, 50, V), 2000000)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.1, 0.1, (V, d)).astype(np.float32)
    walks = rng.randint(0, V // 2, (P, L)).astype(np.int32)  # rows >= V/2 never an input
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    hn, hc = run_o2(node0, ctx0, walks, seeds, w, neg, table, 0.005, 1.0, tsi.MODE_HOGWILD,
                    hot_share=hot_share)
    sn, sc = run_o2(node0, ctx0, walks, seeds, w, neg, table, 0.005, 1.0, tsi.MODE_SEQUENTIAL)
    np.testing.assert_array_equal(hn[V // 2:], node0[V // 2:])
    assert np.isfinite(hn).all() and np.isfinite(hc).all()

    def cos(a, b):
        a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
        return a @ b / np.sqrt((a @ a) * (b @ b))
    touched = np.unique(walks)
    cn = cos(hn[touched] - node0[touched], sn[touched] - node0[touched])
    cc = cos(hc - ctx0, sc - ctx0)
    print("hogwild vs sequential cosine: node %.5f ctx %.5f" % (cn, cc))
    assert cn > 0.985 and cc > 0.965, (cn, cc)


@pytest.mark.parametrize("kernel", [0, 1, 3])  # automatic (direct here), direct, streaming
def test_o2_hogwild_deterministic_when_walks_disjoint(kernel):
    """Walks that share no row (inputs, positives) and draw no shared negative are independent:
    every Hogwild kernel then equals the sequential run bit for bit (same per-pair arithmetic,
    plain stores for rows outside the hot bitmap)."""
    rng = np.random.RandomState(6)
    V, d, L, w, neg = 4096, 128, 16, 3, 0  # no negatives -> rows touched = the walk's own
    P = V // L
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.1, 0.1, (V, d)).astype(np.float32)
    walks = rng.permutation(V).reshape(P, L).astype(np.int32)
    seeds = np.zeros(P, np.uint64)
    table = np.zeros(1, np.uint32)
    a = run_o2(node0, ctx0, walks, seeds, w, neg, table, 0.05, 1.0, tsi.MODE_HOGWILD,
               opts={"o2_kernel": kernel})
    b = run_o2(node0, ctx0, walks, seeds, w, neg, table, 0.05, 1.0, tsi.MODE_SEQUENTIAL)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_o2_dropin_per_walk_numpy_and_tensor():
    """train_o2 with the reference signature: numpy tables mutated in place, seeds from the global
    numpy RNG, Vocab-like path items, return value = non-None count."""
    z, pre = KAT_O2, "o2_d2_n4_w3_"
    d, neg, w, V, L, P = [int(x) for x in z[pre + "params"]]
    lr, alpha = [float(x) for x in z[pre + "lr_alpha"]]
    node, ctx = z[pre + "node0"].copy(), z[pre + "ctx0"].copy()
    tnode, tctx = dev(node.copy()), dev(ctx.copy())

    class V_:
        def __init__(self, i):
            self.index = i
    for p in range(P):
        path = [V_(int(x)) if x >= 0 else None for x in z[pre + "walks"][p]]
        np.random.seed(1000 * 0 + p)
        r = tsi.train_o2(node, ctx, path, lr, neg, w, z[pre + "table"], py_alpha=alpha, py_size=d,
                         py_work=np.zeros(d, np.float32))
        assert r == z[pre + "ret"][p]
        np.random.seed(1000 * 0 + p)
        tsi.train_o2(tnode, tctx, path, lr, neg, w, dev(z[pre + "table"]), py_alpha=alpha)
    np.testing.assert_allclose(node, z[pre + "node1"], atol=tol_for(float(z[pre + "margin"])))
    np.testing.assert_allclose(ctx, z[pre + "ctx1"], atol=tol_for(float(z[pre + "margin"])))
    np.testing.assert_array_equal(tnode.cpu().numpy(), node)


@pytest.mark.parametrize("route", ["host", "device"])
def test_dropin_per_call_cost_independent_of_table_sizes(route):
    """The per-call drop-ins touch only the rows a walk / edge can touch: numpy tables on the host
    route (libcome's host twin in place) or forced down the device route (cached device mirrors,
    the negative table uploaded once).  Per-call time must not grow with T (1e4 -> 2e7 slots) or
    V (2e3 -> 2e6 rows), and the numpy results must equal the CUDA-tensor path's bit for bit."""
    prev = tsi.set_numpy_route(route)
    try:
        _per_call_cost(route)
    finally:
        tsi.set_numpy_route(prev)


def _per_call_cost(route):
    import time

    class V_:
        def __init__(self, i):
            self.index = i
    rng = np.random.RandomState(12)
    d, neg, w, calls = 64, 5, 3, 40
    times = {}
    for V, T in ((2000, 10_000), (2_000_000, 20_000_000)):
        table = orc.make_table(rng.randint(1, 50, V), T)
        node = rng.uniform(-1, 1, (V, d)).astype(np.float32)
        ctx = np.zeros_like(node)
        tnode, tctx, ttab = dev(node), dev(ctx), dev(table)
        paths = [[V_(int(x)) for x in rng.randint(0, V, 30)] for _ in range(calls + 1)]
        edges = [[V_(int(x)) for x in rng.randint(0, V, 2)] for _ in range(calls + 1)]
        np.random.seed(3)
        tsi.train_o2(node, ctx, paths[0], 0.05, neg, w, table)  # warm-up: uploads the table
        tsi.train_o1(node, edges[0], 0.05, neg, table)
        torch.cuda.synchronize()
        t0 = time.time()
        for p, e in zip(paths[1:], edges[1:]):
            tsi.train_o2(node, ctx, p, 0.05, neg, w, table)
            tsi.train_o1(node, e, 0.05, neg, table)
        times[(V, T)] = (time.time() - t0) / calls
        np.random.seed(3)
        for p, e in zip(paths, edges):
            tsi.train_o2(tnode, tctx, p, 0.05, neg, w, ttab)
            tsi.train_o1(tnode, e, 0.05, neg, ttab)
        np.testing.assert_array_equal(tnode.cpu().numpy(), node)
        np.testing.assert_array_equal(tctx.cpu().numpy(), ctx)
    small, big = times[(2000, 10_000)], times[(2_000_000, 20_000_000)]
    print("per call (%s route): small tables %.3f ms, large tables %.3f ms" % (
        route, small * 1e3, big * 1e3))
    assert big < 2.0 * small + 2e-3, times


# ---- O1 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(KAT_O1["names"]))
def test_o1_kat_bit_exact_vs_oracle_and_golden(name):
    z, pre = KAT_O1, "o1_%s_" % name
    d, neg, V, E = [int(x) for x in z[pre + "params"]]
    lr = float(z[pre + "lr"][0])
    node = run_o1(z[pre + "node0"], z[pre + "edges"], z[pre + "seeds"], neg, z[pre + "table"], lr)
    n_ref = z[pre + "node0"].copy()
    orc.sgns_o1(n_ref, z[pre + "edges"], z[pre + "seeds"], neg, z[pre + "table"], lr,
                dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node, n_ref)
    np.testing.assert_allclose(node, z[pre + "node1"], rtol=0,
                               atol=tol_for(float(z[pre + "margin"])))


@pytest.mark.parametrize("d,neg,V,E", [(128, 5, 5000, 3000), (2, 4, 34, 78), (256, 10, 300, 500),
                                       (100, 20, 50, 200), (128, 5, 3, 50), (512, 1, 100, 64)])
@pytest.mark.parametrize("chunk", [0, 7, -1])
def test_o1_random_bit_exact_vs_oracle(d, neg, V, E, chunk):
    """Sequential mode vs the oracle bit for bit: the per-edge kernel (chunk 0) and the run kernel
    k_sgns_o1_runs (o1_chunk = 7: the input row held over runs of edges sharing it; edges sorted
    by their first endpoint so runs form, self-loops and negatives equal to the held row
    included; o1_chunk = -1, the default: one chunk of every edge in order)."""
    rng = np.random.RandomState(d + neg + V)
    table = orc.make_table(rng.randint(1, 30, V), 5 * V + 7)
    node0 = rng.uniform(-0.5, 0.5, (V, d)).astype(np.float32)
    edges = rng.randint(0, V, (E, 2)).astype(np.int32)
    edges[::17, 1] = edges[::17, 0]  # self loops
    if chunk:
        edges = edges[np.argsort(edges[:, 0], kind="stable")]
    seeds = rng.randint(0, 2 ** 48, E, dtype=np.int64).astype(np.uint64)
    with options(o1_chunk=chunk):
        node = run_o1(node0, edges, seeds, neg, table, 0.2)
    n_ref = node0.copy()
    orc.sgns_o1(n_ref, edges, seeds, neg, table, 0.2, dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node, n_ref)


def test_o1_dropin_per_edge():
    z, pre = KAT_O1, "o1_d2_n4_"
    d, neg, V, E = [int(x) for x in z[pre + "params"]]
    node = z[pre + "node0"].copy()

    class V_:
        def __init__(self, i):
            self.index = i
    for e in range(E):
        np.random.seed(50000 + e)
        r = tsi.train_o1(node, [V_(int(z[pre + "edges"][e, 0])), V_(int(z[pre + "edges"][e, 1]))],
                         float(z[pre + "lr"][0]), neg, z[pre + "table"], py_size=d)
        assert r == 2
    np.testing.assert_allclose(node, z[pre + "node1"], atol=tol_for(float(z[pre + "margin"])))


# ---- community gradient / GMM responsibilities -------------------------------------------------

def test_community_grad_vs_golden():
    z = np.load(os.path.join(GOLDEN, "community.npz"))
    for name in z["names"]:
        p = name + "_"
        beta, lr = [float(x) for x in z[p + "scal"]]
        x = dev(z[p + "x0"])
        ce.community_grad(x, dev(z[p + "pi"]), dev(z[p + "mu"]), dev(z[p + "inv"]), beta, lr,
                          int(z[p + "iters"]))
        np.testing.assert_allclose(x.cpu().numpy(), z[p + "x1"], rtol=1e-5, atol=1e-5,
                                   err_msg=name)


_MFMA_COMM = [(64, 1000, 7, 3), (128, 777, 5, 2), (128, 300, 1, 1), (128, 4097, 4, 2),
              (64, 129, 3, 1)]
_VALU_COMM = [(96, 200, 3, 2), (256, 150, 3, 2), (500, 37, 2, 1)]


@pytest.mark.parametrize("d,V,K,iters,kern", [c + (k,) for c in _MFMA_COMM for k in (2, 3)] +
                         [c + (2,) for c in _VALU_COMM])
def test_community_grad_vs_oracle(d, V, K, iters, kern):
    """MFMA path (d = 64, 128; ragged row tiles; community_async = 2: k_community16 on fp32
    16x16x4 MFMAs with one row tile per wavefront, 3: k_community_b16, fp32 operands as three
    bf16 parts on 16x16x32 MFMAs), VALU path
    (d = 96) and the wide VALU path (d = 256, 500: matrices streamed in row chunks) against the
    numpy restatement of community_embeddings.py:61-78: fp32 contractions in another order,
    rtol/atol 2e-5; the clip at +-5 is exercised (beta large)."""
    with options(community_async=kern):
        _community_vs_oracle(d, V, K, iters)


def _community_vs_oracle(d, V, K, iters):
    rng = np.random.RandomState(d + V)
    x0 = rng.normal(size=(V, d)).astype(np.float32)
    A = rng.normal(size=(K, d, d)) / np.sqrt(d)
    cov = np.einsum("kij,klj->kil", A, A) + np.eye(d)[None] * 0.5
    inv = np.linalg.inv(cov.astype(np.float32)).astype(np.float32)
    mu = rng.normal(size=(K, d)).astype(np.float32)
    pi = rng.dirichlet(np.ones(K), V).astype(np.float32)
    for beta in (0.05, 40.0):
        x = dev(x0)
        ce.community_grad(x, dev(pi), dev(mu), dev(inv), beta, 0.1, iters)
        ref = orc.community_train(x0, pi, mu, inv, beta, 0.1, iters)
        np.testing.assert_allclose(x.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


def test_community_train_node_subset_with_repeats():
    """Community2Vec.train on a node list with repeats inside a chunk (counted once) and across
    chunks (counted per chunk), as the reference's grad_input[node_index] += batch does."""
    from come_amd.community_embeddings import Community2Vec
    from come_amd.model import Model
    rng = np.random.RandomState(8)
    V, d, K = 300, 64, 3
    np.random.seed(1)
    m = Model((np.arange(1, V + 1), np.full(V, 2)), size=d, table_size=1000, k=K, device=DEV)
    A = rng.normal(size=(K, d, d)) / np.sqrt(d)
    inv = np.linalg.inv((np.einsum("kij,klj->kil", A, A) + 0.5 * np.eye(d)).astype(np.float32))
    m.centroid = dev(rng.normal(size=(K, d)).astype(np.float32))
    m.inv_covariance_mat = dev(inv.astype(np.float32))
    m.pi = dev(rng.dirichlet(np.ones(K), V).astype(np.float32))
    x0 = m.node_embedding.cpu().numpy()
    nodes = list(rng.randint(1, V + 1, 90)) + [5, 5, 5, 7] + [5] * 3
    cm = Community2Vec.__new__(Community2Vec)
    cm.lr, cm.distributed, cm.group = 0.1, False, None
    cm.train(nodes, m, 2.0, chunksize=10, iter=2)
    ref = orc.community_train(x0, m.pi.cpu().numpy(), m.centroid.cpu().numpy(), inv, 2.0, 0.1, 2,
                              chunksize=10, rows=np.array(nodes) - 1)
    np.testing.assert_allclose(m.node_embedding.cpu().numpy(), ref, rtol=2e-5, atol=2e-5)


def test_gmm_resp_vs_golden():
    z = load_golden("gmm_resp")
    for name in z["names"]:
        p = name + "_"
        pc = orc.precision_cholesky(z[p + "cov"])
        args = ce.gmm_resp_params(z[p + "w"], z[p + "mu"], pc, DEV)
        pi = ce.gmm_resp(dev(z[p + "X"]), *args).cpu().numpy()
        np.testing.assert_allclose(pi, z[p + "pi"], rtol=0, atol=2e-5, err_msg=name)
        np.testing.assert_allclose(pi.sum(1), 1.0, atol=1e-5)


# ---- whole Karate flow (adsc_Karate.py:104-137, workers=1) -------------------------------------

def test_karate_flow_deterministic():
    from come_amd.community_embeddings import Community2Vec
    from come_amd.context_embeddings import Context2Vec
    from come_amd.model import Model
    from come_amd.node_embeddings import Node2Vec
    z = np.load(os.path.join(GOLDEN, "karate.npz"))
    size, neg, ws, lr, alpha, beta, T = z["hyper"]
    deg = dict(zip(z["degree_ids"].tolist(), z["degree_counts"].tolist()))
    np.random.seed(42)
    m = Model(deg, size=int(size), table_size=int(T), k=2)
    np.testing.assert_array_equal(m.node_embedding.cpu().numpy(), z["node_init"])
    nl = Node2Vec(workers=1, negative=int(neg), lr=float(lr), deterministic=True)
    cl = Context2Vec(window_size=int(ws), workers=1, negative=int(neg), lr=float(lr),
                     deterministic=True)
    np.random.seed(100)
    nl.train(m, edges=z["edges"], iter=1, chunksize=20)
    np.testing.assert_allclose(m.node_embedding.cpu().numpy(), z["after_o1_pre"], atol=1e-3)
    np.random.seed(101)
    cl.train(m, paths=z["walks"], total_nodes=z["walks"].size, alpha=float(alpha), chunksize=20)
    np.testing.assert_allclose(m.node_embedding.cpu().numpy(), z["after_o2_pre_node"], atol=1e-3)
    np.testing.assert_allclose(m.context_embedding.cpu().numpy(), z["after_o2_pre_ctx"], atol=1e-3)
    np.random.seed(102)
    nl.train(m, edges=z["edges"], iter=1, chunksize=20)
    np.random.seed(103)
    cl.train(m, paths=z["walks"], total_nodes=z["walks"].size, alpha=float(alpha), chunksize=20)
    np.testing.assert_allclose(m.node_embedding.cpu().numpy(), z["after_loop_node"], atol=1e-3)
    # community step on the reference's own fitted GMM parameters
    m.node_embedding.copy_(dev(z["after_loop_node"]))
    m.centroid, m.inv_covariance_mat, m.pi = (dev(z["gmm_centroid"]), dev(z["gmm_inv"]),
                                              dev(z["gmm_pi"]))
    cm = Community2Vec(m, reg_covar=1e-5, lr=float(lr))
    cm.train(list(range(1, 35)), m, float(beta), chunksize=20, iter=5)
    np.testing.assert_allclose(m.node_embedding.cpu().numpy(), z["after_com_node"], atol=1e-5)


# ---- packed negative table (come_pack_table) ---------------------------------------------------

def unpack_words(words, T):
    """Host decode of the packed words: table[64w + i] = base + popcount(bits & (2^(i+1)-1))."""
    w = words.cpu().numpy().view(np.uint32).reshape(-1, 4)
    base = w[:, 0].astype(np.int64)
    bits = (w[:, 3].astype(np.uint64) << np.uint64(32)) | w[:, 2].astype(np.uint64)
    i = np.arange(64, dtype=np.uint64)
    on = ((bits[:, None] >> i[None, :]) & np.uint64(1)).astype(np.int64)
    return (base[:, None] + np.cumsum(on, 1)).reshape(-1)[:T]


@pytest.mark.parametrize("V,T", [(34, 5000), (1000, 200000), (3, 64), (7, 50), (5000, 12345),
                                 (100000, 1000003)])
def test_pack_table_exact_on_make_table(V, T):
    rng = np.random.RandomState(V + T)
    counts = (rng.pareto(1.5, V) * 5 + 1).astype(np.int64)
    table = orc.make_table(counts, T)
    p = tsi.pack_table(dev(table))
    assert p is not None and p.T == T
    np.testing.assert_array_equal(unpack_words(p.words, T), table.astype(np.int64))


def test_pack_table_refuses_non_unit_steps():
    t = np.arange(0, 300, 2, dtype=np.uint32)  # steps of 2
    assert tsi.pack_table(dev(t)) is None
    t = np.array([5, 4, 4, 4], np.uint32)  # decreasing
    assert tsi.pack_table(dev(t)) is None


@pytest.mark.parametrize("d,neg,w,V,L,P,T", [(128, 5, 5, 2000, 80, 40, 100000),
                                             (2, 4, 3, 34, 20, 20, 5000),
                                             (256, 10, 5, 500, 60, 10, 64 * 77 + 5),
                                             (100, 20, 2, 3, 30, 6, 64)])
def test_o2_o1_packed_table_bit_exact(d, neg, w, V, L, P, T):
    rng = np.random.RandomState(d + V + T)
    table = orc.make_table(rng.randint(1, 60, V), T)
    packed = tsi.pack_table(dev(table))
    assert packed is not None
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.2, 0.2, (V, d)).astype(np.float32)
    walks = rng.randint(0, V, (P, L)).astype(np.int32)
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    node, ctx = dev(node0.copy()), dev(ctx0.copy())
    tsi.sgns_o2(node, ctx, dev(walks), dev(seeds), w, neg, packed, 0.05, 0.9,
                tsi.MODE_SEQUENTIAL)
    n_ref, c_ref = node0.copy(), ctx0.copy()
    orc.sgns_o2(n_ref, c_ref, walks, seeds, w, neg, table, 0.05, 0.9, dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node.cpu().numpy(), n_ref)
    np.testing.assert_array_equal(ctx.cpu().numpy(), c_ref)
    edges = rng.randint(0, V, (3 * P, 2)).astype(np.int32)
    eseeds = rng.randint(0, 2 ** 48, 3 * P, dtype=np.int64).astype(np.uint64)
    tsi.sgns_o1(node, dev(edges), dev(eseeds), neg, packed, 0.2, tsi.MODE_SEQUENTIAL)
    orc.sgns_o1(n_ref, edges, eseeds, neg, table, 0.2, dot_mode=orc.DOT_WAVE64)
    np.testing.assert_array_equal(node.cpu().numpy(), n_ref)


def test_o2_hogwild_packed_equals_plain_when_walks_disjoint():
    """Hogwild with disjoint walks is deterministic; packed and plain tables give identical
    tables (same draws)."""
    rng = np.random.RandomState(3)
    V, d, P, L = 4000, 128, 64, 40
    table = orc.make_table(rng.randint(1, 50, V), 100000)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.2, 0.2, (V, d)).astype(np.float32)
    walks = rng.permutation(V)[:P * L].reshape(P, L).astype(np.int32)
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    out = []
    for t in (dev(table), tsi.pack_table(dev(table))):
        node, ctx = dev(node0.copy()), dev(ctx0.copy())
        tsi.sgns_o2(node, ctx, dev(walks), dev(seeds), 5, 0, t, 0.05, 1.0, tsi.MODE_HOGWILD)
        out.append((node.cpu().numpy(), ctx.cpu().numpy()))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


# ---- edge shapes and sizes ---------------------------------------------------------------------

@pytest.mark.parametrize("case", ["empty_batch", "single_node_walks", "window_gt_len",
                                  "all_none", "d512", "d257", "one_walk_long", "V1"])
def test_o2_edge_shapes_bit_exact(case):
    """Empty batch, length-1 walks (no pairs), window wider than the walk, walks of None only,
    the widest rows (d = 512, one 2-KB row per 4 wave instructions) and a masked odd width
    (d = 257), one long walk, a one-node vocabulary (every draw collides with the positive)."""
    rng = np.random.RandomState(hash(case) % 1000)
    d, neg, w, V, L, P = {"empty_batch": (128, 5, 5, 50, 10, 0),
                          "single_node_walks": (128, 5, 5, 50, 1, 7),
                          "window_gt_len": (64, 3, 9, 40, 6, 9),
                          "all_none": (128, 5, 5, 50, 20, 3),
                          "d512": (512, 4, 3, 60, 25, 6),
                          "d257": (257, 2, 2, 30, 15, 5),
                          "one_walk_long": (128, 5, 5, 500, 4000, 1),
                          "V1": (16, 5, 2, 1, 12, 3)}[case]
    table = orc.make_table(rng.randint(1, 30, V), 997) if V > 1 else np.zeros(97, np.uint32)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.2, 0.2, (V, d)).astype(np.float32)
    walks = rng.randint(0, V, (P, L)).astype(np.int32)
    if case == "all_none":
        walks[:] = -1
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    n_ref, c_ref = node0.copy(), ctx0.copy()
    if P:
        orc.sgns_o2(n_ref, c_ref, walks, seeds, w, neg, table, 0.05, 1.0,
                    dot_mode=orc.DOT_WAVE64)
    # sequential mode, and the Hogwild kernels (direct, streaming) on ONE wavefront without
    # contended rows (walks then run in order): bit-exact with the oracle; the free Hogwild launch
    # (every walk in flight, derived hot rows) finite and leaving rows no walk touches unchanged
    runs = [(tsi.MODE_SEQUENTIAL, None, None),
            (tsi.MODE_HOGWILD, {"o2_kernel": 1, "max_waves": 1}, None),
            (tsi.MODE_HOGWILD, {"o2_kernel": 3, "max_waves": 1}, None)]
    for mode, opts, hot in runs:
        node, ctx = dev(node0.copy()), dev(ctx0.copy())
        tsi.sgns_o2(node, ctx, dev(walks.reshape(P, L)), dev(seeds), w, neg, dev(table), 0.05,
                    1.0, mode, opts=opts, hot=hot)
        np.testing.assert_array_equal(node.cpu().numpy(), n_ref, err_msg=str(opts))
        np.testing.assert_array_equal(ctx.cpu().numpy(), c_ref, err_msg=str(opts))
    node, ctx = dev(node0.copy()), dev(ctx0.copy())
    tsi.sgns_o2(node, ctx, dev(walks.reshape(P, L)), dev(seeds), w, neg, dev(table), 0.05, 1.0,
                tsi.MODE_HOGWILD)
    assert torch.isfinite(node).all() and torch.isfinite(ctx).all()
    untouched = np.setdiff1d(np.arange(V), walks[walks >= 0])
    np.testing.assert_array_equal(node.cpu().numpy()[untouched], node0[untouched])
    if case in ("empty_batch", "single_node_walks", "all_none"):
        np.testing.assert_array_equal(n_ref, node0)


def test_o2_o1_rows_beyond_2_32_elements():
    """Rows whose element offset exceeds 2^32 (V x d > 4.29e9: the reference's 32-bit
    `word2_index * size` would wrap, the kernels use 64-bit offsets).  Compact problem on the
    host oracle, the same problem scattered onto rows >= 2^32 / d of 17 GB device tables:
    touched rows bit-identical."""
    d, Vc, V = 256, 40, 16_800_000
    if torch.cuda.get_device_properties(0).total_memory < 48 * 2 ** 30:
        pytest.skip("needs ~36 GB of device memory")
    rng = np.random.RandomState(7)
    big = np.sort(rng.choice(np.arange(2 ** 32 // d - 20, V), Vc, replace=False)).astype(np.int64)
    assert big[-1] * d > 2 ** 32
    table_c = orc.make_table(rng.randint(1, 20, Vc), 3001)
    node0 = rng.uniform(-1, 1, (Vc, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.2, 0.2, (Vc, d)).astype(np.float32)
    walks_c = rng.randint(0, Vc, (6, 30)).astype(np.int32)
    edges_c = rng.randint(0, Vc, (20, 2)).astype(np.int32)
    seeds = rng.randint(0, 2 ** 48, 6, dtype=np.int64).astype(np.uint64)
    eseeds = rng.randint(0, 2 ** 48, 20, dtype=np.int64).astype(np.uint64)
    n_ref, c_ref = node0.copy(), ctx0.copy()
    orc.sgns_o2(n_ref, c_ref, walks_c, seeds, 5, 5, table_c, 0.05, 1.0, dot_mode=orc.DOT_WAVE64)
    orc.sgns_o1(n_ref, edges_c, eseeds, 5, table_c, 0.2, dot_mode=orc.DOT_WAVE64)
    node = torch.zeros((V, d), dtype=torch.float32, device=DEV)
    ctx = torch.zeros((V, d), dtype=torch.float32, device=DEV)
    bi = torch.from_numpy(big).to(DEV)
    node[bi] = dev(node0)
    ctx[bi] = dev(ctx0)
    try:
        tsi.sgns_o2(node, ctx, dev(big[walks_c].astype(np.int32)), dev(seeds), 5, 5,
                    dev(big[table_c].astype(np.uint32)), 0.05, 1.0, tsi.MODE_SEQUENTIAL)
        tsi.sgns_o1(node, dev(big[edges_c].astype(np.int32)), dev(eseeds), 5,
                    dev(big[table_c].astype(np.uint32)), 0.2, tsi.MODE_SEQUENTIAL)
        np.testing.assert_array_equal(node[bi].cpu().numpy(), n_ref)
        np.testing.assert_array_equal(ctx[bi].cpu().numpy(), c_ref)
    finally:
        del node, ctx
        torch.cuda.empty_cache()


@pytest.mark.parametrize("w", [1, 2, 5])
def test_o2_hogwild_single_walk_sees_its_own_writebacks(w):
    """One walk in flight, nodes that leave the window and re-enter at the very next boundary
    (period 2w + 2) and centers whose positive row comes back as a later positive: the
    wavefront must read back its own write-backs (no stale L1 line), so Hogwild without
    contended rows equals the sequential run (<= 1e-5 abs; measured bit-exact)."""
    rng = np.random.RandomState(w)
    V, d, L = 2 * w + 2, 128, 6 * (2 * w + 2)
    table = np.zeros(1, np.uint32)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.5, 0.5, (V, d)).astype(np.float32)
    walks = np.resize(rng.permutation(V), L).reshape(1, L).astype(np.int32)
    seeds = np.zeros(1, np.uint64)
    h = run_o2(node0, ctx0, walks, seeds, w, 0, table, 0.1, 1.0, tsi.MODE_HOGWILD)
    s = run_o2(node0, ctx0, walks, seeds, w, 0, table, 0.1, 1.0, tsi.MODE_SEQUENTIAL)
    np.testing.assert_allclose(h[0], s[0], rtol=0, atol=1e-5)
    np.testing.assert_allclose(h[1], s[1], rtol=0, atol=1e-5)
