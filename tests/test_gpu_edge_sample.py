"""Edges sampled by weight on the device (come_edge_cdf, come_edge_sample) against their CPU twins
bit for bit, the sampled frequencies, Node2Vec.train(weights=) against the manual chain of the
same launches, Node2Vec.loss(weights=), and tier C of the Hogwild O1 launch on a
sampled corpus, where heavy edges repeat."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as orc

import come_amd.training_sdg_inner as tsi
from come_amd import _lib, cpu
from edge_sample_common import (CDF_SIZES, check_frequencies, g12_edges, lognormal_weights,
                                spread_weights)
import sgns_loss_cases as sc
from tierc_inputs import log_sigmoid, sgns_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


@pytest.mark.parametrize("E", CDF_SIZES)
def test_cdf_kernel_equals_cpu_twin(E):
    w = spread_weights(E, seed=100 + E % 97)
    want = cpu.edge_cdf(w)
    got = tsi.edge_cdf(dev(w))
    assert got.dtype == torch.int64 and got.shape == (E,)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("bad", [np.nan, -2.0, None])
def test_cdf_kernel_status_word(bad):
    w = lognormal_weights(5000)
    if bad is None:
        w[:] = 0
    else:
        w[4321] = bad
    with pytest.raises(ValueError):
        tsi.edge_cdf(dev(w))
    good = lognormal_weights(5000)  # the status word and the maximum are reset per call
    np.testing.assert_array_equal(tsi.edge_cdf(dev(good)).cpu().numpy().view(np.uint64),
                                  cpu.edge_cdf(good))


@pytest.mark.parametrize("E,S,offset", [(70_001, 100_003, 2 ** 32 - 5), (1, 777, 0)])
def test_sampler_kernel_equals_cpu_twin(E, S, offset):
    w = lognormal_weights(E)
    edges = np.random.RandomState(6).randint(0, 50_000, (E, 2)).astype(np.int32)
    ecdf = cpu.edge_cdf(w)
    want, wi = cpu.sample_edges(edges, ecdf, S, seed=(77 << 32) | 5, offset=offset,
                                return_index=True)
    got, gi = tsi.sample_edges(dev(edges), dev(ecdf), S, seed=(77 << 32) | 5, offset=offset,
                               return_index=True)
    np.testing.assert_array_equal(gi.cpu().numpy(), wi)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(
        tsi.sample_edges(dev(edges), dev(ecdf), S, seed=(77 << 32) | 5, offset=offset)
        .cpu().numpy(), want)


def test_sampler_kernel_no_samples_writes_nothing():
    edges, w = g12_edges()
    ed, ecdf = dev(edges), dev(cpu.edge_cdf(w))
    out = torch.full((64, 2), -77, dtype=torch.int32, device=DEV)
    idx = torch.full((64,), -77, dtype=torch.int64, device=DEV)
    rc = _lib.lib().come_edge_sample(_lib.ptr(ed), _lib.ptr(ecdf), len(w), 0, 3, 0, _lib.ptr(out),
                                     _lib.ptr(idx), _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and (out == -77).all() and (idx == -77).all()
    assert tsi.sample_edges(ed, ecdf, 0, 3).shape == (0, 2)
    p = ctypes.c_void_p(0)
    assert _lib.lib().come_edge_sample(p, p, 0, 5, 3, 0, p, p, p) == -1


def test_device_frequencies_follow_the_weights():
    edges, w = g12_edges()
    rows, index = tsi.sample_edges(dev(edges), tsi.edge_cdf(dev(w)), 1_000_000, seed=2024,
                                   return_index=True)
    index = index.cpu().numpy()
    assert check_frequencies(index, w) == 15
    assert not (index == 0).any()
    np.testing.assert_array_equal(rows.cpu().numpy(), edges[index])


def _model(V=64, d=128):
    from come_amd.model import Model
    return Model((np.arange(1, V + 1), np.arange(1, V + 1) % 7 + 1), size=d, table_size=5000, k=2,
                 device=DEV)


def _graph64(oov):
    """(edge ids [E, 2], weights) over nodes 1..63 of a 64-node model; with ``oov`` one more row
    joins node 64 -- which has no other edge -- to an id outside the vocabulary."""
    rng = np.random.RandomState(8)
    edges = rng.randint(1, 64, (300, 2))
    w = rng.lognormal(0, 1, 300).astype(np.float32)
    w[17] = 0.0
    if oov:
        edges = np.concatenate([edges[:100], [[64, 9999]], edges[100:]])
        w = np.concatenate([w[:100], [50.0], w[100:]]).astype(np.float32)
    return edges, w


@pytest.mark.parametrize("oov", [False, True])
def test_node2vec_train_weights_deterministic_equals_manual_chain(oov):
    from come_amd.node_embeddings import Node2Vec
    m = _model()
    x0 = m.node_embedding.clone()
    edges, w = _graph64(oov)
    n2v = Node2Vec(lr=0.1, negative=5, deterministic=True)
    np.random.seed(41)
    pairs = n2v.train(m, edges, iter=2, weights=w)
    got = m.node_embedding.clone()
    # the same launches by hand, from the same state of the global numpy RNG
    rows = n2v._edge_rows(m, edges)
    wz = w.copy()
    wz[rows[:, 0] < 0] = 0.0
    S = int((wz > 0).sum())
    assert S == len(w) - 1 - int(oov) and pairs == 2 * 2 * S
    ecdf = tsi.edge_cdf(dev(wz))
    x = x0.clone()
    np.random.seed(41)
    for _ in range(2):
        s64 = int(np.random.randint(0, 2 ** 64, dtype=np.uint64))
        draws, index = tsi.sample_edges(dev(rows), ecdf, S, s64, return_index=True)
        assert (draws >= 0).all() and (dev(wz)[index] > 0).all()  # the OOV row is never drawn
        seeds = tsi.draw_seeds(S)
        tsi.sgns_o1(x, draws, dev(seeds), 5, m.negative_table(), 0.1, tsi.MODE_SEQUENTIAL,
                    hot=None)
    assert torch.equal(got, x) and not torch.equal(got, x0)
    # an explicit seed: pass k draws from the stream seed + k
    m.node_embedding.copy_(x0)
    np.random.seed(41)
    n2v.train(m, edges, iter=2, weights=w, seed=1000, samples=77)
    x = x0.clone()
    np.random.seed(41)
    for k in range(2):
        draws = tsi.sample_edges(dev(rows), ecdf, 77, 1000 + k)
        tsi.sgns_o1(x, draws, dev(tsi.draw_seeds(77)), 5, m.negative_table(), 0.1,
                    tsi.MODE_SEQUENTIAL, hot=None)
    assert torch.equal(m.node_embedding, x)
    if oov:
        # node 64's only edge is never trained; without negatives (which may land on any row)
        # nothing else can touch its row
        m.node_embedding.copy_(x0)
        Node2Vec(lr=0.1, negative=0, deterministic=True).train(m, edges, iter=2, weights=w)
        assert torch.equal(m.node_embedding[63], x0[63])
        assert not torch.equal(m.node_embedding[:63], x0[:63])


def test_node2vec_train_without_weights_is_unchanged():
    from come_amd.node_embeddings import Node2Vec
    m = _model()
    x0 = m.node_embedding.clone()
    edges, _ = _graph64(True)
    n2v = Node2Vec(lr=0.1, negative=5, deterministic=True)
    np.random.seed(43)
    p_omitted = n2v.train(m, edges, iter=2)
    a, state = m.node_embedding.clone(), np.random.random_sample(3)
    m.node_embedding.copy_(x0)
    np.random.seed(43)
    p_none = n2v.train(m, edges, iter=2, weights=None)
    assert p_none == p_omitted == 2 * 2 * 300
    assert torch.equal(m.node_embedding, a)
    np.testing.assert_array_equal(np.random.random_sample(3), state)
    with pytest.raises(ValueError):
        n2v.train(m, edges, samples=10)


def test_node2vec_weighted_loss():
    from come_amd.node_embeddings import Node2Vec
    m = _model(V=300, d=100)
    rng = np.random.RandomState(4)
    edges = rng.randint(1, 301, (2000, 2))
    edges[7] = (5, 9999)  # an endpoint outside the vocabulary: the edge is skipped
    w = rng.lognormal(0, 1, 2000)
    n2v = Node2Vec()
    x = m.node_embedding.cpu().numpy().astype(np.float64)
    rows = n2v._edge_rows(m, edges)
    ok = (rows >= 0).all(1)
    r, wk = rows[ok], w[ok]
    ref = float(-(wk * log_sigmoid(np.einsum("pd,pd->p", x[r[:, 1]], x[r[:, 0]]))).sum())
    # test_gpu_sgns_loss.py's tolerance for the unweighted loss (fp32 dots of the same rows, the
    # derived dot bound twice), each term scaled by its weight
    bound = 2 * sc.dot_bound_factor(100) * (wk[:, None] * np.abs(x[r[:, 0]])
                                            * np.abs(x[r[:, 1]])).sum()
    for backend in ("torch", "native"):
        got = n2v.loss(m, edges, backend=backend, weights=w)
        print("Node2Vec.loss(weights) %s %.6f float64 %.6f bound %.3g" % (backend, got, ref,
                                                                           bound))
        assert abs(got - ref) <= bound + 1e-12 * ref
        unit = n2v.loss(m, edges, backend=backend, weights=np.ones(2000))
        plain = n2v.loss(m, edges, backend=backend)
        assert abs(unit - plain) <= 1e-12 * plain
    with pytest.raises(ValueError):
        n2v.loss(m, edges, weights=w[:-1])


@pytest.fixture(scope="module")
def c2_weighted():
    """C2's SBM (100 blocks x 1,000 nodes, ~1M edges), 2% of the edges held out as in
    tests/test_gpu_tierc.py, with seeded log-normal(0, 1) weights; the negative table from the
    strengths of the kept edges."""
    from come_amd.graph import sbm
    g = sbm(100, 1000, 0.016, 4.04e-5, seed=0)
    rng = np.random.RandomState(31)
    e = g.edges[rng.permutation(len(g.edges))].astype(np.int32)
    k = len(e) // 50
    node0 = rng.uniform(-1, 1, (g.V, 128)).astype(np.float32)
    seeds = rng.randint(0, 2 ** 48, len(e) - k, dtype=np.int64).astype(np.uint64)
    w = np.random.RandomState(33).lognormal(0.0, 1.0, len(e)).astype(np.float32)
    train, wt = e[k:], w[k:]
    strength = (np.bincount(train[:, 0], wt.astype(np.float64), minlength=g.V)
                + np.bincount(train[:, 1], wt.astype(np.float64), minlength=g.V))
    table = orc.make_table(strength, 10_000_000)
    return g, table, train, wt, e[:k], w[:k], node0, seeds


def test_o1_hogwild_on_sampled_edges_matches_sequential_oracle(c2_weighted):
    """test_gpu_tierc.py's O1 recipe on a corpus of S = len(train) draws by weight (heavy edges
    repeat, so more wavefronts share rows than on a plain edge list): the GPU Hogwild launch and
    the sequential oracle on the same list with the same seeds, held-out losses -- the weighted
    reference loss -sum w log sigma(u.v) and the SGNS loss -- within the project's tier-C bar of
    1%.  The reversed-order oracle run of that recipe (a printed figure, not an
    assertion) is left out to keep the test short."""
    g, table, train, wt, held, wh, node0, seeds = c2_weighted
    n, lr = 5, 0.1
    rng = np.random.RandomState(32)
    neg = table[rng.randint(0, len(table), (len(held), n))].astype(np.int64)

    def losses(x):
        ref = float(-(wh * log_sigmoid(np.einsum("pd,pd->p", x[held[:, 1]].astype(np.float64),
                                                 x[held[:, 0]].astype(np.float64)))).sum())
        return ref, sgns_loss(x, x, held[:, 0], held[:, 1], neg)

    l0 = losses(node0)
    draws, index = tsi.sample_edges(dev(train), tsi.edge_cdf(dev(wt)), len(train), seed=34,
                                    return_index=True)
    corpus = draws.cpu().numpy()
    repeats = np.bincount(index.cpu().numpy(), minlength=len(train))
    node = dev(node0)
    tab = dev(table)
    hot = tsi.hot_rows(tab, g.V, int(tsi.DEFAULT_HOT_P * len(table)))
    tsi.sgns_o1(node, draws, dev(seeds), n, tab, lr, tsi.MODE_HOGWILD, hot=hot)
    torch.cuda.synchronize()
    hog = node.cpu().numpy()
    assert np.isfinite(hog).all()
    l_hog = losses(hog)
    seq = node0.copy()
    orc.sgns_o1_hogwild(seq, corpus, seeds, n, table, lr, threads=1)
    l_seq = losses(seq)
    print("O1 on %d sampled edges (%d distinct, most repeated %d times): held-out loss (weighted "
          "reference / SGNS): init %.1f / %.5f  seq %.1f / %.5f  gpu-hogwild %.1f / %.5f" % (
              (len(corpus), int((repeats > 0).sum()), int(repeats.max())) + l0 + l_seq + l_hog))
    assert l_seq[1] < l0[1] - 0.05
    for a, b in zip(l_hog, l_seq):
        assert abs(a - b) / abs(b) < 0.01, (l_hog, l_seq)  # SURVEY.md §8c tier C
