"""The top-k kernels (csrc/come_topk.hip) on the GPU: the float64 contract of tests/topk_common.py
on real-valued data (both kernels, every metric, with and without exclusion, forced chunk counts),
exact integer-valued data bit for bit against a stable sort and against the CPU twin, adversarial
base orders, the cosine and NaN edge cases, guard bands, determinism and the Python layer
(neighbors.Index / knn_graph, Model.most_similar / nearest_to_centroids)."""
import ctypes

import numpy as np
import pytest

import topk_common as tc
from come_amd import _lib, cpu, neighbors
from come_amd._lib import ptr, stream_handle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def put(a, offset=0):
    """The host array on the device, `offset` floats past a 16-byte boundary."""
    flat = torch.empty((a.size + 4,), dtype=torch.float32, device=dev())
    assert flat.data_ptr() % 16 == 0
    view = flat[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a, copy=True)))
    assert view.data_ptr() % 16 == 4 * offset
    return view


def gpu_topk(q, b, k, metric, exclude=None, chunks=None, offset=0, base_sq=None):
    ex = None if exclude is None else torch.from_numpy(np.array(exclude, copy=True)).to(dev())
    idx, score = neighbors.topk(put(q), put(b, offset), k, metric=metric, exclude=ex,
                                chunks=chunks, base_sq=base_sq)
    assert idx.dtype == torch.int64 and score.dtype == torch.float32
    return idx.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("case", tc.real_cases(), ids=tc.case_id)
def test_contract_on_real_data(case):
    metric, d, off, Q, V, k, chunks, ex = case
    q, b, exclude = tc.real_data(case)
    idx, score = gpu_topk(q, b, k, metric, exclude, chunks, off)
    tc.check_contract(q, b, k, metric, idx, score, exclude, who="come_topk")


@pytest.mark.parametrize("chunks", [1, 3, 7])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("metric, d, offset", [("dot", 64, 0), ("dot", 128, 0), ("l2", 64, 0),
                                               ("l2", 128, 0), ("cosine", 64, 0), ("dot", 64, 1),
                                               ("l2", 64, 1), ("cosine", 64, 1)])
def test_exact_data_bit_for_bit(metric, d, offset, k, chunks):
    """Integer-valued data: idx and score equal the stable sort of the exact scores and the CPU
    twin, with ties inside tiles, across tiles and across chunks (both kernels)."""
    Q, V = 33, 1000
    q, b = tc.exact_data(metric, d, Q, V)
    exclude = (np.arange(Q, dtype=np.int32) * 31 + 500) % V
    exclude[::3] = -1
    for ex in (None, exclude):
        want = tc.exact_reference(q, b, k, metric, ex)
        tc.assert_same_bits(gpu_topk(q, b, k, metric, ex, chunks, offset), want, "come_topk")
        tc.assert_same_bits(cpu.topk(q, b, k, metric=metric, exclude=ex, threads=4), want,
                            "come_cpu_topk")


@pytest.mark.parametrize("metric", tc.METRICS)
def test_exact_data_several_workgroups_and_the_plan(metric):
    q, b = tc.exact_data(metric, 64, 300, 4099, seed=3)
    own = np.arange(300, dtype=np.int32)
    want = tc.exact_reference(q, b, 64, metric, own)
    tc.assert_same_bits(gpu_topk(q, b, 64, metric, own), want, "plan")
    tc.assert_same_bits(gpu_topk(q, b, 64, metric, own, chunks=7), want, "chunks 7")


@pytest.mark.parametrize("rising", [True, False], ids=["rising", "falling"])
@pytest.mark.parametrize("metric, d", [("dot", 128), ("cosine", 64), ("l2", 128), ("dot", 100)])
def test_adversarial_base_orders(metric, d, rising):
    """V = 4099, k = 64, the base sorted by query 0's score: rising with the index, every row
    passes its filter and the insertion runs on every tile; falling, nothing passes after the
    first k."""
    rng = np.random.RandomState(11 + d)
    b = rng.randn(4099, d).astype(np.float32)
    q = rng.randn(33, d).astype(np.float32)
    s, _, _ = tc.scores64(q[:1], b, metric)
    order = np.argsort(s[0], kind="stable")
    b = np.ascontiguousarray(b[order if rising else order[::-1]])
    for chunks in (1, 3):
        idx, score = gpu_topk(q, b, 64, metric, chunks=chunks)
        tc.check_contract(q, b, 64, metric, idx, score, who="adversarial")
    if rising:
        assert (idx[0] >= 4099 - 64 - 8).all()  # query 0's neighbours are the last rows


@pytest.mark.parametrize("offset", [0, 1], ids=["mfma", "valu"])
def test_cosine_zero_rows_and_zero_query(offset):
    q, b, zeros = tc.cosine_zero_data()
    k = len(zeros)
    idx, score = gpu_topk(q, b, k, "cosine", offset=offset)
    assert idx[0].tolist() == zeros and (score[0] == 0).all()
    assert idx[1].tolist() == list(range(k)) and (score[1] == 0).all()
    tc.assert_same_bits((idx, score), tc.exact_reference(q, b, k, "cosine"), "zero rows")


@pytest.mark.parametrize("d", [64, 100])
@pytest.mark.parametrize("metric", tc.METRICS)
def test_nan_row_is_never_returned(metric, d):
    rng = np.random.RandomState(5)
    b = rng.randn(1000, d).astype(np.float32)
    q = rng.randn(33, d).astype(np.float32)
    b[17, 3] = np.nan
    b[640] = np.nan
    idx, score = gpu_topk(q, b, 64, metric, chunks=3)
    assert not np.isin(idx, (17, 640)).any() and not np.isnan(score).any()
    tc.check_contract(q, b, 64, metric, idx, score, who="nan")


def test_padded_tail_when_fewer_than_k_candidates():
    rng = np.random.RandomState(6)
    b = rng.randn(5, 64).astype(np.float32)
    q = b[[0, 3, 4]].copy()
    for metric in tc.METRICS:
        for off in (0, 1):
            idx, score = gpu_topk(q, b, 8, metric, np.array([0, 3, -1], np.int32), offset=off)
            assert (idx[:2, 4:] == -1).all() and (idx[2, 5:] == -1).all() and idx[2, 4] >= 0
            assert (score[:2, 4:] == (np.inf if metric == "l2" else -np.inf)).all()
            tc.check_contract(q, b, 8, metric, idx, score, np.array([0, 3, -1]), who="tail")


FILL = 0xA5


def guarded(shape, dtype, pad_bytes):
    """(view, check): a `shape` / `dtype` view into a flat buffer of byte 0xA5 with pads of
    max(pad_bytes, 4 KiB) (rounded up to 16 bytes) on both sides; check() asserts the pads are
    intact."""
    item = torch.empty((), dtype=dtype).element_size()
    pad = -(-max(int(pad_bytes), 4096) // 16) * 16
    n = int(np.prod(shape)) * item
    flat = torch.full((pad + n + pad,), FILL, dtype=torch.uint8, device=dev())
    view = flat[pad:pad + n].view(dtype).view(shape)

    def check(what):
        for name, part in (("front", flat[:pad]), ("back", flat[pad + n:])):
            bad = int((part != FILL).sum())
            assert bad == 0, "%s: %d byte(s) of the %s pad overwritten" % (what, bad, name)
    return view, check


@pytest.mark.parametrize("d, Q, V, k, chunks", [(128, 129, 1000, 10, 3), (64, 33, 4099, 64, 7),
                                                (100, 33, 1000, 10, 3), (64, 1, 5, 8, 1)])
@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_guard_bands_and_determinism(d, Q, V, k, chunks, metric):
    """idx, score and the scratch sit between sentinel bands wide enough for a whole 128-query
    tile of output; the bands are intact after the call, whose outputs are those of
    neighbors.topk, twice over bit for bit."""
    rng = np.random.RandomState(8)
    q, b = rng.randn(Q, d).astype(np.float32), rng.randn(V, d).astype(np.float32)
    tq, tb = put(q), put(b)
    want_idx, want_score = neighbors.topk(tq, tb, k, metric=metric, chunks=chunks)
    runs = []
    for _ in range(2):
        idx, ci = guarded((Q, k), torch.int32, 128 * k * 4)
        score, cs = guarded((Q, k), torch.float32, 128 * k * 4)
        nbytes = neighbors.scratch_bytes(Q, V, k, chunks, False)
        scratch, cscr = guarded((nbytes // 4,), torch.int32, 128 * k * 8)
        _lib.check(_lib.lib().come_topk(ptr(tq), Q, ptr(tb), V, d, k, _lib.TOPK_METRICS[metric],
                                        None, None, chunks, ptr(scratch), ptr(idx), ptr(score),
                                        stream_handle(dev())), "come_topk")
        torch.cuda.synchronize()
        for c, what in ((ci, "idx"), (cs, "score"), (cscr, "scratch")):
            c(what)
        assert torch.equal(idx.long(), want_idx)
        assert torch.equal(score.view(torch.int32), want_score.view(torch.int32))
        runs.append((idx.cpu().numpy().tobytes(), score.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]


def test_index_search_row_sqnorms_and_knn_graph():
    rng = np.random.RandomState(9)
    X = put(rng.randn(1000, 64).astype(np.float32))
    Qs = put(rng.randn(33, 64).astype(np.float32))
    sq = neighbors.row_sqnorms(X)
    x64 = X.cpu().numpy().astype(np.float64)
    assert np.allclose(sq.cpu().numpy(), (x64 * x64).sum(1), rtol=64 * tc.U, atol=0)
    for metric in tc.METRICS:
        index = neighbors.Index(X, metric)
        i1, s1 = index.search(Qs, 10)
        i2, s2 = neighbors.topk(Qs, X, 10, metric=metric)
        assert torch.equal(i1, i2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
        gi, gs = neighbors.knn_graph(X, 10, metric=metric)
        bi, bs = neighbors.knn_graph(X, 10, metric=metric, batch=300)
        assert torch.equal(gi, bi) and torch.equal(gs.view(torch.int32), bs.view(torch.int32))
        assert gi.shape == (1000, 10) and not (gi == torch.arange(1000, device=gi.device)[:, None]).any()
        tc.check_contract(X.cpu().numpy(), X.cpu().numpy(), 10, metric, gi.cpu().numpy(),
                          gs.cpu().numpy(), np.arange(1000), who="knn_graph")


def test_model_most_similar_maps_ids_and_excludes_the_query():
    from come_amd.model import Model
    ids = np.array([1, 3, 4, 9, 10, 12, 20, 21, 22, 30, 31, 33, 40, 41, 50, 51, 60, 70, 80, 90])
    np.random.seed(3)
    m = Model({int(i): 1 + int(i) % 5 for i in ids}, size=64, table_size=1000, k=3,
              device="cuda:0")
    assert not m._contiguous
    rng = np.random.RandomState(4)
    m.context_embedding = torch.from_numpy(rng.randn(len(ids), 64).astype(np.float32)).to(dev())
    m.centroid = torch.from_numpy(rng.randn(3, 64).astype(np.float32)).to(dev())
    for table, emb in (("node", m.node_embedding), ("context", m.context_embedding)):
        query = np.array([9, 1, 90, 33])
        got, score = m.most_similar(query, topn=5, table=table)
        assert got.shape == (4, 5) and got.dtype == np.int64 and score.dtype == np.float32
        assert np.isin(got, ids).all() and not (got == query[:, None]).any()
        e = emb.cpu().numpy()
        rows = np.searchsorted(ids, query)
        tc.check_contract(e[rows], e, 5, "cosine", np.searchsorted(ids, got), score, rows,
                          who="most_similar " + table)
    one, _ = m.most_similar(9, topn=3)
    assert one.shape == (1, 3) and np.array_equal(one[0], m.most_similar([9], topn=5)[0][0, :3])
    far, _ = m.most_similar([1], topn=64)  # more than the 19 other nodes: the tail is id -1
    assert (far[0, :19] > 0).all() and (far[0, 19:] == -1).all()
    with pytest.raises(KeyError, match="not in the vocabulary"):
        m.most_similar([9, 2])
    with pytest.raises(ValueError):
        m.most_similar([9], table="centroid")
    rows, dist = m.nearest_to_centroids(4)
    e = m.node_embedding.cpu().numpy()
    tc.check_contract(m.centroid.cpu().numpy(), e, 4, "l2", rows.cpu().numpy(), dist.cpu().numpy(),
                      who="nearest_to_centroids")
