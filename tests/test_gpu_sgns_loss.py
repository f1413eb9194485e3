"""The SGNS losses on the GPU (come_sgns_o2_loss, come_sgns_pairs_loss and the Python layer above
them) against the CPU twins and the float64 numpy restatement of tests/sgns_loss_cases.py.

Against the twin a walk's value must agree to 1e-11 relative: the operands, the fp32 dot order
and the float64 summation order are the same and every term is positive, so only the two libms'
exp / log1p differ (a few ulp of 1e-16 each); an fp32 softplus or another dot order would be off
by about 1e-7.  Against float64 numpy the derived bound of sgns_loss_cases applies.

Every raw call places walk_out, loss_out and pairs_out inside canary-filled buffers and checks the
canaries afterwards.
"""
import ctypes
import functools

import numpy as np
import pytest

from come_amd import _lib, cpu
from come_amd import training_sdg_inner as tsi
import sgns_loss_cases as sc
from tierc_inputs import heldout_o2_pairs, sgns_loss

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 32
CANARY = -1234.5678


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def t(a):
    a = np.array(a)  # a copy: the cases are frozen
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.as_tensor(a, device=dev())


def guarded(n):
    """A float64 buffer of n values between two canary bands; (whole buffer, the inner view)."""
    buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float64, device=dev())
    return buf, buf[GUARD:GUARD + n]


def intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:GUARD] == CANARY).all() and (b[GUARD + n:] == CANARY).all()


def raw_o2(node, ctx, walks, seeds, window, negative, table, with_walks=True, stream=None):
    """come_sgns_o2_loss on device tensors as they are (views included); table: an int32 tensor,
    a PackedTable or None.  Returns (total, pairs, per-walk numpy or None)."""
    V, d = node.shape
    P, L = walks.shape
    tp, T, flag = (None, 0, 0) if table is None else tsi._table_args(table)
    wbuf, wview = guarded(P)
    obuf, oview = guarded(2)  # the total, then the count
    handle = _lib.stream_handle(node.device)
    if stream is not None:
        torch.cuda.synchronize()  # the canaries are filled on the current stream
        handle = ctypes.c_void_p(stream.cuda_stream)
    _lib.check(_lib.lib().come_sgns_o2_loss(
        _lib.ptr(node), _lib.ptr(ctx), V, d, _lib.ptr(walks), P, L, _lib.ptr(seeds), window,
        negative, tp, T, flag, _lib.ptr(wview) if with_walks else None, _lib.ptr(oview),
        _lib.ptr(oview[1:]), handle), "come_sgns_o2_loss")
    if stream is not None:
        stream.synchronize()
    assert intact(wbuf, P) and intact(obuf, 2)
    if not with_walks:
        assert (wview.cpu().numpy() == CANARY).all()
    return (float(oview[0].item()), int(oview.view(torch.int64)[1].item()),
            wview.cpu().numpy() if with_walks else None)


def raw_pairs(inp, out, rin, rpos, neg, with_pairs=True):
    V, d = inp.shape
    M = rin.shape[0]
    n = 0 if neg is None else neg.shape[1]
    pbuf, pview = guarded(M)
    obuf, oview = guarded(2)
    _lib.check(_lib.lib().come_sgns_pairs_loss(
        _lib.ptr(inp), _lib.ptr(out), V, d, _lib.ptr(rin), _lib.ptr(rpos),
        _lib.ptr(neg) if n else None, M, n, _lib.ptr(pview) if with_pairs else None,
        _lib.ptr(oview), _lib.ptr(oview[1:]), _lib.stream_handle(inp.device)),
        "come_sgns_pairs_loss")
    assert intact(pbuf, M) and intact(obuf, 2)
    return (float(oview[0].item()), int(oview.view(torch.int64)[1].item()),
            pview.cpu().numpy() if with_pairs else None)


@functools.lru_cache(maxsize=None)
def twin(d, window, negative, kind="zipf", p=sc.P, length=sc.L, hot=False):
    """The CPU twin's (total, pairs, per walk) of a case, computed once."""
    node, ctx = sc.tables(d)
    walks, seeds = sc.walks_case(p, length, hot=hot)
    total, pairs, per_walk = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative,
                                              sc.neg_table(kind), return_walks=True, threads=4)
    per_walk.setflags(write=False)
    return total, pairs, per_walk


def run_case(d, window, negative, kind="zipf", p=sc.P, length=sc.L, hot=False, numpy_ref=True,
             packed=False):
    node, ctx = (t(a) for a in sc.tables(d))
    walks, seeds = (t(a) for a in sc.walks_case(p, length, hot=hot))
    table = t(sc.neg_table(kind))
    if packed:
        table = tsi.pack_table(table)
        assert table is not None
    total, pairs, per_walk = raw_o2(node, ctx, walks, seeds, window, negative, table)
    ref_total, ref_pairs, ref_walk = twin(d, window, negative, kind, p, length, hot)
    what = "d=%d w=%d n=%d %s P=%d L=%d" % (d, window, negative, kind, p, length)
    rel = np.abs(per_walk - ref_walk) / np.maximum(ref_walk, 1e-300)
    print("%s: vs twin max rel %.3g, total %.6f twin %.6f" % (what, rel[ref_walk > 0].max()
                                                            if (ref_walk > 0).any() else 0.0,
                                                            total, ref_total))
    assert pairs == ref_pairs, what
    assert (np.abs(per_walk - ref_walk) <= 1e-11 * ref_walk).all(), what
    assert abs(total - ref_total) <= 1e-11 * ref_total, what
    if numpy_ref:
        ref, bound, n_pairs = sc.o2_reference(d, window, negative, kind, p, length, hot)
        assert pairs == n_pairs
        assert (np.abs(per_walk - ref) <= bound).all(), what
    return total, pairs, per_walk


@pytest.mark.parametrize("d", sc.WIDTHS + (256,) + sc.GAP_WIDTHS)
def test_parity_sweep(d):
    """Every VEC instantiation, full and ragged rows (GAP_WIDTHS: rows that end two to four
    registers before the instantiation's width); one, two and four chunks of negatives."""
    walks, _ = sc.walks_case()
    for negative in (0, 5, 20):
        _, pairs, _ = run_case(d, 5, negative)
        assert pairs == tsi.count_o2_pairs(np.where(walks >= sc.V, -1, walks), 5)


@pytest.mark.parametrize("window,length", [(0, 40), (1, 40), (31, 40), (32, 40), (100, 40),
                                           (40, 70)])
def test_windows(window, length):
    """Window spans below and above a wavefront's 64 lanes (the last case: entries read per
    pair)."""
    run_case(128, window, 5, length=length)


@pytest.mark.parametrize("kind", ["collision", "oob"])
def test_tables_and_packed_form(kind):
    plain = run_case(100, 5, 5, kind, hot=True)
    packed = run_case(100, 5, 5, kind, hot=True, packed=True)
    assert plain[0] == packed[0] and plain[1] == packed[1]
    assert plain[2].tobytes() == packed[2].tobytes()


def test_more_walks_than_wavefronts_in_flight():
    run_case(64, 2, 2, p=40000, length=4, numpy_ref=False)


@pytest.mark.parametrize("d", [128, 100])
def test_tables_four_byte_aligned(d):
    """node / ctx as views starting one float into their storage."""
    node, ctx = sc.tables(d)
    views = []
    for a in (node, ctx):
        flat = torch.zeros(a.size + 1, dtype=torch.float32, device=dev())
        flat[1:] = t(a).reshape(-1)
        views.append(flat[1:].view(a.shape))
        assert views[-1].data_ptr() % 8 == 4
    walks, seeds = (t(a) for a in sc.walks_case())
    total, pairs, per_walk = raw_o2(views[0], views[1], walks, seeds, 5, 5,
                                    t(sc.neg_table("zipf")))
    ref_total, ref_pairs, ref_walk = twin(d, 5, 5)
    assert pairs == ref_pairs
    assert (np.abs(per_walk - ref_walk) <= 1e-11 * ref_walk).all()


@pytest.mark.parametrize("d", sc.GAP_WIDTHS)
def test_last_row_at_the_end_of_its_allocation(d):
    """Row V - 1 ends where the table's memory ends, and what follows holds 1e30: a lane that read
    past the row's d floats and let the value into a dot would throw the walk's value far off."""
    node, ctx = sc.tables(d)
    views = []
    for a in (node, ctx):
        flat = torch.full((a.size + 512,), 1e30, dtype=torch.float32, device=dev())
        flat[:a.size] = t(a).reshape(-1)
        views.append(flat[:a.size].view(a.shape))
    walks = np.array(sc.walks_case()[0])
    walks[4:, 2] = sc.V - 1  # most walks visit the last row, as centre and as partner
    seeds = sc.walks_case()[1]
    table = np.array(sc.neg_table("zipf"))
    table[-400:] = sc.V - 1  # and draw it as a negative
    total, pairs, per_walk = raw_o2(views[0], views[1], t(walks), t(seeds), 5, 5, t(table))
    t_total, t_pairs, t_walk = cpu.sgns_o2_loss(node, ctx, walks, seeds, 5, 5, table,
                                                return_walks=True)
    assert pairs == t_pairs
    assert (np.abs(per_walk - t_walk) <= 1e-11 * t_walk).all()
    last = np.full(64, sc.V - 1, np.int32)
    total, counted, per_pair = raw_pairs(views[0], views[1], t(last), t(last),
                                         t(np.full((64, 5), sc.V - 1, np.int32)))
    t_total, _, t_pair = cpu.sgns_pairs_loss(node, ctx, last, last,
                                             np.full((64, 5), sc.V - 1, np.int32),
                                             return_pairs=True)
    assert counted == 64 and (np.abs(per_pair - t_pair) <= 1e-11 * t_pair).all()


def test_determinism_and_stray_writes():
    d, window, negative = 200, 5, 5
    host = sc.tables(d) + sc.walks_case() + (sc.neg_table("zipf"),)
    node, ctx, walks, seeds, table = (t(a) for a in host)
    a = raw_o2(node, ctx, walks, seeds, window, negative, table)
    b = raw_o2(node, ctx, walks, seeds, window, negative, table)
    c = raw_o2(node, ctx, walks, seeds, window, negative, table, with_walks=False)
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    s = raw_o2(node, ctx, walks, seeds, window, negative, table, stream=side)
    assert a[0] == b[0] == c[0] == s[0] and a[1] == b[1] == c[1] == s[1]
    assert a[2].tobytes() == b[2].tobytes() == s[2].tobytes()
    for dev_t, h in zip((node, ctx, walks, seeds, table), host):
        assert dev_t.cpu().numpy().tobytes() == h.tobytes()
    # P > 0 without a pair: 0.0 and 0 are written
    z = raw_o2(node, ctx, walks[1:3].contiguous(), seeds[1:3].contiguous(), window, negative,
               table)
    assert z[0] == 0.0 and z[1] == 0 and (z[2] == 0.0).all()


@functools.lru_cache(maxsize=None)
def heldout_lists():
    walks, _ = sc.walks_case(400, 40, seed=9)
    walks = np.where(walks >= sc.V, -1, walks)
    rin, rpos, neg = heldout_o2_pairs(walks, 5, 5, sc.neg_table("zipf"), 5000, 24)
    out = rin.astype(np.int32), rpos.astype(np.int32), np.ascontiguousarray(neg, np.int32)
    for a in out:
        a.setflags(write=False)
    return out


def test_pairs_entry_equals_twin_and_tierc():
    d = 128
    rin, rpos, neg = heldout_lists()
    node, ctx = sc.tables(d)
    total, counted, per_pair = raw_pairs(t(node), t(ctx), t(rin), t(rpos), t(neg))
    t_total, t_counted, t_pair = cpu.sgns_pairs_loss(node, ctx, rin, rpos, neg, return_pairs=True)
    assert counted == t_counted == len(rin)
    assert (np.abs(per_pair - t_pair) <= 1e-11 * t_pair).all()
    assert abs(total - t_total) <= 1e-11 * t_total
    ref, bound = sc.pair_values(d, rin.astype(np.int64), rpos.astype(np.int64),
                                neg.astype(np.int64), np.ones(neg.shape, bool))
    assert (np.abs(per_pair - ref) <= bound).all()
    assert abs(total - sgns_loss(node, ctx, rin, rpos, neg) * len(rin)) <= bound.sum()
    # the total does not depend on pair_out; two runs are bitwise equal
    again = raw_pairs(t(node), t(ctx), t(rin), t(rpos), t(neg), with_pairs=False)
    assert again[0] == total and again[1] == counted


@pytest.mark.parametrize("d", (128, 63, 512) + sc.GAP_WIDTHS)
def test_pairs_entry_invalid_rows_collisions_and_o1_form(d):
    rin, rpos, neg = (np.array(a[:300]) for a in heldout_lists())
    node, ctx = sc.tables(d)
    rin[5], rpos[9], rin[11] = -1, sc.V, sc.V + 3          # dropped pairs
    neg[20, 2], neg[21, 0] = -7, sc.V                      # skipped negatives
    neg[30, 1] = rpos[30]                                  # counted as given
    total, counted, per_pair = raw_pairs(t(node), t(ctx), t(rin), t(rpos), t(neg))
    t_total, t_counted, t_pair = cpu.sgns_pairs_loss(node, ctx, rin, rpos, neg, return_pairs=True)
    assert counted == t_counted == 297 and (per_pair[[5, 9, 11]] == 0.0).all()
    assert (np.abs(per_pair - t_pair) <= 1e-11 * t_pair).all()
    assert abs(total - t_total) <= 1e-11 * t_total
    # no negatives, inp is out (O1's form)
    x = t(node)
    total, counted, per_pair = raw_pairs(x, x, t(rin), t(rpos), None)
    t_total, t_counted, t_pair = cpu.sgns_pairs_loss(node, node, rin, rpos, return_pairs=True)
    assert counted == t_counted == 297
    assert (np.abs(per_pair - t_pair) <= 1e-11 * t_pair).all()


def _model(V=200, d=64):
    from come_amd.model import Model
    st = np.random.get_state()
    m = Model((np.arange(1, V + 1), np.arange(1, V + 1) % 7 + 1), size=d, table_size=5000, k=2,
              device=dev())
    np.random.set_state(st)
    rng = np.random.RandomState(2)
    m.context_embedding = t(rng.uniform(-1, 1, (V, d)).astype(np.float32))
    return m


def test_context2vec_loss():
    from come_amd.context_embeddings import Context2Vec
    from come_amd.embedding import walks_to_rows
    m = _model()
    rng = np.random.RandomState(3)
    paths = rng.randint(1, 201, (50, 12))
    c2v = Context2Vec(window_size=3, negative=4, batch_walks=7)
    state = np.random.get_state()
    small = c2v.loss(m, paths, alpha=0.5)
    after = np.random.get_state()
    assert state[0] == after[0] and (state[1] == after[1]).all() and state[2:] == after[2:]
    big = Context2Vec(window_size=3, negative=4, batch_walks=1 << 20).loss(m, paths, alpha=0.5)
    assert abs(small - big) <= 1e-12 * abs(big)
    # the same value straight from the entry, with the seeds loss() takes by default
    ab = np.random.RandomState(0).randint(0, 2 ** 24, size=100).astype(np.uint64)
    seeds = (ab[0::2] << np.uint64(24)) + ab[1::2]
    rows = walks_to_rows(m, paths)
    rows = rows if isinstance(rows, torch.Tensor) else t(rows)
    total, pairs = tsi.sgns_o2_loss(m.node_embedding, m.context_embedding, rows, t(seeds), 3, 4,
                                    m.negative_table())
    assert pairs == tsi.count_o2_pairs(rows.cpu().numpy(), 3) and pairs > 0
    assert big == 0.5 * total
    assert c2v.loss(m, paths, alpha=0.5, mean=True) == pytest.approx(small / pairs, rel=1e-12)
    assert c2v.loss(m, paths, alpha=0.5, return_pairs=True) == (small, pairs)
    # explicit seeds are used; return_walks adds up to the total
    other = c2v.loss(m, paths, seeds=seeds + np.uint64(1))
    assert other != 2 * small
    total, pairs, per_walk = tsi.sgns_o2_loss(m.node_embedding, m.context_embedding, rows,
                                              t(seeds), 3, 4, m.negative_table(),
                                              return_walks=True)
    assert abs(float(per_walk.sum()) - total) <= 1e-12 * total


def test_node2vec_native_loss_matches_torch():
    from come_amd.node_embeddings import Node2Vec
    m = _model(V=300, d=100)
    rng = np.random.RandomState(4)
    edges = rng.randint(1, 301, (2000, 2))
    edges[7] = (5, 9999)  # an endpoint outside the vocabulary: the edge is skipped by both
    n2v = Node2Vec()
    ref = n2v.loss(m, edges)
    got = n2v.loss(m, edges, backend='native')
    x = m.node_embedding.cpu().numpy().astype(np.float64)
    rows = n2v._edge_rows(m, edges)
    rows = rows[(rows >= 0).all(1)]
    # both sum fp32 dots (in different orders) of the same rows: twice the derived dot bound
    bound = 2 * sc.dot_bound_factor(100) * (np.abs(x[rows[:, 0]]) * np.abs(x[rows[:, 1]])).sum()
    print("Node2Vec.loss torch %.6f native %.6f bound %.3g" % (ref, got, bound))
    assert abs(got - ref) <= bound + 1e-12 * ref
    with pytest.raises(ValueError):
        n2v.loss(m, edges, backend='triton')
