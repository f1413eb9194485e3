"""The SGNS losses on the host (no GPU): the CPU twins come_cpu_sgns_o2_loss /
come_cpu_sgns_pairs_loss against the float64 numpy restatement of tests/sgns_loss_cases.py (its
docstring derives the bound), the skip rules, thread independence, the held-out loss of
tests/tierc_inputs.py, walks against lists, the trainer's objective, and argument validation.
"""
import ctypes

import numpy as np
import pytest

from come_amd import _lib, cpu
from come_amd import training_sdg_inner as tsi
import sgns_loss_cases as sc
from tierc_inputs import heldout_o2_pairs, sgns_loss


def check_walks(got, ref, bound, what):
    worst = np.max(np.abs(got - ref) / np.maximum(bound, 1e-300))
    print("%s: max |diff| / bound %.3g (max |diff| %.3g)" % (what, worst, np.abs(got - ref).max()))
    assert (np.abs(got - ref) <= bound).all(), what


@pytest.mark.parametrize("d", sc.WIDTHS)
def test_o2_twin_matches_float64_numpy(d):
    node, ctx = sc.tables(d)
    walks, seeds = sc.walks_case()
    table = sc.neg_table("zipf")
    in_range = np.where(walks >= sc.V, -1, walks)  # come_count_o2_pairs does not know V
    for negative in (0, 1, 5, 20):
        for window in (0, 1, 5, 40):
            ref, bound, pairs_ref = sc.o2_reference(d, window, negative)
            total, pairs, per_walk = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative,
                                                      table, return_walks=True, threads=1)
            what = "d=%d n=%d w=%d" % (d, negative, window)
            assert pairs == pairs_ref == tsi.count_o2_pairs(in_range, window), what
            check_walks(per_walk, ref, bound, what)
            assert abs(total - ref.sum()) <= bound.sum(), what
            assert per_walk[1] == 0.0 and per_walk[2] == 0.0  # the all -1 and one-node walks
            if window == 0:
                assert total == 0.0 and pairs == 0


@pytest.mark.parametrize("kind", ["collision", "oob"])
def test_skip_rules(kind):
    """A draw equal to the positive row, or outside [0, V), is consumed and skipped."""
    d, window, negative = 100, 5, 5
    walk, rin, rpos, draws, used = sc.o2_enumeration(window, negative, kind, hot=True)
    if kind == "collision":
        assert (draws == rpos[:, None]).sum() >= 1  # the restatement did skip collisions
    else:
        assert (draws >= sc.V).sum() >= 1
    assert (~used).sum() >= 1
    node, ctx = sc.tables(d)
    walks, seeds = sc.walks_case(hot=True)
    ref, bound, pairs_ref = sc.o2_reference(d, window, negative, kind, hot=True)
    total, pairs, per_walk = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative,
                                              sc.neg_table(kind), return_walks=True, threads=1)
    assert pairs == pairs_ref
    check_walks(per_walk, ref, bound, kind)
    # counting the skipped draws would leave the bound: the rule is observable
    val_all, _ = sc.pair_values(d, rin, rpos, np.minimum(draws, sc.V - 1), draws >= 0)
    assert abs(val_all.sum() - ref.sum()) > 10 * bound.sum()


def test_threads_reproducibility_and_read_only():
    d, window, negative, p = 65, 5, 5, 200  # >= 64 walks: the twin really splits them
    node, ctx = (a.copy() for a in sc.tables(d))
    walks, seeds = sc.walks_case(p)
    table = sc.neg_table("zipf").copy()
    before = [a.copy() for a in (node, ctx, walks, seeds, table)]
    t1, p1, w1 = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table, True, 1)
    t4, p4, w4 = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table, True, 4)
    t4b, _, w4b = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table, True, 4)
    t4c, p4c = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table, False, 4)
    assert w1.tobytes() == w4.tobytes() == w4b.tobytes()
    assert p1 == p4 == p4c and t4 == t4b == t4c  # bitwise for a fixed `threads`
    assert abs(t1 - t4) <= 1e-12 * abs(t1)
    for a, b in zip((node, ctx, walks, seeds, table), before):
        assert a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def heldout():
    """heldout_o2_pairs-shaped lists: M = 5000 pairs of held-out walks, n = 5, d = 128."""
    walks, _ = sc.walks_case(400, 40, seed=9)
    walks = np.where(walks >= sc.V, -1, walks)  # tierc_inputs.sgns_loss indexes unchecked
    rin, rpos, neg = heldout_o2_pairs(walks, 5, 5, sc.neg_table("zipf"), 5000, 24)
    assert len(rin) == 5000
    return rin.astype(np.int32), rpos.astype(np.int32), np.ascontiguousarray(neg, np.int32)


def test_pairs_twin_equals_tierc_heldout_loss(heldout):
    d = 128
    rin, rpos, neg = heldout
    node, ctx = sc.tables(d)
    M = len(rin)
    total, counted, per_pair = cpu.sgns_pairs_loss(node, ctx, rin, rpos, neg, return_pairs=True,
                                                   threads=3)
    ref, bound = sc.pair_values(d, rin.astype(np.int64), rpos.astype(np.int64),
                                neg.astype(np.int64), np.ones(neg.shape, bool))
    assert counted == M
    check_walks(per_pair, ref, bound, "held-out pairs")
    tierc = sgns_loss(node, ctx, rin, rpos, neg) * M
    print("pairs twin %.6f tierc %.6f bound %.3g" % (total, tierc, bound.sum()))
    assert abs(total - tierc) <= bound.sum()
    assert (neg == rpos[:, None]).sum() >= 1  # a negative equal to the positive is in the lists


def test_pairs_twin_invalid_rows_and_collisions(heldout):
    d = 128
    rin, rpos, neg = (a[:300].copy() for a in heldout)
    node, ctx = sc.tables(d)
    rin[5], rpos[9], rin[11] = -1, sc.V, sc.V + 3          # dropped pairs
    neg[20, 2], neg[21, 0] = -7, sc.V                      # skipped negatives
    neg[30, 1] = rpos[30]                                  # counted as given
    total, counted, per_pair = cpu.sgns_pairs_loss(node, ctx, rin, rpos, neg, return_pairs=True)
    keep = np.ones(300, bool)
    keep[[5, 9, 11]] = False
    used = (neg >= 0) & (neg < sc.V)
    ref, bound = sc.pair_values(d, np.where(keep, rin, 0).astype(np.int64),
                                np.where(keep, rpos, 0).astype(np.int64), neg.astype(np.int64),
                                used)
    ref, bound = np.where(keep, ref, 0.0), np.where(keep, bound, 0.0)
    assert counted == 297 and (per_pair[~keep] == 0.0).all()
    check_walks(per_pair, ref, bound, "edited lists")
    assert abs(total - ref.sum()) <= bound.sum()
    # the collision is counted: without it pair 30 would be lower by a whole term
    G, _ = sc.grams(d)
    assert abs(per_pair[30] - ref[30]) < 0.1 * np.logaddexp(0.0, G[rin[30], rpos[30]])
    # no negatives at all, inp is out (O1's form)
    t0, c0 = cpu.sgns_pairs_loss(node, node, rin, rpos)
    n64 = node.astype(np.float64)
    ref0 = np.logaddexp(0.0, -(n64 @ n64.T)[rin[keep], rpos[keep]]).sum()
    bound0 = sc.dot_bound_factor(d) * (np.abs(n64) @ np.abs(n64).T)[rin[keep], rpos[keep]].sum()
    assert c0 == 297 and abs(t0 - ref0) <= bound0 + 1e-12 * ref0


@pytest.mark.parametrize("kind", ["zipf", "collision"])
def test_walk_entry_equals_pairs_entry_on_its_own_lists(kind):
    """The lists the walk entry enumerates -- pairs in order, negatives from come_lcg_table_draws,
    collisions set to -1 -- give the same per-walk sums through the pairs entry."""
    d, window, negative = 200, 5, 5
    node, ctx = sc.tables(d)
    walks, seeds = sc.walks_case(hot=True)
    table = sc.neg_table(kind)
    walk, rin, rpos, draws, used = sc.o2_enumeration(window, negative, kind, hot=True)
    for p in range(sc.P):  # the library's own draw helper agrees with the restated LCG
        mine = draws[walk == p].reshape(-1)
        out = np.empty(len(mine), np.uint32)
        if len(mine):
            _lib.check(_lib.lib().come_lcg_table_draws(int(seeds[p]), len(mine), _lib.ptr(table),
                                                       len(table), _lib.ptr(out)), "draws")
        assert (out == mine).all()
    neg = np.where(draws == rpos[:, None], -1, draws).astype(np.int32)
    _, pairs, per_walk = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table,
                                          return_walks=True)
    _, counted, per_pair = cpu.sgns_pairs_loss(node, ctx, rin.astype(np.int32),
                                               rpos.astype(np.int32), neg, return_pairs=True)
    assert counted == pairs == len(walk)
    sums = np.zeros(sc.P)
    for p, v in zip(walk, per_pair):  # in pair order, as the walk entry adds them
        sums[p] += v
    assert (np.abs(sums - per_walk) <= 1e-12 * np.abs(per_walk)).all()


@pytest.mark.parametrize("cfg", [(50, 8, 20, 12, 3, 4, 0.025), (40, 16, 30, 10, 5, 5, 0.1),
                                 (64, 130, 16, 20, 2, 3, 0.025)])
def test_loss_is_the_objective_the_trainer_descends(cfg):
    """One sequential come_cpu_sgns_o2 pass lowers the loss of the same walks and seeds (a numpy
    simulation of the reference update gave 3273.7 -> 3264.3, 7631.5 -> 4275.4, 2644.5 ->
    2112.3 on these configurations)."""
    v, d, p, length, window, negative, lr = cfg
    rng = np.random.RandomState(v + d)
    node = rng.uniform(-1, 1, (v, d)).astype(np.float32)
    ctx = rng.uniform(-1, 1, (v, d)).astype(np.float32)
    share = 1.0 / np.arange(1, v + 1) ** 0.75
    table = rng.choice(v, 5003, p=share / share.sum()).astype(np.uint32)
    table.sort()
    walks = rng.randint(0, v, (p, length)).astype(np.int32)
    seeds = rng.randint(0, 2 ** 48, p, dtype=np.int64).astype(np.uint64)
    before, pairs = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table)
    trained = cpu.sgns_o2(node, ctx, walks, seeds, window, negative, table, lr, 1.0,
                          cpu.MODE_SEQUENTIAL, 1)
    after, pairs2 = cpu.sgns_o2_loss(node, ctx, walks, seeds, window, negative, table)
    print("cfg %s: %.1f -> %.1f over %d pairs" % (cfg, before, after, pairs))
    assert pairs == pairs2 == trained
    assert after < before


def test_validation_without_a_device():
    L = _lib.lib()
    p, q = ctypes.c_void_p(0), ctypes.c_void_p(16)
    for gpu in (True, False):
        tail = (0, q, q, q, q) if gpu else (q, q, q, 1)
        f = L.come_sgns_o2_loss if gpu else L.come_cpu_sgns_o2_loss

        def call(**k):
            args = [k.get(n, v) for n, v in (
                ("node", q), ("ctx", q), ("V", 10), ("d", 8), ("walks", q), ("P", 1), ("L", 10),
                ("seeds", q), ("window", 5), ("negative", 5), ("table", q), ("T", 10))]
            t = list(tail)
            if "loss_out" in k:
                t[2 if gpu else 1] = k["loss_out"]
            if "flags" in k and gpu:
                t[0] = k["flags"]
            return f(*(args + t))
        for kw, msg in (({"V": 0}, b"V must be"), ({"V": 1 << 31}, b"V must fit"),
                        ({"d": 0}, b"d must be"), ({"d": 513}, b"d must be"),
                        ({"negative": 21}, b"negative must be"), ({"negative": -1}, b"negative"),
                        ({"table": p}, b"non-empty table"), ({"T": 0}, b"non-empty table"),
                        ({"P": -1}, b"must be >= 0"), ({"window": -1}, b"must be >= 0"),
                        ({"L": 10001}, b"L must be <= 10000"), ({"node": p}, b"null"),
                        ({"seeds": p}, b"null"), ({"walks": p}, b"null"),
                        ({"loss_out": p}, b"null")):
            assert call(**kw) == -1 and msg in L.come_last_error(), (gpu, kw)
        assert call(P=0, node=p, ctx=p, walks=p, seeds=p, loss_out=p) == 0  # a no-op
        if gpu:
            assert call(flags=7) == -1 and b"flags" in L.come_last_error()
            assert call(flags=_lib.TABLE_PACKED, table=ctypes.c_void_p(8)) == -1
            assert b"16-byte aligned" in L.come_last_error()
        else:
            assert f(q, q, 10, 8, q, 1, 10, q, 5, 5, q, 10, q, q, q, 0) == -1
            assert b"threads" in L.come_last_error()
    for gpu in (True, False):
        f = L.come_sgns_pairs_loss if gpu else L.come_cpu_sgns_pairs_loss
        last = q if gpu else 1

        def pcall(**k):
            return f(*[k.get(n, v) for n, v in (
                ("inp", q), ("out", q), ("V", 10), ("d", 8), ("rows_in", q), ("rows_pos", q),
                ("rows_neg", q), ("M", 3), ("negative", 2), ("pair_out", q), ("loss_out", q),
                ("pairs_out", q), ("last", last))])
        for kw, msg in (({"V": -3}, b"V must be"), ({"d": 600}, b"d must be"),
                        ({"negative": 30}, b"negative must be"), ({"M": -1}, b"M must be"),
                        ({"inp": p}, b"null"), ({"rows_pos": p}, b"null"),
                        ({"rows_neg": p}, b"null"), ({"loss_out": p}, b"null")):
            assert pcall(**kw) == -1 and msg in L.come_last_error(), (gpu, kw)
        assert pcall(M=0, inp=p, out=p, rows_in=p, rows_pos=p, loss_out=p) == 0
