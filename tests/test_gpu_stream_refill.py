"""The Hogwild O2 kernel (k_sgns_o2_stream) across draw refills, re-read rows and walk ends.

The kernel keeps 128 draws per wavefront in two batches of 64 and refills one every 64 draws, keeps
one pair of rows in flight, and after a *general* pair (tests/test_gpu_stream_paths.py) at
d <= 128 waits for its write-backs and reads the next pair's rows again instead of patching the
copies it holds.  Here several walks of very different lengths share one launch (a wavefront's
draw and prefetch state starts afresh with every walk), n runs over values that let a pair's draws
straddle the two batches at every alignment, and general pairs fall on refills and on walk ends.

Bars, as tests/test_gpu_stream_paths.py: Hogwild mode with max_waves=1 equals the sequential
oracle (WAVE64 dot order) BIT FOR BIT, update counter included; with contended rows (float-atomic
deltas) tier B, <= 1e-3 abs and > 95% of the elements within 1e-5, and two launches from the same
tables agree bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

import come_amd.training_sdg_inner as tsi

from test_gpu_stream_paths import (DEV, LR, aliased_corpus, check_exact, classify, dev, lcg_slots,
                                   oracle, pairs_of, run, tables)

pytestmark = pytest.mark.gpu
SHAPES = [(128, 5), (128, 3), (128, 1), (100, 5), (64, 5), (256, 10), (256, 7), (128, 0)]
LENS = (3, 40, 2, 40, 13, 40)  # fewer than 64 draws in all between walks with many refills
L, W = 40, 5
V_BIG, T_BIG, ROWS = 4096, 16_000_057, 128  # 11,100 draws at n = 10, each its own slot


def padded(rows_of_walk):
    walks = np.full((len(rows_of_walk), L), -1, np.int32)
    for p, r in enumerate(rows_of_walk):
        walks[p, :len(r)] = r
    return walks


def owned(n, kinds, seed):
    """len(LENS) walks on V_BIG rows, walk p on its own rows [128p, 128p + 128): distinct positions
    among the first 64, plain draws cycled through the last 63 (no repeat within 63 draws
    >= 2 (n + 1)), aliased draws from 3 rows: the walk's last two nodes and row 128p + 64.
    kinds(p, q, npairs): pair q of walk p draws aliased.  Each walk owns its table slots (seeds
    re-drawn until they are free), so every draw is exactly the intended row."""
    rng = np.random.RandomState(300 + seed)
    walks = padded([ROWS * p + rng.permutation(64)[:m] for p, m in enumerate(LENS)])
    table = np.zeros(T_BIG, np.uint32)
    owner = np.zeros(T_BIG, bool)
    seeds = np.zeros(len(LENS), np.uint64)
    for p, m in enumerate(LENS):
        npairs = len(pairs_of(walks[p], W, V_BIG))
        for _ in range(400):
            seed_p = np.uint64(rng.randint(0, 2 ** 48, dtype=np.int64))
            slots = lcg_slots(seed_p, npairs * n, T_BIG)
            if len(np.unique(slots)) == len(slots) and not owner[slots].any():
                break
        else:
            raise AssertionError("could not place walk %d" % p)
        owner[slots] = True
        seeds[p] = seed_p
        pool = ROWS * p + 65 + rng.permutation(63)
        three = np.array([walks[p, m - 1], walks[p, m - 2], ROWS * p + 64])
        vals, c = [], 0
        for q in range(npairs):
            if kinds(p, q, npairs):
                tk = three[rng.randint(0, 3, n)]
                tk[-1:] = tk[:1]  # n >= 2: at least one repeat, whatever the next pair draws
                vals.extend(tk)
            else:
                vals.extend(pool[(c + np.arange(n)) % 63])
                c += n
        table[slots] = np.array(vals, np.uint32)
    return walks, seeds, table


@functools.lru_cache(maxsize=2)  # a table is 64 MB
def plain_corpus(n):
    return owned(n, lambda p, q, m: False, 0)


@functools.lru_cache(maxsize=2)  # a table is 64 MB
def alternating_corpus(n):
    """Even walks: aliased draws in pairs 0, 2, 4, ... and in the last pair; odd walks: in pairs
    1, 3, ... -- an aliased last pair of walk p is followed by a plain first pair of walk p + 1."""
    return owned(n, lambda p, q, m: (q % 2 == 0 or q == m - 1) if p % 2 == 0 else q % 2 == 1, 1)


def small_corpus(V, n, seed):
    """The same walk lengths on V = 40 rows with a 61-slot table: nearly every pair is general."""
    rng = np.random.RandomState(400 + seed)
    walks = padded([rng.randint(0, V, m) for m in LENS])
    table = rng.randint(0, V, 61).astype(np.uint32)
    seeds = rng.randint(0, 2 ** 48, len(LENS), dtype=np.int64).astype(np.uint64)
    return walks, seeds, table


@pytest.mark.parametrize("d,n", SHAPES)
def test_refills_on_plain_pairs(d, n):
    walks, seeds, table = plain_corpus(n)
    flags = classify(walks, seeds, table, W, n, V_BIG)
    assert [len(f) for f in flags] == [len(pairs_of(wk, W, V_BIG)) for wk in walks]
    assert all(all(f[:-1]) for f in flags)  # every pair but a walk's last (no next pair)
    draws = [len(f) * n for f in flags]
    if n > 0:
        assert draws[0] < 64 and draws[2] < 64 and min(draws[1], draws[3], draws[5]) > 5 * 64
    check_exact(V_BIG, d, walks, seeds, W, n, table)


@pytest.mark.parametrize("d,n", SHAPES)
def test_refills_on_general_pairs(d, n):
    V = 40
    walks, seeds, table = small_corpus(V, n, n)
    flags = classify(walks, seeds, table, W, n, V)
    if n > 1:  # a refill every 64 / n pairs: general pairs fall on many of them
        assert sum(not x for f in flags for x in f) > 0.3 * sum(len(f) for f in flags)
    check_exact(V, d, walks, seeds, W, n, table)


@pytest.mark.parametrize("d,n", SHAPES)
def test_general_and_plain_pairs_alternate_across_refills_and_walk_ends(d, n):
    walks, seeds, table = alternating_corpus(n)
    flags = classify(walks, seeds, table, W, n, V_BIG)
    if n > 1:
        for p, f in enumerate(flags):
            want = [(q % 2 == 0 or q == len(f) - 1) if p % 2 == 0 else q % 2 == 1
                    for q in range(len(f))]
            assert not any(x for x, a in zip(f, want) if a)  # aliased draws: general
            if len(f) > 4:
                assert any(f)
        assert not flags[0][-1] and flags[1][0]  # general last pair, then a plain first pair
        assert flags[1][0] and not flags[1][1] and flags[1][2]
    check_exact(V_BIG, d, walks, seeds, W, n, table)


@pytest.mark.parametrize("hot_kind", ["all", "alternate"])
@pytest.mark.parametrize("d,n", [(128, 5), (100, 5), (64, 5), (256, 10)])
def test_hot_rows_through_the_reread(d, n, hot_kind):
    """Every pair aliased, its rows hot: what a general pair reads again was just changed by its own
    float atomics.  Tier B against the oracle; a re-read that raced its own atomic or store would
    make two launches differ."""
    V = 64
    walks, seeds, table = aliased_corpus(V, n, W, P=6, L=L)
    word = -1 if hot_kind == "all" else 0x55555555
    hot = torch.full(((V + 31) // 32,), word, dtype=torch.int32, device=DEV)
    node0, ctx0 = tables(V, d, d + n)
    got = run(node0, ctx0, walks, seeds, W, n, table, hot=hot)
    again = run(node0, ctx0, walks, seeds, W, n, table, hot=hot)
    ref = oracle(node0, ctx0, walks, seeds, W, n, table)
    for a, b in zip(got[:2], ref[:2]):
        diff = np.abs(a - b)
        assert diff.max() <= 1e-3, diff.max()                    # tier B
        assert np.mean(diff <= 1e-5) > 0.95, np.mean(diff <= 1e-5)
    np.testing.assert_array_equal(got[0], again[0])
    np.testing.assert_array_equal(got[1], again[1])
    assert got[2] == again[2]


GUARD = 128  # rows behind the tables' V rows: allocated, never to be touched


def run_guarded(node0, ctx0, walks, seeds, n, table):
    """run() on the first V rows of tables that have GUARD more rows behind them."""
    V = len(node0)
    rng = np.random.RandomState(7)
    full = [dev(np.concatenate([t, rng.uniform(-1, 1, (GUARD, t.shape[1])).astype(np.float32)]))
            for t in (node0, ctx0)]
    before = [t[V:].clone() for t in full]
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    tsi.sgns_o2(full[0][:V], full[1][:V], dev(walks), dev(seeds), W, n, dev(table), LR, 1.0,
                tsi.MODE_HOGWILD, opts={"o2_kernel": 3, "max_waves": 1}, update_count=cnt,
                hot=None)
    torch.cuda.synchronize()
    for t, b in zip(full, before):
        assert torch.equal(t[V:], b)  # no row past V written
    return full[0][:V].cpu().numpy(), full[1][:V].cpu().numpy(), int(cnt.item())


@pytest.mark.parametrize("corpus", ["plain", "general"])
@pytest.mark.parametrize("d,n", [(128, 3), (256, 7), (128, 0)])
def test_fewer_negatives_than_the_kernel_holds_and_bad_table_values(d, n, corpus):
    """n below the instantiation's MAXN (5, 10), some table slots holding values >= V: such a draw
    is consumed and skipped, and neither it nor a lane past n reaches a row.  The reference: the
    oracle has no range test, so it gets the rows the bad values name, each with a context row
    whose dot with any input row is far past +-6 (the bad rows are 1e6 e_0, every input row starts
    with |x_0| >= 0.5) -- pyx:141 then skips the target: no update, no count, nothing added to
    `work`.  That the oracle did skip every one of them is asserted: its bad rows stay as given."""
    if corpus == "plain":
        V = V_BIG
        walks, seeds, table = plain_corpus(n)
    else:
        V = 40
        walks, seeds, table = small_corpus(V, n, n)
    table = table.copy()
    used = np.unique(np.concatenate([lcg_slots(s, len(pairs_of(wk, W, V)) * n, len(table))
                                     for wk, s in zip(walks, seeds)])) if n else np.array([], int)
    bad = used[::5]
    table[bad[0::2]] = V + 3
    table[bad[1::2]] = V + 100
    node0, ctx0 = tables(V, d, d + n)
    node0[:, 0] = np.where(node0[:, 0] < 0, -1.0, 1.0) * (0.5 + 0.5 * np.abs(node0[:, 0]))
    got = run_guarded(node0, ctx0, walks, seeds, n, table)
    node_x = np.concatenate([node0, np.zeros((101, d), np.float32)])
    ctx_x = np.concatenate([ctx0, np.zeros((101, d), np.float32)])
    ctx_x[V:, 0] = 1e6
    ref = oracle(node_x, ctx_x, walks, seeds, W, n, table)
    np.testing.assert_array_equal(ref[1][V:], ctx_x[V:])  # the oracle skipped every bad target
    np.testing.assert_array_equal(got[0], ref[0][:V])
    np.testing.assert_array_equal(got[1], ref[1][:V])
    assert got[2] == ref[2]
    assert n == 0 or len(bad) > 0
