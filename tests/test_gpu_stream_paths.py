"""The two per-pair paths of the Hogwild O2 kernel (k_sgns_o2_stream) and the switch between them.

A pair is *plain* when no context-table row of it repeats, equals its center, or is a row of the
next pair, every draw is a row of the table, and the next pair's input row is another one; a plain
pair skips the duplicate scan and the patches of prefetched copies and takes all its sigmoids in
one vector step.  Every other pair takes the general body.  Here the corpora are built so that
every pair is aliased, every pair is plain, or the two alternate inside a walk (`classify` restates
the kernel's test on the CPU and the tests assert what they built before they launch).

Bars, as tests/test_gpu_stream.py::test_one_wavefront_bit_exact_with_shared_rows: the streaming
kernel in Hogwild mode with max_waves=1 (one wavefront takes the walks in order) equals the
sequential oracle (WAVE64 dot order) BIT FOR BIT, and its update counter equals the oracle's; with
contended rows (float-atomic deltas) tier B, <= 1e-3 abs and > 95% of the elements within 1e-5, as
test_gpu_stream.py::test_one_wavefront_contended_rows_tier_b.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as orc

import come_amd.training_sdg_inner as tsi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LCG_MUL, LCG_ADD, MASK48 = np.uint64(25214903917), np.uint64(11), np.uint64((1 << 48) - 1)
SHAPES = [(128, 5), (128, 3), (100, 5), (64, 5), (256, 10), (256, 7), (128, 0)]
LR = 0.05


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def lcg_slots(seed, count, T):
    """Table slots of `count` consecutive draws from `seed` (pyx:133-134)."""
    nr = np.uint64(seed)
    out = np.empty(count, np.int64)
    with np.errstate(over="ignore"):
        for k in range(count):
            out[k] = int((nr >> np.uint64(16)) % np.uint64(T))
            nr = (nr * LCG_MUL + LCG_ADD) & MASK48
    return out


def pairs_of(walk, w, V):
    """(center row, input row) of a walk's pairs in the kernel's order (pyx:494-508)."""
    L = len(walk)
    out = []
    for i in range(L):
        if not 0 <= walk[i] < V:
            continue
        for j in range(max(0, i - w), min(L, i + w + 1)):
            if j != i and 0 <= walk[j] < V:
                out.append((int(walk[i]), int(walk[j])))
    return out


def classify(walks, seeds, table, w, n, V):
    """Per walk, per pair: True = plain by the kernel's definition (the last pair of a walk has
    no next pair and is general)."""
    res = []
    for walk, seed in zip(walks, seeds):
        pr = pairs_of(walk, w, V)
        t = table[lcg_slots(seed, len(pr) * n, len(table))].astype(np.int64).reshape(len(pr), n)
        flags = []
        for q, (ci, cj) in enumerate(pr):
            if q + 1 == len(pr):
                flags.append(False)
                continue
            nci, ncj = pr[q + 1]
            cur, nxt = list(t[q]), list(t[q + 1])
            flags.append(ncj != cj and len(set(cur)) == n and ci not in cur and ci not in nxt
                         and all(0 <= x < V for x in cur)
                         and not (set(cur) & (set(nxt) | {nci})))
        res.append(flags)
    return res


def tables(V, d, seed):
    rng = np.random.RandomState(seed)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    node0[::7] *= 3.0  # some dots past +-6: skipped targets (pyx:141)
    ctx0 = rng.uniform(-0.3, 0.3, (V, d)).astype(np.float32)
    return node0, ctx0


def aliased_corpus(V, n, w=3, P=6, L=12, seed=0):
    """Walks that backtrack (a-b-a-b) or stay among 3 nodes, one with an immediate repeat; every
    draw is one of 3 rows, two of them walk nodes: duplicate negatives, negatives equal to the
    center, to the next pair's center and to the next pair's negatives, in every pair."""
    rng = np.random.RandomState(100 + seed)
    walks = np.empty((P, L), np.int32)
    for p in range(P):
        a, b, c = rng.choice(V, 3, replace=False)
        if p % 2 == 0:
            walks[p] = np.where(np.arange(L) % 2 == 0, a, b)
        else:
            walks[p] = rng.choice([a, b, c], L)
    walks[1, 4] = walks[1, 5]  # the next pair's input row is this pair's
    rows = np.array([walks[0, 0], walks[0, 1], (walks[0, 0] + 1) % V], np.uint32)
    table = rows[rng.randint(0, 3, 61)]
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    return walks, seeds, table


V_BIG, N_WALKS, T_BIG = 4096, 64, 4_000_037


def owned_corpus(n, kinds, w=3, L=8, seed=0, backtrack=()):
    """64 walks on 4,096 rows, walk p on its own rows [64p, 64p + 64): positions among the first 32
    (distinct, or a-b-a-b for the walks in `backtrack`), plain draws from the last 31, cycled (no
    draw repeats within 31 consecutive draws >= 2 (n + 1)), aliased draws from 3 rows: the walk's
    last two nodes and row 64p + 32.  kinds(p, q, npairs) says whether pair q of walk p draws
    aliased.  Each walk owns its table slots (seeds re-drawn until they are free), so the table
    gives every draw exactly the intended row."""
    rng = np.random.RandomState(200 + seed)
    walks = np.empty((N_WALKS, L), np.int32)
    for p in range(N_WALKS):
        nodes = 64 * p + rng.permutation(32)[:L]
        walks[p] = np.where(np.arange(L) % 2 == 0, nodes[0], nodes[1]) if p in backtrack else nodes
    table = np.zeros(T_BIG, np.uint32)
    owner = np.zeros(T_BIG, bool)
    seeds = np.zeros(N_WALKS, np.uint64)
    for p in range(N_WALKS):
        npairs = len(pairs_of(walks[p], w, V_BIG))
        for _ in range(400):
            seed_p = np.uint64(rng.randint(0, 2 ** 48, dtype=np.int64))
            slots = lcg_slots(seed_p, npairs * n, T_BIG)
            if len(np.unique(slots)) == len(slots) and not owner[slots].any():
                break
        else:
            raise AssertionError("could not place walk %d" % p)
        owner[slots] = True
        seeds[p] = seed_p
        pool = 64 * p + 33 + rng.permutation(31)
        three = np.array([walks[p, L - 1], walks[p, L - 2], 64 * p + 32])
        vals, c = [], 0
        for q in range(npairs):
            if kinds(p, q, npairs):
                tk = three[rng.randint(0, 3, n)]
                tk[-1:] = tk[:1]  # at least one repeat, whatever the next pair draws
                vals.extend(tk)
            else:
                vals.extend(pool[(c + np.arange(n)) % 31])
                c += n
        table[slots] = np.array(vals, np.uint32)
    return walks, seeds, table


@functools.lru_cache(maxsize=None)
def plain_corpus(n):
    return owned_corpus(n, lambda p, q, m: False)


@functools.lru_cache(maxsize=None)
def mixed_corpus(n):
    """Walk by walk: p % 4 == 0 all plain, 1 all aliased (p % 8 == 1 backtracking), 2 alternating
    from an aliased first pair to an aliased last pair, 3 alternating from a plain first pair."""
    def kinds(p, q, m):
        return {0: False, 1: True, 2: q % 2 == 0 or q == m - 1, 3: q % 2 == 1}[p % 4]
    return owned_corpus(n, kinds, seed=1, backtrack=set(range(1, N_WALKS, 8)))


def run(node0, ctx0, walks, seeds, w, n, table, hot=None):
    node, ctx = dev(node0), dev(ctx0)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    tsi.sgns_o2(node, ctx, dev(walks), dev(seeds), w, n, dev(table), LR, 1.0, tsi.MODE_HOGWILD,
                opts={"o2_kernel": 3, "max_waves": 1}, update_count=cnt, hot=hot)
    torch.cuda.synchronize()
    return node.cpu().numpy(), ctx.cpu().numpy(), int(cnt.item())


def oracle(node0, ctx0, walks, seeds, w, n, table):
    n_ref, c_ref = node0.copy(), ctx0.copy()
    orc.reset_updates()
    orc.sgns_o2(n_ref, c_ref, walks, seeds, w, n, table, LR, 1.0, dot_mode=orc.DOT_WAVE64)
    return n_ref, c_ref, orc.updates()


def check_exact(V, d, walks, seeds, w, n, table):
    node0, ctx0 = tables(V, d, d + n)
    got = run(node0, ctx0, walks, seeds, w, n, table)
    ref = oracle(node0, ctx0, walks, seeds, w, n, table)
    assert not np.array_equal(ref[0], node0)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
    assert got[2] == ref[2]
    return ref[2]


@pytest.mark.parametrize("d,n", SHAPES)
@pytest.mark.parametrize("V", [8, 64])
def test_every_pair_aliased(V, d, n):
    w = 3
    walks, seeds, table = aliased_corpus(V, n, w)
    flags = classify(walks, seeds, table, w, n, V)
    if n > 0:  # without negatives a pair aliases only through its input row
        assert not any(any(f) for f in flags)
    check_exact(V, d, walks, seeds, w, n, table)


@pytest.mark.parametrize("d,n", SHAPES)
def test_every_pair_plain(d, n):
    w = 3
    walks, seeds, table = plain_corpus(n)
    assert len(np.unique(walks)) == walks.size  # disjoint walks, distinct positions
    for walk, seed in zip(walks, seeds):
        npairs = len(pairs_of(walk, w, V_BIG))
        t = table[lcg_slots(seed, npairs * n, T_BIG)]
        for s in range(max(0, len(t) - 2 * (n + 1) + 1)):  # no repeat in 2 (n + 1) draws
            assert len(set(t[s:s + 2 * (n + 1)])) == 2 * (n + 1)
    flags = classify(walks, seeds, table, w, n, V_BIG)
    assert all(all(f[:-1]) for f in flags)  # every pair but a walk's last (no next pair)
    upd = check_exact(V_BIG, d, walks, seeds, w, n, table)
    targets = sum(len(f) for f in flags) * (1 + n)
    print("target updates %d of %d targets" % (upd, targets))
    assert 0 < upd <= targets


@pytest.mark.parametrize("d,n", SHAPES)
def test_plain_and_aliased_pairs_alternate(d, n):
    w = 3
    walks, seeds, table = mixed_corpus(n)
    flags = classify(walks, seeds, table, w, n, V_BIG)
    if n > 0:
        assert all(all(f[:-1]) for f in flags[0::4]) and not any(any(f) for f in flags[1::4])
        for f in flags[2::4]:  # aliased first and last, alternating in between
            assert not f[0] and not f[-2] and f[1] and not f[2] and f[3]
        for f in flags[3::4]:
            assert f[0] and not f[1] and f[2]
    check_exact(V_BIG, d, walks, seeds, w, n, table)


@pytest.mark.parametrize("d,n", [(128, 5), (256, 10), (100, 5)])
def test_holes_short_walks_and_wide_window(d, n):
    """Walks with -1 entries, walks shorter than the window (w = 5, 1 to 4 valid positions), in
    the mixed corpus: the pairs around a hole change which pair is the next one."""
    w = 5
    walks, seeds, table = mixed_corpus(n)
    walks = walks.copy()
    walks[2, 3] = -1
    walks[3, 0] = -1
    walks[5, 1:3] = -1
    walks[6, 4:] = -1  # 4 valid positions < window
    walks[7, 2:] = -1
    walks[9, 1:] = -1  # one position: no pair
    walks[10, :] = -1
    check_exact(V_BIG, d, walks, seeds, w, n, table)


def test_walks_of_one_position():
    """L = 1: no pair, nothing written, no update counted."""
    walks, seeds, table = mixed_corpus(5)
    node0, ctx0 = tables(V_BIG, 128, 1)
    got = run(node0, ctx0, walks[:, :1].copy(), seeds, 3, 5, table)
    np.testing.assert_array_equal(got[0], node0)
    np.testing.assert_array_equal(got[1], ctx0)
    assert got[2] == 0


@pytest.mark.parametrize("hot_kind", ["all", "table_share"])
@pytest.mark.parametrize("d,n", [(128, 5), (256, 10)])
def test_contended_rows_tier_b(d, n, hot_kind):
    """Hot rows take float-atomic deltas (row + g*in, rounded twice, instead of fma) in both
    paths: one wavefront against the sequential oracle within tier B."""
    w = 3
    walks, seeds, table = mixed_corpus(n)
    if hot_kind == "all":
        hot = torch.full(((V_BIG + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    else:  # the rows the aliased pairs draw hold the most slots
        counts = np.bincount(table, minlength=V_BIG)[1:]
        hot = tsi.hot_rows(dev(table), V_BIG, int(np.median(counts[counts > 0])) + 1)
        nh = int(np.unpackbits(hot.cpu().numpy().view(np.uint8)).sum())
        assert 0 < nh < V_BIG
    node0, ctx0 = tables(V_BIG, d, d + n)
    got = run(node0, ctx0, walks, seeds, w, n, table, hot=hot)
    ref = oracle(node0, ctx0, walks, seeds, w, n, table)
    for a, b in zip(got[:2], ref[:2]):
        diff = np.abs(a - b)
        assert diff.max() <= 1e-3, diff.max()                    # tier B
        assert np.mean(diff <= 1e-5) > 0.95, np.mean(diff <= 1e-5)
