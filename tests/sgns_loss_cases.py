"""Inputs and the float64 numpy restatement for the SGNS loss tests (TEST INFRASTRUCTURE; used by
tests/test_sgns_loss_host.py and tests/test_gpu_sgns_loss.py).

The restatement is written from the entry's contract in include/come.h, not from the library:
train_o2's pair enumeration (pyx:494-508), the LCG draws (pyx:133-134), the two skip rules and
np.logaddexp on exact float64 dots.  Every row comes from a table of V = 300 rows, so the float64
dots are looked up in the V x V Gram matrix of the tables (and sum_j |u_j c_j|, which the error
bound needs, in the Gram matrix of their absolute values).

Bound (derived, not measured): the fp32 dot in the WAVE64 order -- an fmaf chain of ceil(d/64)
steps per lane, then six butterfly additions -- is off by at most (ceil(d/64) + 6) * 2^-24 *
sum_j |u_j c_j| to first order, and softplus has slope <= 1, so a term moves by no more than that.
A walk's (pair's) value may differ from float64 by the sum of the bound over its terms plus 1e-12
of the value for the libm.  A numpy simulation of the order on uniform(-1, 1) rows stayed below
0.14 of the bound.
"""
import functools

import numpy as np

V, P, L, T = 300, 37, 23, 4099
WIDTHS = (1, 63, 64, 65, 100, 128, 200, 512)
# widths in the lower part of a kernel instantiation's range (VEC = 4: 129..256, VEC = 8: 257..512),
# where more than the last 64-element register of a row passes d
GAP_WIDTHS = (130, 191, 300, 447)
LCG_MUL, LCG_ADD, LCG_MASK = 25214903917, 11, (1 << 48) - 1
HOT = 17  # the row that holds 90% of the collision table


def dot_bound_factor(d):
    return (-(-d // 64) + 6) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def tables(d, seed=3, rows=V):
    """(node, ctx) uniform(-1, 1) fp32 [rows x d], frozen."""
    rng = np.random.RandomState(1000 * seed + d)
    node = rng.uniform(-1, 1, (rows, d)).astype(np.float32)
    ctx = rng.uniform(-1, 1, (rows, d)).astype(np.float32)
    node.setflags(write=False)
    ctx.setflags(write=False)
    return node, ctx


@functools.lru_cache(maxsize=None)
def grams(d, seed=3, rows=V):
    """float64 node @ ctx.T and |node| @ |ctx|.T."""
    node, ctx = (a.astype(np.float64) for a in tables(d, seed, rows))
    return node @ ctx.T, np.abs(node) @ np.abs(ctx).T


@functools.lru_cache(maxsize=None)
def walks_case(p=P, length=L, seed=5, hot=False):
    """(walks int32 [p x length], seeds uint64 [p]): random rows with trailing padding on some
    walks, walk 0 with interior -1, walk 1 all -1, walk 2 one node, walk 3 with an entry V + 5;
    `hot`: every other walk visits row HOT."""
    rng = np.random.RandomState(seed)
    w = rng.randint(0, V, (p, length)).astype(np.int32)
    for r in range(4, p, 5):
        w[r, rng.randint(2, length):] = -1
    if hot:
        w[:, 1] = HOT
    w[0, [min(3, length - 1), min(4, length - 1), length // 2]] = -1
    w[1, :] = -1
    w[2, 1:] = -1
    w[3, min(6, length - 1)] = V + 5
    seeds = rng.randint(0, 2 ** 48, p, dtype=np.int64).astype(np.uint64)
    w.setflags(write=False)
    seeds.setflags(write=False)
    return w, seeds


@functools.lru_cache(maxsize=None)
def neg_table(kind):
    """uint32 [T], non-decreasing with steps of 0 or 1 (so it packs): 'zipf' a power-law over the
    V rows; 'collision' row HOT on more than 90% of the slots; 'oob' a power-law over V + 40 ids,
    so the last ones lie outside [0, V)."""
    ids = V + 40 if kind == "oob" else V
    if kind == "collision":
        counts = np.ones(ids, np.int64)
        counts[HOT] = T - (ids - 1)
    else:
        share = 1.0 / np.arange(1, ids + 1) ** 0.75
        counts = np.maximum(1, np.floor(share / share.sum() * (T - ids)).astype(np.int64))
        counts[0] += T - counts.sum()
    t = np.repeat(np.arange(ids), counts).astype(np.uint32)
    assert len(t) == T and t.max() == ids - 1
    t.setflags(write=False)
    return t


def enumerate_o2(walks, seeds, window, negative, table):
    """train_o2's pairs and draws, restated: per pair the walk, the input row (node), the positive
    row (ctx), the n raw draws and a mask of the draws that take part (not the positive, inside
    [0, V)).  Returns (walk [M], rin [M], rpos [M], draws [M x n] int64, used [M x n] bool)."""
    walk, rin, rpos, draws = [], [], [], []
    tl, tn = table.tolist(), len(table)
    for p in range(walks.shape[0]):
        idx = walks[p].tolist()
        nr = int(seeds[p])
        n_pos = min(len(idx), 10000)
        for i in range(n_pos):
            if not 0 <= idx[i] < V:
                continue
            for j in range(max(0, i - window), min(n_pos, i + window + 1)):
                if j == i or not 0 <= idx[j] < V:
                    continue
                row = []
                for _ in range(negative):
                    row.append(tl[(nr >> 16) % tn])
                    nr = (nr * LCG_MUL + LCG_ADD) & LCG_MASK
                walk.append(p)
                rin.append(idx[j])
                rpos.append(idx[i])
                draws.append(row)
    m = len(walk)
    draws = np.array(draws, np.int64).reshape(m, negative)
    rpos_a = np.array(rpos, np.int64)
    used = (draws != rpos_a[:, None]) & (draws < V)
    return np.array(walk, np.int64), np.array(rin, np.int64), rpos_a, draws, used


def pair_values(d, rin, rpos, neg, used, seed=3, rows=V):
    """(value [M], bound [M]) in float64 of pairs (rin, rpos, neg[used]) on tables(d, seed)."""
    G, A = grams(d, seed, rows)
    safe = np.where(used, neg, 0)
    val = np.logaddexp(0.0, -G[rin, rpos])
    bnd = A[rin, rpos].copy()
    if neg.shape[1]:
        val = val + np.where(used, np.logaddexp(0.0, G[rin[:, None], safe]), 0.0).sum(1)
        bnd = bnd + np.where(used, A[rin[:, None], safe], 0.0).sum(1)
    return val, dot_bound_factor(d) * bnd + 1e-12 * val


@functools.lru_cache(maxsize=None)
def o2_enumeration(window, negative, table_kind, p=P, length=L, hot=False):
    w, s = walks_case(p, length, hot=hot)
    return enumerate_o2(w, s, window, negative, neg_table(table_kind))


def o2_reference(d, window, negative, table_kind="zipf", p=P, length=L, hot=False):
    """(per-walk value [p], per-walk bound [p], pairs) of the float64 restatement."""
    walk, rin, rpos, draws, used = o2_enumeration(window, negative, table_kind, p, length, hot)
    val, bnd = pair_values(d, rin, rpos, draws, used)
    return (np.bincount(walk, weights=val, minlength=p),
            np.bincount(walk, weights=bnd, minlength=p), len(walk))
