"""The hot-row and quiet-row rules of come_hot.hip restated in numpy float64 (no device code), from
the sentence in DESIGN.md §3.1 and the contract in include/come.h:

    row r is hot    iff  counts[r] >= min_count
    row r is quiet  iff  0 <= r + id_shift < V
                    and  counts[r] < hot_min
                    and  visitors * counts[r + id_shift]^(1/power) / sum_u counts[u]^(1/power) <= eps

counts[v] = the number of table slots holding the value v.  The table stores node *ids* that the
kernels use as *rows*, so with ids 1..V row r's degree sizes the slots of the value r + 1: that is
id_shift = 1, the product's setting.

The reference of tests/test_quiet_rule_host.py (what the rule means) and of
tests/test_gpu_quiet_rows.py, tests/test_gpu_guard_bands.py (what the kernels compute).
"""
import math

import numpy as np


def table_counts(table, V):
    """counts[v] = occurrences of v in `table` (uint32 values; an int32 view is read as uint32),
    int64 [V].  Values >= V are ignored, as the kernels ignore them."""
    t = np.ascontiguousarray(table)
    if t.dtype == np.int32:
        t = t.view(np.uint32)
    t = t.astype(np.int64)
    return np.bincount(t[t < V], minlength=int(V)).astype(np.int64)


def hot_bits(counts, min_count):
    """Boolean [V]: the rows holding at least min_count slots."""
    return np.asarray(counts, np.int64) >= int(min_count)


def quiet_bits(counts, V, visitors, eps, hot_min, power=0.75, id_shift=1):
    """(quiet, total, margin): the boolean vector [V] of the quiet rows, the float64 sum
    sum_u counts[u]^(1/power) (correctly rounded: math.fsum) and every row's relative margin
    |x_own - bound| / bound, x_own = counts[r + id_shift]^(1/power) and bound = eps * total /
    visitors the value of x_own at which the third condition flips.  A row whose decision no
    rounding can change has margin inf: r + id_shift outside [0, V), and every row at eps = 0,
    where x_own is 0 or >= 1 and the bound is 0."""
    V = int(V)
    counts = np.asarray(counts, np.int64)
    assert counts.shape == (V,) and (counts >= 0).all()
    x = counts.astype(np.float64) ** (1.0 / float(power))
    total = math.fsum(x.tolist())
    if not total > 0.0:
        raise ValueError("no table slot holds a row: every share is 0 / 0")
    rows = np.arange(V, dtype=np.int64)
    own = rows + int(id_shift)
    held = (own >= 0) & (own < V)
    x_own = np.zeros(V, np.float64)
    x_own[held] = x[own[held]]
    expected = float(visitors) * x_own / total
    quiet = held & (counts < int(hot_min)) & (expected <= float(eps))
    bound = float(eps) * total / float(visitors)
    margin = np.full(V, np.inf)
    if bound > 0.0:
        margin[held] = np.abs(x_own[held] - bound) / bound
    return quiet, total, margin


def pack_bits(flags):
    """Boolean [V] -> uint32 [ceil(V / 32)]: bit b of word w is row 32 w + b; the bits past V in
    the last word are 0."""
    flags = np.asarray(flags, bool)
    words = (len(flags) + 31) // 32
    padded = np.zeros(32 * words, np.uint8)
    padded[:len(flags)] = flags
    return np.packbits(padded.reshape(words, 32), axis=1, bitorder="little").view("<u4").reshape(
        words).astype(np.uint32)


def unpack_bits(words, V):
    """uint32 (or int32) words -> boolean [V] of the first V rows (the tail is not returned:
    compare the words themselves to see it)."""
    w = np.ascontiguousarray(words)
    if w.dtype == np.int32:
        w = w.view(np.uint32)
    w = w.astype("<u4")
    assert 32 * len(w) >= V
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:int(V)].astype(bool)
