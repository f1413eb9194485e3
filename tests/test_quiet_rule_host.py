"""What the quiet-row rule means, on the numpy float64 restatement in
tests/quiet_rule.py -- no GPU, no libcome.

The rule promises that a row held in the stream kernel's LDS ring has at most eps expected
concurrent visitors.  It estimates a row's share of walk visits from the negative table; here the
promise is checked against the truth the table was built from, visitors * deg[r] / sum(deg), which
the table does not enter.  The estimate is only right with the shift by one row (the table stores
node ids that the kernels use as rows): with id_shift 0 or -1 the same check fails on every input.
tests/test_gpu_quiet_rows.py holds the kernels to this reference bit for bit.
"""
import numpy as np
import pytest

import quiet_cases as qc
import quiet_rule as qr

# Table quantisation: id r + 1 gets count^0.75 / Z of the T slots rounded to whole slots, so its c
# slots stand for a true mass within one slot of c, and c^(4/3) is below the true value by a
# factor of at most (1 + 1/c)^(4/3).  On the inputs below the quiet row with the most slots of its
# own has c >= 18 at every eps (asserted), which bounds the excess at (19/18)^(4/3) - 1 = 7.5%.
# Measured: the worst ratio true visitors / eps over the 15 cases is 1.033 (V = 4097, eps 0.05);
# over seeds 0..7 of every input, 1.062.  The wrong shifts give 1.26 .. 1209.
TOL = 0.08
MIN_SLOTS = 18


def worst_ratio(V, T, visitors, seed, eps, id_shift=None):
    """(largest true expected visitor count among the rows marked quiet) / eps, the quiet vector
    and the slot counts; id_shift None = the reference's default, the product's shift."""
    deg, table = qc.degree_table(V, T, seed)
    counts = qr.table_counts(table, V)
    true_visitors = visitors * deg / deg.sum()
    shift = {} if id_shift is None else {"id_shift": id_shift}
    quiet, _, _ = qr.quiet_bits(counts, V, visitors, eps, T + 1, **shift)
    assert quiet.any()
    return true_visitors[quiet].max() / eps, quiet, counts


@pytest.mark.parametrize("eps", qc.EPS)
@pytest.mark.parametrize("V,T,visitors,seed", qc.INPUTS)
def test_quiet_rows_have_at_most_eps_true_visitors(V, T, visitors, seed, eps):
    """Every row the rule marks quiet has true expected visitors <= eps (1 + TOL), TOL = 0.08
    (measured worst over these cases: 1.033 eps; see TOL above), and the marking is neither empty
    nor everything."""
    ratio, quiet, counts = worst_ratio(V, T, visitors, seed, eps)
    own = counts[1:][quiet[:-1]]
    print("V=%d T=%d eps=%g: %d quiet rows, worst true visitors / eps = %.4f, most own slots %d"
          % (V, T, eps, quiet.sum(), ratio, own.max()))
    assert 0 < quiet.sum() < V
    assert own.max() >= MIN_SLOTS  # what TOL was worked out for
    assert ratio <= 1.0 + TOL, ratio


@pytest.mark.parametrize("id_shift", [0, -1])
@pytest.mark.parametrize("eps", qc.EPS)
@pytest.mark.parametrize("V,T,visitors,seed", qc.INPUTS)
def test_other_shifts_break_the_promise(V, T, visitors, seed, eps, id_shift):
    """The same check fails without the shift by one row: a row's own slots (shift 0) or the row
    before's (-1) say nothing about its degree, so some marked row has well over eps visitors."""
    ratio, _, _ = worst_ratio(V, T, visitors, seed, eps, id_shift)
    print("V=%d T=%d eps=%g id_shift=%d: worst true visitors / eps = %.3f"
          % (V, T, eps, id_shift, ratio))
    assert ratio > 1.0 + TOL, ratio


def synthetic_counts(V, seed):
    """Slot counts with a heavy tail and rows that hold no slot at all."""
    rng = np.random.RandomState(seed)
    counts = rng.zipf(1.5, V).clip(1, 5000).astype(np.int64)
    counts[rng.rand(V) < 0.3] = 0
    counts[0], counts[V - 1] = 0, 3
    return counts


@pytest.mark.parametrize("V", [1, 33, 1000])
def test_shift_outside_the_table_marks_nothing(V):
    counts = synthetic_counts(V, V)
    for shift in (V, V + 7, -V, -V - 7):
        quiet, total, margin = qr.quiet_bits(counts, V, 1.0, 1e30, counts.sum() + 1,
                                             id_shift=shift)
        assert not quiet.any() and np.isinf(margin).all() and total > 0


def test_last_row_is_never_quiet_at_shift_1():
    """Row V - 1's own count would be in the slots of the value V, which the table does not hold."""
    for V in (1, 2, 33, 1000):
        counts = synthetic_counts(V, V)
        for eps in (0.0, 0.4, 1e30):
            quiet, _, _ = qr.quiet_bits(counts, V, 1.0, eps, counts.sum() + 1)
            assert not quiet[V - 1]
            if V > 1 and eps == 1e30:
                assert quiet[:V - 1].all()


@pytest.mark.parametrize("id_shift", [1, 0, -1])
def test_eps_0_marks_the_cold_rows_whose_own_value_has_no_slot(id_shift):
    V = 1000
    counts = synthetic_counts(V, 5)
    hot_min = 40
    quiet, _, margin = qr.quiet_bits(counts, V, 7.0, 0.0, hot_min, id_shift=id_shift)
    own = np.arange(V) + id_shift
    want = np.zeros(V, bool)
    for r in range(V):
        want[r] = 0 <= own[r] < V and counts[r] < hot_min and counts[own[r]] == 0
    assert np.array_equal(quiet, want) and 0 < quiet.sum() < V
    assert np.isinf(margin).all()  # 0 <= 0 and c^(1/power) >= 1 > 0: no rounding decides


def test_hot_min_1_leaves_only_rows_without_a_slot():
    V = 1000
    counts = synthetic_counts(V, 6)
    quiet, total, _ = qr.quiet_bits(counts, V, 50.0, 0.4, 1)
    assert quiet.any() and not counts[quiet].any()
    everything, _, _ = qr.quiet_bits(counts, V, 50.0, 1e30, 1)
    assert np.array_equal(everything[:V - 1], counts[:V - 1] == 0)
    assert np.array_equal(qr.hot_bits(counts, 1), counts > 0)


def test_hot_min_above_T_excludes_nothing():
    V = 1000
    counts = synthetic_counts(V, 7)
    T = int(counts.sum())
    quiet, total, _ = qr.quiet_bits(counts, V, 50.0, 0.4, T + 1)
    x = counts.astype(np.float64) ** (4.0 / 3.0)
    want = np.append(50.0 * x[1:] / total <= 0.4, False)
    assert np.array_equal(quiet, want) and 0 < quiet.sum() < V - 1
    assert not qr.hot_bits(counts, T + 1).any()
    some, _, _ = qr.quiet_bits(counts, V, 50.0, 0.4, 40)
    assert np.array_equal(some, want & (counts < 40)) and some.sum() < quiet.sum()


def test_sum_and_margin():
    counts = np.array([0, 8, 27, 1], np.int64)
    quiet, total, margin = qr.quiet_bits(counts, 4, 2.0, 0.5, 100, power=1.0 / 3.0)
    assert total == 512 + 19683 + 1
    bound = 0.5 * total / 2.0
    np.testing.assert_allclose(margin[:3], np.abs(np.array([512., 19683., 1.]) - bound) / bound,
                               rtol=1e-15)
    assert np.isinf(margin[3])
    assert quiet.tolist() == [True, False, True, False]
    with pytest.raises(ValueError):
        qr.quiet_bits(np.zeros(4, np.int64), 4, 2.0, 0.5, 100)


def test_table_counts_ignores_values_past_V():
    table = np.array([0, 3, 3, 4, 5, 0xFFFFFFFF, 0x80000000, 2], np.uint32)
    assert qr.table_counts(table, 4).tolist() == [1, 0, 1, 2]
    assert qr.table_counts(table.view(np.int32), 4).tolist() == [1, 0, 1, 2]
    assert qr.table_counts(table, 6).tolist() == [1, 0, 1, 2, 1, 1]


@pytest.mark.parametrize("V", [1, 31, 32, 33, 64, 4097])
def test_bitmap_packing(V):
    flags = np.random.RandomState(V).rand(V) < 0.5
    flags[V - 1] = True
    words = qr.pack_bits(flags)
    assert words.dtype == np.uint32 and words.shape == ((V + 31) // 32,)
    for r in range(V):
        assert bool(int(words[r // 32]) >> (r % 32) & 1) == flags[r]
    assert int(words[-1]) >> ((V - 1) % 32 + 1) == 0  # nothing past row V - 1
    assert np.array_equal(qr.unpack_bits(words, V), flags)
    assert np.array_equal(qr.unpack_bits(words.view(np.int32), V), flags)
