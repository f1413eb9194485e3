"""The windowed stream kernel (k_sgns_o2_stream<VEC <= 2, ..., WINDOW = true>): quiet input rows
held in the wavefront's LDS ring over a walk window (read once per stay, written back once).

Bars, as for the kernel without the ring (tests/test_gpu_stream.py):
  * one wavefront (max_waves=1), the stream kernel forced (o2_kernel=3), no contended rows, every
    row quiet: the launch must equal the sequential oracle (WAVE64 dot order) BIT FOR BIT on both
    WHOLE tables -- a row left in the ring, or written back twice out of order, shows;
  * walks in flight that share no row: bit for bit as well;
  * an empty quiet bitmap: the same bits as the launch without one.
Contended (hot) rows are updated by float-atomic deltas, which round differently from the
oracle's fma (tier B, tests/test_gpu_stream.py), so no launch with hot rows can equal the oracle
bit for bit, with or without the ring.  The walk that alternates quiet, ordinary and hot inputs is
therefore held bit for bit to the same launch without a quiet bitmap (one wavefront: the ring
holds exactly the value the other kernel stores and reads back), and to the oracle within tier B.

Walks (V = 5,000, n = 5, L = 200): immediate backtracks a, b, a, b; the same row again at distance
exactly 2w and at 2w + 1 (a slot leaving as its alias enters); -1 holes; 1, w and w + 1 valid
entries; 200 positions over a small pool and over the whole vocabulary (across the 64-position
chunk refill); the launch's last walk ends with a full window.  Instantiations: d = 128
(<2, true>), 100 (<2, false>), 64 (<1, false>); w = 5 and 2.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

import come_amd.training_sdg_inner as tsi
from test_gpu_stream import dev, disjoint_case, oracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
V, N, L, LR, T = 5000, 5, 200, 0.05, 200_003


def bitmap(rows):
    """CUDA int32 bitmap [ceil(V / 32)] with the bits of `rows` (bool [V]) set."""
    idx = np.flatnonzero(rows).astype(np.uint32)
    bits = np.zeros((V + 31) // 32, np.uint32)
    np.bitwise_or.at(bits, idx >> 5, np.uint32(1) << (idx & 31))
    return dev(bits)


def run(node0, ctx0, walks, seeds, w, table, hot, quiet, opts):
    node, ctx = dev(node0), dev(ctx0)
    tsi.sgns_o2(node, ctx, dev(walks), dev(seeds), w, N, table, LR, 1.0, tsi.MODE_HOGWILD,
                opts=opts, hot=hot, quiet=quiet)
    torch.cuda.synchronize()
    return node.cpu().numpy(), ctx.cpu().numpy()


def edge_walks(w, rng):
    """The walks of the module docstring, [P, L] int32, -1 = None."""
    rows = []

    def fresh(k):  # k distinct rows
        return rng.choice(V, k, replace=False)

    a, b = fresh(2)  # immediate backtracks, then on
    rows.append(np.concatenate([np.tile([a, b], 20), fresh(L - 40)]))
    x = fresh(L)  # the same row at distance exactly 2w and at 2w + 1
    x[30 + 2 * w] = x[30]
    x[90 + 2 * w + 1] = x[90]
    x[150 + 2 * w] = x[150]
    x[150 + 4 * w] = x[150]  # a chain: the slot outlives its first position's window
    rows.append(x)
    h = fresh(L)  # holes
    h[rng.choice(L, 40, replace=False)] = -1
    h[100:100 + 2 * w + 3] = -1  # and one wider than the window
    rows.append(h)
    for k in (1, w, w + 1):  # short walks
        s = np.full(L, -1)
        s[:k] = fresh(k)
        rows.append(s)
    rows.append(rng.choice(fresh(12), L))  # many aliases inside every window
    rows.append(rng.randint(0, V, L))
    rows.append(fresh(L))  # the last walk ends with a full window
    return np.stack(rows).astype(np.int32)


def problem(d, seed):
    rng = np.random.RandomState(seed)
    table = orc.make_table(rng.randint(1, 40, V), T)
    node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
    ctx0 = rng.uniform(-0.3, 0.3, (V, d)).astype(np.float32)
    return rng, table, node0, ctx0


@pytest.mark.parametrize("w", [5, 2])
@pytest.mark.parametrize("d", [128, 100, 64])
def test_one_wavefront_every_row_quiet_bit_exact(d, w):
    rng, table, node0, ctx0 = problem(d, 7 * d + w)
    walks = edge_walks(w, rng)
    seeds = rng.randint(0, 2 ** 48, len(walks), dtype=np.int64).astype(np.uint64)
    got = run(node0, ctx0, walks, seeds, w, dev(table), None, bitmap(np.ones(V, bool)),
              {"o2_kernel": 3, "max_waves": 1})
    ref = oracle(node0, ctx0, walks, seeds, w, N, table, LR)
    assert not np.array_equal(ref[0], node0)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])


@pytest.mark.parametrize("d", [128, 100, 64])
def test_quiet_ordinary_and_hot_inputs_alternate(d):
    """Rows 0, 1, 2 mod 3 are quiet, ordinary and hot: every window mixes the three paths."""
    w = 5
    rng, table, node0, ctx0 = problem(d, 11 * d)
    walks = np.stack([rng.randint(0, V, L), np.arange(L) + 17,
                      rng.choice(rng.choice(V, 15, replace=False), L)]).astype(np.int32)
    seeds = rng.randint(0, 2 ** 48, len(walks), dtype=np.int64).astype(np.uint64)
    kind = np.arange(V) % 3
    hot, quiet = bitmap(kind == 2), bitmap(kind == 0)
    opts = {"o2_kernel": 3, "max_waves": 1}
    got = run(node0, ctx0, walks, seeds, w, dev(table), hot, quiet, opts)
    same = run(node0, ctx0, walks, seeds, w, dev(table), hot, None, opts)
    np.testing.assert_array_equal(got[0], same[0])
    np.testing.assert_array_equal(got[1], same[1])
    ref = oracle(node0, ctx0, walks, seeds, w, N, table, LR)
    for a, b in zip(got, ref):
        assert np.abs(a - b).max() <= 1e-3  # tier B: the hot rows' atomics


def test_disjoint_walks_in_flight_bit_exact():
    """256 walks in flight that share no row, every row quiet: the sequential order's bits."""
    P, Ld, w, d = 256, 12, 2, 128
    node0, ctx0, walks, seeds, table = disjoint_case(P, Ld, w, N, d, pool=6, T=(1 << 26) - 5,
                                                     seed=1285)
    quiet = torch.full(((len(node0) + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    node, ctx = dev(node0), dev(ctx0)
    tsi.sgns_o2(node, ctx, dev(walks), dev(seeds), w, N, dev(table), LR, 1.0, tsi.MODE_HOGWILD,
                opts={"o2_kernel": 3}, hot=None, quiet=quiet)
    torch.cuda.synchronize()
    ref = oracle(node0, ctx0, walks, seeds, w, N, table, LR)
    assert not np.array_equal(ref[1], ctx0)
    np.testing.assert_array_equal(node.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(ctx.cpu().numpy(), ref[1])


def test_empty_quiet_bitmap_equals_none():
    d, w = 128, 5
    rng, table, node0, ctx0 = problem(d, 3)
    walks = edge_walks(w, rng)
    seeds = rng.randint(0, 2 ** 48, len(walks), dtype=np.int64).astype(np.uint64)
    opts = {"o2_kernel": 3, "max_waves": 1}
    got = run(node0, ctx0, walks, seeds, w, dev(table), None, bitmap(np.zeros(V, bool)), opts)
    ref = run(node0, ctx0, walks, seeds, w, dev(table), None, None, opts)
    np.testing.assert_array_equal(got[0], ref[0])
    np.testing.assert_array_equal(got[1], ref[1])
