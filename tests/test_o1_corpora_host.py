"""CPU checks of tests/o1_corpora.py: the corpora have the properties the GPU tests of the Hogwild
O1 kernels (tests/test_gpu_o1_hogwild.py) rest on, and the float64 reference of the hub case tells
a launch that loses updates from one that keeps them."""
import numpy as np
import pytest

import o1_corpora as oc
from oracle import oracle as orc


def test_exp_table_and_lcg_match_the_oracle():
    np.testing.assert_array_equal(oc.exp_table(), orc.exp_table())
    s = 123456789012
    slots = oc.lcg_slots(np.array([s], np.uint64), 3, 1000)[0]
    for k in range(3):
        assert slots[k] == (s >> 16) % 1000
        s = orc.lcg_next(s)


def test_runs_and_oracle_edges():
    edges = np.array([[3, 1], [3, 3], [-1, 2], [3, 2], [4, 9], [4, 1], [3, 0]], np.int32)
    assert oc.runs_of(edges, 8) == [(0, 4, 3), (5, 6, 4), (6, 7, 3)]
    assert oc.oracle_edges(edges, 8).tolist() == [[3, 1], [3, 3], [-1, -1], [3, 2], [-1, -1],
                                                  [4, 1], [3, 0]]


@pytest.mark.parametrize("n", [0, 5, 20])
def test_matching_corpus(n):
    """The builder's own assertions (no row and no table slot shared by two edges, draws equal to
    u, to v and repeated) plus the shape the issue fixes: 5 rows per edge, every 17th edge a
    self-loop, the endpoints -1 and V + 3."""
    E, d = 512, 8
    node0, edges, seeds, table = oc.matching_corpus(E, n, d, seed=n)
    V = node0.shape[0]
    assert V == 5 * E and edges.shape == (E, 2) and seeds.shape == (E,)
    ok = oc.valid_edges(edges, V)
    assert edges[5, 0] == -1 and edges[11, 1] == V + 3 and (~ok).sum() == 2
    loops = np.flatnonzero(edges[:, 0] == edges[:, 1])
    assert set(loops) == set(range(0, E, 17))
    ends = edges[ok].ravel()
    assert len(np.unique(ends)) == 2 * ok.sum() - len(loops)  # every endpoint row has one edge
    if n:
        drawn = table[oc.lcg_slots(seeds[ok], 2 * n, len(table))]
        assert (drawn // 5 == np.flatnonzero(ok)[:, None]).all()
        assert (drawn % 5 >= 2).any()  # the pool


@pytest.mark.parametrize("E,align,max_run,n,own", [(370, 6, 4, 5, True), (370, 6, 8, 5, False),
                                                   (372, 93, 8, 15, False), (372, 93, 4, 0, True)])
def test_star_corpus(E, align, max_run, n, own):
    """The builder's own assertions (one run per first endpoint, no run across a multiple of
    `align`, several runs per block, rows disjoint across blocks, distinct leaves) plus: the
    last block is partial where E says so, and with own_rows=False no drawn row is an endpoint."""
    node0, edges, seeds, table = oc.star_corpus(E, align, max_run, n, 8, seed=3, own_rows=own)
    V = node0.shape[0]
    assert oc.valid_edges(edges, V).all() and (np.diff(edges[:, 0]) >= 0).all()
    runs = oc.runs_of(edges, V)
    assert max(b - a for a, b, _ in runs) <= min(max_run, align)
    assert sum(b - a for a, b, _ in runs) == E
    if n and not own:
        drawn = table[oc.lcg_slots(seeds, 2 * n, len(table))]
        assert not np.isin(drawn, edges).any()
    # a different seed gives a different corpus, the same seed the same one
    again = oc.star_corpus(E, align, max_run, n, 8, seed=3, own_rows=own)
    assert all(np.array_equal(a, b) for a, b in zip((node0, edges, seeds, table), again))


def test_shared_corpus():
    node0, edges, seeds, table = oc.shared_corpus(300, 40, 5, 8, seed=1)
    assert node0.shape == (40, 8) and edges.shape == (300, 2)
    # every row is an endpoint of several edges: nothing here is private
    assert np.bincount(edges[oc.valid_edges(edges, 40)].ravel(), minlength=40).min() >= 2


def test_o1_ref64_is_the_oracle_without_negatives():
    """The float64 restatement against the C oracle (fp32 rows, WAVE64 dots) on a few edges with
    a self-loop and a skipped edge: the same updates up to fp32 rounding."""
    rng = np.random.RandomState(2)
    node0 = rng.uniform(-0.5, 0.5, (12, 16)).astype(np.float32)
    edges = rng.randint(0, 12, (40, 2)).astype(np.int32)
    edges[7, 1] = edges[7, 0]
    edges[9, 0] = -1
    ref = node0.copy()
    orc.sgns_o1(ref, edges, np.zeros(40, np.uint64), 0, np.zeros(4, np.uint32), 0.2,
                dot_mode=orc.DOT_WAVE64)
    got = oc.o1_ref64(node0, edges, 0.2)
    assert not np.array_equal(ref, node0)
    np.testing.assert_allclose(got, ref, rtol=0, atol=40 * 2.0 ** -24)


@pytest.mark.parametrize("orient", [0, 1])
def test_hub_reference_separates_lost_updates_from_stale_reads(orient):
    """hub_corpus(2048, 128, orient) at lr = 5e-5, all in float64.  A launch that reads the hub as
    it was before the launch for every edge but loses no update ("fully stale") ends 1.08% of the
    hub's drift (0.0245) from the sequential run; B = 4 x that + the fp32 rounding term is 4.4%
    of the drift.  Losing every eighth hub update ends at 12.2% of the drift = 2.75 B, every
    second at 49.6% = 11.2 B (the same to three digits for both orientations): the bar of
    tests/test_gpu_o1_hogwild.py::test_hub_loses_no_update passes the first and fails the
    others."""
    E, d, lr = 2048, 128, 5e-5
    node0, edges, _, _ = oc.hub_corpus(E, d, orient)
    assert (edges[:, 1 - orient] == 0).all() and sorted(edges[:, orient]) == list(range(1, E + 1))
    seq = oc.o1_ref64(node0, edges, lr)
    stale = oc.o1_ref64(node0, edges, lr, stale_row=0)
    drift = np.linalg.norm(seq[0] - node0[0])
    B = 4 * np.linalg.norm(stale[0] - seq[0]) + np.sqrt(d) * 2.0 ** -24 * np.sqrt(E)
    assert 0.005 * drift < np.linalg.norm(stale[0] - seq[0]) < 0.02 * drift
    for k, share in ((8, 0.122), (2, 0.496)):
        lost = oc.o1_ref64(node0, edges, lr, drop_every=k, drop_row=0)
        dist = np.linalg.norm(lost[0] - seq[0])
        print("orient %d: every %d-th hub update lost: %.4g = %.1f%% of the drift = %.2f B" % (
            orient, k, dist, 100 * dist / drift, dist / B))
        assert dist > 2 * B
        assert abs(dist / drift - share) < 0.01
    # every leaf is updated exactly once and reads the hub once
    assert (np.abs(seq[1:] - node0[1:]).max(axis=1) > 0).all()
