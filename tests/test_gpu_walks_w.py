"""Edge-weighted walks on the GPU (come_walk_cdf / k_walk_cdf, come_random_walks_w /
k_random_walks_w): thresholds, status, walks and trial counts bit-identical to the CPU twins (the
same arithmetic and step body, csrc/come_walk_pq.h), come_random_walks' stream on unit weights,
the exact weighted step frequencies, and the Python entry points."""
import functools

import numpy as np
import pytest

from come_amd import _lib, cpu
from come_amd import graph_utils as gu
from come_amd.graph import CSRGraph, chung_lu, random_walks
from walks_pq_common import SETTINGS
from walks_w_common import check_distribution_w, count_zero_edge, g12w

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def big():
    """chung_lu(20000, 10) with seeded log-normal weights (some of them 0), rows ascending, on the
    host and the device, with the twin's wcdf, starts (dead ends, -1 and V among them) and an emit
    map; built once and never modified."""
    d = dev()
    g = chung_lu(20000, 10.0)
    assert (g.degree == 0).any()
    rng = np.random.RandomState(4)
    ew = rng.lognormal(0.0, 1.5, len(g.edges)).astype(np.float32)
    ew[::37] = 0.0
    gw = CSRGraph(g.V, g.edges, weights=ew)
    np.testing.assert_array_equal(gw.col, g.col)
    # a node all of whose edges drew a 0 would be an all-zero row: give those edges weight 1
    dead = (gw.strength == 0) & (gw.degree > 0)
    ew[dead[g.edges[:, 0]] | dead[g.edges[:, 1]]] = 1.0
    gw = CSRGraph(g.V, g.edges, weights=ew)
    assert not ((gw.strength == 0) & (gw.degree > 0)).any() and (gw.weights == 0).sum() > 1000
    starts = rng.randint(0, g.V, 1000).astype(np.int32)
    starts[3::50] = -1
    starts[4::50] = g.V
    starts[5::50] = np.flatnonzero(g.degree == 0)[0]
    emit = rng.permutation(g.V).astype(np.int32)
    col, w = cpu.sort_weighted_adjacency(gw.rowptr, gw.col.astype(np.int32), gw.weights)
    host = dict(rowptr=gw.rowptr, col=col, w=w, wcdf=cpu.walk_cdf(gw.rowptr, w).view(np.int32),
                starts=starts, emit=emit, g=gw)
    t = {k: torch.from_numpy(v).to(d) for k, v in host.items() if k != "g"}
    return host, t


def device_cdf(rowptr, w):
    """come_walk_cdf itself: (wcdf uint32 numpy, status)."""
    d = dev()
    tr, tw = torch.from_numpy(rowptr).to(d), torch.from_numpy(w).to(d)
    out = torch.full((len(w),), 0x5A5A5A5A, dtype=torch.int32, device=d)
    status = torch.full((1,), 7, dtype=torch.int32, device=d)
    _lib.check(_lib.lib().come_walk_cdf(_lib.ptr(tr), _lib.ptr(tw), len(rowptr) - 1,
                                        _lib.ptr(out), _lib.ptr(status), _lib.stream_handle(d)),
               "come_walk_cdf")
    return out.cpu().numpy().view(np.uint32), int(status)


def test_cdf_kernel_equals_cpu_twin():
    """Lane-built rows (up to 32 entries), wave-built rows (the hubs of the power-law graph, of
    every length modulo 64), and one row of 70,000 entries for the long-row loop."""
    host, _ = big()
    deg = np.diff(host["rowptr"])
    assert deg.max() > 64 and ((deg > 0) & (deg <= 32)).any() and (deg == 0).any()
    rng = np.random.RandomState(5)
    hub = rng.lognormal(0.0, 2.0, 70000).astype(np.float32)
    hub[:100] = 0.0  # a long run of zero-mass entries at the head
    hub[rng.randint(100, 70000, 5000)] = 0.0
    edge = np.concatenate([np.ones(33, np.float32), np.ones(32, np.float32),
                           np.ones(64, np.float32), np.ones(65, np.float32)])
    w = np.concatenate([host["w"], hub, edge])
    nnz = int(host["rowptr"][-1])
    rowptr = np.concatenate([host["rowptr"], nnz + 70000 + np.cumsum([0, 33, 32, 64, 65])])
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    ref, ref_status = cpu.walk_cdf(rowptr, w, threads=2, return_status=True)
    got, status = device_cdf(rowptr, w)
    assert status == ref_status == 0
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(got[:nnz], host["wcdf"].view(np.uint32))
    # invalid weights: the same status, and the same words (rows that cannot be used hold 2^32-1)
    for at, val in ((nnz + 50000, np.nan), (7, -1.0), (nnz + 69999, np.inf)):
        bad = w.copy()
        bad[at] = val
        ref, ref_status = cpu.walk_cdf(rowptr, bad, threads=2, return_status=True)
        got, status = device_cdf(rowptr, bad)
        assert status == ref_status == 1, (at, val)
        np.testing.assert_array_equal(got, ref)
    bad = w.copy()
    bad[nnz:nnz + 70000] = 0.0  # a long all-zero row
    assert device_cdf(rowptr, bad)[1] == cpu.walk_cdf(rowptr, bad, return_status=True)[1] == 1
    bad = w.copy()
    lo, hi = host["rowptr"][np.flatnonzero(deg == 3)[0]:][:2]
    bad[lo:hi] = 0.0  # a short all-zero row
    assert device_cdf(rowptr, bad)[1] == cpu.walk_cdf(rowptr, bad, return_status=True)[1] == 1


@pytest.mark.parametrize("p,q", [(1.0, 1.0), (0.25, 4.0), (1.0 / 16, 16.0)])
def test_walker_kernel_equals_cpu_twin(p, q):
    """test_p4_kernel_equals_cpu_twin's shapes: P = 257 and 1000 leave ragged last workgroups,
    the offset beyond 2^32 reaches the counter's high word."""
    host, t = big()
    seed = 2 ** 40 + 11
    wcdf = host["wcdf"].view(np.uint32)
    for P in (1, 257, 1000):
        hs, ds = np.ascontiguousarray(host["starts"][-P:]), t["starts"][-P:].contiguous()
        for L in (1, 17, 40):
            for alpha in (0.0, 0.2):
                for off in (0, 2 ** 33 + 5):
                    for em in (False, True):
                        trials = torch.zeros(1, dtype=torch.int64, device=ds.device)
                        got = gu.device_walks(t["rowptr"], t["col"], ds, L, alpha=alpha, seed=seed,
                                              walk_offset=off, emit=t["emit"] if em else None,
                                              p=p, q=q, wadj=(t["col"], t["wcdf"]),
                                              trials_out=trials)
                        ref, ref_trials = cpu.random_walks_w(
                            host["rowptr"], host["col"], wcdf, hs, L, alpha=alpha, p=p, q=q,
                            seed=seed, walk_offset=off, emit=host["emit"] if em else None,
                            return_trials=True, threads=2)
                        np.testing.assert_array_equal(got.cpu().numpy(), ref,
                                                      err_msg=str((P, L, alpha, off, em)))
                        assert int(trials) == ref_trials, (P, L, alpha, off, em)
    assert (ref == -1).any() and ref_trials > 0


def test_unit_weights_equal_come_random_walks():
    host, t = big()
    unit = torch.ones_like(t["w"])
    wadj = gu.weighted_adjacency(t["rowptr"], t["col"], unit)
    assert torch.equal(wadj[0], t["col"])
    for L, alpha, off, em in ((1, 0.0, 0, None), (17, 0.2, 2 ** 33 + 5, t["emit"]),
                              (40, 0.0, 5, None), (40, 0.3, 0, t["emit"])):
        ref = gu.device_walks(t["rowptr"], t["col"], t["starts"], L, alpha=alpha, seed=77,
                              walk_offset=off, emit=em)
        trials = torch.zeros(1, dtype=torch.int64, device=ref.device)
        got = gu.device_walks(t["rowptr"], t["col"], t["starts"], L, alpha=alpha, seed=77,
                              walk_offset=off, emit=em, wadj=wadj, trials_out=trials)
        assert torch.equal(got, ref), (L, alpha, off)
        assert int(trials) == int((ref[:, 1:] >= 0).sum())  # one block per step, none rejected


@pytest.mark.parametrize("p,q", [(1.0, 1.0), SETTINGS[0], SETTINGS[3], (1.0 / 256, 4.0)])
def test_device_step_frequencies_are_the_exact_weighted_probabilities(p, q):
    d = dev()
    rowptr, col, w = g12w(scramble=np.random.RandomState(3))  # device_walks sorts the rows
    starts = torch.arange(12, dtype=torch.int32, device=d).repeat(1500)
    walks = gu.device_walks(torch.from_numpy(rowptr).to(d), torch.from_numpy(col).to(d), starts,
                            20, seed=12, p=p, q=q,
                            weights=torch.from_numpy(w).to(d)).cpu().numpy()
    checked, first = check_distribution_w(walks, rowptr, col, w, p, q)
    assert checked >= 20 and first >= 20, (checked, first)
    assert count_zero_edge(walks) == 0
    # and they are the twin's walks on the sorted rows
    cs, ws = cpu.sort_weighted_adjacency(rowptr, col, w)
    np.testing.assert_array_equal(
        walks, cpu.random_walks_w(rowptr, cs, cpu.walk_cdf(rowptr, ws), starts.cpu().numpy(), 20,
                                  p=p, q=q, seed=12))


def test_python_entry_points():
    host, t = big()
    g = host["g"]
    cs, wcdf = gu.weighted_adjacency(t["rowptr"], torch.from_numpy(g.col).to(t["col"].device),
                                     torch.from_numpy(g.weights).to(t["col"].device))
    assert torch.equal(cs, t["col"]) and torch.equal(wcdf, t["wcdf"])
    kw = dict(alpha=0.1, seed=21, walk_offset=9, p=0.25, q=4.0)
    ref = gu.device_walks(t["rowptr"], t["col"], t["starts"], 33, wadj=(cs, wcdf), **kw)
    via_graph = random_walks(g, 1, 33, device=t["starts"].device, starts=t["starts"], **kw)
    assert torch.equal(via_graph, ref)
    # weighted=False, and a graph without weights: today's walks (over the graph's own row order)
    plain = CSRGraph(g.V, g.edges)
    np.testing.assert_array_equal(plain.col, g.col)
    own = torch.from_numpy(g.col).to(t["col"].device)
    unweighted = gu.device_walks(t["rowptr"], own, t["starts"], 33, **kw)
    assert not torch.equal(unweighted, ref)
    for graph, flag in ((g, False), (plain, None)):
        got = random_walks(graph, 1, 33, device=t["starts"].device, starts=t["starts"],
                           weighted=flag, **kw)
        assert torch.equal(got, unweighted)
    first_order = random_walks(plain, 1, 33, device=t["starts"].device, starts=t["starts"],
                               alpha=0.1, seed=21, walk_offset=9)
    assert torch.equal(first_order, gu.device_walks(t["rowptr"], own, t["starts"], 33, alpha=0.1,
                                                    seed=21, walk_offset=9))
    with pytest.raises(ValueError, match="needs a graph with weights"):
        random_walks(plain, 1, 5, device=t["starts"].device, starts=t["starts"], weighted=True)
    bad = t["w"].clone()
    bad[5] = float("nan")
    with pytest.raises(ValueError, match="edge weights"):
        gu.weighted_adjacency(t["rowptr"], t["col"], bad)
    with pytest.raises(_lib.ComeError, match="q in"):
        gu.device_walks(t["rowptr"], t["col"], t["starts"], 33, q=17.0, wadj=(cs, wcdf))
