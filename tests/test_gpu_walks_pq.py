"""The device (p, q) walker (come_random_walks_pq, k_random_walks_pq) on the GPU: bit-identical to
its CPU twin (the same step body, csrc/come_walk_pq.h) with the trial count, the first-order
walker's stream at p = q = 1, the exact node2vec step frequencies, and the Python entry points."""
import functools

import numpy as np
import pytest

from come_amd import _lib, cpu
from come_amd import graph_utils as gu
from come_amd.graph import chung_lu, random_walks
from walks_pq_common import SETTINGS, check_distribution, g12

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def big():
    """chung_lu(20000, 10) on the host and the device, with starts (dead ends, -1 and V among
    them) and an emit map; built once and never modified."""
    d = dev()
    g = chung_lu(20000, 10.0)
    assert (g.degree == 0).any()
    rng = np.random.RandomState(4)
    starts = rng.randint(0, g.V, 1000).astype(np.int32)
    starts[3::50] = -1
    starts[4::50] = g.V
    starts[5::50] = np.flatnonzero(g.degree == 0)[0]
    emit = rng.permutation(g.V).astype(np.int32)
    col = g.col.astype(np.int32)
    host = dict(rowptr=g.rowptr, col=col, cs=cpu.sorted_adjacency(g.rowptr, col), starts=starts,
                emit=emit, g=g)
    t = {k: torch.from_numpy(v).to(d) for k, v in host.items() if k != "g"}
    return host, t


def pq_entry(t, starts, L, alpha, p, q, seed, offset, emit, cs, trials=None):
    """come_random_walks_pq itself (device_walks routes p = q = 1 to come_random_walks)."""
    out = torch.full((starts.numel(), L), 0x5A5A5A5A, dtype=torch.int32, device=starts.device)
    _lib.check(_lib.lib().come_random_walks_pq(
        _lib.ptr(t["rowptr"]), _lib.ptr(t["col"]), None if cs is None else _lib.ptr(cs),
        t["rowptr"].numel() - 1, _lib.ptr(starts), starts.numel(), L, alpha, p, q, seed, offset,
        None if emit is None else _lib.ptr(emit), _lib.ptr(out),
        None if trials is None else _lib.ptr(trials), _lib.stream_handle(starts.device)),
        "come_random_walks_pq")
    return out


@pytest.mark.parametrize("p,q", SETTINGS + [(0.5, 1.0)])
def test_p4_kernel_equals_cpu_twin(p, q):
    """(0.5, 1) runs no N(prev) search and (2, 1) no search at all; P = 257 and 1000 leave ragged
    last workgroups; the offset beyond 2^32 reaches the counter's high word."""
    host, t = big()
    seed = 2 ** 40 + 11
    for P in (1, 257, 1000):
        hs, ds = np.ascontiguousarray(host["starts"][-P:]), t["starts"][-P:].contiguous()
        for L in (1, 17, 40):
            for alpha in (0.0, 0.2):
                for off in (0, 2 ** 33 + 5):
                    for em in (False, True):
                        trials = torch.zeros(1, dtype=torch.int64, device=ds.device)
                        got = gu.device_walks(t["rowptr"], t["col"], ds, L, alpha=alpha, seed=seed,
                                              walk_offset=off, emit=t["emit"] if em else None,
                                              p=p, q=q, col_sorted=t["cs"], trials_out=trials)
                        ref, ref_trials = cpu.random_walks_pq(
                            host["rowptr"], host["col"], hs, L, alpha=alpha, p=p, q=q, seed=seed,
                            walk_offset=off, emit=host["emit"] if em else None,
                            col_sorted=host["cs"], return_trials=True, threads=2)
                        np.testing.assert_array_equal(got.cpu().numpy(), ref,
                                                      err_msg=str((P, L, alpha, off, em)))
                        assert int(trials) == ref_trials, (P, L, alpha, off, em)
    assert (ref == -1).any() and ref_trials > 0


def test_p1_unit_bias_equals_come_random_walks():
    host, t = big()
    for L, alpha, off, em in ((1, 0.0, 0, None), (17, 0.2, 2 ** 33 + 5, t["emit"]),
                              (40, 0.0, 5, None), (40, 0.3, 0, t["emit"])):
        ref = gu.device_walks(t["rowptr"], t["col"], t["starts"], L, alpha=alpha, seed=77,
                              walk_offset=off, emit=em)
        trials = torch.zeros(1, dtype=torch.int64, device=ref.device)
        for cs in (None, t["cs"]):
            got = pq_entry(t, t["starts"], L, alpha, 1.0, 1.0, 77, off, em, cs, trials)
            assert torch.equal(got, ref), (L, alpha, off)
        # one block per step taken, none rejected: twice, the entry adds to trials_out
        steps = int(((ref[:, 1:] >= 0).sum()))
        assert int(trials) == 2 * steps


@pytest.mark.parametrize("p,q", SETTINGS)
def test_device_step_frequencies_are_the_exact_node2vec_probabilities(p, q):
    d = dev()
    rowptr, col = g12()
    starts = torch.arange(12, dtype=torch.int32, device=d).repeat(400)
    w = gu.device_walks(torch.from_numpy(rowptr).to(d), torch.from_numpy(col).to(d), starts, 20,
                        seed=12, p=p, q=q).cpu().numpy()
    seen, checked = check_distribution(w, rowptr, col, p, q)
    assert seen == 32 and checked >= 50, (seen, checked)
    # and they are the twin's walks (device_walks built col_sorted itself)
    np.testing.assert_array_equal(
        w, cpu.random_walks_pq(rowptr, col, starts.cpu().numpy(), 20, p=p, q=q, seed=12))


def test_python_entry_points_and_streams():
    host, t = big()
    np.testing.assert_array_equal(gu.sorted_adjacency(t["rowptr"], t["col"]).cpu().numpy(),
                                  host["cs"])
    kw = dict(alpha=0.1, seed=21, walk_offset=9, p=0.25, q=4.0)
    ref = gu.device_walks(t["rowptr"], t["col"], t["starts"], 33, col_sorted=t["cs"], **kw)
    via_graph = random_walks(host["g"], 1, 33, device=t["starts"].device, starts=t["starts"], **kw)
    assert torch.equal(via_graph, ref)
    side = torch.cuda.Stream(t["starts"].device)
    side.wait_stream(torch.cuda.current_stream(t["starts"].device))
    with torch.cuda.stream(side):
        on_side = gu.device_walks(t["rowptr"], t["col"], t["starts"], 33, col_sorted=t["cs"], **kw)
    side.synchronize()
    assert torch.equal(on_side, ref)
    assert not torch.equal(ref, gu.device_walks(t["rowptr"], t["col"], t["starts"], 33,
                                                alpha=0.1, seed=21, walk_offset=9))
    with pytest.raises(_lib.ComeError, match="q in"):
        gu.device_walks(t["rowptr"], t["col"], t["starts"], 33, p=1.0, q=17.0)
    with pytest.raises(_lib.ComeError, match="col_sorted"):
        pq_entry(t, t["starts"], 5, 0.0, 0.5, 1.0, 1, 0, None, None)
