"""Deterministic coverage of the O1 kernels in Hogwild mode (k_sgns_o1, k_sgns_o1_runs and the
launch arithmetic of come_sgns_o1_ex): the hot bitmap, the float-atomic write-backs, the flush of a
held row at a run's and a chunk's end, the last partial chunk, the grid stride over chunks and the
automatic chunk size -- none of which runs in sequential mode.  Corpora: tests/o1_corpora.py.

The oracle is orc.sgns_o1 in its WAVE64 dot order throughout.  Bars:
  a. one chunk (o1_chunk = E: one wavefront takes every edge in order), rows shared by every
     edge, no contended row: BIT FOR BIT;
  b. 512 edges that share no row, per-edge kernel / chunks of 7 / the default launch, without and
     with every row in the hot bitmap: BIT FOR BIT (a row's single update is one fp32 add of the
     same operands whether a store or an atomic carries it; a self-loop's two updates are two
     adds in order in both kernels), rows of no edge untouched;
  c. runs of edges sharing u, chunks = blocks of private rows, four wavefronts striding over 62
     chunks / the uncapped grid / the automatic chunk size: BIT FOR BIT;
  d. the same with every row hot: leaves and single-edge runs bit for bit, the centre of a run of
     r edges within (r + 1) 2^-24 per element;
  e. corpus a with every row hot: tier B (<= 1e-3 abs, > 95% of elements within 1e-5);
  f. a hub of 2048 leaves, only the hub hot: the hub's row within B of the float64 sequential run,
     B = 4 x (what reading the hub fully stale costs) + fp32 rounding; losing every eighth update
     would cost 2.75 B (tests/test_o1_corpora_host.py);
  g. hot="auto" equals the explicit bitmap at default_hot_share(d), plain and packed table.
"""
import functools

import numpy as np
import pytest
import torch

import o1_corpora as oc
from oracle import oracle as orc

import come_amd.training_sdg_inner as tsi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# every pair selects its own <VEC, FULL, MAXN> instantiation of both kernels
GRID = [(128, 5), (100, 5), (64, 5), (33, 15), (256, 10), (200, 7), (512, 3), (300, 20), (128, 0)]
MASKED = [(128, 5), (100, 5), (200, 7), (300, 20)]  # d not a multiple of 64: lane-masked atomics
STAR_GRID = [(128, 5), (100, 5), (256, 10), (33, 15)]
LR = 0.2
STAR_LR = 0.025  # keeps every centre row below 1 after its run (the rounding bound of case d)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def all_hot(V):
    return torch.full(((V + 31) // 32,), -1, dtype=torch.int32, device=DEV)


def run(corpus, n, lr, hot, opts, table=None):
    node0, edges, seeds, tab = corpus
    node = dev(node0)
    tsi.sgns_o1(node, dev(edges), dev(seeds), n, dev(tab) if table is None else table, lr,
                tsi.MODE_HOGWILD, opts=opts, hot=hot)
    torch.cuda.synchronize()
    return node.cpu().numpy()


def oracle(corpus, n, lr):
    node0, edges, seeds, tab = corpus
    ref = node0.copy()
    orc.sgns_o1(ref, oc.oracle_edges(edges, len(node0)), seeds, n, tab, lr,
                dot_mode=orc.DOT_WAVE64)
    ref.setflags(write=False)
    return ref


# corpora and their oracle results, computed once and shared by the cases that use them
@functools.lru_cache(maxsize=None)
def shared_case(d, n):
    corpus = oc.shared_corpus(300, 40, n, d, seed=d + n)
    return corpus, oracle(corpus, n, LR)


@functools.lru_cache(maxsize=None)
def matching_case(d, n):
    corpus = oc.matching_corpus(512, n, d, seed=10 * d + n)
    return corpus, oracle(corpus, n, LR)


@functools.lru_cache(maxsize=None)
def star_case(E, align, max_run, d, n, own_rows):
    corpus = oc.star_corpus(E, align, max_run, n, d, seed=10 * d + n, own_rows=own_rows)
    return corpus, oracle(corpus, n, STAR_LR)


# ---- a. one chunk, shared rows, cold -----------------------------------------------------------

@pytest.mark.parametrize("d,n", GRID)
def test_one_chunk_shared_rows_bit_exact(d, n):
    """o1_chunk = E: the launch has one chunk, so one wavefront of its workgroup runs the 300
    edges over 40 rows in order (the other three find no chunk) -- held rows, negatives equal to
    the held row and to v, self-loops, skipped endpoints, every row shared."""
    corpus, ref = shared_case(d, n)
    got = run(corpus, n, LR, None, {"o1_chunk": len(corpus[1])})
    assert not np.array_equal(ref, corpus[0])
    np.testing.assert_array_equal(got, ref)


# ---- b. matching corpus ------------------------------------------------------------------------

SHAPES = {"edge": {"o1_chunk": 0}, "chunk7": {"o1_chunk": 7}, "default": None}
MATCHING = [("default", False, d, n) for d, n in GRID] + [
    (shape, hot, d, n) for shape in SHAPES for hot in (False, True)
    if (shape, hot) != ("default", False) for d, n in MASKED]


@pytest.mark.parametrize("shape,hot,d,n", MATCHING)
def test_matching_edges_bit_exact(shape, hot, d, n):
    """512 edges in flight that share no row (o1_corpora.matching_corpus), so every order of the
    wavefronts gives the sequential result.  With every row in the bitmap each update goes out as
    a float atomic: one fp32 add of the operands the plain path adds, and a self-loop's second
    add follows its first from the same wavefront -- still bit for bit.  Rows of no processed
    edge (the skipped edges', unused pool rows) must come back as they went in: a lane mask or an
    index that is off by a row shows there.

    This test found the run kernel summing a hot self-loop's two changes into one flushed delta,
    fl(m + fl(w1 + w2)) where the oracle and k_sgns_o1 have fl(fl(m + w1) + w2): one ulp off in
    the 31 self-loops' rows (rows 85 k), every other row exact.  k_sgns_o1_runs now sends a hot
    held row's delta before a self-loop's second update, so a run of one edge writes what
    k_sgns_o1 writes; these cases are the regression test."""
    corpus, ref = matching_case(d, n)
    node0, edges = corpus[0], corpus[1]
    V = len(node0)
    got = run(corpus, n, LR, all_hot(V) if hot else None, SHAPES[shape])
    idle = np.ones(V, bool)
    idle[edges[oc.valid_edges(edges, V)].ravel()] = False
    assert idle.sum() >= 3 * 512
    np.testing.assert_array_equal(got[idle], node0[idle])
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, "rows that differ: %s, max |diff| %.3g" % (
        bad[:40], np.abs(got - ref).max())


# ---- c / d. star corpus, run kernel ------------------------------------------------------------

# (E, align, launch options).  370 = 6 * 61 + 4: the 62nd chunk is partial.  max_waves = 1 caps the
# grid at one workgroup = four wavefronts, each striding over 15 or 16 chunks.  o1_chunk = -1 with
# that cap: come_sgns_o1_ex sizes the chunk as ceil(E / (4 * workgroups)) = ceil(372 / 4) = 93,
# so the corpus is built with align = 93 and each of the four wavefronts takes one block.
STAR_LAUNCHES = {"capped": (370, 6, {"o1_chunk": 6, "max_waves": 1}),
                 "uncapped": (370, 6, {"o1_chunk": 6}),
                 "auto": (372, 93, {"o1_chunk": -1, "max_waves": 1})}


@pytest.mark.parametrize("d,n", STAR_GRID)
@pytest.mark.parametrize("launch", list(STAR_LAUNCHES))
def test_star_runs_cold_bit_exact(launch, d, n):
    """Runs of 1..4 edges sharing u, several per chunk, draws from the star's own rows (the held
    row, leaves already stored) and pool; rows private to a chunk, so the launch is deterministic
    and must equal the oracle.  A missing flush at a chunk's end, a wrong last chunk, a chunk run
    twice or not at all and a chunk size other than the corpus' block all show."""
    E, align, opts = STAR_LAUNCHES[launch]
    corpus, ref = star_case(E, align, 4, d, n, True)
    got = run(corpus, n, STAR_LR, None, opts)
    bad = np.flatnonzero((got != ref).any(axis=1))
    assert bad.size == 0, "rows that differ: %s, max |diff| %.3g" % (
        bad[:20], np.abs(got - ref).max())


@pytest.mark.parametrize("d,n", STAR_GRID)
@pytest.mark.parametrize("launch", list(STAR_LAUNCHES))
def test_star_runs_all_rows_hot(launch, d, n):
    """The same launches with every row in the bitmap and draws from the pools only, so the launch
    never reads from memory a row it updates atomically (a wavefront's cached copy of such a row
    is not refreshed by the atomic -- by design for contended rows).

    A leaf is updated once: memory gets fl(leaf + work), the operands of the plain path.  The
    centre of a run gets fl(m + du), du the run's summed changes (in two parts, each its own
    atomic, when the run holds a self-loop: the delta is sent before the self-loop's second
    update).  With R updates of the centre (R = r edges, + 1 if one of them is the self-loop;
    leaves are distinct, so at most one is) the oracle rounds R times, the kernel at most R times
    too (the first add into an empty du is exact, each atomic rounds once); every rounding is at
    most half an ulp of a value below 1, 2^-25.  So |got - oracle| <= 2 R 2^-25 <= (r + 1) 2^-24,
    and R = 1 (a run of one edge, never a self-loop here) is bit for bit."""
    E, align, opts = STAR_LAUNCHES[launch]
    corpus, ref = star_case(E, align, 8, d, n, False)
    node0, edges = corpus[0], corpus[1]
    V = len(node0)
    got = run(corpus, n, STAR_LR, all_hot(V), opts)
    bound = np.zeros(V)
    for a, b, u in oc.runs_of(edges, V):
        if b - a > 1:
            bound[u] = (b - a + 1) * 2.0 ** -24
    centres = bound > 0
    assert centres.sum() > 20 and np.abs(ref[centres]).max() < 1.0
    exact = ~centres  # leaves, centres of single-edge runs, pool rows
    bad = np.flatnonzero((got[exact] != ref[exact]).any(axis=1))
    assert bad.size == 0, "rows that differ: %s" % np.flatnonzero(exact)[bad][:20]
    diff = np.abs(got.astype(np.float64) - ref)
    over = np.flatnonzero((diff > bound[:, None]).any(axis=1) & centres)
    assert over.size == 0, "centre rows past (r + 1) 2^-24: %s, max %.3g" % (
        over[:20], diff[over].max())
    assert (got[centres] != ref[centres]).any()  # the atomic path ran: cold is bit-equal to ref


# ---- e. one chunk, shared rows, all rows hot ---------------------------------------------------

@pytest.mark.parametrize("d,n", [(128, 5), (100, 5)])
def test_one_chunk_shared_rows_hot_tier_b(d, n):
    """Corpus a with every row updated by float-atomic deltas, one wavefront: tier B, as
    tests/test_gpu_stream.py::test_one_wavefront_contended_rows_tier_b."""
    corpus, ref = shared_case(d, n)
    got = run(corpus, n, LR, all_hot(len(corpus[0])), {"o1_chunk": len(corpus[1])})
    diff = np.abs(got - ref)
    print("max |diff| %.3g, share within 1e-5 %.4f" % (diff.max(), np.mean(diff <= 1e-5)))
    assert diff.max() <= 1e-3, diff.max()
    assert np.mean(diff <= 1e-5) > 0.95, np.mean(diff <= 1e-5)


# ---- f. no update lost -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hub_refs(orient):
    E, d, lr = 2048, 128, 5e-5
    corpus = oc.hub_corpus(E, d, orient)
    seq = oc.o1_ref64(corpus[0], corpus[1], lr)
    stale = oc.o1_ref64(corpus[0], corpus[1], lr, stale_row=0)
    return corpus, seq, stale


@pytest.mark.parametrize("orient,chunk", [(0, 0), (1, 8), (1, 0), (0, 8)])
def test_hub_loses_no_update(orient, chunk):
    """2048 edges on one hub whose bit is set, lr = 5e-5, n = 0.  orient 0, per-edge kernel: the
    hub is pair 2's input, every edge adds to it atomically.  orient 1, chunks of 8: the hub is
    the held row of 256 chunks, each flushing its delta atomically.  The other two launches put
    the hub at pair 1 of the per-edge kernel and at pair 2 of the run kernel (runs of one edge),
    the two remaining places where a hot bit is read.  Wavefronts may read the hub
    stale (that is Hogwild); what they may not do is lose an update.  Against the float64
    sequential run the hub must lie within B = 4 |stale - seq| + sqrt(d) 2^-24 sqrt(E) -- four
    times what reading the hub as it was before the launch for every edge costs, plus fp32
    rounding of E adds; losing every eighth update costs 2.75 B
    (tests/test_o1_corpora_host.py).  Each leaf is updated once from one read of the hub."""
    (node0, edges, seeds, table), seq, stale = hub_refs(orient)
    E, d = len(edges), node0.shape[1]
    corpus = (node0, edges, seeds, table)
    hot = torch.zeros((E + 1 + 31) // 32, dtype=torch.int32, device=DEV)
    hot[0] = 1
    got = run(corpus, 0, 5e-5, hot, {"o1_chunk": chunk}).astype(np.float64)
    B = 4 * np.linalg.norm(stale[0] - seq[0]) + np.sqrt(d) * 2.0 ** -24 * np.sqrt(E)
    leaf_bound = 4 * np.abs(stale[1:] - seq[1:]).max() + 2.0 ** -23
    dist = np.linalg.norm(got[0] - seq[0])
    leaf = np.abs(got[1:] - seq[1:]).max()
    cold = run(corpus, 0, 5e-5, None, {"o1_chunk": chunk}).astype(np.float64)
    print("orient %d chunk %d: hub %.3g (B = %.3g, drift %.3g), leaves %.3g (bound %.3g); "
          "hot=None (not asserted: a race): hub %.3g" % (
              orient, chunk, dist, B, np.linalg.norm(seq[0] - node0[0]), leaf, leaf_bound,
              np.linalg.norm(cold[0] - seq[0])))
    assert dist <= B, (dist, B)
    assert leaf <= leaf_bound, (leaf, leaf_bound)


# ---- g. derived bitmap -------------------------------------------------------------------------

@pytest.mark.parametrize("d", [128, 256])
def test_derived_hot_bitmap_matches_explicit(d):
    """hot="auto" (hot_rows == NULL: the library derives the bitmap from the table, plain or
    packed) equals the explicit come_hot_rows bitmap at default_hot_share(d) bit for bit, and
    differs from hot=None.  Star corpus without draws (n = 0), four wavefronts of one chunk each;
    the table is Zipf with its heaviest rows on centres of runs of four or more edges, whose
    atomic delta rounds differently from the plain store."""
    E, align, _ = STAR_LAUNCHES["auto"]
    corpus, _ = star_case(E, align, 8, d, 0, False)
    node0, edges = corpus[0], corpus[1]
    V = len(node0)
    rng = np.random.RandomState(d)
    long_runs = [u for a, b, u in oc.runs_of(edges, V) if b - a >= 4 and u > 0]  # row 0: no id
    assert len(long_runs) > 20
    rest = np.setdiff1d(np.arange(1, V), long_runs)
    order = np.concatenate([long_runs, rng.permutation(rest)])  # rows, heaviest first
    # exponent 1.2: most of the ~700 rows stay below 5 slots of the table, the head far above
    counts = np.ones(V, np.float64)
    counts[order - 1] = np.sort(rng.zipf(1.2, V - 1).astype(np.float64).clip(1, 1e10))[::-1]
    T = int(5.5 / tsi.default_hot_share(d))  # a hot row holds at least 5 slots
    table = orc.make_table(counts, T)
    tab = dev(table)
    packed = tsi.pack_table(tab)
    assert packed is not None
    explicit = tsi.hot_rows(tab, V, max(1, int(tsi.default_hot_share(d) * T)))
    bits = np.unpackbits(explicit.cpu().numpy().view(np.uint8), bitorder="little")[:V]
    assert 10 < bits.sum() < V // 2, bits.sum()
    assert bits[long_runs[:10]].all()
    opts = {"max_waves": 1}
    ref = run(corpus, 0, STAR_LR, explicit, opts, table=tab)
    for t in (tab, packed):
        got = run(corpus, 0, STAR_LR, "auto", opts, table=t)
        np.testing.assert_array_equal(got, ref)
    cold = run(corpus, 0, STAR_LR, None, opts, table=tab)
    assert not np.array_equal(cold, ref)
