"""come_quiet_rows (k_table_counts, k_quiet_sum, k_quiet_bits) and the product's way to it
(training_sdg_inner.quiet_rows, Model.quiet_rows, Context2Vec.quiet_rows) against the numpy float64
restatement of the rule in tests/quiet_rule.py.

The bitmap must equal the reference word for word, tail bits included, `counts` exactly and `sum`
within 1e-12 relative (an unordered fp64 atomic sum of at most 20000 terms).  Only the device's
pow() and the order of the sum can differ from the reference, by a few 1e-16: before anything is
launched every case asserts that no row sits within 1e-9 (relative) of its bound, so no row is
left out of the comparison (smallest margin over all cases: 3.0e-3, printed per case).  A case whose
bitmap would be empty or full shows little, so that is asserted on the reference too, and so is
that the case can see the mistakes it is there for: the hot exclusion changes the bitmap, reading
counts[r] for counts[r + id_shift] changes it, a cold row past V would be marked.
"""
import functools
import math

import numpy as np
import pytest
import torch

import quiet_cases as qc
import quiet_rule as qr
from come_amd import _lib
from come_amd._lib import ptr, stream_handle
import come_amd.training_sdg_inner as tsi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INVALID = -1  # COME_E_INVALID
MIN_MARGIN = 1e-9
JUNK = np.array([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF], np.uint32)


def dev(a):
    a = np.array(a)  # a copy: the cached inputs are read-only
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(DEV)


def heavy_rows(V, n, rng):
    """n row numbers with a heavy tail over a random order of the rows: some rows often, many
    never."""
    return rng.permutation(V)[(rng.zipf(1.3, n) - 1) % V].astype(np.uint32)


@functools.lru_cache(maxsize=None)
def make_input(V, T, kind):
    """uint32 [T], read-only.  runs: make_table's (whole wavefronts of one value: the
    uniform-wave shortcut); shuffled: the same slots in random order (per-lane atomics); run7 /
    run65: runs of that length, whose boundaries fall at every offset inside a wavefront; junk:
    shuffled, with values >= V strewn in and one stretch of them longer than two wavefronts;
    heavy: one heavy-tailed draw per slot."""
    rng = np.random.RandomState(V + T % 1000)
    seed = {64: 6, 4097: 0, 20000: 0}.get(V, 1)
    if kind == "runs":
        table = qc.degree_table(V, T, seed)[1].copy()
    elif kind in ("shuffled", "junk"):
        table = rng.permutation(qc.degree_table(V, T, seed)[1])
        if kind == "junk":
            where = rng.rand(T) < 0.05
            table[where] = rng.choice(np.concatenate([JUNK, np.array([V, V + 1], np.uint32)]),
                                      int(where.sum()))
            if T > 400:
                table[T // 3:T // 3 + 150] = 0xFFFFFFFF
    elif kind in ("run7", "run65"):
        run = int(kind[3:])
        table = np.repeat(heavy_rows(V, -(-T // run), rng), run)[:T].copy()
    elif kind == "heavy":
        table = heavy_rows(V, T, rng)
    else:
        raise ValueError(kind)
    assert table.shape == (T,) and table.dtype == np.uint32
    table.setflags(write=False)
    return table


def hot_min_of(counts, hot, T):
    """The hot threshold of a case: 1, T + 1 (nothing hot) or, for "share", the slot count that
    makes 5-30 rows hot."""
    if hot == "one":
        return 1
    if hot == "none":
        return T + 1
    c = int(np.sort(counts)[-8])
    n = int((counts >= c).sum())
    assert c >= 2 and 5 <= n <= 30, (c, n)
    return c


def split_visitors(counts, V, eps, hot_min, power, id_shift):
    """A visitor count that puts the bound between the two middle values of counts[own]^(1/power)
    among the rows the integer conditions leave: some of them quiet, some not, none borderline."""
    x = counts.astype(np.float64) ** (1.0 / power)
    own = np.arange(V) + id_shift
    left = (own >= 0) & (own < V) & (counts < hot_min)
    xs = np.unique(x[own[left]])
    assert len(xs) >= 2, xs
    lo, hi = xs[len(xs) // 2 - 1], xs[len(xs) // 2]
    bound = math.sqrt(lo * hi) if lo > 0 else hi / 2
    return eps * math.fsum(x.tolist()) / bound


def reference(table, V, T, id_shift, power, eps, hot, visitors):
    counts = qr.table_counts(table, V)
    hot_min = hot_min_of(counts, hot, T)
    if visitors is None:
        visitors = split_visitors(counts, V, eps, hot_min, power, id_shift)
    quiet, total, margin = qr.quiet_bits(counts, V, visitors, eps, hot_min, power=power,
                                         id_shift=id_shift)
    return counts, hot_min, visitors, quiet, total, margin


class Buffers(object):
    """counts [V], sum [1] and bits [ceil(V / 32)] on the device, every byte 0xFF.  counts is the
    front of a longer buffer whose rest is 0: a kernel that looked at rows past V would find them
    cold, and mark them where the rule lets it."""

    def __init__(self, V):
        flat = torch.zeros(V + 64, dtype=torch.int32, device=DEV)
        self.counts = flat[:V]
        self.counts.fill_(-1)
        self.total = torch.full((8,), 0xFF, dtype=torch.uint8, device=DEV).view(torch.float64)
        self.bits = torch.full(((V + 31) // 32,), -1, dtype=torch.int32, device=DEV)


def call(table, T, V, power, id_shift, visitors, eps, hot_min, counts, total, bits):
    table, counts, total, bits = (None if t is None else ptr(t)
                                  for t in (table, counts, total, bits))
    return _lib.lib().come_quiet_rows(table, T, V, power, id_shift, visitors, eps, hot_min,
                                      counts, total, bits, stream_handle(DEV))


def check_outputs(buf, counts, total, quiet):
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf.counts.cpu().numpy().view(np.uint32), counts)
    got = float(buf.total[0])
    assert abs(got - total) <= 1e-12 * total, (got, total)
    np.testing.assert_array_equal(buf.bits.cpu().numpy().view(np.uint32), qr.pack_bits(quiet))


# id, V, T, table, id_shift, power, eps, hot, visitors (None: split_visitors)
CASES = [
    ("product", 20000, 2000000, "runs", 1, 0.75, 0.4, "share", 1408.0),
    ("shuffled", 4097, 100003, "shuffled", 1, 0.75, 0.05, "share", 300.0),
    ("shift0-power1", 4097, 100003, "runs", 0, 1.0, 1.6, "none", 300.0),
    ("junk-shift-1", 4097, 100003, "junk", -1, 0.75, 0.4, "share", 300.0),
    ("run7-eps0", 4097, 100003, "run7", 1, 0.75, 0.0, "share", 300.0),
    ("wave", 64, 2560, "runs", 1, 0.75, 0.4, "share", 11.0),
    ("run65-power1", 64, 2560, "run65", 1, 1.0, 0.05, "none", None),
    ("shift-V", 64, 2560, "runs", 64, 0.75, 1.6, "none", 11.0),
    ("V33-T65-hot1", 33, 65, "run7", 1, 0.75, 0.4, "one", None),
    ("V32-T64", 32, 64, "heavy", 1, 0.75, 1.6, "share", None),
    ("V31-T63-junk", 31, 63, "junk", 0, 0.75, 0.05, "none", None),
    ("V33-T5-tail", 33, 5, "short", -1, 0.75, 0.0, "none", 3.0),
]


@pytest.mark.parametrize("name,V,T,kind,id_shift,power,eps,hot,visitors", CASES,
                         ids=[c[0] for c in CASES])
def test_exact_bitmap_counts_and_sum(name, V, T, kind, id_shift, power, eps, hot, visitors):
    """The device words, counts and sum against the reference; the quiet rows disjoint from
    come_hot_rows at the same threshold; every output rewritten in full (buffers of 0xFF bytes,
    two calls on the same buffers)."""
    if kind == "short":  # shorter than a wavefront; no slot holds row 32 = V - 1
        table = np.array([3, 3, 7, 0xFFFFFFFF, 31], np.uint32)
    else:
        table = make_input(V, T, kind)
    counts, hot_min, visitors, quiet, total, margin = reference(table, V, T, id_shift, power, eps,
                                                                hot, visitors)
    print("%s: %d of %d rows quiet, %d hot (>= %d slots), visitors %.6g, smallest margin %.3g"
          % (name, quiet.sum(), V, (counts >= hot_min).sum(), hot_min, visitors, margin.min()))
    assert margin.min() >= MIN_MARGIN  # no row is borderline: every row is compared
    own = np.arange(V) + id_shift
    held = (own >= 0) & (own < V)
    if held.any():
        assert 0 < quiet.sum() < V
    else:
        assert not quiet.any()  # id_shift = V: the kernel has to clear words of 0xFF
    if hot == "share":  # ... and the case sees a missing hot exclusion
        cold_too = qr.quiet_bits(counts, V, visitors, eps, T + 1, power=power,
                                 id_shift=id_shift)[0]
        assert (cold_too & ~quiet).any()
    if id_shift != 0 and held.any():  # ... and counts[r] read for counts[r + id_shift]
        unshifted = qr.quiet_bits(counts, V, visitors, eps, hot_min, power=power, id_shift=0)[0]
        assert ((unshifted & held) != quiet).any()
    if name == "V33-T5-tail":  # ... and a missing r < V: row 33 (cold in Buffers) would be quiet
        assert V % 32 and counts[V - 1] == 0 and eps == 0.0 and id_shift == -1

    tab = dev(table)
    buf = Buffers(V)
    for _ in range(2):
        assert call(tab, T, V, power, id_shift, visitors, eps, hot_min, buf.counts, buf.total,
                    buf.bits) == 0
        check_outputs(buf, counts, total, quiet)
    hot_counts = torch.full((V,), -1, dtype=torch.int32, device=DEV)
    hot_words = torch.full(((V + 31) // 32,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().come_hot_rows(ptr(tab), T, V, hot_min, ptr(hot_counts), ptr(hot_words),
                                        stream_handle(DEV)), "come_hot_rows")
    np.testing.assert_array_equal(hot_words.cpu().numpy().view(np.uint32),
                                  qr.pack_bits(qr.hot_bits(counts, hot_min)))
    assert not bool((hot_words & buf.bits).any())


@pytest.mark.parametrize("visitors,want", [(1.0, True), (2.0, False)])
def test_one_row(visitors, want):
    """V = 1 (a bitmap of one bit is always empty or full, so both): row 0 holds every slot, its
    share is 1 and it is quiet iff visitors <= eps.  At id_shift = 1 it never is."""
    table = np.array([0, 0, 0xFFFFFFFF, 0, 0], np.uint32)
    tab = dev(table)
    counts = qr.table_counts(table, 1)
    assert counts.tolist() == [4]
    for id_shift in (0, 1):
        quiet, total, margin = qr.quiet_bits(counts, 1, visitors, 1.6, 6, id_shift=id_shift)
        assert quiet.tolist() == [want and id_shift == 0] and margin.min() >= MIN_MARGIN
        buf = Buffers(1)
        assert call(tab, 5, 1, 0.75, id_shift, visitors, 1.6, 6, buf.counts, buf.total,
                    buf.bits) == 0
        check_outputs(buf, counts, total, quiet)


def test_python_entry_matches_the_reference():
    """training_sdg_inner.quiet_rows (its own scratch, the default power and shift)."""
    V, T = 4097, 100003
    table = make_input(V, T, "shuffled")
    counts, hot_min, visitors, quiet, _, margin = reference(table, V, T, 1, 0.75, 0.05, "share",
                                                            300.0)
    assert margin.min() >= MIN_MARGIN and 0 < quiet.sum() < V
    bits = tsi.quiet_rows(dev(table), V, visitors, 0.05, hot_min)
    assert bits.dtype == torch.int32
    np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), qr.pack_bits(quiet))


NAN = float("nan")
BAD = [
    ("V=0", dict(V=0)), ("V<0", dict(V=-5)), ("T=0", dict(T=0)),
    ("table=NULL", dict(table=None)), ("counts=NULL", dict(counts=None)),
    ("sum=NULL", dict(total=None)), ("bits=NULL", dict(bits=None)),
    ("power=0", dict(power=0.0)), ("power<0", dict(power=-0.75)), ("power=NaN", dict(power=NAN)),
    ("visitors=0", dict(visitors=0.0)), ("visitors<0", dict(visitors=-3.0)),
    ("visitors=NaN", dict(visitors=NAN)), ("eps<0", dict(eps=-1e-9)), ("eps=NaN", dict(eps=NAN)),
]


@pytest.mark.parametrize("what,bad", BAD, ids=[b[0] for b in BAD])
def test_invalid_arguments_are_refused_and_write_nothing(what, bad):
    V, T = 33, 65
    tab = dev(make_input(V, T, "run7"))
    outs = dict(counts=torch.full((4 * V,), 0xA5, dtype=torch.uint8, device=DEV),
                total=torch.full((8,), 0xA5, dtype=torch.uint8, device=DEV),
                bits=torch.full((8,), 0xA5, dtype=torch.uint8, device=DEV))
    args = dict(table=tab, T=T, V=V, power=0.75, id_shift=1, visitors=11.0, eps=0.4, hot_min=5)
    args.update(outs)
    args.update(bad)
    rc = call(args["table"], args["T"], args["V"], args["power"], args["id_shift"],
              args["visitors"], args["eps"], args["hot_min"], args["counts"], args["total"],
              args["bits"])
    torch.cuda.synchronize()
    assert rc == INVALID, (what, rc)
    assert b"quiet_rows" in _lib.lib().come_last_error()
    for name, t in outs.items():
        assert bool((t == 0xA5).all()), (what, name)
    # and the same buffers are fine for a good call
    good = dict(args)
    good.update(table=tab, T=T, V=V, power=0.75, visitors=11.0, eps=0.4, **outs)
    assert call(good["table"], good["T"], good["V"], good["power"], good["id_shift"],
                good["visitors"], good["eps"], good["hot_min"], good["counts"], good["total"],
                good["bits"]) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(outs["counts"].cpu().numpy().view(np.uint32),
                                  qr.table_counts(make_input(V, T, "run7"), V))


# ---- the product's way to the kernel ----

PV, PT, PD = 4097, 100003, 128


def product_model(d=PD, ids=None):
    from come_amd.model import Model
    deg = qc.degree_table(PV, PT, 0)[0]
    np.random.seed(0)
    ids = np.arange(1, PV + 1) if ids is None else ids
    return Model((ids, deg.copy()), size=d, table_size=PT, k=2, device=DEV)


def share_for(counts, T):
    """(share, hot_min): a table share that makes 5-30 rows hot, hot_min = max(1, int(share T))."""
    hot_min = hot_min_of(counts, "share", T)
    share = (hot_min + 0.5) / T
    assert max(1, int(share * T)) == hot_min
    return share, hot_min


def model_reference(model, visitors, eps, hot_min, some=True):
    counts = qr.table_counts(model.table_host, model.vocab_size)
    quiet, _, margin = qr.quiet_bits(counts, model.vocab_size, visitors, eps, hot_min)
    assert margin.min() >= MIN_MARGIN
    assert not some or 0 < quiet.sum() < model.vocab_size
    return qr.pack_bits(quiet)


def words(t):
    return t.cpu().numpy().view(np.uint32)


def test_model_quiet_rows():
    model = product_model()
    np.testing.assert_array_equal(model.table_host, qc.degree_table(PV, PT, 0)[1])
    share, hot_min = share_for(qr.table_counts(model.table_host, PV), PT)
    waves, w, eps = 60, 2, 0.05
    got = model.quiet_rows(waves, w, eps, share)
    want = model_reference(model, waves * (2 * w + 1), eps, hot_min)
    np.testing.assert_array_equal(words(got), want)
    assert model.quiet_rows(waves, w, eps, share) is got  # cached
    hot = model.hot_rows(share)
    np.testing.assert_array_equal(
        words(hot), qr.pack_bits(qr.hot_bits(qr.table_counts(model.table_host, PV), hot_min)))
    assert bool(hot.any()) and not bool((hot & got).any())
    # the default eps is DEFAULT_QUIET_EPS
    np.testing.assert_array_equal(
        words(model.quiet_rows(waves, w, None, share)),
        model_reference(model, waves * (2 * w + 1), tsi.DEFAULT_QUIET_EPS, hot_min))
    assert model.quiet_rows(waves, w, 0.0, share) is None
    assert model.quiet_rows(waves, w, -0.4, share) is None
    # a new table: the bitmap of the new table, wherever the allocator put it
    model.counts = model.counts[::-1].copy()
    old_table = model.table_host.copy()
    del got, hot
    model.make_table()
    assert not np.array_equal(model.table_host, old_table)
    share2, hot_min2 = share_for(qr.table_counts(model.table_host, PV), PT)
    want2 = model_reference(model, waves * (2 * w + 1), eps, hot_min2)
    assert not np.array_equal(want2, want)
    np.testing.assert_array_equal(words(model.quiet_rows(waves, w, eps, share2)), want2)


def test_model_quiet_rows_needs_ids_1_to_V():
    ids = np.arange(1, PV + 1)
    ids[-1] = PV + 5
    model = product_model(ids=ids)
    assert model.quiet_rows(60, 2, 0.4, 1e-3) is None
    assert model.hot_rows(1e-3) is not None


def launch_waves(c2v, walks):
    """The wavefronts a Hogwild launch of `walks` walks keeps in flight, as DESIGN.md §3.1 and
    Context2Vec.quiet_rows' docstring state it."""
    opts = c2v.launch_opts or {}
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    waves = 4 * (opts.get("o2_blocks_per_cu", 0) or tsi.QUIET_BLOCKS_PER_CU) * cus
    if opts.get("max_waves", 0) > 0:
        waves = min(waves, opts["max_waves"])
    return max(1, min(waves, walks, c2v.batch_walks))


def test_context2vec_quiet_rows():
    from come_amd.context_embeddings import Context2Vec
    model = product_model()
    share, hot_min = share_for(qr.table_counts(model.table_host, PV), PT)
    kw = dict(window_size=2, negative=5, hot_share=share, quiet_eps=0.2)
    seen = set()
    # the last two are whole grids: thousands of wavefronts on 4097 rows leave no row quiet, but
    # the bitmap is still the one of that many wavefronts
    for extra, walks in ((dict(), 100), (dict(launch_opts={"max_waves": 64}), 100000),
                         (dict(batch_walks=50), 100000),
                         (dict(launch_opts={"o2_kernel": 3}), 100000),
                         (dict(launch_opts={"o2_kernel": 3, "o2_blocks_per_cu": 2}), 100000)):
        c2v = Context2Vec(**dict(kw, **extra))
        waves = launch_waves(c2v, walks)
        seen.add(waves)
        got = c2v.quiet_rows(model, walks)
        assert got is model.quiet_rows(waves, 2, 0.2, share), (extra, waves)
        np.testing.assert_array_equal(words(got), model_reference(model, waves * 5, 0.2, hot_min,
                                                                  some=waves <= 100))
    assert len(seen) == 5  # five different launches, five different rules
    # no bitmap where the windowed stream kernel does not run, or the rule is switched off
    assert Context2Vec(**dict(kw, window_size=6)).quiet_rows(model, 100) is None
    assert Context2Vec(**dict(kw, negative=6)).quiet_rows(model, 100) is None
    assert Context2Vec(**dict(kw, quiet_eps=0)).quiet_rows(model, 100) is None
    assert PV < 32 * 200
    assert Context2Vec(**kw).quiet_rows(model, 200) is None  # the direct kernel's launch
    assert Context2Vec(**dict(kw, launch_opts={"o2_kernel": 3})).quiet_rows(model, 200) \
        is not None
    wide = product_model(d=256)
    assert Context2Vec(**kw).quiet_rows(wide, 100) is None
    assert wide.quiet_rows(100, 2, 0.2, share) is not None


@pytest.mark.parametrize("deterministic", [False, True])
def test_train_rows_asks_for_the_bitmap_only_in_hogwild_mode(deterministic):
    from come_amd.context_embeddings import Context2Vec
    model = product_model()
    calls = []
    real = model.quiet_rows

    def spy(*args, **kwargs):
        calls.append(args)
        return real(*args, **kwargs)

    model.quiet_rows = spy
    rng = np.random.RandomState(4)
    P = 100
    rows = rng.randint(0, PV, (P, 8)).astype(np.int32)
    seeds = rng.randint(0, 2 ** 48, P, dtype=np.int64).astype(np.uint64)
    c2v = Context2Vec(window_size=2, negative=5, deterministic=deterministic)
    before = model.node_embedding.clone()
    c2v.train_rows(model, rows, seeds)
    torch.cuda.synchronize()
    assert not torch.equal(before, model.node_embedding)
    if deterministic:
        assert calls == []
    else:
        assert calls == [(launch_waves(c2v, P), 2, tsi.DEFAULT_QUIET_EPS, None)]
