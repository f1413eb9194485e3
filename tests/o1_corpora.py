"""Edge corpora for deterministic tests of the Hogwild O1 kernels (k_sgns_o1, k_sgns_o1_runs) and a
float64 restatement of O1 without negatives.  No GPU here: tests/test_o1_corpora_host.py checks the
builders on the CPU, tests/test_gpu_o1_hogwild.py runs the kernels over what they build.

Every builder returns ``node0, edges, seeds, table`` (float32 [V, d], int32 [E, 2], uint64 [E],
uint32 [T]) and asserts the properties its tests rely on:

  * shared_corpus:   few rows, every row shared by many edges -- only for launches in which one
                     wavefront takes every edge in order;
  * matching_corpus: no row is read or written by two edges, so any number of wavefronts in any
                     order computes what the sequential oracle computes;
  * star_corpus:     runs of edges sharing their first endpoint (what k_sgns_o1_runs holds in
                     registers), rows private to a block of `align` consecutive edges, so a launch
                     whose chunks are those blocks is deterministic;
  * hub_corpus:      every edge touches row 0 -- the contended row whose updates must not be lost.
"""
import numpy as np

LCG_MUL, LCG_ADD, MASK48 = np.uint64(25214903917), np.uint64(11), np.uint64((1 << 48) - 1)
POOL = 3                    # private rows per edge / star that are drawn but never an endpoint
TABLE_SLOTS = (1 << 21) - 5  # odd size: slot = (state >> 16) % T is a real modulo


def lcg_slots(seeds, count, T):
    """Table slots of `count` consecutive draws from each seed (pyx:133-134)."""
    nr = np.asarray(seeds, np.uint64).copy()
    out = np.empty((len(nr), count), np.int64)
    with np.errstate(over="ignore"):
        for k in range(count):
            out[:, k] = ((nr >> np.uint64(16)) % np.uint64(T)).astype(np.int64)
            nr = (nr * LCG_MUL + LCG_ADD) & MASK48
    return out


def exp_table():
    """EXP_TABLE as generated from pyx:531-533 (float32 [1000])."""
    q = np.arange(1000, dtype=np.float32) / np.float32(1000)
    e = np.exp((q.astype(np.float64) * 2.0 - 1.0) * 6.0).astype(np.float32)
    return (e.astype(np.float64) / (e.astype(np.float64) + 1.0)).astype(np.float32)


def valid_edges(edges, V):
    """Mask of the edges the kernels process: both endpoints in [0, V)."""
    e = np.asarray(edges, np.int64)
    return ((e >= 0) & (e < V)).all(axis=1)


def oracle_edges(edges, V):
    """`edges` for the CPU oracle, which skips an edge only for a negative endpoint and would
    index past the table for one >= V (the kernels skip both): such endpoints become -1."""
    out = np.array(edges, np.int32)
    out[~valid_edges(edges, V)] = -1
    return out


def runs_of(edges, V):
    """[(first edge, one past the last, u)] of the maximal runs of processed edges with the same
    first endpoint -- what k_sgns_o1_runs holds in registers when a chunk contains the run."""
    ok = valid_edges(edges, V)
    out = []
    for e in np.flatnonzero(ok):
        u = int(edges[e, 0])
        if out and out[-1][2] == u:  # a skipped edge in between does not end the run
            out[-1][1] = int(e) + 1
        else:
            out.append([int(e), int(e) + 1, u])
    return [tuple(r) for r in out]


def _place(rng, seeds, e, draws, T, owner, me):
    """Re-draw seeds[e] until the slots of its `draws` draws are free or already `me`'s; claims
    them and returns them."""
    for _ in range(400):
        s = lcg_slots(seeds[e:e + 1], draws, T)[0]
        if np.isin(owner[s], (-1, me)).all():
            owner[s] = me
            return s
        seeds[e] = np.uint64(rng.randint(0, 2 ** 48, dtype=np.int64))
    raise AssertionError("could not place edge %d" % e)


def shared_corpus(E, V, n, d, seed):
    """E edges over V rows sorted by their first endpoint, every 17th a self-loop, one edge with an
    endpoint of -1 and one with V + 3 (both skipped); draws from a table over every row."""
    rng = np.random.RandomState(seed)
    assert E >= 18
    table = np.sort(rng.randint(0, V, 997)).astype(np.uint32)
    node0 = rng.uniform(-0.5, 0.5, (V, d)).astype(np.float32)
    edges = rng.randint(0, V, (E, 2)).astype(np.int32)
    edges[::17, 1] = edges[::17, 0]
    edges = edges[np.argsort(edges[:, 0], kind="stable")]
    edges[5, 0] = -1
    edges[11, 1] = V + 3
    seeds = rng.randint(0, 2 ** 48, E, dtype=np.int64).astype(np.uint64)
    ok = valid_edges(edges, V)
    assert (~ok).sum() == 2 and (edges[ok, 0] == edges[ok, 1]).sum() >= E // 17 - 2
    assert (np.diff(edges[ok, 0]) >= 0).all()
    assert len(runs_of(edges, V)) < ok.sum()  # some first endpoint is held over several edges
    assert table.max() < V
    return node0, edges, seeds, table


def matching_corpus(E, n, d, seed, T=TABLE_SLOTS):
    """E edges that share nothing.  Edge e owns rows [5e, 5e + 5): u = 5e, v = 5e + 1 (every 17th
    edge is the self-loop (u, u)) and a pool of 3 rows that is never an endpoint; edge 5 has u = -1
    and edge 11 v = V + 3 (skipped: their rows are never written).  Its 2n draws hit table slots
    no other edge draws (the seed is re-drawn until so), mapped to its own u, its own v or its
    pool: draws equal to u, equal to v and repeated draws all occur."""
    rng = np.random.RandomState(seed)
    assert E >= 18
    B = 2 + POOL
    V = E * B
    base = np.arange(E) * B
    edges = np.stack([base, base + 1], axis=1).astype(np.int32)
    edges[::17, 1] = edges[::17, 0]
    edges[5, 0] = -1
    edges[11, 1] = V + 3
    ok = valid_edges(edges, V)
    seeds = rng.randint(0, 2 ** 48, E, dtype=np.int64).astype(np.uint64)
    node0 = rng.uniform(-0.5, 0.5, (V, d)).astype(np.float32)
    draws = 2 * n
    if n == 0:
        T = 64  # no draws: a placeholder table
    owner = np.full(T, -1, np.int64)
    table = np.zeros(T, np.uint32)
    for e in np.flatnonzero(ok):
        s = _place(rng, seeds, e, draws, T, owner, e)
        cand = np.concatenate([np.unique(edges[e]), base[e] + 2 + np.arange(POOL)])
        table[s] = rng.choice(cand, draws)
    # what was built
    slots = lcg_slots(seeds, draws, T)
    drawn = table[slots].astype(np.int64)  # [E, 2n] rows drawn (skipped edges draw nothing)
    row_owner = np.full(V, -1, np.int64)
    for e in np.flatnonzero(ok):
        assert (owner[slots[e]] == e).all()
        rows = np.unique(np.concatenate([edges[e], drawn[e]]))
        assert (row_owner[rows] == -1).all(), "row shared by two edges"
        row_owner[rows] = e
    for e in np.flatnonzero(~ok):
        assert (row_owner[base[e]:base[e] + B] == -1).all()
    if n:
        u, v = edges[ok, 0:1], edges[ok, 1:2]
        p1, p2 = drawn[ok][:, :n], drawn[ok][:, n:]
        assert (p1 == u).any() and (p2 == v).any()    # a negative equal to the pair's input row
        assert (p1 == v).any() and (p2 == u).any()    # equal to the positive: skipped (pyx:135)
        assert n == 1 or any(len(np.unique(r)) < len(r) for r in p1)
    return node0, edges, seeds, table


def star_corpus(E, align, max_run, n, d, seed, own_rows=True, T=TABLE_SLOTS):
    """E edges sorted into runs (u_s, v_s1), (u_s, v_s2), ... of 1..max_run edges, one run per
    centre u_s; no run crosses a multiple of `align` and every block of `align` edges holds
    several.  The leaves of a star are distinct rows; in some runs of two or more edges one leaf is
    u_s itself.  Every row belongs to one star: its centre, its leaves and a pool of 3 rows that is
    never an endpoint.  Draws hit slots no other star draws, mapped to the star's own rows and
    pool (own_rows=False: the pool only, so no drawn row is ever written by the launch)."""
    rng = np.random.RandomState(seed)
    assert align >= 2 and E >= 2
    lengths, pos = [], 0
    while pos < E:
        room = min(align - pos % align, E - pos)
        cap = min(max_run, room)
        if pos % align == 0 and room > 1:
            cap = min(cap, room - 1)  # the block's first run leaves room for a second
        lengths.append(int(rng.randint(1, cap + 1)))
        pos += lengths[-1]
    edges = np.empty((E, 2), np.int32)
    star = np.empty(E, np.int64)
    rows_of_star, row, e = [], 0, 0
    for s, r in enumerate(lengths):
        centre, leaves = row, row + 1 + np.arange(r)
        pool = row + 1 + r + np.arange(POOL)
        rows_of_star.append((centre, leaves.copy(), pool))
        if r >= 2 and s % 3 == 0:
            leaves[rng.randint(r)] = centre
        edges[e:e + r, 0] = centre
        edges[e:e + r, 1] = leaves
        star[e:e + r] = s
        row, e = row + 1 + r + POOL, e + r
    V = row
    seeds = rng.randint(0, 2 ** 48, E, dtype=np.int64).astype(np.uint64)
    node0 = rng.uniform(-0.4, 0.4, (V, d)).astype(np.float32)
    draws = 2 * n
    table = np.zeros(T if n else 64, np.uint32)
    if n:
        owner = np.full(T, -1, np.int64)
        for e in range(E):
            _place(rng, seeds, e, draws, T, owner, star[e])
        for s, (centre, leaves, pool) in enumerate(rows_of_star):
            mine = np.flatnonzero(owner == s)
            cand = np.concatenate([[centre], leaves, pool]) if own_rows else pool
            table[mine] = rng.choice(cand, len(mine))
    # what was built
    runs = runs_of(edges, V)
    assert [b - a for a, b, _ in runs] == lengths
    assert len({u for _, _, u in runs}) == len(runs), "a first endpoint forms two runs"
    per_block = np.zeros((E + align - 1) // align, np.int64)
    for a, b, u in runs:
        assert a // align == (b - 1) // align, "run crosses a multiple of align"
        per_block[a // align] += 1
        leaves = edges[a:b, 1]
        assert len(np.unique(leaves)) == b - a
        assert b - a >= 2 or leaves[0] != u  # a self-loop only inside a longer run
    size = np.minimum(align, E - align * np.arange(len(per_block)))
    assert (per_block[size > 1] >= 2).all()
    loops = edges[:, 0] == edges[:, 1]
    assert loops.any() and (~loops).any()
    assert min(lengths) == 1 and max(lengths) >= min(max_run, align - 1, 4)
    drawn = table[lcg_slots(seeds, draws, T)].astype(np.int64) if n else np.zeros((E, 0), np.int64)
    row_block = np.full(V, -1, np.int64)
    row_star = np.full(V, -1, np.int64)
    for e in range(E):
        rows = np.unique(np.concatenate([edges[e], drawn[e]]))
        assert np.isin(row_star[rows], (-1, star[e])).all(), "row shared by two stars"
        assert np.isin(row_block[rows], (-1, e // align)).all(), "row shared by two blocks"
        row_star[rows], row_block[rows] = star[e], e // align
    if n:
        written = np.unique(edges)
        if own_rows:
            assert np.isin(drawn, written).any()  # negatives that read rows the launch writes
            assert (drawn[:, :n] == edges[:, :1]).any()  # ... the held row among them
        else:
            assert not np.isin(drawn, written).any()
    return node0, edges, seeds, table


def hub_corpus(E, d, orient):
    """Row 0 is the hub of E leaves (rows 1..E): edges (leaf_i, 0) for orient = 0, (0, leaf_i) for
    orient = 1; for n = 0 (no draws: seeds and table are placeholders).  Rows are
    uniform(-0.3, 0.3) + 0.1, so every dot product stays inside the +-6 band of the sigmoid
    table and every edge updates both of its rows."""
    rng = np.random.RandomState(7)
    node0 = (rng.uniform(-0.3, 0.3, (E + 1, d)) + 0.1).astype(np.float32)
    leaf = np.arange(1, E + 1, dtype=np.int32)
    hub = np.zeros(E, np.int32)
    edges = np.stack([leaf, hub] if orient == 0 else [hub, leaf], axis=1).astype(np.int32)
    x = node0.astype(np.float64)
    assert np.abs(x[1:] @ x[0]).max() < 4.0  # far inside +-6: stays so while the hub drifts
    return node0, edges, np.zeros(E, np.uint64), np.zeros(64, np.uint32)


def o1_ref64(node0, edges, lr, stale_row=None, drop_every=0, drop_row=None):
    """O1 without negatives (pyx:444-448 with negative = 0) in float64, edges in order: pair 1
    moves node[u] along node[v], pair 2 node[v] along the updated node[u]; the sigmoid is the
    reference's table lookup, a dot outside +-6 is skipped (pyx:141-143).

    stale_row: every read of that row returns its value before the launch, while its updates
    still accumulate -- the worst a Hogwild launch does to a contended row when it loses no
    update ("fully stale").  drop_every = k: every k-th update of drop_row (default: stale_row)
    is lost, as a plain store over a concurrent update loses it."""
    tab = exp_table().astype(np.float64)
    x = np.asarray(node0, np.float64).copy()
    x0 = x.copy()
    if drop_row is None:
        drop_row = stale_row
    seen = 0

    def read(r):
        return x0[r] if r == stale_row else x[r]

    def pair(inp, pos):
        nonlocal seen
        a, b = read(inp), read(pos)
        f = float(a @ b)
        if f <= -6.0 or f >= 6.0:
            return
        g = (1.0 - tab[int((f + 6.0) * 83.0)]) * lr
        if drop_every and inp == drop_row:
            seen += 1
            if seen % drop_every == 0:
                return
        x[inp] = x[inp] + g * b

    for u, v in np.asarray(edges, np.int64):
        if u < 0 or v < 0 or u >= len(x) or v >= len(x):
            continue
        pair(u, v)
        pair(v, u)
    return x
