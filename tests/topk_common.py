"""What the top-k tests share (tests/test_topk_host.py: the CPU twin; tests/test_gpu_topk.py: the
kernels): the float64 contract, the cases on real-valued data and the exact (integer-valued) data
whose answer is fully determined.

The contract, per query i and base row j, with s* the float64 scores and u = 2^-24:

    tolerance   dot     2 d u |q_i| |b_j|
                cosine  (4 d + 16) u
                l2      4 (d + 2) u (|q_i|^2 + |b_j|^2)

(the fp32 dot-product bound gamma_d sum |q_c b_c| <= d u |q| |b|, plus the norms' roundings for
cosine, doubled because the MFMA's summation order is not the chain's; for l2 the bound
tests/test_gpu_kmeans.py uses for the same expression)

    (a) the returned indices are distinct, in [0, V) or the -1 tail, never the excluded row
    (b) |score - s*[idx]| <= tol
    (c) best first; equal adjacent scores in ascending index
    (d) no wrong member: every returned element has s* >= sigma_k - 2 tol
    (e) no missing member: every base row with s* > sigma_(k+1) + 2 tol is returned

(d) and (e) are per element (l2: on the negated distance), so no query is left out.
"""
import numpy as np

U = 2.0 ** -24
METRICS = ("dot", "cosine", "l2")


def scores64(q, b, metric):
    """(rank [Q, V], tol [Q, V], cand [Q, V]): the float64 scores as a rank value (larger is
    better: the negated distance for l2), the tolerance, and which pairs are candidates at all (a
    NaN score is none)."""
    q64, b64 = q.astype(np.float64), b.astype(np.float64)
    d = q.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = q64 @ b64.T
        qn, bn = np.sqrt((q64 * q64).sum(1)), np.sqrt((b64 * b64).sum(1))
        if metric == "dot":
            s = dot
            tol = 2 * d * U * qn[:, None] * bn[None, :]
        elif metric == "cosine":
            iq = np.where(qn > 0, 1.0 / qn, np.where(qn == 0, 0.0, qn))
            ib = np.where(bn > 0, 1.0 / bn, np.where(bn == 0, 0.0, bn))
            s = dot * iq[:, None] * ib[None, :]
            tol = np.full(s.shape, (4 * d + 16) * U)
        else:
            sq = (qn * qn)[:, None] + (bn * bn)[None, :]
            s = -np.maximum(0.0, sq - 2 * dot)
            tol = 4 * (d + 2) * U * sq
    cand = ~np.isnan(s)
    return s, np.where(cand, tol, 0.0), cand


def check_contract(q, b, k, metric, idx, score, exclude=None, who="topk"):
    """Asserts (a) - (e) for every query.  idx int [Q, k], score fp32 [Q, k] as returned."""
    Q, V = q.shape[0], b.shape[0]
    idx = np.asarray(idx, np.int64)
    score = np.asarray(score)
    assert idx.shape == (Q, k) and score.shape == (Q, k) and score.dtype == np.float32, who
    s, tol, cand = scores64(q, b, metric)
    if exclude is not None:
        ex = np.asarray(exclude, np.int64)
        rows = np.nonzero(ex >= 0)[0]
        cand[rows, ex[rows]] = False
    s = np.where(cand, s, -np.inf)
    sign = -1.0 if metric == "l2" else 1.0
    ncand = cand.sum(1)
    order = np.sort(s, axis=1)[:, ::-1]  # best first (non-candidates: -inf, last)
    for i in range(Q):
        n = int(min(k, ncand[i]))
        got, sc = idx[i], score[i].astype(np.float64) * sign
        # (a)
        assert (got[n:] == -1).all() and (sc[n:] == -np.inf).all(), (who, i, "tail", got, sc)
        g = got[:n]
        assert ((g >= 0) & (g < V)).all() and len(set(g.tolist())) == n, (who, i, "indices", g)
        assert cand[i, g].all(), (who, i, "an excluded or NaN row was returned", g)
        # (b)
        err = np.abs(sc[:n] - s[i, g])
        assert (err <= tol[i, g]).all(), (who, i, "score", float((err / np.maximum(tol[i, g], 1e-300)).max()))
        # (c)
        f = score[i, :n] * np.float32(sign)
        assert (f[:-1] >= f[1:]).all(), (who, i, "order", f)
        eq = f[:-1] == f[1:]
        assert (g[:-1][eq] < g[1:][eq]).all(), (who, i, "ties not in ascending index", g)
        if n == 0:
            continue
        # (d)
        sigma_k = order[i, n - 1]
        assert (s[i, g] >= sigma_k - 2 * tol[i, g]).all(), (who, i, "wrong member")
        # (e)
        sigma_k1 = order[i, n] if n < V else -np.inf
        must = np.nonzero(cand[i] & (s[i] > sigma_k1 + 2 * tol[i]))[0]
        missing = np.setdiff1d(must, g)
        assert missing.size == 0, (who, i, "missing member", missing[:8])


# ---- cases on real-valued data ----------------------------------------------------------------
# (d, offset, Q, V, k, chunks, exclude); offset = 1 puts the base one float off 16-byte alignment
# (the VALU kernel at d = 64); chunks None = the plan's own; exclude: None, "self" (query i is base
# row i), "far" (a row in another chunk than the query's best match)
def real_cases():
    cases = []
    widths = ((64, 0), (128, 0), (100, 0), (64, 1))
    shapes = ((1, 1000, 10, 3, None), (33, 4099, 64, 7, "self"), (129, 1000, 1, 1, "far"),
              (300, 4099, 10, 3, "far"), (33, 5, 8, 1, None), (129, 4099, 10, 7, None),
              (1, 4099, 64, 1, "self"), (33, 1000, 64, 3, "far"))
    n = 0
    for mi, metric in enumerate(METRICS):
        for wi, (d, off) in enumerate(widths):
            for s in range(3):  # three of the eight shapes per (metric, width), rotating
                Q, V, k, chunks, ex = shapes[(n + s * 3 + mi) % len(shapes)]
                cases.append((metric, d, off, Q, V, k, chunks, ex))
            n += 1
    # V = 20,000: the plan's own chunks, and the shape with the most near-ties (l2, k = 64)
    cases += [("l2", 128, 0, 300, 20000, 64, None, None), ("cosine", 64, 0, 300, 20000, 10, None, "self"),
              ("dot", 100, 0, 33, 20000, 10, 7, "far"), ("dot", 128, 0, 129, 5, 8, 3, "self")]
    return cases


def case_id(c):
    metric, d, off, Q, V, k, chunks, ex = c
    return "%s-d%d%s-Q%d-V%d-k%d-c%s-%s" % (metric, d, "+1" if off else "", Q, V, k, chunks, ex)


_DATA = {}


def real_data(c):
    """(q, b, exclude or None) of a case: N(0, 1) rows scaled per row by 2^[-2, 2] (so norms vary);
    cached, read-only."""
    if c in _DATA:
        return _DATA[c]
    metric, d, off, Q, V, k, chunks, ex = c
    rng = np.random.RandomState(1000 + 7 * d + Q + V)
    b = (rng.randn(V, d) * 2.0 ** rng.uniform(-2, 2, (V, 1))).astype(np.float32)
    q = (rng.randn(Q, d) * 2.0 ** rng.uniform(-2, 2, (Q, 1))).astype(np.float32)
    exclude = None
    if ex == "self":
        rows = rng.permutation(V)[:Q] if Q <= V else rng.randint(0, V, Q)
        q = b[rows].copy()
        exclude = rows.astype(np.int32)
    elif ex == "far":
        s, _, _ = scores64(q, b, metric)
        exclude = ((s.argmax(1) + V // 2) % V).astype(np.int32)
        exclude[::5] = -1
    for a in (q, b) + ((exclude,) if exclude is not None else ()):
        a.setflags(write=False)
    _DATA[c] = (q, b, exclude)
    return _DATA[c]


# ---- exact data: integer-valued fp32, every score exact -----------------------------------------
def exact_data(metric, d, Q, V, seed=0):
    """(q, b): entries in {-2 .. 2} (dot, l2) or +-1 (cosine, d = 64: every norm is 8).  The base
    is V draws from a pool of 40 rows, so every row has about V / 40 duplicates spread over all
    chunks and tiles; rows 31 | 32 (a base-tile boundary), V // 3 - 1 | V // 3 + 40 and 0 | V - 1
    (other chunks at chunks = 3, 7) are made equal on purpose."""
    rng = np.random.RandomState(seed + d)
    if metric == "cosine":
        pool = rng.choice([-1.0, 1.0], (40, d))
        q = rng.choice([-1.0, 1.0], (Q, d))
    else:
        pool = rng.randint(-2, 3, (40, d)).astype(np.float64)
        q = rng.randint(-2, 3, (Q, d)).astype(np.float64)
    b = pool[rng.randint(0, 40, V)]
    if V > 40:
        b[32] = b[31]
        b[min(V - 1, V // 3 + 40)] = b[V // 3 - 1]
        b[V - 1] = b[0]
    return q.astype(np.float32), b.astype(np.float32)


def cosine_zero_data():
    """(q, b, zeros): d = 64, +-1 / 0 entries.  Query 0 is all ones, query 1 all zeros.  Base rows
    are all -1 (cosine -1 with query 0) except `zeros`, which score exactly 0 with query 0: three
    are zero rows, three have as many +1 as -1; 31 | 32 sit on a base-tile boundary."""
    b = -np.ones((100, 64), np.float32)
    zeros = [3, 31, 32, 40, 77, 99]
    for j in (3, 40, 99):
        b[j] = 0.0
    for j in (31, 32, 77):
        b[j, :32] = 1.0
    q = np.ones((2, 64), np.float32)
    q[1] = 0.0
    return q, b, zeros


def exact_reference(q, b, k, metric, exclude=None):
    """(idx int64 [Q, k], score fp32 [Q, k]) of exact data: a stable sort of the exact scores, the
    excluded row left out, the tail padded."""
    q64, b64 = q.astype(np.float64), b.astype(np.float64)
    dot = q64 @ b64.T
    if metric == "dot":
        s = dot
    elif metric == "cosine":
        qn, bn = np.sqrt((q64 * q64).sum(1)), np.sqrt((b64 * b64).sum(1))
        iq = np.where(qn > 0, 1.0 / np.where(qn > 0, qn, 1.0), 0.0)
        ib = np.where(bn > 0, 1.0 / np.where(bn > 0, bn, 1.0), 0.0)
        s = dot * ib[None, :] * iq[:, None]
    else:
        s = (q64 * q64).sum(1)[:, None] + (b64 * b64).sum(1)[None, :] - 2 * dot
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)  # exact in fp32
    Q, V = s.shape
    rank = -s if metric == "l2" else s.copy()
    if exclude is not None:
        rows = np.nonzero(np.asarray(exclude) >= 0)[0]
        rank[rows, np.asarray(exclude, np.int64)[rows]] = -np.inf
    order = np.argsort(-rank, axis=1, kind="stable")[:, :k]
    idx = np.full((Q, k), -1, np.int64)
    score = np.full((Q, k), np.inf if metric == "l2" else -np.inf, np.float32)
    for i in range(Q):
        o = order[i][np.isfinite(rank[i, order[i]])]
        idx[i, :len(o)] = o
        score[i, :len(o)] = s[i, o]
    return idx, score


def assert_same_bits(got, want, who):
    gi, gs = got
    wi, ws = want
    assert np.array_equal(np.asarray(gi, np.int64), wi), (who, "idx")
    assert np.array_equal(np.asarray(gs).view(np.int32), ws.view(np.int32)), (who, "score bits")
