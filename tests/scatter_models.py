"""Inputs, float64 references and fp32 summation models for the accuracy tests of the GMM M-step
sums (tests/test_gpu_scatter_accuracy.py; checked on the CPU by tests/test_scatter_models_host.py).

The scatter S_k = sum_i r_ik (x_i - m_k)(x_i - m_k)^T is the one sum here whose fp32 accumulation
length grows with the problem: a workgroup adds all the rows of its chunk into one set of fp32
accumulators, 614 rows in the suite's largest whole-matrix test, 6 135 at the benchmarked 1M rows
and 61 350 at 10M.  The yardstick is the plain fp32 running sum of the same operands in the same
chunks (`fp32_running_sum`: one rounding per row, what k_gmm_cov_valu and float32 numpy do); a
kernel's error against float64 is held to a small multiple of that sum's error on the same inputs
(`RMS_BAR`, `MAX_BAR`).  `blocked_sum` models the other orders the kernels use -- one rounding per
4 or 16 rows, six bf16 part products per 16 rows -- and a truncating adder, the defect the bar has
to catch.  No GPU import."""
import numpy as np

# A kernel passes when its RMS error is <= RMS_BAR x the running sum's and its largest error
# <= MAX_BAR x the running sum's largest.  Valid fp32 orders of the same sum measured 0.2-1.8x of
# the running sum's RMS (d = 32, 4 seeds, both input kinds, 614 to 61 350 rows per chunk), which
# 2x covers; the largest of ~1k entries of another noise realisation is looser, hence 3x.  A
# round-toward-zero accumulator lies at 2.5-4x (614 rows) to 5-10x (61 350).
RMS_BAR, MAX_BAR = 2.0, 3.0
HARD_ZERO_SHARE = 0.30  # of the 'hard' responsibilities, set to exactly 0


def rows_per_chunk(V, chunks):
    """come_gmm_scatter's chunk length for a request of `chunks`: ceil(V / chunks) rounded up to
    the 64-row block.  (used_chunks(V, chunks) of them hold rows.)"""
    per = -(-V // chunks)
    return max(64, -(-per // 64) * 64)


def used_chunks(V, chunks):
    return -(-V // rows_per_chunk(V, chunks))


def inputs(R, chunks, K, d, kind, seed):
    """fp32 X [V, d] ~ N(0, 1), resp [V, K], means [K, d] ~ 0.5 N(0, 1), V = R chunks - 5 (a ragged
    last chunk).  kind 'dirichlet': Dirichlet(1) rows.  kind 'hard', what late EM iterations
    produce: softmax of 8 N(0, 1) logits, exactly 30% of the entries set to 0, then eight of the
    others to exactly 1.0 and eight to the fp32 denormal 1e-40."""
    V = R * chunks - 5
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((V, d)).astype(np.float32)
    means = (0.5 * rng.standard_normal((K, d))).astype(np.float32)
    if kind == "dirichlet":
        resp = rng.dirichlet(np.ones(K), V).astype(np.float32)
    elif kind == "hard":
        z = 8.0 * rng.standard_normal((V, K))
        z = np.exp(z - z.max(1, keepdims=True))
        resp = (z / z.sum(1, keepdims=True)).astype(np.float32).ravel()
        order = rng.permutation(V * K)
        nz = int(round(HARD_ZERO_SHARE * V * K))
        resp[order[:nz]] = 0.0
        resp[order[nz:nz + 8]] = 1.0
        resp[order[nz + 8:nz + 16]] = np.float32(1e-40)
        resp = resp.reshape(V, K)
    else:
        raise ValueError(kind)
    return X, resp, means


def model_features(d):
    """The features the models are evaluated on: all at d <= 32, else two 16-blocks -- 0..15 and
    64..79 at d >= 80 (32..47 at d = 64), so that the subset holds entries of a diagonal 32 x 32
    (and 64 x 64) output tile and of an off-diagonal one, which k_gmm_cov_fb3 forms differently."""
    if d <= 32:
        return np.arange(d)
    hi = 64 if d >= 80 else 32 if d >= 48 else d - 16
    return np.concatenate([np.arange(16), np.arange(hi, hi + 16)])


def ref64(X, resp, means, feats=None):
    """[K, F, F] float64 scatter matrices of the fp32 operands (all features by default)."""
    X64 = X.astype(np.float64)
    out = []
    for k in range(resp.shape[1]):
        D = X64 - means[k].astype(np.float64)
        if feats is not None:
            D = D[:, feats]
        out.append((resp[:, k].astype(np.float64)[:, None] * D).T @ D)
    return np.stack(out)


def _round32(v, mode):
    """float64 -> fp32, to nearest even or toward zero."""
    r = v.astype(np.float32)
    if mode == "zero":
        over = np.abs(r.astype(np.float64)) > np.abs(v)
        r = np.where(over, np.nextafter(r, np.float32(0.0)), r)
    elif mode != "nearest":
        raise ValueError(mode)
    return r


def _bf16(v):
    """fp32 -> the nearest-even bf16 value, as fp32."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def _bf16_parts(v):
    """v = p1 + p2 + p3 + (below 2^-24 |v|): the kernels' bf16_split3, every difference exact."""
    p1 = _bf16(v)
    r1 = v - p1
    p2 = _bf16(r1)
    return p1, p2, _bf16(r1 - p2)


# the part products of one multiply-add in k_gmm_cov_bf3's order: (part of A, part of B)
_PART_PRODUCTS = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))


def blocked_sum(X, resp, means, chunks=1, feats=None, group=1, mode="nearest", parts=False):
    """[K, F, F] float64 holding the fp32 result of the scatter summed in this order: each chunk
    (come_gmm_scatter's chunking of a request for `chunks`) keeps one fp32 accumulator per entry
    and adds the exact (float64) sum of each `group` consecutive rows' terms fl32(r) d_i d_j,
    d = x - m in float64, with ONE rounding (`mode`: 'nearest' or 'zero', a truncating adder);
    the chunks are then added in chunk order in fp32.  parts=True, the bf16-part kernels' form:
    E = fl32(fl32(sqrt(r)) fl32(x - m)) split into three bf16 parts, and each of the six part
    products of order <= 2, summed exactly over the group's rows, added with one rounding."""
    V, d = X.shape
    K = resp.shape[1]
    feats = np.arange(d) if feats is None else np.asarray(feats)
    F = len(feats)
    per = rows_per_chunk(V, chunks)
    C = -(-V // per)
    assert per % group == 0
    # rows padded to C x per with zero weights: their terms are exact zeros
    Xp = np.zeros((C * per, F), np.float32)
    Wp = np.zeros((C * per, K), np.float32)
    Xp[:V], Wp[:V] = X[:, feats], resp
    Xp, Wp = Xp.reshape(C, per, F), Wp.reshape(C, per, K)
    M = means[:, feats]
    acc = np.zeros((C, K, F, F), np.float32)
    B = 64
    for b in range(0, per, B):
        x, w = Xp[:, b:b + B], Wp[:, b:b + B]
        G = x.shape[1] // group
        if parts:
            E = np.sqrt(w)[..., None] * (x[:, :, None, :] - M[None, None])  # fp32 [C, B, K, F]
            P = [p.astype(np.float64).reshape(C, G, group, K, F) for p in _bf16_parts(E)]
            T = [np.einsum("cgskf,cgske->cgkfe", P[a_], P[b_]) for a_, b_ in _PART_PRODUCTS]
        else:
            D = x.astype(np.float64)[:, :, None, :] - M.astype(np.float64)[None, None]
            wD = (w.astype(np.float64)[..., None] * D).reshape(C, G, group, K, F)
            T = [np.einsum("cgskf,cgske->cgkfe", wD, D.reshape(C, G, group, K, F))]
        for g in range(G):
            for t in T:
                acc = _round32(acc.astype(np.float64) + t[:, g], mode)
    out = acc[0]
    for c in range(1, C):
        out = _round32(out.astype(np.float64) + acc[c].astype(np.float64), mode)
    return out.astype(np.float64)


def fp32_running_sum(X, resp, means, chunks=1, feats=None):
    """The plain fp32 reference: acc = fl32(acc + fl32(r) d_i d_j) row by row within a chunk, the
    chunks added in order (blocked_sum with one rounding per row, to nearest)."""
    return blocked_sum(X, resp, means, chunks, feats, group=1, mode="nearest")


def stats(S, ref):
    """(RMS relative error sqrt(mean(e^2) / mean(ref^2)), max |e| / max |ref|, mean signed
    relative error of the diagonal) of [K, F, F] S against ref.  The third is for printing only: a
    truncating adder shows there as a negative bias that grows linearly with the length."""
    S, ref = np.asarray(S, np.float64), np.asarray(ref, np.float64)
    e = S - ref
    rms = float(np.sqrt((e ** 2).mean() / (ref ** 2).mean()))
    mx = float(np.abs(e).max() / np.abs(ref).max())
    de, dr = np.diagonal(e, axis1=-2, axis2=-1), np.diagonal(ref, axis1=-2, axis2=-1)
    return rms, mx, float((de / dr).mean())


def within_bar(st, model_st):
    """The error budget: st (a kernel's stats) against the running-sum model's on the same
    inputs."""
    return st[0] <= RMS_BAR * model_st[0] and st[1] <= MAX_BAR * model_st[1]


def row_sums_model(resp, X, blocks):
    """The M-step's other sums over rows, gmm.resp_sum and gmm.resp_t_x, as per-row fp32 running
    sums over `blocks` row blocks (fl32(acc + r) and fl32(acc + r x), the product in float64), the
    blocks and the rows past the last whole block added in float64 as those functions do.
    Returns (nk [K], sx [K, d]) float64."""
    V, K = resp.shape
    n = V // blocks * blocks
    r = resp[:n].reshape(blocks, n // blocks, K).astype(np.float64)
    x = X[:n].reshape(blocks, n // blocks, -1).astype(np.float64)
    nk = np.zeros((blocks, K), np.float32)
    sx = np.zeros((blocks, K, X.shape[1]), np.float32)
    for i in range(n // blocks):
        nk = (nk.astype(np.float64) + r[:, i]).astype(np.float32)
        sx = (sx.astype(np.float64) + r[:, i, :, None] * x[:, i, None, :]).astype(np.float32)
    tr, tx = resp[n:].astype(np.float64), X[n:].astype(np.float64)
    return nk.astype(np.float64).sum(0) + tr.sum(0), sx.astype(np.float64).sum(0) + tr.T @ tx


def row_sums_ref64(resp, X):
    r = resp.astype(np.float64)
    return r.sum(0), r.T @ X.astype(np.float64)


def flat_stats(S, ref):
    """stats' first two measures for a vector or matrix without a diagonal."""
    e = np.asarray(S, np.float64) - ref
    return (float(np.sqrt((e ** 2).mean() / (ref ** 2).mean())),
            float(np.abs(e).max() / np.abs(ref).max()))
