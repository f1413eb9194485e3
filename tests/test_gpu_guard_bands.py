"""Stray writes and read-only inputs: every output of the C-ABI's device entry points sits between
two pads of byte 0xA5, large enough to hold a whole-tile overrun (128 rows of the output for the
row-tiled kernels, at least 4 KiB), at ragged shapes; after the call the pads must still hold 0xA5
and every const input must be bit for bit what it was.  The values themselves are checked elsewhere
(the tests of each kernel); here only that the output was written at all.

The pads are multiples of 16 bytes, so the guarded views are 16-byte aligned and the MFMA paths run;
a second pass puts the views (and one operand) at +4 bytes for the entry points that then fall
back to their VALU kernels.  test_guard_checker_sees_a_byte_in_either_pad runs on CPU tensors
(it needs no GPU): that is how the checker itself is known to work.
"""
import numpy as np
import pytest

from come_amd import _lib
from come_amd._lib import options, ptr, stream_handle

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FILL = 0xA5
ROWS = [1, 15, 17, 127, 129]
COMPS = [1, 3, 5, 17]


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def guarded(shape, dtype, pad_bytes, device=None, offset=0):
    """(view, check): a contiguous `shape` / `dtype` view into one flat buffer filled with byte
    0xA5, with max(pad_bytes, 4 KiB) rounded up to 16 bytes in front of it (+ `offset` bytes) and
    behind it.  check() raises AssertionError if a byte of either pad is no longer 0xA5."""
    device = dev() if device is None else device
    shape = tuple(int(s) for s in np.atleast_1d(shape))
    item = torch.empty((), dtype=dtype).element_size()
    pad = -(-max(int(pad_bytes), 4096) // 16) * 16
    assert offset % item == 0
    n = int(np.prod(shape)) * item
    flat = torch.full((pad + offset + n + pad,), FILL, dtype=torch.uint8, device=device)
    assert flat.data_ptr() % 16 == 0
    view = flat[pad + offset:pad + offset + n].view(dtype).view(shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == offset % 16

    def check(what="buffer"):
        for name, part in (("front", flat[:pad + offset]), ("back", flat[pad + offset + n:])):
            bad = torch.nonzero(part != FILL)
            assert bad.numel() == 0, "%s: %d byte(s) of the %s pad overwritten, the first at pad " \
                "offset %d of %d" % (what, bad.numel(), name, int(bad[0]), part.numel())

    check.flat, check.pad = flat, pad + offset
    return view, check


def test_guard_checker_sees_a_byte_in_either_pad():
    cpu = torch.device("cpu")
    for dtype, offset in ((torch.float32, 0), (torch.float32, 4), (torch.float64, 0),
                          (torch.uint8, 0)):
        view, check = guarded((3, 5), dtype, 100, device=cpu, offset=offset)
        assert view.data_ptr() % 16 == offset and check.pad == 4096 + offset
        check()
        view.view(torch.uint8).fill_(0)  # the interior is the caller's
        check()
        for pos in (0, check.pad - 1, check.pad + view.numel() * view.element_size(),
                    check.flat.numel() - 1):
            check.flat[pos] = 0
            with pytest.raises(AssertionError, match="pad overwritten"):
                check()
            check.flat[pos] = FILL
            check()
    view, check = guarded((2, 8), torch.float32, 128 * 8 * 4 + 1, device=cpu)
    assert check.pad == 4112  # rounded up to 16 bytes


class Call(object):
    """One guarded call: out(...) makes guarded outputs, const(...) registers inputs that must come
    back unchanged, done() synchronises and checks pads, inputs and that outputs were written."""

    def __init__(self, what, offset=0):
        self.what, self.offset, self.outs, self.ins = what, offset, [], []

    def out(self, shape, dtype, pad_bytes, written=True, offset=None):
        off = self.offset if offset is None else offset
        if off % torch.empty((), dtype=dtype).element_size():
            off = 0
        view, check = guarded(shape, dtype, pad_bytes, offset=off)
        self.outs.append((view, check, written))
        return view

    def const(self, *tensors):
        for a in tensors:
            self.ins.append((a, a.clone()))
        return tensors if len(tensors) > 1 else tensors[0]

    def done(self):
        torch.cuda.synchronize()
        for i, (view, check, written) in enumerate(self.outs):
            check("%s, output %d" % (self.what, i))
            if written and view.numel():
                assert bool((view.reshape(-1).view(torch.uint8) != FILL).any()), \
                    "%s: output %d was not written" % (self.what, i)
        for i, (a, before) in enumerate(self.ins):
            same = torch.equal(a.reshape(-1).view(torch.uint8),
                               before.reshape(-1).view(torch.uint8))
            assert same, "%s: const input %d changed" % (self.what, i)


def ok(rc, what):
    _lib.check(rc, what)


def f32(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device=dev())


def at4(a):
    """A contiguous copy of `a` at +4 bytes from a 16-byte boundary (the VALU kernels' route)."""
    v = torch.empty(a.numel() + 1, dtype=a.dtype, device=a.device)[1:].view(a.shape)
    v.copy_(a)
    assert v.data_ptr() % 16 == 4
    return v


def mixture(V, K, d, seed, lower=False):
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((V, d))
    P = np.triu(rng.standard_normal((K, d, d)) / np.sqrt(d)) + 2 * np.eye(d)
    if lower:
        P[K // 2] = P[K // 2].T.copy()
    mp = np.matmul(rng.standard_normal((K, 1, d)) * 0.3, P)[:, 0]
    ln = np.log(rng.dirichlet(np.ones(K)))
    return f32(X), f32(P), f32(mp), f32(ln)


# form -> (d, gmm_resp16 / community_async, lower factor, views at +4)
MIX_FORMS = {"b16-64": (64, 3, False, 0), "b16-128": (128, 3, False, 0),
             "f32-64": (64, 2, False, 0), "f32-128": (128, 2, False, 0),
             "full-64": (64, 3, True, 0), "full-128": (128, 2, True, 0),
             "valu-100": (100, 3, False, 0), "wide-200": (200, 3, False, 0),
             "valu-64+4": (64, 3, False, 4), "valu-128+4": (128, 3, False, 4),
             "valu-100+4": (100, 3, False, 4), "wide-200+4": (200, 3, False, 4)}


@pytest.mark.parametrize("form", list(MIX_FORMS))
def test_gmm_estep_and_resp(form):
    d, r16, lower, off = MIX_FORMS[form]
    L = _lib.lib()
    for V in ROWS:
        for K in COMPS:
            X, P, mp, ln = mixture(V, K, d, V + K, lower and K > 1)
            if off:
                P = at4(P)
            c = Call("come_gmm_estep %s V=%d K=%d" % (form, V, K), off)
            c.const(X, P, mp, ln)
            resp = c.out((V, K), torch.float32, 128 * K * 4)
            lse = c.out((V,), torch.float32, 128 * 4)
            resp2 = c.out((V, K), torch.float32, 128 * K * 4)
            with options(gmm_resp16=r16):
                ok(L.come_gmm_estep(ptr(X), V, d, ptr(P), ptr(mp), ptr(ln), K, ptr(resp), ptr(lse),
                                    stream_handle(X.device)), c.what)
                ok(L.come_gmm_resp(ptr(X), V, d, ptr(P), ptr(mp), ptr(ln), K, ptr(resp2),
                                   stream_handle(X.device)), c.what)
            c.done()


SCATTER_FORMS = {"cov3-64": (64, 3, 0), "cov4-64": (64, 4, 0), "cov5-64": (64, 5, 0),
                 "cov3-128": (128, 3, 0), "cov4-128": (128, 4, 0), "cov5-128": (128, 5, 0),
                 "valu-100": (100, 4, 0), "wide-200": (200, 4, 0), "valu-64+4": (64, 4, 4),
                 "valu-128+4": (128, 4, 4), "valu-100+4": (100, 4, 4), "wide-200+4": (200, 4, 4)}


@pytest.mark.parametrize("form", list(SCATTER_FORMS))
def test_gmm_scatter(form):
    """chunks = 3: at V = 129 the rows split into three partial sums in `scratch` (64 rows per
    chunk at least), below that one chunk writes scatter_out directly and scratch is not used."""
    d, cov, off = SCATTER_FORMS[form]
    L = _lib.lib()
    chunks = 3
    for V in ROWS:
        for K in COMPS:
            rng = np.random.RandomState(V + K)
            X = f32(rng.standard_normal((V, d)))
            R = f32(rng.dirichlet(np.ones(K), V))
            M = f32(rng.standard_normal((K, d)))
            if off:
                X = at4(X)
            c = Call("come_gmm_scatter %s V=%d K=%d" % (form, V, K), off)
            c.const(X, R, M)
            out = c.out((K, d, d), torch.float32, d * d * 4)
            scratch = c.out((chunks, K, d, d), torch.float32, d * d * 4, written=V > 128)
            with options(gmm_cov_async=cov):
                ok(L.come_gmm_scatter(ptr(X), V, d, ptr(R), ptr(M), K, chunks, ptr(scratch),
                                      ptr(out), stream_handle(X.device)), c.what)
            c.done()


@pytest.mark.parametrize("d", [17, 100, 128])
def test_gmm_params(d):
    K = 3
    rng = np.random.RandomState(d)
    n = 3 * d + 20
    Y = rng.standard_normal((K, n, d))
    nk = rng.uniform(50.0, 500.0, K)
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float64), device=dev())  # noqa: E731
    S = t64(np.einsum("kni,knj->kij", Y, Y) * (nk[:, None, None] / n))
    nk_, mu, w = t64(nk), t64(rng.standard_normal((K, d))), t64(rng.dirichlet(np.ones(K)))
    c = Call("come_gmm_params d=%d" % d)
    c.const(S, nk_, mu, w)
    cov = c.out((K, d, d), torch.float64, d * d * 8)
    pc = c.out((K, d, d), torch.float64, d * d * 8)
    e_pc = c.out((K, d, d), torch.float32, d * d * 4)
    e_mp = c.out((K, d), torch.float32, d * 4)
    e_ln = c.out((K,), torch.float32, 4)
    info = c.out((K,), torch.int32, 4)
    ok(_lib.lib().come_gmm_params(ptr(S), ptr(nk_), ptr(mu), ptr(w), K, d, 1e-5, ptr(cov), ptr(pc),
                                  ptr(e_pc), ptr(e_mp), ptr(e_ln), ptr(info),
                                  stream_handle(S.device)), c.what)
    c.done()
    assert info.cpu().numpy().tolist() == [0] * K


@pytest.mark.parametrize("form", [f for f in MIX_FORMS if not MIX_FORMS[f][2]])
def test_community_grad_leaves_the_rows_past_v(form):
    """x holds V + 128 rows and the call is given V: rows >= V and both pads stay as they were."""
    d, kern, _, off = MIX_FORMS[form]
    L = _lib.lib()
    for V in ROWS:
        for K in COMPS:
            rng = np.random.RandomState(V + K + d)
            A = rng.standard_normal((K, d, d)) / np.sqrt(d)
            inv = f32(np.linalg.inv(A @ A.transpose(0, 2, 1) + 0.5 * np.eye(d)))
            mu = f32(rng.standard_normal((K, d)))
            pi = f32(rng.dirichlet(np.ones(K), V))
            if off:
                inv = at4(inv)
            c = Call("come_community_grad %s V=%d K=%d" % (form, V, K), off)
            c.const(pi, mu, inv)
            x = c.out((V + 128, d), torch.float32, 128 * d * 4)
            x.copy_(f32(rng.standard_normal((V + 128, d))))
            before = x.clone()
            with options(community_async=kern):
                ok(L.come_community_grad(ptr(x), V, d, ptr(pi), ptr(mu), ptr(inv), K, 0.5, 0.1, 2,
                                         stream_handle(x.device)), c.what)
            c.done()
            assert torch.equal(x[V:].view(torch.int32), before[V:].view(torch.int32)), c.what
            assert not torch.equal(x[:V], before[:V]), c.what


@pytest.mark.parametrize("form", ["b16-64", "b16-128", "valu-100", "wide-200", "valu-64+4",
                                  "valu-128+4", "valu-100+4", "wide-200+4"])
def test_community_loss(form):
    d, _, _, off = MIX_FORMS[form]
    L = _lib.lib()
    for V in ROWS:
        for K in COMPS:
            X, P, mp, ln = mixture(V, K, d, V + K)
            pi = f32(np.random.RandomState(V).dirichlet(np.ones(K), V))
            if off:
                P = at4(P)
            c = Call("come_community_loss %s V=%d K=%d" % (form, V, K), off)
            c.const(X, pi, P, mp, ln)
            rows = c.out((V,), torch.float32, 128 * 4)
            total = c.out((1,), torch.float64, 8)
            ok(L.come_community_loss(ptr(X), V, d, ptr(pi), ptr(P), ptr(mp), ptr(ln), K, ptr(rows),
                                     ptr(total), stream_handle(X.device)), c.what)
            c.done()


KMEANS_FORMS = {"mfma-64": (64, 0), "mfma-128": (128, 0), "valu-100": (100, 0),
                "wide-200": (200, 0), "valu-64+4": (64, 4), "valu-128+4": (128, 4)}


@pytest.mark.parametrize("form", list(KMEANS_FORMS))
def test_kmeans_lloyd_assign_update(form):
    """chunks = 3 (more chunks than 16-row blocks at small V: the unused ones must stay untouched
    too); the scratch at its documented chunks * (8 + 4 K d + 4 K) bytes."""
    d, off = KMEANS_FORMS[form]
    L = _lib.lib()
    chunks = 3
    for V in ROWS:
        for K in COMPS:
            rng = np.random.RandomState(V + K)
            X = f32(rng.standard_normal((V, d)))
            C = f32(rng.standard_normal((K, d)))
            if off:
                X = at4(X)
            c = Call("come_kmeans_lloyd %s V=%d K=%d" % (form, V, K), off)
            c.const(X, C)
            scratch = c.out((chunks * (8 + 4 * K * d + 4 * K),), torch.uint8, 128 * d * 4, offset=0)
            labels = c.out((V,), torch.int32, 128 * 4)
            mind = c.out((V,), torch.float32, 128 * 4)
            sums = c.out((K, d), torch.float64, K * d * 8)
            counts = c.out((K,), torch.int64, 8)
            inertia = c.out((1,), torch.float64, 8)
            ok(L.come_kmeans_lloyd(ptr(X), V, d, ptr(C), K, chunks, ptr(scratch), ptr(labels),
                                   ptr(mind), ptr(sums), ptr(counts), ptr(inertia),
                                   stream_handle(X.device)), c.what)
            c.done()
            assert int(counts.sum()) == V

            c = Call("come_kmeans_assign %s V=%d K=%d" % (form, V, K), off)
            c.const(X, C)
            labels2 = c.out((V,), torch.int32, 128 * 4)
            mind2 = c.out((V,), torch.float32, 128 * 4)
            ok(L.come_kmeans_assign(ptr(X), V, d, ptr(C), K, ptr(labels2), ptr(mind2),
                                    stream_handle(X.device)), c.what)
            c.done()
            assert torch.equal(labels, labels2)

            c = Call("come_kmeans_update %s V=%d K=%d" % (form, V, K), off)
            c.const(sums, counts)
            centers = c.out((K, d), torch.float32, K * d * 4)
            centers.copy_(C)
            stats = c.out((1,), torch.float64, 8)  # stats2[1] is documented as not written
            ok(L.come_kmeans_update(ptr(centers), ptr(sums), ptr(counts), K, d, ptr(stats),
                                    stream_handle(X.device)), c.what)
            c.done()


@pytest.mark.parametrize("d,off", [(64, 0), (100, 0), (200, 0), (3, 0), (64, 4)])
def test_kmeans_pp_step_pick_sample(d, off):
    from come_amd import kmeans
    L = _lib.lib()
    for V in ROWS:
        for T in (1, 3, 16):
            rng = np.random.RandomState(V + T)
            X = f32(rng.standard_normal((V, d)))
            if off:
                X = at4(X)
            closest = f32(rng.uniform(0.5, 4.0 * d, V))
            cand = torch.as_tensor(rng.randint(0, V, T).astype(np.int32), device=dev())
            u = torch.as_tensor(rng.uniform(0, 1, T), device=dev())
            cus = torch.cuda.get_device_properties(X.device).multi_processor_count
            chunks, per = kmeans.pp_plan(V, d, T, cus)
            s = stream_handle(X.device)
            c = Call("come_kmeans_pp_step d=%d V=%d T=%d" % (d, V, T), off)
            c.const(X, closest, cand)
            dist = c.out((V, T), torch.float32, 128 * T * 4)
            ppot = c.out((chunks, T), torch.float64, T * 8)
            pots = c.out((T,), torch.float64, T * 8)
            ok(L.come_kmeans_pp_step(ptr(X), V, d, ptr(closest), ptr(cand), T, chunks, ptr(dist),
                                     ptr(ppot), ptr(pots), s), c.what)
            c.done()
            c = Call("come_kmeans_pp_pick d=%d V=%d T=%d" % (d, V, T), off)
            c.const(dist, ppot, pots)
            closest2 = c.out((V,), torch.float32, 128 * 4)
            cpot = c.out((chunks,), torch.float64, 8)
            best = c.out((1,), torch.int32, 4)
            pot = c.out((1,), torch.float64, 8)
            ok(L.come_kmeans_pp_pick(ptr(dist), V, T, ptr(ppot), ptr(pots), chunks, ptr(closest2),
                                     ptr(cpot), ptr(best), ptr(pot), s), c.what)
            c.done()
            c = Call("come_kmeans_pp_sample d=%d V=%d T=%d" % (d, V, T), off)
            c.const(closest2, cpot, u)
            cand2 = c.out((T,), torch.int32, T * 4)
            ok(L.come_kmeans_pp_sample(ptr(closest2), V, ptr(cpot), chunks, per, ptr(u), T,
                                       ptr(cand2), s), c.what)
            c.done()
            assert 0 <= int(cand2.min()) and int(cand2.max()) < V


@pytest.mark.parametrize("n", [4, 260])
def test_delta_begin_end(n):
    L = _lib.lib()
    rng = np.random.RandomState(n)
    W, S = f32(rng.standard_normal(n)), f32(rng.standard_normal(n))
    c = Call("come_delta_begin n=%d" % n)
    c.const(W, S)
    D = c.out((n,), torch.float32, 4096)
    Down = c.out((n,), torch.float32, 4096)
    ok(L.come_delta_begin(ptr(W), ptr(S), ptr(D), ptr(Down), n, stream_handle(W.device)), c.what)
    c.done()
    assert torch.equal(D, W - S) and torch.equal(Down, D)
    c = Call("come_delta_end n=%d" % n)
    Dsum = c.const(D * 2)
    c.const(Down)
    W2 = c.out((n,), torch.float32, 4096)
    S2 = c.out((n,), torch.float32, 4096)
    W2.copy_(W)
    S2.copy_(S)
    ok(L.come_delta_end(ptr(W2), ptr(S2), ptr(Dsum), ptr(Down), n, stream_handle(W.device)), c.what)
    c.done()
    assert torch.equal(S2, S + Dsum)


@pytest.mark.parametrize("d", [4, 100])
@pytest.mark.parametrize("rows", [1, 33])
def test_delta_flags_gather_scatter(rows, d):
    L = _lib.lib()
    rng = np.random.RandomState(rows + d)
    S = f32(rng.standard_normal((rows, d)))
    W = S.clone()
    changed = sorted(set(rng.randint(0, rows, max(1, rows // 3)).tolist()))
    W[changed, d - 1] += 1.0
    s = stream_handle(W.device)
    c = Call("come_delta_flags rows=%d d=%d" % (rows, d))
    c.const(W, S)
    flags = c.out((rows,), torch.uint8, 4096)
    ok(L.come_delta_flags(ptr(W), ptr(S), rows, d, ptr(flags), s), c.what)
    c.done()
    idx = torch.nonzero(flags)[:, 0].contiguous()
    assert idx.cpu().numpy().tolist() == changed
    n = idx.numel()
    c = Call("come_delta_gather rows=%d d=%d" % (rows, d))
    c.const(W, S, idx)
    D = c.out((n, d), torch.float32, 128 * d * 4)
    Down = c.out((n, d), torch.float32, 128 * d * 4)
    ok(L.come_delta_gather(ptr(W), ptr(S), ptr(idx), n, d, ptr(D), ptr(Down), s), c.what)
    c.done()
    assert torch.equal(D, W[idx] - S[idx]) and torch.equal(Down, D)
    c = Call("come_delta_scatter rows=%d d=%d" % (rows, d))
    Dsum = c.const(D * 2)
    c.const(Down, idx)
    W2 = c.out((rows, d), torch.float32, 128 * d * 4)
    S2 = c.out((rows, d), torch.float32, 128 * d * 4)
    W2.copy_(W)
    S2.copy_(S)
    ok(L.come_delta_scatter(ptr(W2), ptr(S2), ptr(idx), n, d, ptr(Dsum), ptr(Down), s), c.what)
    c.done()
    keep = torch.ones(rows, dtype=torch.bool, device=W.device)
    keep[idx] = False
    assert torch.equal(W2[keep], W[keep]) and torch.equal(S2[keep], S[keep])
    assert torch.equal(S2[idx], S[idx] + Dsum)


@pytest.mark.parametrize("T", [63, 64, 65])
def test_pack_table(T):
    table = torch.as_tensor((np.arange(T) // 7).astype(np.int32), device=dev())  # steps of 0 / 1
    c = Call("come_pack_table T=%d" % T)
    c.const(table)
    packed = c.out((16 * ((T + 63) // 64),), torch.uint8, 4096)
    status = c.out((1,), torch.int32, 4)
    ok(_lib.lib().come_pack_table(ptr(table), T, ptr(packed), ptr(status),
                                  stream_handle(table.device)), c.what)
    c.done()
    assert int(status[0]) == 0


@pytest.mark.parametrize("V", [31, 32, 33])
def test_hot_rows(V):
    table = torch.as_tensor(np.random.RandomState(V).randint(0, V, 5000).astype(np.int32),
                            device=dev())
    c = Call("come_hot_rows V=%d" % V)
    c.const(table)
    counts = c.out((V,), torch.int32, 4096)
    bits = c.out(((V + 31) // 32,), torch.int32, 4096)
    ok(_lib.lib().come_hot_rows(ptr(table), table.numel(), V, 150, ptr(counts), ptr(bits),
                                stream_handle(table.device)), c.what)
    c.done()
    assert torch.equal(counts.long(), torch.bincount(table.long(), minlength=V))


@pytest.mark.parametrize("V", [31, 32, 33])
def test_quiet_rows(V):
    table = torch.as_tensor(np.random.RandomState(V).randint(0, V, 5000).astype(np.int32),
                            device=dev())
    c = Call("come_quiet_rows V=%d" % V)
    c.const(table)
    counts = c.out((V,), torch.int32, 4096)
    total = c.out((1,), torch.float64, 4096)
    bits = c.out(((V + 31) // 32,), torch.int32, 4096)
    # ~161 slots a row: about half the rows' successors are at or below the bound of 160
    ok(_lib.lib().come_quiet_rows(ptr(table), table.numel(), V, 1.0, 1, 5000.0 / 160.0, 1.0, 175,
                                  ptr(counts), ptr(total), ptr(bits), stream_handle(table.device)),
       c.what)
    c.done()
    assert torch.equal(counts.long(), torch.bincount(table.long(), minlength=V))
    assert float(total[0]) == 5000.0


@pytest.mark.parametrize("P,Lw,staged", [(1, 1, 0), (257, 17, 0), (1, 1, 1), (257, 17, 1),
                                         (257, 17, "pq"), (257, 17, "w")])
def test_random_walks(P, Lw, staged):
    """come_random_walks with direct (0) and LDS-staged (1) stores, and the two other entry points
    of the staged launch body, come_random_walks_pq and come_random_walks_w, at (p, q) = (0.25, 4)."""
    Vg = 50
    rng = np.random.RandomState(P)
    deg = rng.randint(0, 5, Vg)  # some nodes without neighbours: their walks end early
    rowptr_h = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col_h = rng.randint(0, Vg, max(1, int(deg.sum()))).astype(np.int32)
    rowptr = torch.as_tensor(rowptr_h, device=dev())
    col = torch.as_tensor(col_h, device=dev())
    starts = torch.as_tensor(rng.randint(0, Vg, P).astype(np.int32), device=dev())
    c = Call("come_random_walks P=%d L=%d staged=%s" % (P, Lw, staged))
    c.const(rowptr, col, starts)
    if staged in (0, 1):
        out = c.out((P, Lw), torch.int32, 128 * Lw * 4)
        with options(walk_staged=staged):
            ok(_lib.lib().come_random_walks(ptr(rowptr), ptr(col), Vg, ptr(starts), P, Lw, 0.1,
                                            12345, 0, None, ptr(out), stream_handle(out.device)),
               c.what)
    else:
        from come_amd import cpu
        ascending = cpu.sorted_adjacency(rowptr_h, col_h)
        if staged == "pq":
            third = torch.as_tensor(ascending, device=dev())
            entry, adj = _lib.lib().come_random_walks_pq, col
        else:
            w = rng.lognormal(0.0, 1.0, len(col_h)).astype(np.float32)
            third = torch.as_tensor(cpu.walk_cdf(rowptr_h, w).view(np.int32), device=dev())
            entry, adj = _lib.lib().come_random_walks_w, torch.as_tensor(ascending, device=dev())
        c.const(third, adj)
        out = c.out((P, Lw), torch.int32, 128 * Lw * 4)
        trials = c.out((1,), torch.int64, 4096)
        trials.zero_()
        ok(entry(ptr(rowptr), ptr(adj), ptr(third), Vg, ptr(starts), P, Lw, 0.1, 0.25, 4.0, 12345,
                 0, None, ptr(out), ptr(trials), stream_handle(out.device)), c.what)
    c.done()
    assert int(out.min()) >= -1 and int(out.max()) < Vg


@pytest.mark.parametrize("d", [128, 100])
def test_sgns_sequential_leaves_the_rows_past_v(d):
    """come_sgns_o2 and come_sgns_o1 in sequential mode on a tiny batch: the tables hold V + 64
    rows, the calls are given V -- rows >= V and the pads stay as they were."""
    from oracle import oracle as orc
    L = _lib.lib()
    V, extra, P, Lw, neg, w = 40, 64, 3, 12, 5, 3
    rng = np.random.RandomState(d)
    table = torch.as_tensor(orc.make_table(rng.randint(1, 50, V), 2000).view(np.int32),
                            device=dev())
    walks = torch.as_tensor(rng.randint(0, V, (P, Lw)).astype(np.int32), device=dev())
    seeds = torch.as_tensor(rng.randint(0, 2 ** 48, P).astype(np.int64), device=dev())
    edges = torch.as_tensor(rng.randint(0, V, (7, 2)).astype(np.int32), device=dev())
    eseeds = torch.as_tensor(rng.randint(0, 2 ** 48, 7).astype(np.int64), device=dev())
    c = Call("come_sgns_o2 / come_sgns_o1 d=%d" % d)
    c.const(table, walks, seeds, edges, eseeds)
    node = c.out((V + extra, d), torch.float32, 128 * d * 4)
    ctx = c.out((V + extra, d), torch.float32, 128 * d * 4)
    node.copy_(f32(rng.uniform(-1, 1, (V + extra, d))))
    ctx.copy_(f32(rng.uniform(-0.1, 0.1, (V + extra, d))))
    node0, ctx0 = node.clone(), ctx.clone()
    s = stream_handle(node.device)
    ok(L.come_sgns_o2(ptr(node), ptr(ctx), V, d, ptr(walks), P, Lw, ptr(seeds), w, neg, ptr(table),
                      table.numel(), 0.1, 1.0, _lib.MODE_SEQUENTIAL, s), c.what)
    ok(L.come_sgns_o1(ptr(node), V, d, ptr(edges), 7, ptr(eseeds), neg, ptr(table), table.numel(),
                      0.2, _lib.MODE_SEQUENTIAL, s), c.what)
    c.done()
    assert torch.equal(node[V:], node0[V:]) and torch.equal(ctx[V:], ctx0[V:])
    assert not torch.equal(node[:V], node0[:V]) and not torch.equal(ctx[:V], ctx0[:V])
