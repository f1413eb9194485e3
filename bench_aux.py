"""Secondary benchmarks for the other hot-path rows (bench.py is the contract line for C3/O2).

  --workload c2   BASELINE configs[1]: O1 (node_embeddings) on a synthetic SBM, 100 blocks x 1000
                  nodes, ~1M edges, d=128, negative=5; a step = one Hogwild pass over all edges
                  (come_sgns_o1); metric pair-updates/s; roofline HBM, (3+n)*d*4 B per pair.
  --workload c4   BASELINE configs[3]: 1M nodes, K=50, d=128: the community-gradient pass
                  (come_community_grad, iters=1) and the GMM responsibility pass
                  (come_gmm_resp); each 2*V*K*d^2 flops; roofline = fp32 MFMA peak 157.3 TFLOP/s
                  (k_community_b16: the bf16 MFMA peak / 6, its six bf16 part products per MAC).
  --workload walks  SURVEY.md §8f row 1, the producer of C3's input: one corpus pass over the C3
                  graph (1M-node power law, every node starts one walk, length 80) on the HIP
                  walker (come_random_walks); metric walk-steps/s; roofline: the measured 1.70
                  random 128-B line reads per step against the Infinity-Cache random-gather rate
                  (8.6 TB/s; 24 algorithmic B per step reported beside it).  CPU baseline: the exact
                  CPython-stream walker (come_walks_reference, native restatement of
                  graph_utils.build_deepwalk_corpus) on host threads.
  --workload kmeans  the k-means initialisation of the C4 GMM fit (1M rows, K=50, d=128): ms per
                  Lloyd iteration of the torch path and of the native kernels (come_amd.kmeans) from
                  the same centres, the torch seedings and the native one (kmeans_plusplus_native,
                  and its pass over X alone against HBM), a full KMeans.fit with each seeding, and
                  the k-means share of a GaussianMixture fit with each kmeans_backend /
                  kmeans_seeding; roofline: X read once against HBM.
  --workload community_loss  the community objective at C4's shape (1M rows, K=50, d=128): ms per
                  pass of come_community_loss (pack + kernel + reduction) and of come_gmm_estep on
                  the same operands in the same run (the loss runs the E-step's MFMA stream and
                  reads V x K x 4 B of pi where the E-step writes and re-reads as much resp), and of
                  community_embeddings.community_loss end to end (factors derived, total read back).
                  Reference: the numpy / scipy formula (multivariate_normal.logpdf weighted by pi)
                  on a row subset, scaled to V.
  --workload sgns_loss  the SGNS losses: on the C3 shape (1M nodes, d=128, negative=5, window=5,
                  131,072 walks x 80, packed table) ms per come_sgns_o2_loss pass and per Hogwild
                  come_sgns_o2 launch on the same walks in the same run, the loss timed again
                  afterwards (same-run spread); then Node2Vec.loss native against torch on 1M
                  edges of the graph taken in random order.  Roofline: (1 + n) rows per pair plus one centre row per centre against
                  HBM (the naive (2 + n) rows per pair beside it).
  --workload c4_diag  diagonal covariances at C4's shape (1M rows, K=50, d=128) and at d=256: ms per
                  come_gmm_estep_diag, come_gmm_diag_moments, come_gmm_diag_scatter, whole EM
                  iteration (its host read included), come_community_grad_diag step and
                  come_community_loss_diag pass, each beside its full-covariance counterpart timed
                  in the same run, bit-identity of every diagonal entry across two passes, and each
                  kernel's roofline: the larger of its compulsory bytes over HBM and its fused
                  multiply-adds over the fp32 vector peak.
  --workload topk  exact top-10 cosine neighbour search over a 1M x 128 table (come_topk through
                  neighbors.Index.search) at Q = 16,384 and Q = 1, beside the torch chain it
                  replaces (normalised matmul + torch.topk over query batches of 2,048) timed in the
                  same run: ms, queries/s, executed flops over the fp32 MFMA peak, and each path's
                  peak device memory over the tables.
Each prints one JSON line.  CPU baselines on a bounded sample: O1 the builder's Hogwild C
restatement of train_o1 (oracle/come_oracle_mt.c; reported beside it as the reference-equivalent
rate, restatement / its calibrated speed-up over the reference's GIL-bound Node2Vec.train,
profiles/r02_cpu_calibration.json); C4 the reference's numpy Community2Vec.train loop restated in
oracle/oracle.py and sklearn predict_proba.  The reference itself never reaches the GPU box.
"""
import argparse
import json
import math
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
F32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: f32-input MFMA = f32 vector peak
BF16_MFMA_PEAK_TFLOPS = 16 * F32_MFMA_PEAK_TFLOPS  # dense bf16 MFMA (~2.5 PF), 16x the f32 rate


def log(*a):
    print("[bench_aux]", *a, file=sys.stderr, flush=True)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0), [a.elapsed_time(b) for a, b in ev]


def c2(args):
    import torch
    import come_amd.training_sdg_inner as tsi
    from come_amd.graph import sbm
    from come_amd.model import Model
    dev = torch.device("cuda", 0)
    g = sbm(100, 1000, 0.016, 4.04e-5, seed=0)
    np.random.seed(1234)
    m = Model(g.degree_by_id(), size=args.dim, table_size=args.table_size, k=100, device=dev)
    edges = torch.from_numpy(g.edges.astype(np.int32)).to(dev)
    E = edges.shape[0]
    np.random.seed(99)
    seeds = [torch.from_numpy(tsi.draw_seeds(E).view(np.int64)).to(dev)
             for _ in range(args.steps + args.warmup)]
    it = iter(range(10 ** 9))

    hot = m.hot_rows(args.hot_p)  # the product's Hogwild launch (Node2Vec.train)
    n_hot = 0 if hot is None else int(np.unpackbits(hot.cpu().numpy().view(np.uint8)).sum())

    table = m.table if args.plain_table else m.negative_table()  # the product's (packed) table

    def step():
        tsi.sgns_o1(m.node_embedding, edges, seeds[next(it) % len(seeds)], args.negative, table,
                    args.lr, tsi.MODE_HOGWILD, hot=hot)
    el, ks = timed(step, args.steps, args.warmup)
    pairs = 2 * E
    n, d = args.negative, args.dim
    bpp = (3 + n) * d * 4
    avg = float(np.mean(ks)) / 1e3
    cpu = None
    if not args.no_cpu_baseline:
        from oracle import oracle as orc
        node = m.node_embedding.cpu().numpy().copy()
        threads = orc.usable_cpus()
        try:
            o1_ratio = float(json.load(open(os.path.join(
                ROOT, "profiles", "r02_cpu_calibration.json")))["o1_ratio_restatement_over_cython"])
        except (OSError, ValueError, KeyError):
            o1_ratio = None
        np.random.seed(98)
        cs = tsi.draw_seeds(E)
        t0 = time.time()
        done = pairs_done = 0
        while time.time() - t0 < args.cpu_seconds:
            p, e = orc.sgns_o1_hogwild(node, g.edges.astype(np.int32), cs, n, m.table_host, args.lr,
                                       threads, max(0.1, args.cpu_seconds - (time.time() - t0)))
            pairs_done += p
            done += e
        cel = time.time() - t0
        cpu = {"value": pairs_done / cel, "unit": "pair-updates/s", "cores": threads,
               "kind": "port",
               "reference_equivalent_value": (pairs_done / cel / o1_ratio) if o1_ratio else None,
               "reference_equivalent_note": "value / %s = the reference's GIL-bound Node2Vec."
                                            "train rate on the same cores (calibrated ratio, "
                                            "profiles/r02_cpu_calibration.json)" % (
                                                "%.1f" % o1_ratio if o1_ratio else "n/a"),
               "sample": "builder's Hogwild C restatement of train_o1 (oracle/come_oracle_mt.c), "
                         "%d threads taking jobs of 150 edges; %d edges in %.1fs.  The "
                         "reference's Node2Vec.train is GIL-bound (one Python call per edge): "
                         "calibrated in the container, this restatement runs %s x the "
                         "reference's Cython train_o1 at 8 threads "
                         "(profiles/r02_cpu_calibration.json)" % (
                             threads, done, cel, "%.1f" % o1_ratio if o1_ratio else "n/a")}
    print(json.dumps({
        "metric": "O1 SGNS pair-updates/sec, SBM 100k nodes / 1M edges, d=128",
        "value": pairs * args.steps / el, "unit": "pair-updates/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
        "higher_is_better": True, "dtype": "f32", "data": "synthetic SBM (seed 0)",
        "config": {"workload": "configs[1]/C2: O1 over %d edges of a 100x1000 SBM, d=%d, "
                               "negative=%d, lr=%g" % (E, d, n, args.lr), "hot_rows": n_hot,
                   "negative_table": "uint32" if args.plain_table else "packed"},
        "roofline": {"bound": "hbm", "achieved": bpp * pairs / avg / 1e9, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": bpp * pairs / avg / 1e9 / HBM_PEAK_GBS,
                     "bytes_per_pair": bpp, "avg_kernel_ms": avg * 1e3},
        "cpu_baseline": cpu}))


def c4(args):
    """N = 1: the three kernels on all V rows.  N > 1 (torchrun, one rank per GPU):
    every rank owns V/N rows of the replicated tables; a community pass = the kernel on the rank's
    rows + one all-gather of the updated rows (RCCL), an EM iteration = local E-step + M-step with
    the sufficient statistics all-reduced (come_amd.gmm distributed=True).  value = all ranks'
    flops / max-over-ranks time (strong scaling: V is fixed)."""
    import torch
    import torch.distributed as dist
    from come_amd import community_embeddings as ce
    from come_amd.distributed import all_gather_rows, shard_range
    from oracle import oracle as orc
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = 0 if args.all_ranks_device0 else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(args.dist_backend)
    V, K, d = args.nodes, args.k, args.dim
    lo, hi = shard_range(V, rank, world)
    rng = np.random.RandomState(2)
    x = torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32)).to(dev)
    A = rng.standard_normal((K, d, d)) / np.sqrt(d)
    cov = np.einsum("kij,klj->kil", A, A) + np.eye(d)[None] * 0.5
    inv = torch.from_numpy(np.linalg.inv(cov.astype(np.float32)).astype(np.float32)).to(dev)
    mu = torch.from_numpy((rng.standard_normal((K, d)) * 0.5).astype(np.float32)).to(dev)
    pi = torch.from_numpy(np.random.RandomState(3).dirichlet(np.ones(K), V).astype(np.float32)
                          ).to(dev)
    w = np.random.RandomState(4).dirichlet(np.ones(K))
    pc, mp, ln = ce.gmm_resp_params(w, mu.cpu().numpy().astype(np.float64),
                                    orc.precision_cholesky(cov), dev)
    flops = 2.0 * V * K * d * d
    # fraction of the MFMA blocks executed on sklearn's upper-triangular precision factors: the
    # bf16-part E-step's 16-wide column tiles x 32-feature steps (k_gmm_resp_b16, 20 of 32 at
    # d = 128) or the fp32 form's 16-wide blocks (k_gmm_resp16t, 36 of 64); the scatter's
    # symmetric 32-wide (10 of 16, k_gmm_cov_bf3) / 16-wide (36 of 64, k_gmm_cov16) tiles
    from come_amd import _lib
    opts = _lib.launch_opts()
    ct = d // 32 if d in (64, 128) else 0
    tri = (ct * (ct + 1) / 2) / (ct * ct) if ct else 1.0
    ct16 = d // 16 if d in (64, 128) else 0
    tri16 = (ct16 * (ct16 + 1) / 2) / (ct16 * ct16) if ct16 else 1.0
    tri_resp = (tri16 if opts.gmm_resp16 == 2 else (ct * (ct + 1)) / (2 * ct * ct)) if ct16 \
        else 1.0
    tri_cov = (tri16 if opts.gmm_cov_async == 3 else tri) if ct16 else 1.0
    cov_kernel = {3: "k_gmm_cov16", 4: "k_gmm_cov_fb3" if d == 128 else "k_gmm_cov_bf3",
                  5: "k_gmm_cov_bf3"}[
        opts.gmm_cov_async] if ct16 else "VALU"
    comm_kernel = {2: "k_community16", 3: "k_community_b16"}[
        opts.community_async] if ct16 else "VALU"
    # k_community_b16 carries each fp32 operand as three bf16 parts and takes six part products
    # per multiply-add: its ceiling is the bf16 MFMA peak / 6, not the fp32 MFMA peak
    comm_bf3 = comm_kernel == "k_community_b16"
    comm_peak = BF16_MFMA_PEAK_TFLOPS / 6 if comm_bf3 else F32_MFMA_PEAK_TFLOPS
    resp_kernel = {2: "k_gmm_resp16t", 3: "k_gmm_resp_b16"}[
        opts.gmm_resp16] if ct16 else "VALU"
    x0 = x.clone()
    xs, pis, x0s = x[lo:hi], pi[lo:hi], x0[lo:hi]

    def community_pass():
        ce.community_grad(xs, pis, mu, inv, 0.01, 0.1, 1)
        if world > 1:
            all_gather_rows(x)
    if world > 1:  # kernel alone on the rank's rows (the exchange excluded)
        _, ks_k = timed(lambda: ce.community_grad(xs, pis, mu, inv, 0.01, 0.1, 1), args.steps,
                        args.warmup)
    el_g, ks_g = timed(community_pass, args.steps, args.warmup)
    el_r, ks_r = timed(lambda: ce.gmm_resp(x0s, pc, mp, ln), args.steps, args.warmup)
    tg, tr = float(np.mean(ks_g)) / 1e3, float(np.mean(ks_r)) / 1e3
    # one GMM EM iteration (come_amd.gmm: E-step kernel + means GEMM + scatter kernel + K
    # Cholesky factorisations), and the M-step scatter kernel alone
    from come_amd import gmm
    gm = gmm.GaussianMixture(K, reg_covar=1e-5, distributed=world > 1)
    gm._n_total = V
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64), device=dev)  # noqa: E731
    gm._set_params(t64(w), mu.double(), t64(cov))
    resp0 = pis.contiguous()

    def em_iter():  # one iteration of GaussianMixture.fit's loop, its host read included
        resp, lse = gmm.estep(x0s, gm._e_pc, gm._e_mp, gm._e_ln)
        info = gm._m_step_params(x0s, resp)
        lb_info = torch.stack([lse.double().sum(), (info != 0).any().double()]).cpu()
        assert lb_info[1] == 0
    el_e, ks_e = timed(em_iter, args.steps, args.warmup)
    el_s, ks_s = timed(lambda: gmm.scatter(x0s, resp0, mu), args.steps, args.warmup)
    te, ts = float(np.mean(ks_e)) / 1e3, float(np.mean(ks_s)) / 1e3
    if world > 1:  # max over ranks of every per-step time
        tk = float(np.mean(ks_k)) / 1e3
        t = torch.tensor([tg, tr, te, ts, tk], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        tg, tr, te, ts, tk = t.tolist()
        dist.barrier()
        if rank != 0:
            dist.destroy_process_group()
            return
    cpu = None
    if not args.no_cpu_baseline and world == 1:
        S = 4000
        xs = x0[:S].cpu().numpy()
        t0 = time.time()
        orc.community_train(xs, pi[:S].cpu().numpy(), mu.cpu().numpy(), inv.cpu().numpy(),
                            0.01, 0.1, 1)
        cel = time.time() - t0
        blas = blas_threads()
        cpu = {"value": 2.0 * S * K * d * d / cel / 1e12, "unit": "TFLOP/s", "cores": 1,
               "kind": "port", "blas_threads": blas,
               "sample": "Community2Vec.train's numpy loop (community_embeddings.py:61-78, "
                         "restated op for op in oracle/oracle.py) on %d of the %d rows: "
                         "%.2fs -> %.0f s per full pass.  cores 1: the loop's time is numpy's "
                         "elementwise pi * inv_cov products and its stacked [150 x d x d] @ "
                         "[150 x d x 1] matmul, which numpy runs on the calling thread whatever "
                         "the BLAS pool (%s BLAS threads were available); the reference adds no "
                         "threading of its own" % (S, V, cel, cel * V / S, blas)}
        from sklearn.mixture import GaussianMixture as SkGMM
        S2 = 20000
        Xs = x0[:S2].cpu().numpy()
        sk = SkGMM(K, covariance_type="full", reg_covar=1e-5, max_iter=1, tol=0.0,
                   weights_init=w, means_init=mu.cpu().numpy().astype(np.float64),
                   precisions_init=np.linalg.inv(cov), random_state=0)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk._check_parameters(Xs)
            sk._initialize_parameters(Xs, np.random.RandomState(0))
            t0 = time.time()
            lpn, lr = sk._e_step(Xs)
            sk._m_step(Xs, lr)
            sel = time.time() - t0
        cpu["gmm_em_iteration_sample"] = (
            "sklearn GaussianMixture E+M step (community_embeddings.py:27's estimator) on %d "
            "rows: %.2fs -> %.1f s per full-size iteration, its GEMMs on %s BLAS threads" % (
                S2, sel, sel * V / S2, blas))
        cpu["gmm_em_iteration_cores"] = blas
    dist_cfg = {}
    if world > 1:
        dist_cfg = {"community_kernel_only_ms": tk * 1e3,
                    "community_exchange": "all_gather_into_tensor of %d x %d fp32 rows (%s)" % (
                        V, d, args.dist_backend),
                    "em_exchange": "all-reduce of K + K d then K d^2 float64 statistics",
                    "parallelism": "row shard x%d, replicated tables" % world}
    print(json.dumps({
        "metric": "community gradient + GMM responsibilities, 1M nodes K=50 d=128",
        "value": flops / tg / 1e12, "unit": "TFLOP/s (community gradient pass)", "n_gpus": world,
        "scaling": "strong",
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": tg * 1e3,
        "higher_is_better": True, "dtype": "f32", "data": "synthetic N(0,1) rows, random SPD",
        "config": {"workload": "configs[3]/C4: V=%d K=%d d=%d" % (V, K, d),
                   "community_kernel": comm_kernel,
                   # what "f32" means for the bf16-part kernels (README)
                   "arithmetic": ("fp32 operands as three bf16 parts, six exact part products per "
                                  "multiply-add on bf16 MFMAs, fp32 accumulation; error vs "
                                  "float64 at the fp32 kernels' level (tests/test_gpu_c4.py)")
                                 if comm_bf3 else "fp32 MFMA (exact fp32 products)",
                   # E-step / scatter: 2 V K d^2 algorithmic flops, of which the kernels execute
                   # only the upper-triangular / symmetric blocks (fractions above)
                   "gmm_resp_kernel": resp_kernel, "gmm_resp_blocks_executed": tri_resp,
                   "gmm_resp_ms": tr * 1e3, "gmm_resp_tflops_effective": flops / tr / 1e12,
                   "gmm_resp_tflops_executed": flops * tri_resp / tr / 1e12,
                   "gmm_scatter_ms": ts * 1e3, "gmm_scatter_tflops_effective": flops / ts / 1e12,
                   "gmm_scatter_kernel": cov_kernel, "gmm_scatter_blocks_executed": tri_cov,
                   "gmm_scatter_tflops_executed": flops * tri_cov / ts / 1e12,
                   "gmm_em_iteration_ms": te * 1e3, **dist_cfg},
        "roofline": {"bound": "mfma", "achieved": flops / tg / 1e12 / world,
                     "peak": comm_peak, "unit": "TFLOP/s (per GPU)",
                     "peak_basis": ("bf16 MFMA peak %.1f / 6 part products per fp32 multiply-add"
                                    % BF16_MFMA_PEAK_TFLOPS) if comm_bf3 else "fp32 MFMA peak",
                     "frac": flops / tg / 1e12 / world / comm_peak,
                     "frac_of_fp32_mfma_peak": flops / tg / 1e12 / world / F32_MFMA_PEAK_TFLOPS,
                     "flops_per_pass": flops, "avg_kernel_ms": tg * 1e3},
        "cpu_baseline": cpu}))


def walks(args):
    import random
    import torch
    from come_amd import graph_utils as gu
    from come_amd.graph import chung_lu
    dev = torch.device("cuda", 0)
    g = chung_lu(args.nodes, 20.0, gamma=2.5, seed=1)
    L = 80
    rowptr = torch.from_numpy(g.rowptr).to(dev)
    col = torch.from_numpy(g.col.astype(np.int32)).to(dev)
    starts = torch.randperm(g.V, device=dev).int()
    out = torch.empty((g.V, L), dtype=torch.int32, device=dev)
    it = iter(range(10 ** 9))

    def step():
        gu.device_walks(rowptr, col, starts, L, alpha=0.0, seed=next(it), out=out)
    el, ks = timed(step, args.steps, args.warmup)
    steps_per_launch = float((out >= 0).sum().item() - g.V)  # moves (the start is not a step)
    avg = float(np.mean(ks)) / 1e3
    bps = 24  # algorithmic: rowptr pair + one col entry + the written entry
    # What bounds it: each step is a dependent chain of random 128-B line reads -- 1.70 requests
    # per step measured (profiles/r03_pmc_walks.json: rowptr line, col line, 17% L2 hits), served
    # by the Infinity Cache (rowptr + col = 88 MB at C3) -> priced against the guide's
    # Infinity-Cache random-gather rate
    req_bytes = 1.70 * 128
    ic_peak = 8600.0  # GB/s, MI355X_MICROARCH.md 'Indexed rows': 38 MB table, random rows (IC)
    cpu = None
    if not args.no_cpu_baseline:
        Gh = gu.Graph(np.arange(1, g.V + 1), g.rowptr, g.col.astype(np.int32), g.degree,
                      np.zeros((0, 2), np.int32))
        from oracle import oracle as orc
        threads = orc.usable_cpus()  # the cgroup quota (16 on the GPU box), not os.cpu_count()
        t0 = time.time()  # one full pass per stream, streams on parallel threads
        w = gu._corpus(Gh, [1] * threads, L, 0.0, [random.Random(s) for s in range(threads)],
                       threads=threads)
        cel = time.time() - t0
        moves = float((w >= 0).sum() - w.shape[0])
        cpu = {"value": moves / cel, "unit": "walk-steps/s", "cores": threads, "kind": "port",
               "sample": "exact CPython-stream walker (come_walks_reference, restating "
                         "graph_utils.build_deepwalk_corpus + __random_walk__), %d streams x one "
                         "pass of %d walks on %d host threads: %.1fs" % (threads, g.V, threads,
                                                                        cel)}
    print(json.dumps({
        "metric": "random-walk steps/sec, 1M-node power-law graph, walk length 80",
        "value": steps_per_launch * args.steps / el, "unit": "walk-steps/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
        "higher_is_better": True, "dtype": "int32", "data": "synthetic Chung-Lu (seed 1)",
        "config": {"workload": "walk corpus pass: V=%d, E=%d, L=%d, alpha=0" % (
            g.V, g.num_edges, L)},
        "roofline": {"bound": "infinity-cache gathers",
                     "achieved": req_bytes * steps_per_launch / avg / 1e9,
                     "peak": ic_peak, "unit": "GB/s",
                     "frac": req_bytes * steps_per_launch / avg / 1e9 / ic_peak,
                     "request_bytes_per_step": req_bytes,
                     "algorithmic_bytes_per_step": bps,
                     "algorithmic_frac_of_hbm": bps * steps_per_launch / avg / 1e9 / HBM_PEAK_GBS,
                     "avg_kernel_ms": avg * 1e3},
        "cpu_baseline": cpu}))


def kmeans_bench(args):
    """The k-means initialisation of the C4 GMM fit (V rows, K clusters, d features): one Lloyd
    iteration of the torch path (GaussianMixture._kmeans_labels' arithmetic: distance matrix,
    argmin, bincount, index_add_, centre update and the host read of the shift) against the native
    one (come_kmeans_lloyd + come_kmeans_update, the shift read every fourth iteration as
    come_amd.kmeans.KMeans runs it), both from the same seeded centres over the same number of
    iterations; the seeding of both; a full KMeans.fit; and the k-means share of a
    GaussianMixture fit with each backend."""
    import torch
    from come_amd import gmm, kmeans
    dev = torch.device("cuda", 0)
    V, K, d = args.nodes, args.k, args.dim
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    mu = torch.randn((K, d), generator=g, device=dev) * 0.5
    lab = torch.randint(0, K, (V,), generator=g, device=dev)
    X = (mu[lab] + torch.randn((V, d), generator=g, device=dev)).contiguous()
    del lab
    xx = (X * X).sum(1)

    def wall(fn, reps=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, out

    def gens():
        a = torch.Generator(device=dev)
        a.manual_seed(11)
        return a
    gm = gmm.GaussianMixture(K)
    gm._kmeans_plusplus(X[:4096].contiguous(), xx[:4096].contiguous(), gens())  # warm-up
    kmeans.kmeans_plusplus(X[:4096].contiguous(), xx[:4096].contiguous(), K, gens())
    seed_torch_ms, C0 = wall(lambda: gm._kmeans_plusplus(X, xx, gens()))
    seed_native_ms, C1 = wall(lambda: kmeans.kmeans_plusplus(X, xx, K, gens()))
    same_seeds = bool(torch.equal(C0, C1))
    C0 = C0.contiguous()
    # the seeding in libcome.so (kmeans_plusplus_native): the whole seeding by the wall clock, and
    # its pass over X (come_kmeans_pp_step: k_pp_step + k_pp_pots) alone by events
    kmeans.kmeans_plusplus_native(X[:4096].contiguous(), K, gens())  # warm-up
    seed_kernels_ms, _ = wall(lambda: kmeans.kmeans_plusplus_native(X, K, gens()))
    trials = 2 + int(math.log(K))
    pp_chunks, _ = kmeans.pp_plan(V, d, trials, kmeans._cus(dev))
    pp_cand = torch.randint(0, V, (trials,), generator=gens(), device=dev).to(torch.int32)
    pp_out = kmeans.pp_step(X, xx, pp_cand, pp_chunks)
    _, ss = timed(lambda: kmeans.pp_step(X, xx, pp_cand, pp_chunks, out=pp_out), args.steps,
                  args.warmup)
    t_step = float(np.mean(ss))
    log("seeding: torch %.1f ms, native estimator's torch chain %.1f ms, kernels %.1f ms; one "
        "step kernel %.3f ms (%d candidates)" % (seed_torch_ms, seed_native_ms, seed_kernels_ms,
                                                 t_step, trials))

    def torch_iter(C):  # gmm.py _kmeans_labels, one iteration
        dist_ = xx[:, None] - 2 * X @ C.t() + (C * C).sum(1)[None]
        labels = torch.argmin(dist_, 1)
        cnt = torch.bincount(labels, minlength=K).float()
        S = torch.zeros((K, d), dtype=torch.float32, device=X.device)
        S.index_add_(0, labels, X)
        newC = torch.where(cnt[:, None] > 0, S / cnt.clamp_min(1)[:, None], C)
        float(((newC - C) ** 2).sum())
        return newC

    def run_torch(n):
        C = C0
        for _ in range(n):
            C = torch_iter(C)
        return C

    def run_native(n):
        C = C0.clone()
        for i in range(1, n + 1):
            _, sums, counts, _ = kmeans.accumulate(X, C)
            shift2 = kmeans.update(C, sums, counts)
            if i % 4 == 0:
                float(shift2)
        return C
    run_torch(args.warmup)
    run_native(args.warmup)
    t_torch, Ct = wall(lambda: run_torch(args.steps))
    t_native, Cn = wall(lambda: run_native(args.steps))
    t_torch /= args.steps
    t_native /= args.steps
    centre_diff = float((Ct - Cn).abs().max())
    Cf = C0.clone()
    _, ks = timed(lambda: kmeans.accumulate(X, Cf), args.steps, args.warmup)
    t_kernel = float(np.mean(ks))
    log("torch %.3f ms / iteration, native %.3f ms (lloyd + reduce launches alone %.3f ms)" % (
        t_torch, t_native, t_kernel))
    fit_ms, km = wall(lambda: kmeans.KMeans(K, random_state=0).fit(X))
    fit_pp_ms, km_pp = wall(lambda: kmeans.KMeans(K, random_state=0, seeding='native').fit(X))
    shares = {}
    for name, backend, seeding in (("torch", "torch", "torch"), ("native", "native", "torch"),
                                   ("native_seeding_native", "native", "native")):
        gmm.GaussianMixture(K, reg_covar=1e-5, max_iter=2, random_state=0, kmeans_max_iter=2,
                            kmeans_backend=backend, kmeans_seeding=seeding).fit(X)  # warm-up:
        # library scratch, BLAS
        m = gmm.GaussianMixture(K, reg_covar=1e-5, n_init=1, random_state=0,
                                kmeans_backend=backend, kmeans_seeding=seeding)
        spent = [0.0]
        inner = m._kmeans_labels

        def timed_init(X_, gen_, inner=inner, spent=spent):
            ms, out = wall(lambda: inner(X_, gen_))
            spent[0] += ms
            return out
        m._kmeans_labels = timed_init
        total_ms, _ = wall(lambda: m.fit(X))
        shares[name] = {"fit_ms": total_ms, "kmeans_ms": spent[0],
                        "kmeans_share": spent[0] / total_ms, "em_iterations": int(m.n_iter_),
                        "lower_bound": float(m.lower_bound_)}
        log("GaussianMixture fit, kmeans_backend=%s, kmeans_seeding=%s: %.0f ms, k-means %.0f ms"
            % (backend, seeding, total_ms, spent[0]))
    mfma_flops = 2.0 * 2 * V * 64 * d  # scores and one-hot sums, K padded to 64
    print(json.dumps({
        "metric": "k-means Lloyd iteration, %d rows K=%d d=%d" % (V, K, d),
        "value": t_native, "unit": "ms per Lloyd iteration (native)", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": t_native,
        "higher_is_better": False, "dtype": "f32",
        "data": "synthetic: %d centres 0.5 N(0,1), unit noise" % K,
        "config": {"workload": "k-means init of the C4 GMM fit: V=%d K=%d d=%d" % (V, K, d),
                   "torch_iteration_ms": t_torch, "native_iteration_ms": t_native,
                   "speedup_vs_torch_iteration": t_torch / t_native,
                   "native_lloyd_launches_ms": t_kernel,
                   "max_centre_difference_after_%d_iterations" % args.steps: centre_diff,
                   "seeding_torch_ms": seed_torch_ms, "seeding_native_ms": seed_native_ms,
                   "seedings_identical": same_seeds,
                   "seeding_native_kernels_ms": seed_kernels_ms,
                   "seeding_kernels_speedup_vs_native_ms": seed_native_ms / seed_kernels_ms,
                   "seeding_trials": trials,
                   "seeding_step_kernel_ms": t_step,
                   "seeding_step_kernel_hbm_gbs": V * d * 4 / (t_step / 1e3) / 1e9,
                   "seeding_step_kernel_hbm_frac": V * d * 4 / (t_step / 1e3) / 1e9 / HBM_PEAK_GBS,
                   "kmeans_fit_ms": fit_ms, "kmeans_fit_n_iter": int(km.n_iter_),
                   "kmeans_fit_seeding_share": seed_native_ms / fit_ms,
                   "kmeans_fit_seeding_native_ms": fit_pp_ms,
                   "kmeans_fit_seeding_native_n_iter": int(km_pp.n_iter_),
                   "gaussian_mixture_fit": shares},
        "roofline": {"bound": "hbm", "achieved": V * d * 4 / (t_kernel / 1e3) / 1e9,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": V * d * 4 / (t_kernel / 1e3) / 1e9 / HBM_PEAK_GBS,
                     "fp32_mfma_frac": mfma_flops / (t_kernel / 1e3) / 1e12 / F32_MFMA_PEAK_TFLOPS,
                     "mfma_flops_per_iteration": mfma_flops, "avg_kernel_ms": t_kernel},
        "cpu_baseline": None}))


def community_loss_bench(args):
    import torch
    from come_amd import _lib
    from come_amd import community_embeddings as ce
    from come_amd import gmm
    dev = torch.device("cuda", 0)
    V, K, d = args.nodes, args.k, args.dim
    rng = np.random.RandomState(2)  # c4's operands
    x = torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32)).to(dev)
    A = rng.standard_normal((K, d, d)) / np.sqrt(d)
    cov = (np.einsum("kij,klj->kil", A, A) + np.eye(d)[None] * 0.5).astype(np.float32)
    mu = (rng.standard_normal((K, d)) * 0.5).astype(np.float32)
    pi_h = np.random.RandomState(3).dirichlet(np.ones(K), V).astype(np.float32)
    pi = torch.from_numpy(pi_h).to(dev)
    mu_t, cov_t = torch.from_numpy(mu).to(dev), torch.from_numpy(cov).to(dev)
    pc, mp, ln = ce.community_loss_params(mu_t, cov_t)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    L, ptr, stream = _lib.lib(), _lib.ptr, _lib.stream_handle(dev)

    def loss_pass():
        _lib.check(L.come_community_loss(ptr(x), V, d, ptr(pi), ptr(pc), ptr(mp), ptr(ln), K, None,
                                         ptr(total), stream), "come_community_loss")
    _, ks_l = timed(loss_pass, args.steps, args.warmup)
    _, ks_e = timed(lambda: gmm.estep(x, pc, mp, ln), args.steps, args.warmup)
    _, ks_l2 = timed(loss_pass, args.steps, args.warmup)  # again after the E-step: same-run spread
    _, ks_p = timed(lambda: ce.community_loss(x, pi, mu_t, cov_t), args.steps, args.warmup)
    tl, te, tl2, tp = (float(np.mean(k)) for k in (ks_l, ks_e, ks_l2, ks_p))
    value = ce.community_loss(x, pi, mu_t, cov_t)
    flops = 2.0 * V * K * d * d
    # the MFMA blocks executed on the upper factors (k_comm_loss_b16 as k_gmm_resp_b16: 16-wide
    # column tiles x 32-feature steps, 20 of 32 at d = 128, 6 of 8 at d = 64); six bf16 part
    # products per multiply-add, so the ceiling is the bf16 MFMA peak / 6
    tri = {128: 20 / 32, 64: 6 / 8}.get(d, 1.0)
    cpu = None
    if not args.no_cpu_baseline:
        from scipy.stats import multivariate_normal
        S = min(V, 2000)
        xs, ps = x[:S].cpu().numpy().astype(np.float64), pi_h[:S].astype(np.float64)
        t0 = time.time()
        sub = sum((ps[:, k] * multivariate_normal(mu[k].astype(np.float64),
                                                  cov[k].astype(np.float64)).logpdf(xs)).sum()
                  for k in range(K))
        cel = time.time() - t0
        sub_gpu = ce.community_loss(x[:S], pi[:S], mu_t, cov_t)
        cpu = {"value": cel * V / S * 1e3, "unit": "ms per pass (scaled)", "kind": "reference",
               "blas_threads": blas_threads(), "subset_rows": S,
               "sample": "sum_k pi[:, k] * scipy.stats.multivariate_normal(mu_k, cov_k).logpdf(x) "
                         "in float64 on %d of the %d rows: %.3f s, scaled by V / %d (the K "
                         "factorisations are counted once per subset, so the scaled figure "
                         "overstates them)" % (S, V, cel, S),
               "subset_total_float64": sub, "subset_total_gpu": sub_gpu}
    print(json.dumps({
        "metric": "community loss, ms per pass, V=%d K=%d d=%d" % (V, K, d),
        "value": tl, "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "higher_is_better": False, "dtype": "f32 (bf16-part MFMA at d = 64, 128)",
        "data": "synthetic (c4's operands, seed 2 / 3)",
        "config": {"workload": "come_community_loss on %d rows, K=%d, d=%d (row_out = NULL)"
                               % (V, K, d)},
        "loss_ms": tl, "loss_ms_min": float(np.min(ks_l)), "loss_ms_second_timing": tl2,
        "estep_ms": te, "estep_ms_min": float(np.min(ks_e)), "loss_over_estep": tl / te,
        "python_community_loss_ms": tp, "total": value,
        "roofline": {"bound": "mfma" if tri < 1.0 else "valu",
                     "achieved": tri * flops / (tl / 1e3) / 1e12,
                     "peak": BF16_MFMA_PEAK_TFLOPS / 6, "unit": "TFLOP/s (executed)",
                     "frac": tri * flops / (tl / 1e3) / 1e12 / (BF16_MFMA_PEAK_TFLOPS / 6),
                     "executed_block_fraction": tri,
                     "dense_equivalent_tflops": flops / (tl / 1e3) / 1e12,
                     "avg_kernel_ms": tl},
        "cpu_baseline": cpu}))


def sgns_loss_bench(args):
    import torch
    import come_amd.training_sdg_inner as tsi
    from come_amd.graph import chung_lu, random_walks
    from come_amd.model import Model
    from come_amd.node_embeddings import Node2Vec
    dev = torch.device("cuda", 0)
    n, d, w, L, B = args.negative, args.dim, 5, 80, 131072
    g = chung_lu(args.nodes, 20.0, gamma=2.5, seed=1, device=dev)  # bench.py's C3 graph
    V = g.V
    B = min(B, V)
    np.random.seed(1234)
    m = Model(g.degree_by_id(), size=d, table_size=args.table_size, k=1, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    starts = torch.randperm(V, generator=gen, device=dev)[:B]
    walks = random_walks(g, 0, L, seed=100, device=dev, starts=starts).contiguous()
    gen.manual_seed(5678)
    seeds = torch.randint(0, 2 ** 48, (B,), generator=gen, device=dev, dtype=torch.int64)
    table = m.negative_table()
    hot = m.hot_rows()
    valid = walks >= 0
    lengths = valid.sum(dim=1).long()
    pairs = int(torch.where(lengths >= w + 1, 2 * w * lengths - w * (w + 1),
                            lengths * (lengths - 1)).sum())
    centres = int((valid & (lengths > 1)[:, None]).sum())
    L_, ptr, stream = tsi._lib.lib(), tsi.ptr, tsi.stream_handle(dev)
    tp, T, flag = tsi._table_args(table)
    out = torch.zeros(2, dtype=torch.float64, device=dev)

    def loss_pass():
        tsi.check(L_.come_sgns_o2_loss(ptr(m.node_embedding), ptr(m.context_embedding), V, d,
                                       ptr(walks), B, L, ptr(seeds), w, n, tp, T, flag, None,
                                       ptr(out), ptr(out.view(torch.int64)[1:]), stream),
                  "come_sgns_o2_loss")

    def train_launch():
        tsi.sgns_o2(m.node_embedding, m.context_embedding, walks, seeds, w, n, table, args.lr, 1.0,
                    tsi.MODE_HOGWILD, hot=hot)
    _, ks_l = timed(loss_pass, args.steps, args.warmup)
    loss_before = float(out[0].item())
    assert int(out.view(torch.int64)[1].item()) == pairs
    _, ks_t = timed(train_launch, args.steps, args.warmup)
    _, ks_l2 = timed(loss_pass, args.steps, args.warmup)  # again after training: same-run spread
    loss_after = float(out[0].item())
    tl, tt, tl2 = (float(np.mean(k)) for k in (ks_l, ks_t, ks_l2))
    row = d * 4
    model_bytes = ((1 + n) * pairs + centres) * row
    naive_bytes = (2 + n) * pairs * row

    # O1: Node2Vec.loss on 1M edges of the graph, native against the torch chain
    E = min(1_000_000, g.num_edges)
    edges = g.edge_ids()[np.random.RandomState(7).choice(g.num_edges, E, replace=False)]
    n2v = Node2Vec()
    rows = torch.from_numpy(n2v._edge_rows(m, edges)).to(dev)
    r0, r1 = rows[:, 0].contiguous(), rows[:, 1].contiguous()
    x = m.node_embedding

    def o1_native():
        return tsi.sgns_pairs_loss(x, x, r0, r1)[0]

    def o1_torch():
        rl = rows[(rows >= 0).all(dim=1)].long()
        dots = (x[rl[:, 1]] * x[rl[:, 0]]).sum(dim=1).double()
        return float(-torch.nn.functional.logsigmoid(dots).sum())
    _, ks_n = timed(o1_native, args.steps, args.warmup)
    _, ks_p = timed(o1_torch, args.steps, args.warmup)
    _, ks_n2 = timed(o1_native, args.steps, args.warmup)
    tn, tpt, tn2 = (float(np.mean(k)) for k in (ks_n, ks_p, ks_n2))
    v_native, v_torch = n2v.loss(m, edges, backend='native'), n2v.loss(m, edges)
    print(json.dumps({
        "metric": "SGNS O2 loss, ms per pass, C3 shape (V=%d d=%d n=%d w=%d, %d walks x %d)"
                  % (V, d, n, w, B, L),
        "value": tl, "unit": "ms", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "higher_is_better": False, "dtype": "f32 dots, f64 softplus and sums",
        "data": "synthetic (bench.py's C3 graph, walker seed 100)",
        "config": {"workload": "come_sgns_o2_loss and the Hogwild come_sgns_o2 launch on the same "
                               "%d walks, packed table; Node2Vec.loss on %d edges" % (B, E),
                   "pairs": pairs, "centres": centres,
                   "negative_table": "packed" if isinstance(table, tsi.PackedTable) else "uint32"},
        "loss_ms": tl, "loss_ms_min": float(np.min(ks_l)), "loss_ms_second_timing": tl2,
        "loss_ms_second_min": float(np.min(ks_l2)),
        "train_ms": tt, "train_ms_min": float(np.min(ks_t)), "loss_over_train": tl / tt,
        "second_loss_over_train": tl2 / tt,
        "loss_total_before_training": loss_before, "loss_total_after_training": loss_after,
        "roofline": {"bound": "hbm", "achieved": model_bytes / (tl / 1e3) / 1e9,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": model_bytes / (tl / 1e3) / 1e9 / HBM_PEAK_GBS,
                     "frac_second_timing": model_bytes / (tl2 / 1e3) / 1e9 / HBM_PEAK_GBS,
                     "model": "(1 + n) rows per pair + one centre row per centre",
                     "model_bytes": model_bytes, "naive_bytes": naive_bytes,
                     "naive_frac": naive_bytes / (tl / 1e3) / 1e9 / HBM_PEAK_GBS,
                     "avg_kernel_ms": tl},
        "node2vec_loss": {"edges": E, "native_ms": tn, "native_ms_second_timing": tn2,
                          "torch_ms": tpt, "native_over_torch": tn / tpt,
                          "native_value": v_native, "torch_value": v_torch,
                          "hbm_frac_native": 2.0 * E * row / (tn / 1e3) / 1e9 / HBM_PEAK_GBS},
        "cpu_baseline": None}))


def c4_diag_bench(args):
    import torch
    from come_amd import _lib
    from come_amd import community_embeddings as ce
    from come_amd import gmm
    dev = torch.device("cuda", 0)
    V, K = args.nodes, args.k
    L, ptr, stream = _lib.lib(), _lib.ptr, _lib.stream_handle(dev)
    pi_h = np.random.RandomState(3).dirichlet(np.ones(K), V).astype(np.float32)
    pi = torch.from_numpy(pi_h).to(dev)
    total = torch.zeros(1, dtype=torch.float64, device=dev)
    shapes = []
    for d in sorted({args.dim, 256}):
        rng = np.random.RandomState(2)
        mu = (rng.standard_normal((K, d)) * 0.5).astype(np.float32)
        var = rng.uniform(0.5, 1.5, (K, d)).astype(np.float32)
        lab = rng.randint(0, K, V)
        x = torch.from_numpy(mu[lab] + rng.standard_normal((V, d)).astype(np.float32)
                             * np.sqrt(var[lab])).to(dev)
        A = rng.standard_normal((K, d, d)) / np.sqrt(d)
        cov = torch.from_numpy((np.einsum("kij,klj->kil", A, A) + np.eye(d)[None] * 0.5)
                               .astype(np.float32)).to(dev)
        mu_t, var_t = torch.from_numpy(mu).to(dev), torch.from_numpy(var).to(dev)
        w = torch.full((K,), 1.0 / K, dtype=torch.float64, device=dev)
        # diagonal operands, and the full-covariance ones of the same mixture size
        ps, mp, ln = (a.float().contiguous() for a in
                      gmm.diag_estep_params(w, mu_t.double(), var_t.double()))
        iv = (1.0 / var_t).contiguous()
        pc_f, mp_f, ln_f = ce.community_loss_params(mu_t, cov)
        inv_f = torch.linalg.inv(cov).contiguous()
        resp = gmm.estep_diag(x, ps, mp, ln)[0]
        gd = gmm.GaussianMixture(K, covariance_type="diag", reg_covar=1e-6)
        gd._n_total = V
        gd._set_params(w, mu_t.double(), var_t.double())
        gf = gmm.GaussianMixture(K, reg_covar=1e-6)
        gf._n_total = V
        gf._set_params(w, mu_t.double(), cov.double())

        def em_iter(g):
            r, lse = g._estep(x)
            info = g._m_step_params(x, r)
            return torch.stack([lse.double().sum(), (info != 0).any().double()]).cpu()

        def loss_diag():
            _lib.check(L.come_community_loss_diag(ptr(x), V, d, ptr(pi), ptr(ps), ptr(mp), ptr(ln),
                                                  K, None, ptr(total), stream), "loss_diag")

        def loss_full():
            _lib.check(L.come_community_loss(ptr(x), V, d, ptr(pi), ptr(pc_f), ptr(mp_f), ptr(ln_f),
                                             K, None, ptr(total), stream), "loss")

        xg = x.clone()
        pairs = {
            "estep": (lambda: gmm.estep_diag(x, ps, mp, ln), lambda: gmm.estep(x, pc_f, mp_f, ln_f)),
            "moments": (lambda: gmm.diag_moments(x, resp),
                        lambda: (gmm.resp_sum(resp), gmm.resp_t_x(resp, x))),
            "scatter": (lambda: gmm.diag_scatter(x, resp, mu_t), lambda: gmm.scatter(x, resp, mu_t)),
            "em_iteration": (lambda: em_iter(gd), lambda: em_iter(gf)),
            "community_step": (lambda: ce.community_grad_diag(xg, pi, mu_t, iv, 0.1, args.lr, 1),
                               lambda: ce.community_grad(xg, pi, mu_t, inv_f, 0.1, args.lr, 1)),
            "loss": (loss_diag, loss_full),
        }
        ms = {}
        for name, (fd, ff) in pairs.items():
            kd = timed(fd, args.steps, args.warmup)[1]
            kf = timed(ff, max(2, args.steps // 2), 1)[1]
            ms[name] = {"diag_ms": float(np.mean(kd)), "diag_ms_min": float(np.min(kd)),
                        "full_ms": float(np.mean(kf)), "full_ms_min": float(np.min(kf)),
                        "full_over_diag": float(np.mean(kf) / np.mean(kd))}
            log("d=%d %s: diag %.3f ms, full %.3f ms" % (d, name, ms[name]["diag_ms"],
                                                        ms[name]["full_ms"]))
        # bit-identity across two passes of every diagonal entry
        def once():
            r, lse = gmm.estep_diag(x, ps, mp, ln)
            nk, sx = gmm.diag_moments(x, resp)
            ssq = gmm.diag_scatter(x, resp, mu_t)
            y = x.clone()
            ce.community_grad_diag(y, pi, mu_t, iv, 0.1, args.lr, 2)
            loss_diag()
            return r, lse, nk, sx, ssq, y, total.clone()
        a, b = once(), once()
        same = all(torch.equal(u, v) for u, v in zip(a, b))
        # roofline: the larger of compulsory bytes / HBM and fused multiply-adds (2 flop) / the fp32
        # peak, which the vector unit and the fp32 MFMA (the moments' unit) share; the timings are
        # taken around the Python wrappers, allocations included, so frac is of wrapper time
        el = float(V) * K * d
        xb, rb = 4.0 * V * d, 4.0 * V * K
        model = {"estep": (xb + rb + 4.0 * V, 2 * el), "moments": (xb + rb, el),
                 "scatter": (xb + rb, 2 * el), "community_step": (2 * xb + rb, 2 * el),
                 "loss": (xb + rb, 2 * el)}
        roof = {}
        for name, (nbytes, fma) in model.items():
            t_mem, t_valu = nbytes / (HBM_PEAK_GBS * 1e6), 2 * fma / (F32_MFMA_PEAK_TFLOPS * 1e9)
            bound = max(t_mem, t_valu)
            roof[name] = {"bytes": nbytes, "fma": fma, "hbm_ms": t_mem, "valu_ms": t_valu,
                          "bound": "hbm" if t_mem >= t_valu else "fp32", "bound_ms": bound,
                          "frac": bound / ms[name]["diag_ms"]}
        shapes.append({"V": V, "K": K, "d": d, "ms": ms, "roofline": roof,
                       "bit_identical_two_passes": bool(same),
                       "chunks": gmm.diag_plan(V, d, K, torch.cuda.get_device_properties(dev)
                                               .multi_processor_count)})
        del x, xg, cov, pc_f, inv_f, resp, gd, gf, a, b
        torch.cuda.empty_cache()
    first = shapes[0]
    print(json.dumps({
        "metric": "diagonal-covariance EM iteration, ms, V=%d K=%d d=%d" % (V, K, first["d"]),
        "value": first["ms"]["em_iteration"]["diag_ms"], "unit": "ms", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "higher_is_better": False, "dtype": "f32",
        "data": "synthetic (blobs with per-feature variances in [0.5, 1.5], seed 2 / 3)",
        "config": {"workload": "diagonal-covariance kernels beside their full-covariance "
                               "counterparts, V=%d K=%d, d in %s" % (V, K, [s_["d"] for s_ in shapes])},
        "shapes": shapes, "cpu_baseline": None}))


def topk_bench(args):
    """Exact top-k neighbour search (come_topk) beside the torch chain it replaces, V rows of d
    floats, k = 10, cosine, at Q = 16,384 and at Q = 1; both paths get the base norms / the
    normalised base computed once, outside the timing."""
    import torch
    from come_amd import neighbors
    dev = torch.device("cuda", 0)
    V, d, k, QB = args.nodes, args.dim, 10, 2048
    g = torch.Generator(device=dev).manual_seed(17)
    base = torch.randn((V, d), generator=g, device=dev, dtype=torch.float32)
    index = neighbors.Index(base, "cosine")
    base_n = torch.nn.functional.normalize(base, dim=1)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    torch.cuda.synchronize()
    rows = []
    for Q in (16384, 1):
        qs = torch.randn((Q, d), generator=g, device=dev, dtype=torch.float32)

        def fused():
            return index.search(qs, k)

        def chain():
            out = []
            for r0 in range(0, Q, QB):
                qn = torch.nn.functional.normalize(qs[r0:r0 + QB], dim=1)
                sc, ix = torch.topk(qn @ base_n.t(), k, dim=1)
                out.append((ix, sc))
            return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

        res = {}
        for name, fn, steps, warm in (("fused", fused, args.steps, args.warmup),
                                      ("torch_chain", chain, min(args.steps, 3), 1),
                                      ("fused_again", fused, args.steps, 1)):
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            _, ks = timed(fn, steps, warm)
            ms = float(np.mean(ks))
            res[name] = {"ms": ms, "ms_min": float(np.min(ks)), "ms_max": float(np.max(ks)),
                         "steps": steps, "queries_per_s": Q / (ms / 1e3),
                         "tflops": 2.0 * Q * V * d / (ms / 1e3) / 1e12,
                         "peak_bytes_over_the_tables":
                             int(torch.cuda.max_memory_allocated(dev) - held)}
        # executed flops of the fused kernel: whole 128-query tiles x whole 32-row base tiles
        chunks, per = neighbors.plan(Q, V, d, k, cus)
        executed = 2.0 * (-(-Q // 128) * 128) * (chunks * per) * d
        for name in ("fused", "fused_again"):
            res[name]["executed_tflops"] = executed / (res[name]["ms"] / 1e3) / 1e12
            res[name]["frac_of_f32_mfma_peak"] = res[name]["executed_tflops"] / F32_MFMA_PEAK_TFLOPS
        (fi, fs), (ti, ts) = fused(), chain()
        same = float((fi == ti).float().mean())
        rows.append({"Q": Q, "chunks": chunks, "rows_per_chunk": per,
                     "scratch_bytes": neighbors.scratch_bytes(Q, V, k, chunks, True),
                     "index_agreement_with_torch": same,
                     "max_abs_score_difference": float((fs - ts).abs().max()), **res})
        log("Q=%d: fused %.3f ms, torch chain %.3f ms, fused again %.3f ms" % (
            Q, res["fused"]["ms"], res["torch_chain"]["ms"], res["fused_again"]["ms"]))
    big = rows[0]
    print(json.dumps({
        "metric": "exact top-%d cosine search, ms per %d queries, V=%d d=%d" % (k, big["Q"], V, d),
        "value": big["fused"]["ms"], "unit": "ms", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "higher_is_better": False, "dtype": "f32 (fp32 MFMA)",
        "data": "synthetic N(0, 1) rows (device generator, seed 17)",
        "config": {"workload": "come_topk (neighbors.Index.search) beside normalised matmul + "
                               "torch.topk over query batches of %d" % QB},
        "roofline": {"bound": "mfma", "achieved": big["fused"]["executed_tflops"],
                     "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s (executed)",
                     "frac": big["fused"]["frac_of_f32_mfma_peak"]},
        "shapes": rows}))


def blas_threads():
    """Threads of the BLAS pool numpy / scipy / sklearn run on in this process (threadpoolctl),
    None if it cannot tell."""
    try:
        from threadpoolctl import threadpool_info
        n = [i.get("num_threads") for i in threadpool_info() if i.get("user_api") == "blas"]
        return max(n) if n else None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["c2", "c4", "walks", "kmeans", "community_loss", "sgns_loss", "c4_diag", "topk"], required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--table-size", type=int, default=100_000_000)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--lr", type=float, default=0.1)  # lr 0.1 for every config
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--hot-p", type=float, default=None,
                    help="c2: contended-row share (default training_sdg_inner.default_hot_share; "
                         "0 = no float-atomic rows)")
    ap.add_argument("--plain-table", action="store_true",
                    help="c2: draw negatives from the uint32 table instead of the product's "
                         "exact packed form (Model.negative_table)")
    ap.add_argument("--dist-backend", default="nccl",
                    help="c4 with N > 1: nccl (= RCCL); gloo only to rehearse on one GPU")
    ap.add_argument("--all-ranks-device0", action="store_true",
                    help="rehearsal: every rank on cuda:0 (needs --dist-backend gloo)")
    ap.add_argument("--opt", action="append", default=[],
                    help="come_set_option knob, e.g. --opt o1_pipe=0 (A/B experiments)")
    args = ap.parse_args()
    if args.opt:
        from come_amd import _lib
        for kv in args.opt:
            k, v = kv.split("=")
            _lib.set_option(k, int(v))
    {"c2": c2, "c4": c4, "walks": walks, "kmeans": kmeans_bench,
     "community_loss": community_loss_bench, "sgns_loss": sgns_loss_bench,
     "c4_diag": c4_diag_bench, "topk": topk_bench}[args.workload](args)


if __name__ == "__main__":
    main()
