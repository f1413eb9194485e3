"""End-to-end ComE on one GPU: the adsc_Karate.py:104-137 flow on a synthetic stochastic block
model, every phase through come_amd (no reference code), with per-phase timings and the NMI of
the GMM communities against the planted blocks.

    python scripts/come_e2e.py [--blocks 100 --block-size 1000 --dim 128 --p 1 --q 1 ...]

Phases (reference file:line): walks (graph_utils.py:187-192 -> device walker), O1 pre-training
(node_embeddings.py:35), O2 pre-training (context_embeddings.py:41), then per outer iteration
O1 + O2 + GMM fit (community_embeddings.py:20-37, GPU EM) + community gradient
(community_embeddings.py:61-78).  --p / --q: node2vec's return / in-out bias of the walks (the
second-order device walker; the default 1, 1 is the uniform walker).  --w-in / --w-out: weights
of the intra- / inter-block edges (the default 1, 1 is the unweighted run); with other values the
walks are edge-weighted (come_random_walks_w) and the model's counts are the node strengths, from
which the negative table, the hot rows and the quiet rows are derived.  --weighted-o1 (off by
default; needs --w-in or --w-out): the O1 passes train edges sampled by weight on the device
(Node2Vec.train(weights=g.edge_weights)) instead of every edge once.  --knn K: the share of each node's K nearest neighbours (cosine,
neighbors.knn_graph over the trained node_embedding) that lie in its own block: a record, no bar.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(blocks=100, block_size=1000, p_in=0.016, p_out=4.04e-5, dim=128, negative=5,
        window=5, walk_length=40, num_walks=5, iters=1, lr=0.025, alpha=1.0, beta=0.1,
        com_iters=5, seed=0, reg_covar=1e-5, n_init=3, deterministic=False, log=print, p=1.0,
        q=1.0, w_in=1.0, w_out=1.0, weighted_o1=False, knn=0):
    import torch
    from sklearn.metrics import normalized_mutual_info_score
    from come_amd.community_embeddings import Community2Vec
    from come_amd.context_embeddings import Context2Vec
    from come_amd.graph import CSRGraph, random_walks, sbm
    from come_amd.model import Model
    from come_amd.node_embeddings import Node2Vec

    dev = torch.device("cuda", 0)
    t = {}

    def tick(name, t0):
        torch.cuda.synchronize(dev)
        t[name] = t.get(name, 0.0) + time.time() - t0

    t0 = time.time()
    g = sbm(blocks, block_size, p_in, p_out, seed=seed)
    labels = np.arange(g.V) // block_size
    weighted = w_in != 1.0 or w_out != 1.0
    if weighted_o1 and not weighted:
        raise ValueError("--weighted-o1 needs edge weights: pass --w-in or --w-out")
    if weighted:  # the same adjacency, intra-block edges w_in, inter-block edges w_out
        same = labels[g.edges[:, 0]] == labels[g.edges[:, 1]]
        g = CSRGraph(g.V, g.edges, weights=np.where(same, w_in, w_out))
    t["graph_s"] = time.time() - t0
    np.random.seed(seed)
    t0 = time.time()
    model = Model(g.degree_by_id(weighted=weighted), size=dim,
                  table_size=max(10 ** 6, 100 * g.V), k=blocks, device=dev)
    tick("model_s", t0)
    t0 = time.time()
    walks = random_walks(g, num_walks, walk_length, seed=seed + 1, device=dev, p=p, q=q)
    walks_ids = torch.where(walks >= 0, walks + 1, walks)  # rows -> node ids (ids = row + 1)
    tick("walks_s", t0)
    edges = g.edge_ids()
    o1w = {"weights": g.edge_weights} if weighted_o1 else {}  # sampler seeds: the numpy RNG
    nl = Node2Vec(lr=lr, negative=negative, deterministic=deterministic)
    cl = Context2Vec(lr=lr, window_size=window, negative=negative, deterministic=deterministic)
    cm = Community2Vec(model, lr=lr, reg_covar=reg_covar)
    cm.g_mixture.n_init = n_init
    pairs = 0
    t0 = time.time()
    nl.train(model, edges=edges, iter=1, **o1w)
    tick("o1_s", t0)
    t0 = time.time()
    pairs += cl.train(model, paths=walks_ids, total_nodes=walks.numel(), alpha=alpha)
    tick("o2_s", t0)
    for _ in range(iters):
        t0 = time.time()
        nl.train(model, edges=edges, iter=1, **o1w)
        tick("o1_s", t0)
        t0 = time.time()
        pairs += cl.train(model, paths=walks_ids, total_nodes=walks.numel(), alpha=alpha)
        tick("o2_s", t0)
        t0 = time.time()
        cm.fit(model)
        tick("gmm_fit_s", t0)
        t0 = time.time()
        cm.train(range(1, g.V + 1), model, beta, iter=com_iters)
        tick("community_s", t0)
    pred = torch.argmax(model.pi, 1).cpu().numpy()
    nmi = float(normalized_mutual_info_score(labels, pred))
    out = {"nodes": g.V, "edges": int(g.num_edges), "blocks": blocks, "dim": dim,
           "o2_pairs": int(pairs), "nmi": nmi,
           "gmm_converged": bool(getattr(cm.g_mixture, "converged_", False)),
           "timings_s": {k: round(v, 4) for k, v in t.items()}}
    if knn > 0:  # the share of each node's K cosine neighbours that lie in its own block
        from come_amd.neighbors import knn_graph
        t0 = time.time()
        nb, _ = knn_graph(model.node_embedding, knn, metric="cosine")
        tick("knn_s", t0)
        nb = nb.cpu().numpy()
        same = (labels[np.maximum(nb, 0)] == labels[:, None]) & (nb >= 0)
        out["knn"] = {"k": knn, "same_block_share": float(same.mean()),
                      "seconds": round(t["knn_s"], 4)}
    if p != 1.0 or q != 1.0:
        out["walk_bias"] = {"p": p, "q": q}
    if weighted:
        out["edge_weights"] = {"w_in": w_in, "w_out": w_out, "weighted_o1": bool(weighted_o1)}
    log(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=100)
    ap.add_argument("--block-size", type=int, default=1000)
    ap.add_argument("--p-in", type=float, default=0.016)
    ap.add_argument("--p-out", type=float, default=4.04e-5)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--walk-length", type=int, default=40)
    ap.add_argument("--num-walks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--n-init", type=int, default=3)
    ap.add_argument("--p", type=float, default=1.0, help="node2vec return bias of the walks")
    ap.add_argument("--q", type=float, default=1.0, help="node2vec in-out bias of the walks")
    ap.add_argument("--w-in", type=float, default=1.0, help="weight of the intra-block edges")
    ap.add_argument("--w-out", type=float, default=1.0, help="weight of the inter-block edges")
    ap.add_argument("--weighted-o1", action="store_true",
                    help="train O1 on edges sampled by weight (needs --w-in or --w-out)")
    ap.add_argument("--knn", type=int, default=0,
                    help="also report the share of each node's K nearest neighbours (cosine, "
                         "neighbors.knn_graph) that lie in its own block (K <= 64)")
    args = ap.parse_args()
    run(blocks=args.blocks, block_size=args.block_size, p_in=args.p_in, p_out=args.p_out,
        dim=args.dim, negative=args.negative, window=args.window, walk_length=args.walk_length,
        num_walks=args.num_walks, iters=args.iters, n_init=args.n_init, p=args.p, q=args.q,
        w_in=args.w_in, w_out=args.w_out, weighted_o1=args.weighted_o1, knn=args.knn)


if __name__ == "__main__":
    main()
