#!/usr/bin/env python3
"""Cost of edge sampling by weight in front of the O1 launch, at C2's shape (sbm(100, 1000, 0.016,
4.04e-5, seed 0): 100k nodes, about 1M edges; d = 128, n = 5, lr 0.1, T = 1e8, the product's
packed table and hot rows -- bench_aux.py's C2 launch).

Two weight sets: seeded log-normal(0, 1) weights (model counts = strengths) and unit weights
(counts = degrees).  Variants alternate inside every round (so drift hits all of them alike), each
launch timed with device events after warm-up rounds, S = E throughout:
    edges-order      sgns_o1 on the plain edge list in G.edges() order (the yardstick: the unchanged
                     O1 pass over the same number of edges; k_sgns_o1_runs finds its input-row runs)
    edges-permuted   the same launch on a random permutation of the list (no runs: what losing them
                     costs, on its own)
    <set>/cdf        come_edge_cdf (once per graph in Node2Vec.train)
    <set>/sample     come_edge_sample, S = E draws (once per pass)
    <set>/o1         sgns_o1 on those draws
Per variant the median, minimum and maximum launch in ms and the run-to-run spread; per weight set
the sampler's and the whole sampled pass's ratio to the launch it feeds and to the yardstick.
Writes one JSON file (default profiles/r16_o1_weighted_bench.json) and prints it.

    python scripts/o1_weighted_bench.py [--rounds 12] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--table-size", type=int, default=100_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_o1_weighted_bench.json"))
    args = ap.parse_args()
    import torch
    import come_amd.training_sdg_inner as tsi
    from come_amd import _lib
    from come_amd.graph import CSRGraph, sbm
    from come_amd.model import Model
    dev = torch.device("cuda", 0)
    g = sbm(100, 1000, 0.016, 4.04e-5, seed=0)
    E = g.num_edges
    ew = np.random.default_rng(16).lognormal(0.0, 1.0, E).astype(np.float32)
    gw = CSRGraph(g.V, g.edges, weights=ew)
    assert np.array_equal(gw.edges, g.edges)
    edges = torch.from_numpy(g.edges.astype(np.int32)).to(dev)  # G.edges() order
    permuted = edges[torch.from_numpy(np.random.default_rng(17).permutation(E)).to(dev)]
    permuted = permuted.contiguous()
    np.random.seed(99)
    seeds = [torch.from_numpy(tsi.draw_seeds(E).view(np.int64)).to(dev) for _ in range(4)]

    sets = {}
    for name, graph, w in (("lognormal", gw, gw.edge_weights), ("unit", g, np.ones(E, np.float32))):
        np.random.seed(1234)
        m = Model(graph.degree_by_id(weighted=name == "lognormal"), size=args.dim,
                  table_size=args.table_size, k=100, device=dev)
        sets[name] = {"model": m, "hot": m.hot_rows(), "table": m.negative_table(),
                      "w": torch.from_numpy(np.ascontiguousarray(w)).to(dev)}
        sets[name]["ecdf"] = tsi.edge_cdf(sets[name]["w"])
        sets[name]["draws"] = tsi.sample_edges(edges, sets[name]["ecdf"], E, 7)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    node0 = sets["unit"]["model"].node_embedding.clone()
    node = node0.clone()

    def o1(rows, s, r):
        tsi.sgns_o1(node, rows, seeds[r % len(seeds)], args.negative, s["table"], args.lr,
                    tsi.MODE_HOGWILD, hot=s["hot"])

    variants = [("edges-order", lambda r: o1(edges, sets["unit"], r)),
                ("edges-permuted", lambda r: o1(permuted, sets["unit"], r))]
    for name, s in sets.items():
        def cdf(r, s=s):  # the entry point alone (no read-back of the status word)
            _lib.check(_lib.lib().come_edge_cdf(_lib.ptr(s["w"]), E, _lib.ptr(s["ecdf"]),
                                                _lib.ptr(status), _lib.stream_handle(dev)),
                       "come_edge_cdf")

        def sample(r, s=s):
            s["draws"] = tsi.sample_edges(edges, s["ecdf"], E, 1000 + r)
        variants += [(name + "/cdf", cdf), (name + "/sample", sample),
                     (name + "/o1", lambda r, s=s: o1(s["draws"], s, r))]

    ms = {name: [] for name, _ in variants}
    for r in range(args.warmup + args.rounds):
        for name, fn in variants:
            node.copy_(node0)  # every launch trains the same table: the clipping sees one state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(r)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    assert int(status.item()) == 0
    res = {"graph": "sbm(100, 1000, 0.016, 4.04e-5, seed 0): V=%d E=%d; lognormal(0, 1) weights, "
                    "seed 16" % (g.V, E),
           "launch": "S = E = %d, d=%d, negative=%d, lr=%g, T=%d (packed), Hogwild with hot rows"
                     % (E, args.dim, args.negative, args.lr, args.table_size),
           "rounds": args.rounds, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "variants": {}, "ratios": {}}
    med = {}
    for name, _ in variants:
        t = np.array(ms[name])
        med[name] = float(np.median(t))
        res["variants"][name] = {"ms_median": med[name], "ms_min": float(t.min()),
                                 "ms_max": float(t.max()),
                                 "spread": float(t.max() / t.min() - 1.0)}
    res["ratios"]["edges-permuted / edges-order"] = med["edges-permuted"] / med["edges-order"]
    for name in sets:
        res["ratios"][name] = {
            "sample / o1 on the draws": med[name + "/sample"] / med[name + "/o1"],
            "sample / edges-order": med[name + "/sample"] / med["edges-order"],
            "(sample + o1) / edges-order":
                (med[name + "/sample"] + med[name + "/o1"]) / med["edges-order"],
            "o1 on the draws / edges-permuted": med[name + "/o1"] / med["edges-permuted"],
            "distinct edges drawn / E":
                float(torch.unique(tsi.sample_edges(edges, sets[name]["ecdf"], E, 7,
                                                    return_index=True)[1]).numel()) / E}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
