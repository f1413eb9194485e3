#!/usr/bin/env python3
"""Throughput of the edge-weighted walker against the uniform walker, on the graph of
`scripts/walks_pq_bench.py` (chung_lu(1M, 20, gamma 2.5, seed 1), alpha = 0).

One launch = 1,048,576 walks x 80.  Variants alternate inside every round (so drift hits all of
them alike), each launch timed with device events after warm-up rounds:
    uniform          come_random_walks, the yardstick (on the ascending adjacency all variants use)
    w-unit(1,1)      come_random_walks_w on unit weights at p = q = 1 (the same walks, through the
                     CDF search)
    w-lognormal(p,q) come_random_walks_w on seeded log-normal weights (sigma 1) at (1, 1),
                     (0.25, 4) and (4, 0.25)
Per variant: walk-steps/s (median launch), trials per step (trials_out / steps taken), the ratio to
the uniform walker and the run-to-run spread (min, max and max/min - 1 of the launches).
come_walk_cdf (sort not included) is timed once per weight set.  Writes one JSON file (default
profiles/r15_walks_weighted_bench.json) and prints it.

    python scripts/walks_weighted_bench.py [--rounds 12] [--warmup 2] [--o2-ms 649] [--out FILE]

--o2-ms: the O2 launch time of the same machine (bench.py's ms_per_step); with it the file also
holds each variant's corpus time as a fraction of that launch (target: under 0.10)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = [("uniform", None, None), ("w-unit(1,1)", "unit", (1.0, 1.0)),
            ("w-lognormal(1,1)", "lognormal", (1.0, 1.0)),
            ("w-lognormal(0.25,4)", "lognormal", (0.25, 4.0)),
            ("w-lognormal(4,0.25)", "lognormal", (4.0, 0.25))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--walks", type=int, default=1 << 20)
    ap.add_argument("--length", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--o2-ms", type=float, default=None)
    ap.add_argument("--out",
                    default=os.path.join(ROOT, "profiles", "r15_walks_weighted_bench.json"))
    args = ap.parse_args()
    import torch
    from come_amd import _lib
    from come_amd import graph_utils as gu
    from come_amd.graph import CSRGraph, chung_lu
    dev = torch.device("cuda", 0)
    g = chung_lu(args.nodes, 20.0, gamma=2.5, seed=1)
    ew = np.random.default_rng(15).lognormal(0.0, 1.0, g.num_edges).astype(np.float32)
    g = CSRGraph(g.V, g.edges, weights=ew)  # the same adjacency, weights on both directions
    L, P = args.length, args.walks
    rowptr = torch.from_numpy(g.rowptr).to(dev)
    col0 = torch.from_numpy(g.col.astype(np.int32)).to(dev)
    row = torch.repeat_interleave(torch.arange(g.V, device=dev), rowptr[1:] - rowptr[:-1])
    key, order = torch.sort((row << 32) | col0.to(torch.int64), stable=True)  # rows ascending
    col = (key & 0xFFFFFFFF).to(torch.int32).contiguous()
    del row, key
    lib, ptr = _lib.lib(), _lib.ptr

    wcdf, cdf_ms = {}, {}
    weights = {"unit": torch.ones(col.numel(), dtype=torch.float32, device=dev),
               "lognormal": torch.from_numpy(g.weights).to(dev)}
    for name, w in weights.items():
        ws = gu._gather_1d(w, order)  # the kernel alone, on weights already in col's order
        out_cdf = torch.zeros(col.numel(), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        times = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.come_walk_cdf(ptr(rowptr), ptr(ws), g.V, ptr(out_cdf), ptr(status),
                                         _lib.stream_handle(dev)), "come_walk_cdf")
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        assert int(status) == 0
        wcdf[name], cdf_ms[name] = out_cdf, times[-1]

    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    starts = torch.cat([torch.randperm(g.V, generator=gen, device=dev)
                        for _ in range((P + g.V - 1) // g.V)])[:P].int().contiguous()
    out = torch.empty((P, L), dtype=torch.int32, device=dev)
    trials = torch.zeros(1, dtype=torch.int64, device=dev)

    def launch(wname, pq, seed):
        if wname is None:
            gu.device_walks(rowptr, col, starts, L, alpha=0.0, seed=seed, out=out)
        else:
            _lib.check(lib.come_random_walks_w(
                ptr(rowptr), ptr(col), ptr(wcdf[wname]), g.V, ptr(starts), P, L, 0.0, pq[0], pq[1],
                seed, 0, None, ptr(out), ptr(trials), _lib.stream_handle(dev)),
                "come_random_walks_w")

    ms = {name: [] for name, _, _ in VARIANTS}
    steps, blocks = {}, {}
    for r in range(args.warmup + args.rounds):
        for name, wname, pq in VARIANTS:
            trials.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(wname, pq, 1000 + r)
            e1.record()
            e1.synchronize()
            if r >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
            if r == args.warmup:  # moves of this launch (the start is not a step)
                steps[name] = int((out >= 0).sum().item()) - int((out[:, 0] >= 0).sum().item())
                blocks[name] = int(trials.item()) if wname is not None else steps[name]
    base = steps["uniform"] / (np.median(ms["uniform"]) * 1e-3)
    res = {"graph": "chung_lu(%d, 20, gamma 2.5, seed 1): E=%d; lognormal(0, 1) weights, seed 15"
                    % (g.V, g.num_edges),
           "launch": "%d walks x %d, alpha = 0" % (P, L), "rounds": args.rounds,
           "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
           "o2_launch_ms": args.o2_ms, "max_degree": int(g.degree.max()),
           "walk_cdf_ms": cdf_ms, "variants": {}}
    for name, _, _ in VARIANTS:
        t = np.array(ms[name])
        rate = steps[name] / (np.median(t) * 1e-3)
        v = {"steps_per_s": rate, "ms_median": float(np.median(t)), "ms_min": float(t.min()),
             "ms_max": float(t.max()), "spread": float(t.max() / t.min() - 1.0),
             "steps_per_launch": steps[name], "trials_per_step": blocks[name] / steps[name],
             "ratio_to_uniform": rate / base}
        if args.o2_ms:
            v["fraction_of_o2_launch"] = float(np.median(t)) / args.o2_ms
        res["variants"][name] = v
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
