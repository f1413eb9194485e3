"""Tier C of the Hogwild O2 launch as a function of the quiet-row rule (Model.quiet_rows: rows with
at most eps expected concurrent visitors stay in the wavefront's LDS ring over a walk window):
held-out loss of one product launch against the sequential oracle, and the launch time (HIP
events), per eps.  eps = 0 is the launch without quiet rows (the parent's kernel and grid).

Cases:
  c3_1m    the bench's own launch, 1,048,576 walks on the 1M-node graph (tests/tierc_inputs.py;
           fixture tests/golden/tierc_c3_1m_seq.json, test_o2_hogwild_at_the_bench_launch's inputs)
  c3_100k  tests/test_gpu_tierc.py's c3_shape: 100k nodes, 10,000 walks, every walk in flight.  The
           product runs the direct kernel there and marks no row quiet (fewer than 32 rows per
           wavefront in flight); this case forces the streaming kernel (o2_kernel=3) to show what
           the rule would do on a small graph.  Its oracle is run here (a few seconds).

    python scripts/tierc_quiet_sweep.py --case c3_1m --eps 0,0.05,0.1,0.2 [--runs 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="c3_1m", choices=["c3_1m", "c3_100k"])
    ap.add_argument("--eps", default="0,0.05,0.1,0.2")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    import come_amd.training_sdg_inner as tsi
    import tierc_inputs as ti
    from oracle import oracle as orc
    dev = torch.device("cuda", 0)
    w, n, lr, d = 5, 5, 0.1, 128
    if args.case == "c3_1m":
        fx = json.load(open(os.path.join(ROOT, "tests", "golden", "tierc_c3_1m_seq.json")))
        x = ti.c3_1m_inputs()
        assert x.digest == fx["inputs_sha256"], "inputs differ from the fixture's"
        V, table, train, seeds, node0 = x.g.V, x.table, x.train, x.seeds, x.node0
        ri, rp, rn = x.heldout(w, n)
        seq_loss, opts = fx["seq_loss"], {}
    else:
        from come_amd.graph import chung_lu, random_walks
        g = chung_lu(100_000, 20.0, gamma=2.5, seed=21)
        V = g.V
        table = orc.make_table(g.degree.astype(np.float64), 100_000_000)
        walks = random_walks(g, 1, 80, seed=22, device="cuda").cpu().numpy()
        rng = np.random.RandomState(23)
        walks = walks[rng.permutation(len(walks))[:12_000]]
        node0 = rng.uniform(-1, 1, (V, d)).astype(np.float32)
        seeds = rng.randint(0, 2 ** 48, 10_000, dtype=np.int64).astype(np.uint64)
        train, held = walks[:10_000], walks[10_000:]
        ri, rp, rn = ti.heldout_o2_pairs(held, w, n, table, 200_000, 24)
        sn, sc = node0.copy(), np.zeros_like(node0)
        orc.sgns_o2_hogwild(sn, sc, train, seeds, w, n, table, lr, 1.0, threads=1)
        seq_loss, opts = ti.sgns_loss(sn, sc, ri, rp, rn), {"o2_kernel": 3}
    tab = torch.from_numpy(table.view(np.int32)).to(dev)
    packed = tsi.pack_table(tab)
    T = len(table)
    hot_min = max(1, int(tsi.DEFAULT_HOT_P * T))
    hot = tsi.hot_rows(tab, V, hot_min)
    tw = torch.from_numpy(np.ascontiguousarray(train)).to(dev)
    ts = torch.from_numpy(np.ascontiguousarray(seeds).view(np.int64)).to(dev)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    waves = min(4 * tsi.QUIET_BLOCKS_PER_CU * cus, tw.shape[0])
    print("case %s: V %d, walks %d, waves in flight with quiet rows %d, seq loss %.5f" % (
        args.case, V, tw.shape[0], waves, seq_loss), flush=True)
    out = {"case": args.case, "seq_loss": seq_loss, "points": []}
    for eps in [float(e) for e in args.eps.split(",")]:
        quiet = tsi.quiet_rows(tab, V, waves * (2 * w + 1), eps, hot_min) if eps > 0 else None
        nq = 0 if quiet is None else int(np.unpackbits(quiet.cpu().numpy().view(np.uint8)).sum())
        for _ in range(args.runs):
            node = torch.from_numpy(node0).to(dev)
            ctx = torch.zeros_like(node)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            tsi.sgns_o2(node, ctx, tw, ts, w, n, packed, lr, 1.0, tsi.MODE_HOGWILD, hot=hot,
                        quiet=quiet, opts=opts or None)
            ev[1].record()
            torch.cuda.synchronize()
            loss = ti.compact_loss(node, ctx, ri, rp, rn)
            pt = {"eps": eps, "quiet_rows": nq, "loss": loss,
                  "rel_to_seq": (loss - seq_loss) / seq_loss,
                  "launch_ms": ev[0].elapsed_time(ev[1])}
            out["points"].append(pt)
            print(json.dumps(pt), flush=True)
            del node, ctx
            torch.cuda.empty_cache()
    if args.out:
        json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
