"""Share of plain pairs in the benchmark's own corpus, counted on the CPU.

k_sgns_o2_stream takes its straight path for a pair whose context-table rows (center, n draws) are
pairwise distinct, all rows of the table, disjoint from the next pair's draws and center (the next
pair may share the center), whose center is not among the next pair's draws, and whose input row
is not the next pair's.  This script rebuilds bench.py's workload (graph, negative table, the
walks and seeds of the first timed step), replays the reference's draw stream (pyx:133-134: one
48-bit LCG per walk, n draws per pair) for a sample of walks and applies that test.

    python scripts/count_plain_pairs.py [--sample 4096] [bench.py's shape arguments]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MUL, ADD, MASK = np.uint64(25214903917), np.uint64(11), np.uint64((1 << 48) - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--mean-degree", type=float, default=20.0)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--walk-length", type=int, default=80)
    ap.add_argument("--walks-per-step", type=int, default=1 << 20)
    ap.add_argument("--table-size", type=int, default=100_000_000)
    args = ap.parse_args()

    import torch

    from come_amd.graph import chung_lu, random_walks
    from come_amd.model import Model

    dev = torch.device("cuda", 0)
    g = chung_lu(args.nodes, args.mean_degree, gamma=2.5, seed=1, device=dev)
    V, n, w, L, B = g.V, args.negative, args.window, args.walk_length, args.walks_per_step
    np.random.seed(1234)
    model = Model(g.degree_by_id(), size=args.dim, table_size=args.table_size, k=1, device=dev)
    total = (args.warmup + args.steps) * B
    gen = torch.Generator(device=dev)
    gen.manual_seed(100)
    starts = torch.cat([torch.randperm(V, generator=gen, device=dev)
                        for _ in range((total + V - 1) // V)])
    lo, S = args.warmup * B, args.sample  # the first walks of the first timed step
    walks = random_walks(g, 0, L, seed=100, device=dev, starts=starts[lo:lo + S],
                         walk_offset=lo).cpu().numpy()
    gen.manual_seed(5678)
    seeds = torch.randint(0, 2 ** 48, (total,), generator=gen, device=dev,
                          dtype=torch.int64)[lo:lo + S].cpu().numpy().astype(np.uint64)
    table = model.table_host
    T = np.uint64(len(table))

    sched = [(i, j) for i in range(L) for j in range(max(0, i - w), min(L, i + w + 1)) if j != i]
    si, sj = np.array([s[0] for s in sched]), np.array([s[1] for s in sched])
    slots = np.empty((S, len(sched) * n), np.int64)  # every walk's draw stream, in order
    nr = seeds.copy()
    with np.errstate(over="ignore"):
        for k in range(slots.shape[1]):
            slots[:, k] = ((nr >> np.uint64(16)) % T).astype(np.int64)
            nr = (nr * MUL + ADD) & MASK

    pairs = plain = 0
    why = dict(repeat=0, center=0, next_draw=0, next_center=0, center_in_next=0, input_row=0,
               out_of_range=0, last_of_walk=0)
    for p in range(S):
        ok = (walks[p, si] >= 0) & (walks[p, si] < V) & (walks[p, sj] >= 0) & (walks[p, sj] < V)
        ci, cj = walks[p, si][ok].astype(np.int64), walks[p, sj][ok].astype(np.int64)
        Q = len(ci)
        if Q == 0:
            continue
        t = table[slots[p, :Q * n]].astype(np.int64).reshape(Q, n)
        ts = np.sort(t, axis=1)
        c = dict(
            repeat=(ts[:, 1:] == ts[:, :-1]).any(1) if n > 1 else np.zeros(Q, bool),
            center=(t == ci[:, None]).any(1),
            out_of_range=(t >= V).any(1),
            next_draw=np.zeros(Q, bool), next_center=np.zeros(Q, bool),
            center_in_next=np.zeros(Q, bool), input_row=np.zeros(Q, bool),
            last_of_walk=np.zeros(Q, bool))
        c["last_of_walk"][-1] = True
        c["next_draw"][:-1] = (t[:-1, :, None] == t[1:, None, :]).any((1, 2))
        c["next_center"][:-1] = (t[:-1] == ci[1:, None]).any(1)
        c["center_in_next"][:-1] = (t[1:] == ci[:-1, None]).any(1)
        c["input_row"][:-1] = cj[1:] == cj[:-1]
        general = np.zeros(Q, bool)
        for k, v in c.items():
            why[k] += int(v.sum())
            general |= v
        pairs += Q
        plain += int((~general).sum())
    print("walks %d, pairs %d, plain %d = %.4f%%, general %d = %.4f%%" % (
        S, pairs, plain, 100.0 * plain / pairs, pairs - plain, 100.0 * (pairs - plain) / pairs))
    print("general pairs by cause (a pair can have several): " + ", ".join(
        "%s %d (%.4f%%)" % (k, v, 100.0 * v / pairs) for k, v in why.items()))


if __name__ == "__main__":
    main()
