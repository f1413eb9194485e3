"""Input-row visits that fall on "quiet" rows in the benchmark's own corpus, counted on the CPU.

k_sgns_o2_stream reads and writes the input row node[walk[j]] for every pair (i, j).  A walk
position j is the input of the pairs of the 2w + 1 centres around it, so a wavefront that kept
the row on chip while j is inside its window would read and write it once per stay instead of
once per pair.  Holding a row is harmless only while few other wavefronts visit it: a row is
*quiet* when

    waves in flight x (2w + 1) x (the row's share of walk visits)  <=  eps

(the expected number of other wavefronts that have the row in their window at the same time).
The visit share is the degree share.  The negative table gives node id v + 1 (row v) its
count^p / Z of the slots, but stores the *id* in them and the kernels use a slot's value as a row
(model.py:97-122, kept as the reference has it): the slots that hold row v + 1 are sized by row v's
count.  So a row's own table share says nothing about its visits on a graph whose ids are
decorrelated from degree, as the benchmark's are; row v's degree share is recovered from the slots
of row v + 1, share_v = slots_{v+1}^(1/p) / sum_u slots_u^(1/p).  Both bases are printed: "table"
(the row's own slots) and "degree" (the slots of the next row, = the node's own degree up to the
table's rounding).  A hot row (>= hot share of the table by its own slots) is never quiet.

This script rebuilds bench.py's graph and negative table, takes a sample of walks (the bench's
own walks of the first timed step when a GPU is present, otherwise uniform random walks of the
same process from a numpy walker) and prints, per eps:
  phi     share of input-row visits (= pairs) that fall on quiet rows
  reuse   visits per stay: a stay is a maximal run of window positions of one node in which
          consecutive occurrences are at most 2w apart (aliases share one slot)
  saving  predicted bytes saved per pair, phi x (1 - 1 / reuse) x 2 x d x 4

    python scripts/count_quiet_visits.py [--sample 4096] [--eps 0.05 0.1 0.2] [bench.py's shape]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def numpy_walks(g, starts, L, rng):
    """Uniform-neighbour walks (alpha = 0) from `starts`; -1 after a node without neighbours."""
    walks = np.full((len(starts), L), -1, np.int32)
    cur = starts.astype(np.int64)
    alive = np.ones(len(starts), bool)
    for t in range(L):
        walks[alive, t] = cur[alive]
        deg = g.degree[cur]
        alive &= deg > 0
        pick = g.rowptr[cur] + np.minimum((rng.random(len(cur)) * deg).astype(np.int64),
                                          np.maximum(deg - 1, 0))
        cur = np.where(alive, g.col[np.minimum(pick, len(g.col) - 1)], cur).astype(np.int64)
    return walks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--eps", type=float, nargs="+", default=[0.025, 0.05, 0.1, 0.2, 0.4])
    ap.add_argument("--waves", type=int, default=8192, help="wavefronts in flight")
    ap.add_argument("--hot-share", type=float, default=5e-6)
    ap.add_argument("--power", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--mean-degree", type=float, default=20.0)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--walk-length", type=int, default=80)
    ap.add_argument("--walks-per-step", type=int, default=1 << 20)
    ap.add_argument("--table-size", type=int, default=100_000_000)
    args = ap.parse_args()

    import torch

    from come_amd import _lib
    from come_amd.graph import chung_lu, random_walks

    V, w, L, B, S, T = (args.nodes, args.window, args.walk_length, args.walks_per_step,
                        args.sample, args.table_size)
    gpu = torch.cuda.is_available()
    g = chung_lu(V, args.mean_degree, gamma=2.5, seed=1,
                 device=torch.device("cuda", 0) if gpu else None)
    # the negative table as Model.make_table builds it (row v = node id v + 1)
    c = np.zeros(V + 1, np.float64)
    c[1:] = g.degree
    table = np.zeros(T, np.uint32)
    _lib.check(_lib.lib().come_make_table(_lib.ptr(c), V, _lib.ptr(table), T, float(args.power)),
               "come_make_table")
    slots = np.bincount(table, minlength=V + 1).astype(np.float64)
    del table
    true_share = g.degree / g.degree.sum()
    hot = slots[:V] >= max(1, int(args.hot_share * T))
    bases = {}
    for name, sl in (("table", slots[:V]), ("degree", slots[1:V + 1])):
        visit = sl ** (1.0 / args.power)
        bases[name] = visit / visit.sum()

    if gpu:
        dev = torch.device("cuda", 0)
        total = (args.warmup + args.steps) * B
        gen = torch.Generator(device=dev)
        gen.manual_seed(100)
        starts = torch.cat([torch.randperm(V, generator=gen, device=dev)
                            for _ in range((total + V - 1) // V)])
        lo = args.warmup * B
        walks = random_walks(g, 0, L, seed=100, device=dev, starts=starts[lo:lo + S],
                             walk_offset=lo).cpu().numpy()
        src = "bench.py's walks %d..%d" % (lo, lo + S - 1)
    else:
        rng = np.random.default_rng(100)
        walks = numpy_walks(g, rng.permutation(V)[:S], L, rng)
        src = "numpy walker, uniform neighbour, one start per sampled node"

    valid = walks >= 0
    pos = np.arange(L)
    # pairs with input position j: centres i in [j - w, j + w], i != j, walk[i] valid
    csum = np.concatenate([np.zeros((S, 1), np.int64), np.cumsum(valid, 1)], 1)
    lo_i, hi_i = np.maximum(pos - w, 0), np.minimum(pos + w, L - 1)
    uses = (csum[:, hi_i + 1] - csum[:, lo_i] - 1) * valid  # per (walk, j), excluding i == j
    uses = np.maximum(uses, 0)
    pairs = int(uses.sum())
    # distance to the previous occurrence of the same node in the walk (L + 1 if none)
    prev = np.full((S, L), L + 1, np.int64)
    for dlt in range(2 * w, 0, -1):
        same = np.zeros((S, L), bool)
        same[:, dlt:] = (walks[:, dlt:] == walks[:, :-dlt]) & valid[:, dlt:]
        prev[same] = dlt
    starts_stay = prev > 2 * w

    print("graph V=%d E=%d, table T=%d, hot rows %d (share >= %g); %d walks (%s), %d pairs, "
          "%.3f pairs per valid position" % (V, g.num_edges, T, int(hot.sum()), args.hot_share, S,
                                             src, pairs, pairs / max(1, int(valid.sum()))))
    for name, visit in bases.items():
        print("basis %-6s: correlation of the recovered visit share with the degree share %.4f" % (
            name, np.corrcoef(visit, true_share)[0, 1]))
    print("waves %d, window %d: a row of mean visit share has %.4f expected concurrent visitors" % (
        args.waves, w, args.waves * (2 * w + 1) / V))
    hot_vis = int(uses[valid & hot[np.maximum(walks, 0)]].sum())
    print("input visits on hot rows: %.4f" % (hot_vis / pairs))
    row_bytes = 2 * args.dim * 4
    for name, eps in [(b, e) for b in bases for e in args.eps]:
        # expected concurrent visitors of each row <= eps
        quiet = (args.waves * (2 * w + 1) * bases[name] <= eps) & ~hot
        q = valid & quiet[np.maximum(walks, 0)]
        qv = int(uses[q].sum())
        stays = int((q & starts_stay & (uses > 0)).sum())
        phi = qv / pairs
        reuse = qv / max(1, stays)
        print("%-6s eps %-6g quiet rows %8d (%.4f of V; degree <= %d)  phi %.4f  reuse %.3f  "
              "saving %.1f B per pair (%.2f%% of 6,580 B)" % (
                  name, eps, int(quiet.sum()), quiet.mean(),
                  int(g.degree[quiet].max()) if quiet.any() else 0, phi, reuse,
                  phi * (1 - 1 / reuse) * row_bytes,
                  100 * phi * (1 - 1 / reuse) * row_bytes / 6580.0))


if __name__ == "__main__":
    main()
