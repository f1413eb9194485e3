"""Context2Vec.loss with distributed=True over two processes (gloo, CPU): every rank evaluates its
shard_walks shard and the float64 total and the integer pair count are all-reduced.  The HIP kernel
needs a GPU, so the workers swap come_amd.training_sdg_inner.sgns_o2_loss for a wrapper of its CPU
twin (come_amd.cpu.sgns_o2_loss: the same arithmetic on host arrays); what is under test is the
sharding, the seeds every rank draws and the exchange.  The kernel itself:
tests/test_gpu_sgns_loss.py."""
import json
import os
import socket
import types

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from come_amd import context_embeddings as c2
from come_amd import cpu
from come_amd import training_sdg_inner as tsi

V, D, T = 120, 20, 3001


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _twin_sgns_o2_loss(node, ctx, walks, seeds, window, negative, table, return_walks=False):
    """training_sdg_inner.sgns_o2_loss's signature on CPU tensors, through the CPU twin."""
    out = cpu.sgns_o2_loss(node.numpy(), ctx.numpy(), walks.numpy(),
                           seeds.numpy().view(np.uint64), window, negative,
                           None if table is None else table.numpy().view(np.uint32),
                           return_walks=return_walks, threads=1)
    return out if not return_walks else (out[0], out[1], torch.from_numpy(out[2]))


def _model():
    rng = np.random.RandomState(11)
    m = types.SimpleNamespace()
    m.vocab_size, m.down_sampling, m._contiguous = V, 0, True
    m.node_embedding = torch.from_numpy(rng.uniform(-1, 1, (V, D)).astype(np.float32))
    m.context_embedding = torch.from_numpy(rng.uniform(-1, 1, (V, D)).astype(np.float32))
    table = torch.from_numpy(np.sort(rng.randint(0, V, T)).astype(np.int32))
    m.negative_table = lambda: table
    m.rows_of = lambda ids: np.where((np.asarray(ids) >= 1) & (np.asarray(ids) <= V),
                                     np.asarray(ids, np.int64) - 1, -1)
    return m


def _run(distributed):
    m = _model()
    paths = np.random.RandomState(12).randint(1, V + 1, (41, 9))  # 41 walks: uneven shards
    trainer = c2.Context2Vec(window_size=2, negative=3, batch_walks=8, distributed=distributed)
    total, pairs = trainer.loss(m, paths, alpha=0.5, return_pairs=True)  # the all-reduced count
    mean = trainer.loss(m, paths, alpha=0.5, mean=True)
    assert mean == total / pairs
    seeds = np.arange(41, dtype=np.uint64) * np.uint64(7919) + np.uint64(5)
    return {"total": total, "pairs": pairs, "mean": mean,
            "seeded": trainer.loss(m, paths, seeds=seeds)}


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tsi.sgns_o2_loss = _twin_sgns_o2_loss
    with open(os.path.join(out_dir, "r%d.json" % rank), "w") as f:
        json.dump(_run(True), f)
    dist.destroy_process_group()


def test_loss_walk_sharded_world2(tmp_path, monkeypatch):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    monkeypatch.setattr(tsi, "sgns_o2_loss", _twin_sgns_o2_loss)  # undone after the test
    single = _run(False)
    r0, r1 = (json.load(open(os.path.join(str(tmp_path), "r%d.json" % r))) for r in range(world))
    assert r0 == r1  # both ranks return the same values
    paths = np.random.RandomState(12).randint(1, V + 1, (41, 9))
    assert single["pairs"] == r0["pairs"] == tsi.count_o2_pairs((paths - 1).astype(np.int32), 2)
    for key in ("total", "mean", "seeded"):
        assert single[key] > 0
        assert abs(r0[key] - single[key]) <= 1e-12 * abs(single[key]), key
    assert single["seeded"] != 2 * single["total"]  # the seeds given are the seeds used
