"""World-size-2 gloo test (CPU) of Node2Vec(distributed=True).train(weights=...): every rank
draws the identical sample list and trains its shard of it, the exchange needs nothing new.

As in tests/test_distributed_trainers.py the O1 launch is replaced by an additive stand-in, so the
delta-sum exchange must reproduce the one-process result up to fp32 summation order; the device
CDF and sampler are replaced by their CPU twins, which draw the same list bit for bit."""
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_distributed_trainers import _fake_o1, _free_port


def _cpu_edge_cdf(weights):
    from come_amd import cpu
    return torch.from_numpy(cpu.edge_cdf(weights.numpy()).view(np.int64))


def _cpu_sample_edges(edges, ecdf, S, seed, offset=0, return_index=False):
    from come_amd import cpu
    assert not return_index
    return torch.from_numpy(cpu.sample_edges(edges.numpy(), ecdf.numpy().view(np.uint64), S, seed,
                                             offset))


def _setup(V=40, d=8, seed=11):
    import come_amd.training_sdg_inner as tsi
    from come_amd.model import Model
    tsi.sgns_o1 = _fake_o1
    tsi.edge_cdf = _cpu_edge_cdf
    tsi.sample_edges = _cpu_sample_edges
    np.random.seed(seed)
    model = Model((np.arange(1, V + 1), np.arange(1, V + 1) % 5 + 1), size=d, table_size=1000,
                  k=1, device="cpu")
    rng = np.random.RandomState(3)
    edges = rng.randint(1, V + 1, (31, 2))
    edges[4] = (V + 7, 3)  # an OOV endpoint: weight 0, never drawn
    weights = rng.lognormal(0, 1, len(edges))
    weights[9] = 0.0
    return model, edges, weights


def _run(model, edges, weights, distributed):
    from come_amd.node_embeddings import Node2Vec
    nl = Node2Vec(lr=0.1, negative=3, distributed=distributed, sync_edges=7, combine="sum")
    return nl.train(model, edges=edges, iter=2, weights=weights, samples=45)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, edges, weights = _setup()
    pairs = _run(model, edges, weights, True)
    np.save(os.path.join(out_dir, "node%d.npy" % rank), model.node_embedding.numpy())
    np.save(os.path.join(out_dir, "rng%d.npy" % rank), np.random.random_sample(4))
    np.save(os.path.join(out_dir, "pairs%d.npy" % rank), np.array([pairs]))
    dist.destroy_process_group()


def test_node2vec_weighted_distributed_world2(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    model, edges, weights = _setup()
    before = model.node_embedding.clone()
    pairs = _run(model, edges, weights, False)
    assert pairs == 2 * 2 * 45
    assert not torch.equal(before, model.node_embedding)
    rng = np.random.random_sample(4)
    ld = lambda n, r: np.load(os.path.join(str(tmp_path), "%s%d.npy" % (n, r)))  # noqa: E731
    for r in range(world):
        np.testing.assert_array_equal(ld("node", r), ld("node", 0))
        np.testing.assert_allclose(ld("node", r), model.node_embedding.numpy(), rtol=0, atol=2e-5)
        np.testing.assert_array_equal(ld("rng", r), rng)
    assert ld("pairs", 0)[0] + ld("pairs", 1)[0] == pairs
