"""bench.py's command line, at a toy size: a plain run prints the result line and measures nothing
beside its timed steps; --dump-outputs writes the same arrays in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dump_is_the_hogwild_kernel_in_walk_order_on_the_given_tables(tmp_path, monkeypatch):
    """dump_outputs against the sequential oracle: the timed trainer's Hogwild launch on one
    wavefront (no contended rows here, so bit-exact, as test_o2_edge_shapes_bit_exact holds the
    kernel to) over the first DUMP_WALKS walks only, from the tables handed in, the model's own
    tables untouched; written are the visited rows, ascending, sampled down to the byte cap."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    from come_amd.context_embeddings import Context2Vec
    from come_amd.model import Model
    from oracle import oracle as orc
    monkeypatch.setattr(bench, "DUMP_WALKS", 48)
    monkeypatch.setattr(bench, "DUMP_TABLE_BYTES", 4 * 128 * 500)
    rng = np.random.RandomState(7)
    V, d, L, w, neg, lr = 5000, 128, 40, 5, 5, 0.1
    dev = torch.device("cuda", 0)
    np.random.seed(3)
    model = Model((np.arange(1, V + 1), rng.randint(1, 50, V)), size=d, table_size=200_000, k=1,
                  device=dev)
    node0 = model.node_embedding.cpu().numpy().copy()
    ctx0 = rng.uniform(-0.1, 0.1, (V, d)).astype(np.float32)
    walks = rng.randint(0, V, (64, L)).astype(np.int32)
    walks[rng.uniform(size=walks.shape) < 0.05] = -1
    seeds = rng.randint(0, 2 ** 48, 64, dtype=np.int64)
    learner = Context2Vec(lr=lr, window_size=w, negative=neg, hot_share=0.0)
    bench.dump_outputs(str(tmp_path), model, learner,
                       (torch.from_numpy(node0).to(dev), torch.from_numpy(ctx0).to(dev)),
                       torch.from_numpy(walks).to(dev), torch.from_numpy(seeds).to(dev))
    n_ref, c_ref = node0.copy(), ctx0.copy()
    orc.sgns_o2(n_ref, c_ref, walks[:48], seeds[:48].view(np.uint64), w, neg, model.table_host,
                lr, 1.0, dot_mode=orc.DOT_WAVE64)
    head = walks[:48]
    rows = np.unique(head[head >= 0])
    assert len(rows) > 500
    rows = rows[np.sort(np.random.RandomState(0).choice(len(rows), 500, replace=False))]
    np.testing.assert_array_equal(np.load(tmp_path / "node_embedding.npy"), n_ref[rows])
    np.testing.assert_array_equal(np.load(tmp_path / "context_embedding.npy"), c_ref[rows])
    assert not np.array_equal(n_ref[rows], node0[rows])  # trained rows
    np.testing.assert_array_equal(model.node_embedding.cpu().numpy(), node0)
    assert not model.context_embedding.any()


@pytest.mark.gpu
def test_plain_run_prints_the_line_and_dumps_reproducible_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    outs = [tmp_path / "dump0", tmp_path / "dump1"]
    # two runs with the same arguments, side by side
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                               "--steps", "3", "--warmup", "1", "--nodes", "60000",
                               "--table-size", "1000000", "--walks-per-step", "8192",
                               "--dump-outputs", str(o)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for o in outs]
    res = [p.communicate(timeout=300) for p in procs]
    for p, (so, se) in zip(procs, res):
        assert p.returncode == 0, se[-2000:]
    lines = [x for x in res[0][0].splitlines() if x.strip()]
    assert len(lines) == 1, res[0][0]
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1
    assert j["unit"] == "pair-updates/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    # ms_per_step is the time of one timed step: value = pairs per step / that time
    assert j["ms_per_step"] > 0
    pairs = j["config"]["pairs_per_step_per_gpu"]
    assert j["value"] * j["ms_per_step"] / 1e3 == pytest.approx(pairs, rel=1e-9)
    # what takes runs of its own is behind --full
    assert j["cpu_baseline"] is None and "secondary" not in j and "sync_measure" not in j
    import bench
    keep = bench.DUMP_TABLE_BYTES // (4 * 128)
    for o in outs:
        assert sorted(os.listdir(o)) == ["context_embedding.npy", "node_embedding.npy"]
        assert sum(os.path.getsize(o / f) for f in os.listdir(o)) <= 64_000_000
    rows = None
    for name in ("node_embedding", "context_embedding"):
        a, b = (np.load(o / (name + ".npy")) for o in outs)
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 128, (name, a.dtype)
        rows = a.shape[0] if rows is None else rows
        assert 1024 <= a.shape[0] <= keep and a.shape[0] == rows  # one row per visited node
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=name)  # bit for bit, run to run
    # the context table starts at zero: the dump holds trained rows
    assert np.abs(np.load(outs[0] / "context_embedding.npy")).max() > 0
