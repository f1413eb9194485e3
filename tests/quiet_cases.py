"""Inputs shared by tests/test_quiet_rule_host.py and tests/test_gpu_quiet_rows.py: heavy-tailed
degrees and the negative table the product builds from them (oracle.make_table, ids 1..V)."""
import functools

import numpy as np

from oracle import oracle as orc

# (V, T, visitors, seed): visitors = wavefronts in flight x (2 window + 1)
INPUTS = [(64, 2560, 11, 6), (333, 20000, 45, 7), (4097, 100003, 300, 0),
          (20000, 400000, 1408, 0), (20000, 2000000, 1408, 0)]
EPS = [0.05, 0.4, 1.6]


@functools.lru_cache(maxsize=None)
def degree_table(V, T, seed):
    """(degrees float64 [V], table uint32 [T]), both read-only: Pareto(1.3) degrees >= 1 (a few
    hubs, most rows near 1) and the table make_table builds from them for rows 0..V-1 with ids
    1..V."""
    deg = np.random.RandomState(seed).pareto(1.3, V) + 1.0
    table = orc.make_table(deg, T)
    deg.setflags(write=False)
    table.setflags(write=False)
    return deg, table
