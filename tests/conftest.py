import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def load_golden(name):
    """The arrays of the fixture `name` as one dict: tests/golden/<name>.npz, or, where that
    archive would pass the 1 MiB limit on committed files, its parts <name>.0.npz, <name>.1.npz,
    ... (written by tests/golden/make_golden.py save_parts; every array is in exactly one)."""
    import glob

    import numpy as np
    parts = sorted(glob.glob(os.path.join(GOLDEN, name + ".[0-9].npz")))
    out = {}
    for p in parts or [os.path.join(GOLDEN, name + ".npz")]:
        with np.load(p) as z:
            for k in z.files:
                assert k not in out, (p, k)
                out[k] = z[k]
    return out


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through libcome.so on cuda:0)")
