import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def load_golden(name):
    """tests/golden/<name>, or the parts <stem>.part<i>.npz it was written in (tools/gen_golden.py save_golden: no
    committed file exceeds 1 MiB) put back together: a dict of the same arrays, pieces <key>@<j> concatenated."""
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    stem = name[:-len(".npz")]
    merged, pieces, i = {}, {}, 0
    while os.path.exists(os.path.join(GOLDEN, "%s.part%d.npz" % (stem, i))):
        with np.load(os.path.join(GOLDEN, "%s.part%d.npz" % (stem, i)), allow_pickle=False) as z:
            for k in z.files:
                if "@" in k:
                    key, j = k.rsplit("@", 1)
                    pieces.setdefault(key, {})[int(j)] = z[k]
                else:
                    merged[k] = z[k]
        i += 1
    if i == 0:
        raise FileNotFoundError(path)
    for key, by_index in pieces.items():
        merged[key] = np.concatenate([by_index[j] for j in sorted(by_index)])
    return merged


@pytest.fixture(scope="session")
def bunny():
    """Vertex block of the reference's data/bun000.ply (40256 x 3, float32)."""
    return np.load(os.path.join(GOLDEN, "bun000_xyz.npy"))
