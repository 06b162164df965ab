import os
import sys

# The bit-exact fixtures under tests/golden/ are recorded with MKL's COMPATIBLE code path, ATen's AVX2
# kernels and one thread (tests/golden/make_golden.py).  Left to themselves MKL and ATen pick their kernels
# by CPU and split the work by thread count, and the CPU oracle's matmuls and elementwise ops then round
# differently on another machine.  Set before torch first dispatches a CPU op.
os.environ["MKL_CBWR"] = "COMPATIBLE"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture
def golden():
    """load_golden, with torch's CPU ops on one thread for the test (as the fixtures were recorded)."""
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield load_golden
    torch.set_num_threads(n)
