#!/usr/bin/env python3
"""Generate tests/golden/mvn_diag.npz by IMPORTING the reference in the build container.

Runs only where /root/reference is mounted (never on the GPU box).  Records, for a few tiny cases, what
the reference's own ``MvnMixture(dim, kernel, diag_only=True, diag_bijector=DefaultDiagBijector(v))
.log_pdf(inputs)`` returns (hmm_layer/MvnMixture.py:125-175, hmm_layer/Utility.py:31-42): fp32 data only.

As shipped, component_log_pdf adds log_det (k1, 1, k2, c) to the transposed distances (k1, batch, c, k2): with
one component the sum broadcasts to (k1, batch, k2, k2), entry [n, i, j] = -0.5 (const + log_det_i + MD_j), and
log_pdf's ``[..., 0]`` keeps j = 0 — every row is given row 0's distance.  The intended density of row i is the
diagonal entry [n, i, i].  Both are recorded: ``log_pdf`` (what log_pdf returns, = entries [n, i, 0]) and
``component_log_pdf_diagonal`` (entries [n, i, i] of the tensor it is cut from).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mvn.py
"""
import os
import sys
import warnings

os.environ["MKL_CBWR"] = "COMPATIBLE"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path[:0] = [REF, os.path.join(REF, "hmm_layer")]

from MvnMixture import MvnMixture            # noqa: E402
from Utility import DefaultDiagBijector     # noqa: E402

CASES = [(1, 5, 1.0), (3, 13, 1.0), (16, 5, 0.25), (16, 13, 1.0), (3, 5, 0.25), (1, 13, 0.25)]   # (d, rows, variance)
N = 40


def main():
    out = {}
    gen = torch.Generator().manual_seed(20240917)
    for i, (d, rows, var) in enumerate(CASES):
        # means and inputs of spread 0.5, scale kernel of spread 0.3: |log_pdf| stays below 100, where fp32's own
        # rounding (the recorded values are fp32) is below 4e-6
        kernel = torch.randn(1, rows, 1, 2 * d, generator=gen) * torch.cat([torch.full((d,), 0.5), torch.full((d,), 0.3)])
        inputs = 0.5 * torch.randn(1, N, d, generator=gen)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # MvnMixture copies its kernel with torch.tensor(tensor)
            mvn = MvnMixture(d, kernel, diag_only=True, diag_bijector=DefaultDiagBijector(np.float32(var)))
            log_pdf = mvn.log_pdf(inputs)             # (1, N, rows)
            comp = mvn.component_log_pdf(inputs)      # (1, N, rows, rows), see above
        assert tuple(log_pdf.shape) == (1, N, rows) and tuple(comp.shape) == (1, N, rows, rows)
        out["case%d_dims" % i] = np.array([d, rows, N], dtype=np.int64)
        out["case%d_variance" % i] = np.array(var, dtype=np.float64)
        out["case%d_kernel" % i] = kernel.numpy()
        out["case%d_inputs" % i] = inputs.numpy()
        out["case%d_log_pdf" % i] = log_pdf.detach().numpy()
        assert torch.equal(comp[..., 0], log_pdf) and float(comp.abs().max()) < 100
        out["case%d_component_log_pdf_diagonal" % i] = torch.diagonal(comp, dim1=-2, dim2=-1).detach().numpy()
    path = os.path.join(HERE, "mvn_diag.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d cases)" % (path, os.path.getsize(path), len(CASES)))


if __name__ == "__main__":
    main()
