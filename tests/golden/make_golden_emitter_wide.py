#!/usr/bin/env python3
"""Generate tests/golden/emitter_wide.npz by IMPORTING the reference in the build container.

Runs only where /root/reference is mounted (never on the GPU box).  Records what the reference's own
``GenePredHMMEmitter(num_copies=c, share_intron_parameters=...)`` returns from ``forward`` (training False and
True) for the gene models above 64 states or 32 kernel rows: 3 copies shared (43 states, 37 rows), 5 copies shared
(71 states, 61 rows) and 18 copies unshared (253 states and rows).  fp32 data only: the input, each model's
emission kernel, its two outputs.

The input (b = 2, L = 24, 15 classes, one-hot nucleotides with N) is handed over as a clone: the reference's
left-pivot k-mer helper mutates its argument (defect D5), so the recorded outputs carry the doubled N mass of
the right-pivot 3-mers — what ``n_mass_compat=True`` / ``d5_compat=True`` reproduce.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_emitter_wide.py
"""
import os
import sys
import types

os.environ["MKL_CBWR"] = "COMPATIBLE"
os.environ["ATEN_CPU_CAPABILITY"] = "avx2"

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path[:0] = [REF, os.path.join(REF, "hmm_layer")]
for n in ("learnMSA", "learnMSA.msa_hmm", "learnMSA.msa_hmm.Utility"):
    sys.modules[n] = types.ModuleType(n)
sys.modules["learnMSA.msa_hmm.Utility"].deserialize = lambda o: o

from hmm_layer.gene_pred_hmm_emitter import GenePredHMMEmitter  # noqa: E402

CODONS = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
              intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
              intron_end_pattern=[("AGN", .99), ("ACN", .01)])
MODELS = [(3, True), (5, True), (18, False)]          # (num_copies, share_intron_parameters)
B, L, S = 2, 24, 15


def main():
    g = torch.Generator().manual_seed(20240918)
    cls = torch.softmax(2 * torch.randn((1, B, L, S), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 5, (1, B, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1)
    out = {"x": x.numpy().copy(), "models": np.array([[c, int(sh)] for c, sh in MODELS], dtype=np.int64)}
    for c, shared in MODELS:
        em = GenePredHMMEmitter(num_copies=c, share_intron_parameters=shared, **CODONS)
        em.build((1, B, L, S))
        with torch.no_grad():
            em.emission_kernel.copy_(torch.randn(em.emission_kernel.shape, generator=g))
        em.recurrent_init()
        tag = "c%d_%s" % (c, "shared" if shared else "unshared")
        E = em(x.clone()).detach()
        Et = em(x.clone(), training=True).detach()
        assert tuple(E.shape) == (1, B, L, 1 + 14 * c) == tuple(Et.shape)
        out[tag + "_kernel"] = em.emission_kernel.detach().numpy().copy()
        out[tag + "_E"] = E.numpy()
        out[tag + "_E_training"] = Et.numpy()
    assert np.array_equal(out["x"], x.numpy())          # the clones took the mutation, not x
    path = os.path.join(HERE, "emitter_wide.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d models)" % (path, os.path.getsize(path), len(MODELS)))


if __name__ == "__main__":
    main()
