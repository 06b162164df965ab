"""bench.py --dump-outputs: what dump_outputs() writes, on CPU tensors (the sampling is host-side indexing)."""
import os

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _outputs(b, L, q):
    g = torch.Generator().manual_seed(5)
    out = torch.rand((1, b, L, q), generator=g)
    ll = torch.randn((1, b), generator=g, dtype=torch.float64)
    part = torch.stack([ll.sum(1), torch.full((1,), float(b), dtype=torch.float64)], 1)
    return out, ll, part


def test_whole_output_when_it_fits(tmp_path):
    out, ll, part = _outputs(6, 50, 3)
    bench.dump_outputs(str(tmp_path), out, ll, part)
    arr = _load(tmp_path)
    assert sorted(arr) == ["gamma_sample", "gamma_sample_sequences", "loglik", "loglik_partials"]
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert np.array_equal(arr["gamma_sample_sequences"], np.arange(6.0))
    assert np.array_equal(arr["gamma_sample"], out[0].numpy())
    assert np.array_equal(arr["loglik"], ll.numpy()) and np.array_equal(arr["loglik_partials"], part.numpy())


def test_seeded_sample_of_sequences_and_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_GAMMA_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_LOGLIK_BYTES", 16)
    out, ll, part = _outputs(5, 400, 3)                # one sequence alone (4800 B) exceeds the share
    runs = []
    for sub in ("a", "b"):
        d = str(tmp_path / sub)
        bench.dump_outputs(d, out, ll, part)
        runs.append(_load(d))
    a, b = runs
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    seqs, pos = a["gamma_sample_sequences"].astype(int), a["gamma_sample_positions"].astype(int)
    assert len(seqs) == 1 and 0 <= seqs[0] < 5
    assert len(pos) == 4096 // (3 * 4 + 8) and np.all(np.diff(pos) > 0) and 0 <= pos[0] and pos[-1] < 400
    assert np.array_equal(a["gamma_sample"], out[0, seqs][:, pos].numpy())
    assert a["gamma_sample"].nbytes <= 4096
    assert np.array_equal(a["loglik"], ll[:, seqs].numpy())        # 5 log-likelihoods exceed their 16-byte share
