"""The round-aware chunk rule on the device: its capacity constants against the occupancy query and the CU count,
and the smallest shape at which it engages (k = 1, b = 2048, L = 8200: 34 816 (sequence, chunk) pairs at T = 512,
1.06 rounds of resident blocks) against the fp64 oracle, against the same chunk length forced by hand, and through the
window diagnostics that size their buffers from hmm_chunk_len."""
import numpy as np
import pytest
import torch

from hmm_layer_amd import engine
from oracle import build as obuild
from oracle import params

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, L = 2048, 8200
SAMPLE = [0, 682, 1365, 2047]
TOL_GAMMA, TOL_LOGLIK_REL = 2e-5, 1e-6          # bench.py's accuracy gates


def model(q):
    if q == 15:
        return params.intended_A15().numpy().astype(np.float32), np.full(15, 1 / 15, dtype=np.float32)
    rng = np.random.default_rng(q)
    A = rng.random((q, q)) ** 3 + 1e-3
    A /= A.sum(-1, keepdims=True)
    pi = rng.random(q) + 0.1
    return A.astype(np.float32), (pi / pi.sum()).astype(np.float32)


def run(q):
    """One posterior pass of the default plan at (1, B, L, q) -> (A, pi, E, gamma, loglik) on the device."""
    A, pi = model(q)
    g = torch.Generator(device=DEV).manual_seed(100 + q)
    E = torch.rand((1, B, L, q), device=DEV, generator=g) * 0.9 + 0.05
    A, pi = torch.tensor(A, device=DEV).unsqueeze(0), torch.tensor(pi, device=DEV)
    out, ll = engine.posterior(A, pi, E)
    torch.cuda.synchronize()
    return A, pi, E, out, ll


def check_against_oracle(A, pi, E, out, ll):
    g64, ll64 = obuild.posterior(A[0].cpu().numpy(), pi.cpu().numpy(), E[0, SAMPLE].cpu().numpy())
    err = float(np.abs(out[0, SAMPLE].cpu().numpy() - g64).max())
    lerr = float(np.max(np.abs(ll[0, SAMPLE].cpu().numpy() - ll64) / np.abs(ll64)))
    print("max |gamma - gamma64| = %.3g, max relative log-likelihood error = %.3g" % (err, lerr))
    assert err < TOL_GAMMA and lerr < TOL_LOGLIK_REL, (err, lerr)


@pytest.fixture(scope="module")
def pass3():
    return run(3)


def test_capacity_constants_match_the_device():
    want, got = engine.plan_capacity(), engine.plan_capacity_device(DEV)
    print(want, got)
    assert got == want
    assert got["cus"] == torch.cuda.get_device_properties(DEV).multi_processor_count


def test_rule_engages_and_matches_the_oracle(pass3):
    T = engine.chunk_len(1, B, L, 3)
    assert T % 16 == 0 and 256 <= T < 512
    check_against_oracle(*pass3)


def test_forced_chunk_gives_the_same_bits(pass3):
    A, pi, E, out, ll = pass3
    T = engine.chunk_len(1, B, L, 3)
    with engine.option(engine.OPT_CHUNK, T):
        assert engine.chunk_len(1, B, L, 3) == T
        out2, ll2 = engine.posterior(A, pi, E)
        torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(ll, ll2)
    with engine.option(engine.OPT_CHUNK, 512):                 # the plan before the rule: other sums, same result
        out3, _ = engine.posterior(A, pi, E)
        torch.cuda.synchronize()
    assert float((out3 - out).abs().max()) < TOL_GAMMA


def test_window_diagnostics_follow_the_chunk(pass3):
    A, pi, E, _, _ = pass3
    engine.posterior(A, pi, E)
    dims = (1, B, L, 3)
    C = -(-L // engine.chunk_len(*dims))
    for seq in (0, B - 1):
        tab = engine.window_table(dims, seq)
        assert tab["psi"].shape == (C,) and len(tab["windows"]) <= 16
    d = engine.exact_detail(dims)
    assert 0 <= d["routed"] <= B and d["window_chunks"] >= 0


def test_gene_model_at_the_same_shape():
    assert 256 <= engine.chunk_len(1, B, L, 15) < 512
    check_against_oracle(*run(15))
