"""Row staging of the apply kernels (stage_row: the four components of a lane go to LDS without a branch, those that
are not in the row to the chain's pad slot) and the paired column sums of the backward step (col_sum2), at the shapes
where staging can go wrong:

  q in {1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16}: every q mod 4, and lanes whose 4-state window lies wholly outside
      the row (q <= 12); dense random A for each, plus the 15- and 7-state gene models
  b = 3, L in {1, 17, 1007} with OPT_CHUNK = 64: a wave holds columns it does not own (3 chains at L = 1 and 17), 48
      chains span three waves at L = 1007, whose last chunk has 47 steps (no multiple of 16 or of 4); L = 1007 also
      with the chunk length the plan chooses

Every case runs the three posterior modes, forward with log alpha, backward and posterior_decode through the C ABI
with every argument in a guard-banded window (tests/memory_contract.py) and the workspaces at exactly the size the
query returns, and checks

  posteriors          |gamma - gamma64| <= 2e-5, |ll - ll64| <= 1e-6 |ll64| against oracle.build.posterior; the log
                      modes after exp(); POST_LOG_NO_LL carries the log-likelihood in an fp32 of that magnitude, which
                      adds its spacing, 2.4e-7 |ll64| (tests/test_engine_gpu.py)
  log alpha, log beta the tolerances of tests/logab_sweep.py (close(), and 1e-6 |ll64| + 2e-4 on forward's loglik)
  posterior_decode    label and conf bit for bit the lowest-index maximum of the rows of posterior's own output
  guard bands         no byte outside an output or workspace window changed, inputs included; every output written

The fp64 references are computed once per (model, L); test_references_agree holds the two oracles against each other
on exactly these inputs without a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import memory_contract as mc
from hmm_layer_amd import engine
from oracle import params, textbook
from oracle import build as obuild

DEV = "cuda:0"
B = 3
QS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16)
MODELS = ["d%d" % q for q in QS] + ["g15", "g7"]
SHAPES = [(1, 64), (17, 64), (1007, 64), (1007, 0)]            # (L, OPT_CHUNK; 0: the plan's own chunk length)


@functools.lru_cache(maxsize=None)
def model(name):
    """-> A (q,q), pi (q) float32.  dQ: dense random; g15 / g7: the gene models."""
    q = int(name[1:])
    rng = np.random.default_rng(9100 + q)
    pi = rng.random(q).astype(np.float32) + 0.1
    pi /= pi.sum()
    if name == "g15":
        return params.intended_A15().numpy().astype(np.float32), pi
    if name == "g7":
        ed = params.edges_simple()
        lg = params.init_logits(ed, 1)
        return params.dense_A(ed, np.where(lg == 0, 1e-30, lg), 7).numpy().astype(np.float32), pi
    A = rng.random((q, q)).astype(np.float32) + 0.02
    return A / A.sum(-1, keepdims=True), pi


@functools.lru_cache(maxsize=None)
def reference(name, L):
    """-> E (B,L,q) fp32 = 0.05 + 0.9 u, and the fp64 references (read only: shared between the cases)."""
    A, pi = model(name)
    q = A.shape[0]
    E = (np.random.default_rng(9200 + 31 * q + L).random((B, L, q)) * 0.9 + 0.05).astype(np.float32)
    g64, ll64 = obuild.posterior(A, pi, E)
    la64, llf64 = textbook.log_alpha(A, pi, E)
    lb64 = textbook.log_beta(A, E)
    for x in (E, g64, ll64, la64, llf64, lb64):
        x.setflags(write=False)
    return E, g64, ll64, la64, llf64, lb64


@pytest.mark.parametrize("L", sorted({L for L, _ in SHAPES}))
@pytest.mark.parametrize("name", MODELS)
def test_references_agree(name, L):
    """The oracle alone: oracle.build.posterior (C) and oracle.textbook (numpy) on these inputs agree to a thousandth
    of the gates, the posteriors are distributions and the log references are finite."""
    A, pi = model(name)
    assert np.abs(A.sum(-1) - 1).max() <= 1e-6 and abs(pi.sum() - 1) <= 1e-6 and (A >= 0).all()
    E, g64, ll64, la64, llf64, lb64 = reference(name, L)
    assert E.min() >= 0.05 and E.max() <= 0.95
    g, ll = textbook.posterior(A, pi, E)
    assert np.isfinite(g64).all() and np.isfinite(ll64).all() and np.isfinite(la64).all() and np.isfinite(lb64).all()
    assert np.abs(g64.sum(-1) - 1).max() <= 1e-9
    assert np.abs(g - g64).max() <= 2e-8
    assert np.abs(ll - ll64).max() <= 1e-9 * np.abs(ll64).max()
    assert np.abs(llf64 - ll64).max() <= 1e-9 * np.abs(ll64).max()


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.mark.gpu
@pytest.mark.parametrize("L,chunk", SHAPES, ids=["L%d-chunk%d" % s for s in SHAPES])
@pytest.mark.parametrize("name", MODELS)
def test_staged_outputs(name, L, chunk):
    from logab_sweep import close
    A, pi = model(name)
    q = A.shape[0]
    E, g64, ll64, la64, llf64, lb64 = reference(name, L)
    dims = (1, B, L, q)
    lib = engine.lib()
    arena = mc.Arena(DEV, margin_bytes=mc.SMALL_MARGIN)
    F64, U8 = torch.float64, torch.uint8
    args = [mc.Arg("A", "inp", _t(A[None])), mc.Arg("pi", "inp", _t(pi[None])), mc.Arg("E", "inp", _t(E[None]))]
    with engine.option(engine.OPT_CHUNK, chunk):               # (the size depends on the chunk length)
        for nm, op in (("ws_post", engine.OP_POSTERIOR), ("ws_fwd", engine.OP_FORWARD), ("ws_bwd", engine.OP_BACKWARD)):
            need = lib.hmm_workspace_bytes(op, *dims)
            assert need > 0
            args.append(mc.Arg(nm, "ws", nbytes=need))
    for nm in ("g0", "g1", "g2", "la", "lb"):
        args.append(mc.Arg(nm, "out", shape=dims))
    for nm in ("ll0", "ll1", "ll2", "llf", "lld"):
        args.append(mc.Arg(nm, "out", shape=dims[:2], dtype=F64))
    args += [mc.Arg("label", "out", shape=dims[:3], dtype=U8, shift=1031), mc.Arg("conf", "out", shape=dims[:3])]
    for a in args:
        arena.add(a)
    for s in arena.slots.values():
        if s.arg.kind == "inp":
            s.prepare(mc.IN_FILLS[0], None)
        elif s.arg.kind == "ws":
            s.prepare(mc.OUT_FILLS[0], "random")
        else:
            s.prepare(mc.BYTE_OUT_FILLS[0] if s.arg.itemsize == 1 else mc.OUT_FILLS[0], None)
    arena.sync()

    P, N = arena.ptr, arena.nbytes
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    eps = engine.EPS

    def ok(rc):
        assert rc == 0, lib.hmm_strerror(rc).decode()

    with engine.option(engine.OPT_CHUNK, chunk):
        for mode, g, ll in ((engine.POST_PROB, "g0", "ll0"), (engine.POST_LOG, "g1", "ll1"),
                            (engine.POST_LOG_NO_LL, "g2", "ll2")):
            ok(lib.hmm_posterior(P("A"), P("pi"), P("E"), *dims, eps, int(mode), P(g), P(ll), P("ws_post"),
                                 N("ws_post"), st))
        ok(lib.hmm_forward(P("A"), P("pi"), P("E"), *dims, eps, P("la"), P("llf"), P("ws_fwd"), N("ws_fwd"), st))
        ok(lib.hmm_backward(P("A"), P("E"), *dims, eps, P("lb"), P("ws_bwd"), N("ws_bwd"), st))
        ok(lib.hmm_posterior_decode(P("A"), P("pi"), P("E"), *dims, eps, None, q, P("label"), P("conf"), P("lld"),
                                    P("ws_post"), N("ws_post"), st))
    arena.check("the six calls")
    assert arena.strays == [], arena.strays

    tag = (name, L, chunk)
    out = {nm: arena.view(nm).clone() for nm in ("g0", "g1", "g2", "la", "lb", "ll0", "ll1", "ll2", "llf", "lld",
                                                  "label", "conf")}
    for nm, v in out.items():
        if v.dtype != U8:
            assert not torch.isnan(v).any(), (tag, nm, "unwritten or NaN")
    n = {nm: v.cpu().numpy()[0] for nm, v in out.items()}
    rel = lambda ll: float(np.abs((ll - ll64) / ll64).max())
    nsp = 2.4e-7 * float(np.abs(ll64).max())
    fig = dict(g0=float(np.abs(n["g0"] - g64).max()), g1=float(np.abs(np.exp(n["g1"]) - g64).max()),
               g2=float(np.abs(np.exp(n["g2"] - n["ll2"][:, None, None]) - g64).max()),
               ll0=rel(n["ll0"]), ll1=rel(n["ll1"]), ll2=rel(n["ll2"]), lld=rel(n["lld"]),
               la=close(n["la"], la64), lb=close(n["lb"], lb64),
               llf=float(np.max(np.abs(n["llf"] - llf64) - (1e-6 * np.abs(llf64) + 2e-4))))
    print("STAGING %s L=%d chunk=%d " % tag + " ".join("%s %.3g" % kv for kv in fig.items()))
    assert fig["g0"] <= 2e-5 and fig["g1"] <= 2e-5, (tag, fig)
    assert fig["g2"] <= 2e-5 + nsp, (tag, fig, nsp)
    for nm in ("ll0", "ll1", "ll2", "lld"):
        assert fig[nm] <= 1e-6, (tag, nm, fig)
    assert fig["la"] <= 0 and fig["lb"] <= 0 and fig["llf"] <= 0, (tag, fig)
    # the fused decode against the probability output it never writes: the lowest index on ties (torch.argmax)
    g0 = out["g0"]
    assert torch.equal(out["label"], g0.argmax(dim=-1).to(U8)), tag
    assert torch.equal(out["conf"].view(torch.int32), g0.max(dim=-1).values.view(torch.int32)), tag
