"""hmm_posterior_grad_large: per-sequence walk (OPT_GLARGE = 1) against per-position GEMMs (= 2).

  python tools/experiments/pg_large_time.py [--prof]

Prints the milliseconds of one call (median of 3 after a warm-up), log mode, a standard-normal upstream gradient:
  * the crossover that sets the default route: walk against GEMMs at b = 1024, L = 200, q = 65 / 100 / 128 on the
    band model of lg_large_time.py;
  * the five-copy gene model (71 states) at b = 1024 x L = 1e4 under both evaluations, next to hmm_loglik_grad_large's
    walk in the same run;
  * the config-5 shape, q = 1027 x b = 1024: time per position from L = 6 and L = 38, next to hmm_posterior's;
  * a five-copy layer step through state_posterior_log_probs(training=True) (forward + backward, emitter included)
    with a cross-entropy loss at b = 32 x L = 9999.
--prof runs the five-copy and config-5 parts only (for rocprofv3 --kernel-trace --stats: tools/prof_one.sh)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lg_large_time import E_of, band, dev, gene5, grad_ms, timed  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from hmm_layer_amd import engine  # noqa: E402


def G_of(E):
    g = torch.Generator(device=dev).manual_seed(7)
    return torch.randn(E.shape, generator=g, device=dev)


def pgrad_ms(route, A, pi, E, G, reps=3):
    with engine.option(engine.OPT_GLARGE, route):
        return timed(lambda: engine.posterior_grad_large(A, pi, E, G, mode=engine.POST_LOG), reps)


def layer_step(b, L):
    from hmm_layer_amd.MsaHmmCell import HmmCell
    from hmm_layer_amd.MsaHMMLayer import MsaHmmLayer
    from hmm_layer_amd.gene_pred_hmm_emitter import GenePredHMMEmitter
    from hmm_layer_amd.gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner
    codons = dict(start_codons=[("ATG", 1.)], stop_codons=[("TAG", .34), ("TAA", .33), ("TGA", .33)],
                  intron_begin_pattern=[("NGT", .99), ("NGC", .005), ("NAT", .005)],
                  intron_end_pattern=[("AGN", .99), ("ACN", .01)])
    g = torch.Generator().manual_seed(1)
    cls = torch.softmax(2 * torch.randn((1, b, L, 15), generator=g), -1)
    nuc = torch.nn.functional.one_hot(torch.randint(0, 4, (1, b, L), generator=g), 5).float()
    x = torch.cat([cls, nuc], -1).to(dev)
    labels = torch.randint(0, 71, (1, b, L), generator=g).to(dev)
    em = GenePredHMMEmitter(**codons, num_copies=5)
    em.build((1, b, L, 15))
    tr = GenePredMultiHMMTransitioner(k=5, initial_exon_len=200, initial_intron_len=4500, initial_ir_len=10000)
    cell = HmmCell([71], 15, em, tr).to(dev)
    layer = MsaHmmLayer(cell, use_prior=False)
    layer.build(x.shape)

    def step():
        for p in cell.parameters():
            p.grad = None
        logp = layer.state_posterior_log_probs(x, training=True)
        (-logp.gather(-1, labels[..., None]).mean()).backward()
    return step


def main():
    prof = "--prof" in sys.argv
    if not prof:
        for q in (65, 100, 128):
            A, pi = band(q)
            E = E_of(1024, 200, q)
            G = G_of(E)
            print("crossover q=%d b=1024 L=200: walk %.2f ms  GEMMs %.2f ms" % (q, pgrad_ms(1, A, pi, E, G),
                                                                              pgrad_ms(2, A, pi, E, G)), flush=True)
            del E, G
    A, pi = gene5()
    E = E_of(1024, 10000, 71)
    G = G_of(E)
    tw, tg, tl = pgrad_ms(1, A, pi, E, G), pgrad_ms(2, A, pi, E, G, reps=1), grad_ms(1, A, pi, E)
    print("gene k=5 q=71 b=1024 L=1e4: walk %.2f ms  GEMMs %.2f ms  (GEMMs / walk %.1fx)  loglik_grad_large walk %.2f ms"
          " (%.2fx)" % (tw, tg, tg / tw, tl, tw / tl), flush=True)
    del E, G
    A, pi = band(1027)
    tp, tgr = {}, {}
    for L in (6, 38):
        E = E_of(1024, L, 1027)
        G = G_of(E)
        tp[L] = timed(lambda: engine.posterior(A, pi, E, mode=engine.POST_LOG))
        tgr[L] = pgrad_ms(0, A, pi, E, G)
        del E, G
    pp, pg = 1e3 * (tp[38] - tp[6]) / 32, 1e3 * (tgr[38] - tgr[6]) / 32
    print("config 5 q=1027 b=1024: posterior %.1f us, posterior gradient %.1f us per position (%.2fx)"
          % (pp, pg, pg / pp), flush=True)
    if prof:
        return
    step = layer_step(32, 9999)
    print("gene k=5 layer step through state_posterior_log_probs b=32 L=9999: %.2f ms" % timed(step), flush=True)


if __name__ == "__main__":
    main()
