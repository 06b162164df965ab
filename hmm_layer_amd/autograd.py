"""Differentiable log-likelihood: the engine's forward pass with the engine's analytic backward.

The reference trains by letting autograd unroll the Python time loop
(hmm_layer/BaseRNN.py:217-227 over HmmCell.forward, hmm_layer/MsaHmmCell.py:73-106), which keeps
every step's tensors alive.  Here the graph holds ONE node: forward = hmm_forward (log-likelihood
only, reads E once), backward = hmm_loglik_grad (hmm_loglik_grad_large above 64 states: one
forward-backward pass producing dA, dpi and dE = w * gamma / E).  Nothing per position is saved between the two.

posterior() is the same for a loss on the state posteriors (Posterior: hmm_posterior forward, hmm_posterior_grad /
hmm_posterior_grad_large backward).  For 65..256 states both have an opt-in node on the per-sequence walks with the
sparse step, whose gradient for A is defined on the support of A: loglik(support_only=...) -> SupportLogLikelihood
(hmm_loglik_grad_walk), posterior(support_only=...) -> SupportPosterior (hmm_posterior_walk forward,
hmm_posterior_grad_walk backward).  class_posterior() is posterior() summed over the states of each class of a class
table, as a model labelled by class is trained: composed from posterior() with torch ops, or, opt-in for 65..256
states, the node ClassPosterior (hmm_class_posterior_walk forward, hmm_class_posterior_grad_walk backward), between
which nothing of size (k,b,L,q) but E is kept.
"""
import torch

from . import engine


class LogLikelihood(torch.autograd.Function):
    """loglik (k,b) fp64 = f(A (k,q,q), pi (k,q), E (k,b,L,q)); all on one HIP device, fp32."""

    @staticmethod
    def forward(ctx, A, pi, E, eps):
        A, pi, E = A.contiguous(), pi.contiguous(), E.contiguous()
        ctx.save_for_backward(A, pi, E)
        ctx.eps = eps
        return engine.forward(A, pi, E, want_log_alpha=False, eps=eps)[1]

    @staticmethod
    def backward(ctx, grad_loglik):
        A, pi, E = ctx.saved_tensors
        grad = engine.loglik_grad if A.shape[-1] <= engine.lib().hmm_grad_max_states() else engine.loglik_grad_large
        dA, dpi, dE, _ = grad(A, pi, E, grad_loglik.to(torch.float32).contiguous(), eps=ctx.eps)
        need = ctx.needs_input_grad
        return (dA if need[0] else None, dpi.reshape(pi.shape) if need[1] else None,
                dE if need[2] else None, None)


class SupportLogLikelihood(torch.autograd.Function):
    """LogLikelihood for 65..256 states through the per-sequence walk with the sparse step (hmm_loglik_grad_walk):
    forward = its log-likelihood form, which checks once that no model was refused; backward = the walk on the same A.
    The gradient for A is exactly 0 wherever A == 0 and LogLikelihood's elsewhere."""

    @staticmethod
    def forward(ctx, A, pi, E, eps):
        A, pi, E = A.contiguous(), pi.contiguous(), E.contiguous()
        ctx.save_for_backward(A, pi, E)
        ctx.eps = eps
        return engine.loglik_grad_walk(A, pi, E, eps=eps, want_grads=False, check=True)[3]

    @staticmethod
    def backward(ctx, grad_loglik):
        A, pi, E = ctx.saved_tensors
        dA, dpi, dE, _ = engine.loglik_grad_walk(A, pi, E, grad_loglik.to(torch.float32).contiguous(), eps=ctx.eps,
                                                 check=False)
        need = ctx.needs_input_grad
        return (dA if need[0] else None, dpi.reshape(pi.shape) if need[1] else None,
                dE if need[2] else None, None)


def loglik(A, pi, E, eps=engine.EPS, support_only=False):
    """Differentiable (k,b) fp64 log-likelihoods.  support_only: False, today's path; True, for 65..256 states where
    hmm_loglik_grad_walk_pays says 1, the walk with the sparse step, whose gradient for A is exactly 0 wherever
    A == 0 (sound where A is scattered from per-edge parameters, as the gene transitioners do; not what a leaf A
    holding exact zeros gets from the default); "always", the same without asking the predicate.  Ignored outside
    65..256 states."""
    if support_only not in (False, True, "always"):
        raise ValueError("support_only must be False, True or \"always\", got %r" % (support_only,))
    if support_only:
        L = engine.lib()
        q = E.shape[-1]
        if L.hmm_loglik_grad_walk_min_states() <= q <= L.hmm_loglik_grad_walk_max_states() and (
                support_only == "always" or L.hmm_loglik_grad_walk_pays(*E.shape) == 1):
            return SupportLogLikelihood.apply(A, pi, E, eps)
    return LogLikelihood.apply(A, pi, E, eps)


class Posterior(torch.autograd.Function):
    """State posteriors (k,b,L,q), probabilities or logs, differentiable in A, pi and E.  Forward =
    hmm_posterior (the chunked kernels), backward = hmm_posterior_grad (its four sweeps per chunk of the
    scan plan, or over whole sequences where the device-side routing says so — 17..64 states per chunk through
    hmm_posterior_grad_scan where its predicate says it pays; hmm_posterior_grad_large above
    64 states) — the reference gets this gradient by autograd through its forward and backward loops
    (hmm_layer/MsaHMMLayer.py:422-521 with training=True)."""

    @staticmethod
    def forward(ctx, A, pi, E, mode, eps):
        A, pi, E = A.contiguous(), pi.contiguous(), E.contiguous()
        ctx.save_for_backward(A, pi, E)
        ctx.mode, ctx.eps = int(mode), eps
        return engine.posterior(A, pi, E, mode=mode, eps=eps)[0]

    @staticmethod
    def backward(ctx, grad_out):
        A, pi, E = ctx.saved_tensors
        grad_out = grad_out.to(torch.float32).contiguous()
        small = A.shape[-1] <= engine.lib().hmm_posterior_grad_max_states()
        post = engine.posterior_grad if small else engine.posterior_grad_large
        if ctx.mode == engine.POST_LOG_NO_LL:
            # out = log gamma + loglik (the reference's no_loglik=True): the log-posterior gradient plus the
            # log-likelihood gradient weighted by the per-sequence sum of the upstream gradient
            dA, dpi, dE = post(A, pi, E, grad_out, mode=engine.POST_LOG, eps=ctx.eps)
            w = grad_out.sum(dim=(2, 3)).contiguous()
            dA2, dpi2, dE2, _ = (engine.loglik_grad if small else engine.loglik_grad_large)(A, pi, E, w, eps=ctx.eps)
            dA, dpi, dE = dA + dA2, dpi + dpi2, dE.add_(dE2)
        else:
            dA, dpi, dE = post(A, pi, E, grad_out, mode=ctx.mode, eps=ctx.eps)
        need = ctx.needs_input_grad
        return (dA if need[0] else None, dpi.reshape(pi.shape) if need[1] else None, dE if need[2] else None, None, None)


class SupportPosterior(torch.autograd.Function):
    """Posterior for 65..256 states through the per-sequence walks with the sparse step: forward =
    hmm_posterior_walk (the walk, not hmm_posterior's per-position GEMMs: the two agree to rounding order only),
    backward = hmm_posterior_grad_walk, which checks that no model was refused.  POST_LOG_NO_LL adds
    hmm_loglik_grad_walk weighted by the per-sequence sum of the upstream gradient, as Posterior composes it.  The
    gradient for A is exactly 0 wherever A == 0 and Posterior's elsewhere."""

    @staticmethod
    def forward(ctx, A, pi, E, mode, eps):
        A, pi, E = A.contiguous(), pi.contiguous(), E.contiguous()
        ctx.save_for_backward(A, pi, E)
        ctx.mode, ctx.eps = int(mode), eps
        return engine.posterior_walk(A, pi, E, mode=mode, eps=eps)[0]

    @staticmethod
    def backward(ctx, grad_out):
        A, pi, E = ctx.saved_tensors
        grad_out = grad_out.to(torch.float32).contiguous()
        if ctx.mode == engine.POST_LOG_NO_LL:
            dA, dpi, dE = engine.posterior_grad_walk(A, pi, E, grad_out, mode=engine.POST_LOG, eps=ctx.eps, check=True)
            w = grad_out.sum(dim=(2, 3)).contiguous()
            dA2, dpi2, dE2, _ = engine.loglik_grad_walk(A, pi, E, w, eps=ctx.eps, check=False)
            dA, dpi, dE = dA + dA2, dpi + dpi2, dE.add_(dE2)
        else:
            dA, dpi, dE = engine.posterior_grad_walk(A, pi, E, grad_out, mode=ctx.mode, eps=ctx.eps, check=True)
        need = ctx.needs_input_grad
        return (dA if need[0] else None, dpi.reshape(pi.shape) if need[1] else None, dE if need[2] else None, None, None)


def posterior(A, pi, E, mode=engine.POST_LOG, eps=engine.EPS, support_only=False):
    """Differentiable state posteriors; mode engine.POST_PROB, POST_LOG or POST_LOG_NO_LL.  support_only has the
    meaning it has in loglik(): False, today's path; True, for 65..256 states where hmm_posterior_grad_walk_pays says
    1, the walks with the sparse step (SupportPosterior), whose gradient for A is exactly 0 wherever A == 0; "always",
    the same without asking the predicate.  Ignored outside 65..256 states."""
    if support_only not in (False, True, "always"):
        raise ValueError("support_only must be False, True or \"always\", got %r" % (support_only,))
    if support_only:
        L = engine.lib()
        q = E.shape[-1]
        if L.hmm_posterior_grad_walk_min_states() <= q <= L.hmm_posterior_grad_walk_max_states() and (
                support_only == "always" or L.hmm_posterior_grad_walk_pays(*E.shape) == 1):
            return SupportPosterior.apply(A, pi, E, mode, eps)
    return Posterior.apply(A, pi, E, mode, eps)


class ClassPosterior(torch.autograd.Function):
    """Class posteriors (k,b,L,C) of 65..256-state models, probabilities or logs, differentiable in A, pi and E
    through the per-sequence walks: forward = hmm_class_posterior_walk, backward = hmm_class_posterior_grad_walk,
    which checks that no model was refused.  Saved between the two: A, pi, E and the (k,b,L,C) probabilities; neither
    the state posteriors nor a gradient of their size exist.  The gradient for A is exactly 0 wherever A == 0."""

    @staticmethod
    def forward(ctx, A, pi, E, table, C, mode, eps):
        A, pi, E = A.contiguous(), pi.contiguous(), E.contiguous()
        log = int(mode) == engine.POST_LOG
        prob, logp, _ = engine.class_posterior_walk(A, pi, E, table, C, eps=eps, prob=True, log=log)
        ctx.save_for_backward(A, pi, E, prob)
        ctx.table, ctx.C, ctx.mode, ctx.eps = table, C, int(mode), eps
        return logp if log else prob

    @staticmethod
    def backward(ctx, grad_out):
        A, pi, E, prob = ctx.saved_tensors
        dA, dpi, dE = engine.class_posterior_grad_walk(A, pi, E, ctx.table, ctx.C, grad_out.to(torch.float32).contiguous(),
                                                       class_prob=prob, mode=ctx.mode, eps=ctx.eps, check=True)
        need = ctx.needs_input_grad
        return (dA if need[0] else None, dpi.reshape(pi.shape) if need[1] else None, dE if need[2] else None,
                None, None, None, None)


class ClassPosteriorSmall(torch.autograd.Function):
    """Class posteriors (k,b,L,C) of models of up to 16 states, probabilities or logs, differentiable in A, pi and E:
    forward = hmm_class_posterior (the chunked pipeline of posterior() with the class sums as its output), backward =
    hmm_class_posterior_grad (posterior_grad's sweeps reading the upstream gradient per class).  Saved between the two:
    A, pi, E and the (k,b,L,C) probabilities; neither the state posteriors nor a gradient of their size exist."""

    @staticmethod
    def forward(ctx, A, pi, E, table, C, mode, eps):
        A, pi, E = A.contiguous(), pi.contiguous(), E.contiguous()
        log = int(mode) == engine.POST_LOG
        prob, logp, _ = engine.class_posterior(A, pi, E, table, C, eps=eps, prob=True, log=log)
        ctx.save_for_backward(A, pi, E, prob)
        ctx.table, ctx.C, ctx.mode, ctx.eps = table, C, int(mode), eps
        return logp if log else prob

    @staticmethod
    def backward(ctx, grad_out):
        A, pi, E, prob = ctx.saved_tensors
        dA, dpi, dE = engine.class_posterior_grad(A, pi, E, ctx.table, ctx.C, grad_out.to(torch.float32).contiguous(),
                                                  class_prob=prob, mode=ctx.mode, eps=ctx.eps)
        need = ctx.needs_input_grad
        return (dA if need[0] else None, dpi.reshape(pi.shape) if need[1] else None, dE if need[2] else None,
                None, None, None, None)


def class_posterior(A, pi, E, state_class, num_classes=None, mode=engine.POST_LOG, eps=engine.EPS, support_only=False,
                    fused=None):
    """Differentiable class posteriors (k,b,L,C): P_c[t] = the sum of the state posteriors of the states that
    `state_class` maps to class c (mode engine.POST_PROB), or log P (POST_LOG; -inf where P is 0).  For 65..256 states
    and at most 16 classes, support_only="always", or True where hmm_class_posterior_walk_pays says 1, takes the fused
    node (ClassPosterior: nothing of size (k,b,L,q) but E and its gradient exists; the gradient for A is exactly 0
    wherever A == 0, as in posterior()).  For up to 16 states, at most 16 classes and E on a HIP device, `fused`
    chooses the fused node of that range (ClassPosteriorSmall: hmm_class_posterior + hmm_class_posterior_grad, nothing
    of size (k,b,L,q) but E and its gradient): None takes it where hmm_class_posterior_grad_pays says 1, True takes it
    without asking (ValueError outside the range or off the device), False never.  Everything else — 17..64 states,
    any other q the engine serves, more classes, a CPU tensor — composes posterior(POST_PROB,
    support_only=support_only) with engine.collapse_posterior (and log) in torch ops.
    On every route a class whose posterior is exactly 0 gives -inf in POST_LOG and passes no gradient."""
    if support_only not in (False, True, "always"):
        raise ValueError("support_only must be False, True or \"always\", got %r" % (support_only,))
    if int(mode) not in (engine.POST_PROB, engine.POST_LOG):
        raise ValueError("class_posterior supports mode POST_PROB or POST_LOG")
    q = E.shape[-1]
    if state_class is None:
        raise ValueError("class_posterior needs a class table (state_class)")
    table, C = engine.class_table(state_class, num_classes, q)
    if fused not in (None, True, False):
        raise ValueError("fused must be None, True or False, got %r" % (fused,))
    small = q <= engine.CLASS_MAX_STATES and C <= 16 and E.is_cuda
    if fused is True and not small:
        raise ValueError("class_posterior(fused=True) serves up to %d states and 16 classes on a HIP device, got q = %d, "
                         "C = %d on %s" % (engine.CLASS_MAX_STATES, q, C, E.device))
    if small and (fused is True or (fused is None and engine.lib().hmm_class_posterior_grad_pays(*E.shape) == 1)):
        return ClassPosteriorSmall.apply(A, pi, E, table, C, mode, eps)
    if support_only and C <= 16:
        L = engine.lib()
        if L.hmm_posterior_walk_min_states() <= q <= L.hmm_posterior_walk_max_states() and (
                support_only == "always" or L.hmm_class_posterior_walk_pays(*E.shape) == 1):
            return ClassPosterior.apply(A, pi, E, table, C, mode, eps)
    P = engine.collapse_posterior(posterior(A, pi, E, mode=engine.POST_PROB, eps=eps, support_only=support_only),
                                  table, C)
    if int(mode) != engine.POST_LOG:
        return P
    # as the node: -inf where a class posterior is exactly 0, and nothing passes through it (torch.log alone would hand
    # grad / 0 to the states of a non-empty class)
    on = P > 0
    return torch.where(on, torch.log(torch.where(on, P, torch.ones_like(P))), torch.full_like(P, float("-inf")))


class GeneEmissions(torch.autograd.Function):
    """E (b,L,q) = fused gene emitter of x (b,L,s+5) and B (rows,s) = softmax(emission_kernel) for one model.
    Forward = hmm_gene_emissions, backward = hmm_gene_emissions_grad, or their _wide forms above 64 states or 32
    kernel rows (engine.gene_emissions_routes_wide); only x, B and the small tables are saved
    (not E, and none of the reference's (b,L,64) 3-mer tensors, hmm_layer/gene_pred_hmm_emitter.py:231-277).
    The gradient of the five nucleotide columns of x is zero."""

    @staticmethod
    def forward(ctx, x, B, state_row, codon, state_codon, add, n_mass):
        x, B = x.contiguous(), B.contiguous()
        ctx.save_for_backward(x, B, state_row, codon, state_codon)
        ctx.add, ctx.n_mass = add, n_mass
        ctx.wide = bool(engine.gene_emissions_routes_wide(state_row.numel(), B.shape[0]))
        fwd = engine.gene_emissions_wide if ctx.wide else engine.gene_emissions
        return fwd(x, B, state_row, codon, state_codon, add=add, n_mass=n_mass)

    @staticmethod
    def backward(ctx, dE):
        x, B, state_row, codon, state_codon = ctx.saved_tensors
        need = ctx.needs_input_grad
        bwd = engine.gene_emissions_grad_wide if ctx.wide else engine.gene_emissions_grad
        dx, dB = bwd(x, B, state_row, codon, state_codon, dE.to(torch.float32).contiguous(),
                     add=ctx.add, n_mass=ctx.n_mass, want_dx=need[0], want_dB=need[1])
        return dx, dB, None, None, None, None, None


def gene_emissions(x, B, state_row, codon, state_codon, add=0.0, n_mass=1):
    """Differentiable fused emitter: E (b,L,q) with gradients for x's class columns and B."""
    return GeneEmissions.apply(x, B, state_row, codon, state_codon, add, n_mass)


class EmbeddingEmissions(torch.autograd.Function):
    """E_out (b,L,q) = E_in * (exp(inv_temperature * log N(x[..., col0:col0+d]; mean, 1/inv_std)) + add)[..., state_row]
    (E_in None: the factor alone).  Forward = hmm_embedding_emissions on a fresh output (E_in survives for the
    backward), backward = hmm_embedding_emissions_grad, or their _wide forms above 64 states or 32 kernel rows
    (engine.embedding_emissions_routes_wide).  Differentiable in E_in, x (embedding columns; every other
    column of its gradient is exactly 0), mean, inv_std and log_norm.  Saved: E_in, x, the three tables and
    state_row — not the factor, and nothing of size b L rows d."""

    @staticmethod
    def forward(ctx, E_in, x, mean, inv_std, log_norm, state_row, col0, d, inv_temperature, add):
        x, mean, inv_std, log_norm = x.contiguous(), mean.contiguous(), inv_std.contiguous(), log_norm.contiguous()
        if E_in is not None:
            E_in = E_in.contiguous()
        ctx.save_for_backward(E_in, x, mean, inv_std, log_norm, state_row)
        ctx.args = (int(col0), int(d), float(inv_temperature), float(add))
        ctx.wide = bool(engine.embedding_emissions_routes_wide(state_row.numel(), mean.shape[0]))
        fwd = engine.embedding_emissions_wide if ctx.wide else engine.embedding_emissions
        return fwd(x, col0, d, mean, inv_std, log_norm, state_row, E=None if E_in is None else E_in.clone(),
                   inv_temperature=inv_temperature, add=add)

    @staticmethod
    def backward(ctx, dE):
        E_in, x, mean, inv_std, log_norm, state_row = ctx.saved_tensors
        col0, d, inv_temperature, add = ctx.args
        need = ctx.needs_input_grad
        tables = any(need[2:5])
        bwd = engine.embedding_emissions_grad_wide if ctx.wide else engine.embedding_emissions_grad
        dE_in, dx, dmean, dinv_std, dlog_norm = bwd(
            x, col0, d, mean, inv_std, log_norm, state_row, dE.to(torch.float32).contiguous(), E_in=E_in,
            inv_temperature=inv_temperature, add=add, want_dE_in=need[0], want_demb=need[1], want_tables=tables,
            dx_out=torch.zeros_like(x) if need[1] else None)
        return (dE_in, dx, dmean if need[2] else None, dinv_std if need[3] else None,
                dlog_norm if need[4] else None, None, None, None, None, None)


def embedding_emissions(E_in, x, mean, inv_std, log_norm, state_row, col0, d, inv_temperature=1.0, add=0.0):
    """Differentiable embedding-emission factor multiplied into E_in (b,L,q) (None: the factor alone)."""
    return EmbeddingEmissions.apply(E_in, x, mean, inv_std, log_norm, state_row, col0, d, inv_temperature, add)


class NucleotideEmissions(torch.autograd.Function):
    """E_out (b,L,q) = E_in * f, f[p][j] = sum_a (x[p][col0+a] + x[p][col0+4] / 4) P[state_nuc[j]][a] on the states
    with state_nuc[j] >= 0 and 1/4 on the others (E_in None: the factor alone).  Forward = hmm_nucleotide_emissions
    on a fresh output (E_in survives for the backward), backward = hmm_nucleotide_emissions_grad; one kernel pair
    serves every model of up to 256 states.  Differentiable in E_in and P; nucleotides are data, the gradient for x
    is None.  Saved: E_in, x, P and state_nuc — not the factor."""

    @staticmethod
    def forward(ctx, E_in, x, P, state_nuc, col0):
        x, P = x.contiguous(), P.contiguous()
        if E_in is not None:
            E_in = E_in.contiguous()
        ctx.save_for_backward(E_in, x, P, state_nuc)
        ctx.col0 = int(col0)
        return engine.nucleotide_emissions(x, col0, P, state_nuc, E=None if E_in is None else E_in.clone())

    @staticmethod
    def backward(ctx, dE):
        E_in, x, P, state_nuc = ctx.saved_tensors
        need = ctx.needs_input_grad
        dE_in, dP = engine.nucleotide_emissions_grad(x, ctx.col0, P, state_nuc, dE.to(torch.float32).contiguous(),
                                                     E_in=E_in, want_dE_in=need[0], want_dP=need[2])
        return dE_in, None, dP, None, None


def nucleotide_emissions(E_in, x, P, state_nuc, col0):
    """Differentiable trainable-nucleotide factor multiplied into E_in (b,L,q) (None: the factor alone)."""
    return NucleotideEmissions.apply(E_in, x, P, state_nuc, col0)
