"""Layer API: log-likelihoods, forward / backward variables and state posteriors of batches of
sequences under k HMMs (drop-in for the reference's hmm_layer/MsaHMMLayer.py).

Every recursion here runs in the HIP engine (hmm_layer_amd.engine -> include/hmm_engine.h):
the layer materialises A, pi and the emission tensor E once (as the reference does,
MsaHMMLayer.py:247-249, 446-452) and makes ONE engine call; the Python time loop, the flips,
stacks and the q x q per-position tensors of the chunked mode do not exist.  Tensors must live
on a HIP device — there is no CPU fallback (the step-at-a-time CPU path is BaseRNN + HmmCell).

Kept from the reference: ``MsaHmmLayer(cell, num_seqs, use_prior, sequence_weights,
parallel_factor)`` with ``build``, ``forward_recursion``, ``backward_recursion``,
``state_posterior_log_probs``, ``apply_sequence_weights``, ``compute_prior``, ``forward``,
``get_config`` / ``from_config``; and the module-level ``_forward_recursion_impl``,
``_backward_recursion_impl``, ``_state_posterior_log_probs_impl`` with their argument lists
(the rnn arguments are accepted and ignored; ``parallel_factor`` is accepted and need not
divide the length — the engine picks its own time chunking).

Training: ``MsaHmmLayer.forward`` is differentiable.  When autograd is recording and a cell
parameter (or the input) requires grad, A, pi and E are built by the cell's torch ops with their
graph and the log-likelihood is ONE autograd node (hmm_layer_amd.autograd.LogLikelihood) whose
backward is the engine's analytic gradient (hmm_loglik_grad) — instead of the reference's
autograd through the unrolled time loop.  ``state_posterior_log_probs`` is differentiable the same
way (hmm_posterior_grad; hmm_posterior_grad_large above 64 states), as training through the posteriors
needs, including the ``no_loglik`` variant; forward / backward variables return inference values.
"""
import torch
import torch.nn as nn

from . import autograd, distributed, engine
from .Bidirectional import Bidirectional
from .BaseRNN import BaseRNN
from .TotalProbabilityCell import TotalProbabilityCell
from .gene_pred_hmm_transitioner import GenePredMultiHMMTransitioner


def _engine_inputs(inputs, cell, end_hints, training):
    """cell parameters + raw inputs -> (A (k,q,q), pi (k,q), E (k,b,L,q)) on the inputs' device."""
    cell.recurrent_init()
    with torch.no_grad():
        em = cell.emitter[0] if len(cell.emitter) == 1 else None
        if em is not None and hasattr(em, "forward_fused") and em.can_fuse(inputs):
            E = em.forward_fused(inputs, end_hints=end_hints, training=training)      # HIP kernel
        else:
            E = cell.emission_probs(inputs, end_hints=end_hints, training=training)
        A = cell.A.detach().to(E.device, torch.float32)
        pi = cell.init_dist.detach().to(E.device, torch.float32).reshape(cell.num_models, cell.max_num_states)
    return A.contiguous(), pi.contiguous(), E.detach().to(torch.float32).contiguous()


def _with_prior(cell, result, return_prior):
    if not return_prior:
        return result
    extra = (cell.get_prior_log_density(), cell.get_aux_loss())
    return (*result, *extra) if isinstance(result, tuple) else (result, *extra)


def _forward_recursion_impl(inputs, cell, rnn=None, total_prob_rnn=None, end_hints=None, return_prior=False,
                            training=False, parallel_factor=1):
    """-> log alpha (k,b,L,q), loglik (k,b) [, prior, aux_loss]   (reference MsaHMMLayer.py:227-282)."""
    A, pi, E = _engine_inputs(inputs, cell, end_hints, training)
    log_alpha, loglik = engine.forward(A, pi, E, want_log_alpha=True, eps=cell.epsilon)
    return _with_prior(cell, (log_alpha, loglik.to(torch.float32)), return_prior)


def _backward_recursion_impl(inputs, cell, reverse_cell=None, rnn_backward=None, total_prob_rnn_rev=None,
                             end_hints=None, return_prior=False, training=False, parallel_factor=1):
    """-> log beta (k,b,L,q) [, prior, aux_loss]   (reference MsaHMMLayer.py:322-381)."""
    A, _, E = _engine_inputs(inputs, cell, end_hints, training)
    return _with_prior(cell, engine.backward(A, E, eps=cell.epsilon), return_prior)


def _state_posterior_log_probs_impl(inputs, cell, reverse_cell=None, bidirectional_rnn=None, total_prob_rnn=None,
                                    total_prob_rnn_rev=None, end_hints=None, return_prior=False, training=False,
                                    no_loglik=False, parallel_factor=1):
    """-> log P(state q at position i | inputs), (k,b,L,q) [, prior, aux_loss]
    (reference MsaHMMLayer.py:422-521); with no_loglik the normaliser is left in
    (log alpha + log beta)."""
    if _wants_grad(inputs, cell):
        # training through the posteriors, as the reference's own test does (training=True): one
        # autograd node, analytic backward (hmm_posterior_grad)
        A, pi, E = _graph_inputs(inputs, cell, end_hints, training, what="posterior")
        mode = engine.POST_LOG_NO_LL if no_loglik else engine.POST_LOG
        support = getattr(cell.transitioner, "support_grad", False)
        return _with_prior(cell, autograd.posterior(A, pi, E, mode=mode, eps=cell.epsilon, support_only=support),
                           return_prior)
    A, pi, E = _engine_inputs(inputs, cell, end_hints, training)
    mode = engine.POST_LOG_NO_LL if no_loglik else engine.POST_LOG
    post, _ = engine.posterior(A, pi, E, mode=mode, eps=cell.epsilon)
    return _with_prior(cell, post, return_prior)


def state_posterior_log_probs_sharded(E_slab, cell, group=None, no_loglik=False):
    """This rank's time slab of emission probabilities E_slab (k, b, Ls, q) on a HIP device -> (log posteriors of the
    slab (k,b,Ls,q) — with no_loglik the normaliser is left in, as in state_posterior_log_probs —, loglik (k,b) fp64
    of the WHOLE sequences).  The counterpart of Viterbi.viterbi_sharded for the posteriors, for models of up to 64
    states; inference only.

    Ranks of `group` hold consecutive slabs in rank order (rank 0 owns position 0; slab lengths may differ).  A and pi
    are taken from the cell exactly as state_posterior_log_probs takes them.  Sequences that the eps clamps decide
    (seqshard.posterior's needs_unsharded) are recomputed unsharded on rank 0 of the group and every rank gets its own
    slab of them back (seqshard.gather_flagged), so what is returned is final.  The caller produces E_slab with
    whatever halo its emitter needs; nothing but the slab operators, the certificates and the flagged sequences is
    exchanged here."""
    from . import seqshard
    if cell.epsilon != engine.EPS:
        raise ValueError("the sequence-sharded posterior runs with the engine's epsilon %g (cell: %g)"
                         % (engine.EPS, cell.epsilon))
    cell.recurrent_init()
    with torch.no_grad():
        E = E_slab.detach().to(torch.float32).contiguous()
        A = cell.A.detach().to(E.device, torch.float32).contiguous()
        pi = cell.init_dist.detach().to(E.device, torch.float32).reshape(cell.num_models, cell.max_num_states).contiguous()
        mode = engine.POST_LOG_NO_LL if no_loglik else engine.POST_LOG
        out, loglik, flagged = seqshard.posterior(A, pi, E, mode=mode, group=group)
        return seqshard.gather_flagged(A, pi, E, out, loglik, flagged, mode=mode, group=group)


def _posterior_probs_host(A, pi, E, eps):
    """State posteriors (k,b,L,q) fp32 and loglik (k,b) fp64 of tensors that are NOT on a HIP device: the cell's
    recursion (both clamps at eps, MsaHmmCell.py:87-88) one position at a time in fp64 torch ops.  It exists so that
    posterior_decode's semantics can be pinned without a GPU; nothing on a HIP device ever comes here."""
    A, pi, E = A.double(), pi.double(), E.double().clamp_min(eps)
    k, b, L, q = E.shape
    alpha = torch.empty_like(E)
    loglik = torch.zeros((k, b), dtype=torch.float64, device=E.device)
    x = pi.clamp_min(eps).unsqueeze(1).expand(k, b, q)
    for t in range(L):
        x = (x if t == 0 else torch.matmul(x, A).clamp_min(eps)) * E[:, :, t]
        s = x.sum(-1, keepdim=True)
        x = x / s
        alpha[:, :, t] = x
        loglik += torch.log(s[..., 0])
    gamma = torch.empty_like(E)
    r = torch.ones((k, b, q), dtype=torch.float64, device=E.device)
    for t in range(L - 1, -1, -1):
        g = alpha[:, :, t] * r
        gamma[:, :, t] = g / g.sum(-1, keepdim=True)
        bh = E[:, :, t] * r
        r = torch.matmul(bh / bh.sum(-1, keepdim=True), A.transpose(1, 2)).clamp_min(eps)
    return gamma.to(torch.float32), loglik


def _wants_grad(inputs, cell):
    if not torch.is_grad_enabled():
        return False
    if torch.is_tensor(inputs) and inputs.requires_grad:
        return True
    mods = [cell.transitioner, *cell.emitter]
    return any(p.requires_grad for m in mods if isinstance(m, nn.Module) for p in m.parameters())


def _graph_inputs(inputs, cell, end_hints, training, what="loglik"):
    """A, pi, E built by the cell's torch ops WITH their autograd graph (training)."""
    limit = (engine.lib().hmm_loglik_grad_large_max_states() if what == "loglik"
             else engine.lib().hmm_posterior_grad_large_max_states())
    if cell.max_num_states > limit:
        # fail before the forward pass, not in backward(): the log-likelihood and posterior gradients cover
        # q <= 4096 (hmm_loglik_grad_large, hmm_posterior_grad_large)
        raise ValueError("training through the HIP engine covers models of at most %d states (got %d); "
                         "wrap inference calls in torch.no_grad()" % (limit, cell.max_num_states))
    cell.recurrent_init()
    em = cell.emitter[0] if len(cell.emitter) == 1 else None
    if em is not None and getattr(em, "fused_training", False) and em.can_fuse(inputs):
        # HIP kernels forward and backward (autograd.GeneEmissions); input nucleotide columns get zero gradient
        E = em.forward_fused_trainable(inputs, end_hints=end_hints, training=training).to(torch.float32)
    else:
        E = cell.emission_probs(inputs, end_hints=end_hints, training=training).to(torch.float32)
    if not E.is_cuda:
        raise engine.EngineError("inputs must live on a HIP device (got %s); the engine has no CPU path" % E.device)
    A = cell.A.to(E.device, torch.float32)
    pi = cell.init_dist.to(E.device, torch.float32).reshape(cell.num_models, cell.max_num_states)
    return A, pi, E


def _loglik_impl(inputs, cell, end_hints=None, training=False):
    """loglik (k,b) fp64 only: reads E once, writes nothing per position.  Differentiable when
    autograd is recording and something upstream requires grad."""
    if not _wants_grad(inputs, cell):
        A, pi, E = _engine_inputs(inputs, cell, end_hints, training)
        return engine.forward(A, pi, E, want_log_alpha=False, eps=cell.epsilon)[1]
    A, pi, E = _graph_inputs(inputs, cell, end_hints, training)
    return autograd.loglik(A, pi, E, eps=cell.epsilon, support_only=getattr(cell.transitioner, "support_grad", False))


class MsaHmmLayer(nn.Module):
    def __init__(self, cell, num_seqs=None, use_prior=True, sequence_weights=None, parallel_factor=1):
        super().__init__()
        self.cell = cell
        self.num_seqs = num_seqs
        self.use_prior = use_prior
        self.parallel_factor = parallel_factor
        if sequence_weights is not None:
            w = torch.as_tensor(sequence_weights, dtype=torch.float32)
            self.register_buffer("sequence_weights", w)
            self.register_buffer("weight_sum", w.sum())
        else:
            self.sequence_weights = None
            self.weight_sum = None
        self.reverse_cell = None
        self.rnn = self.rnn_backward = self.bidirectional_rnn = None
        self.total_prob_rnn = self.total_prob_rnn_rev = None
        self.built = False

    def build(self, input_shape=None):
        """Creates the reverse cell and the plumbing-path layers (step-at-a-time drivers over the
        same cells; the engine path does not need them)."""
        if self.built:
            return
        self.reverse_cell = self.cell.make_reverse_direction_offspring()
        self.rnn = BaseRNN(self.cell, batch_first=True, return_sequences=True, return_state=True)
        self.rnn_backward = BaseRNN(self.reverse_cell, batch_first=True, return_sequences=True, return_state=True)
        self.bidirectional_rnn = Bidirectional(self.rnn, merge_mode="concat" if self.parallel_factor > 1 else "sum",
                                               backward_layer=self.rnn_backward)
        if self.parallel_factor > 1:
            self.total_prob_rnn = BaseRNN(TotalProbabilityCell(self.cell), batch_first=True,
                                          return_sequences=True, return_state=True)
            self.total_prob_rnn_rev = BaseRNN(TotalProbabilityCell(self.reverse_cell, reverse=True),
                                              batch_first=True, return_sequences=True, return_state=True,
                                              reverse=True)
        self.built = True

    # -- recursions (engine) --------------------------------------------------------------
    def forward_recursion(self, inputs, end_hints=None, return_prior=False, training=False):
        return _forward_recursion_impl(inputs, self.cell, self.rnn, self.total_prob_rnn, end_hints=end_hints,
                                       return_prior=return_prior, training=training,
                                       parallel_factor=self.parallel_factor)

    def backward_recursion(self, inputs, end_hints=None, return_prior=False, training=False):
        return _backward_recursion_impl(inputs, self.cell, self.reverse_cell, self.rnn_backward,
                                        self.total_prob_rnn_rev, end_hints=end_hints, return_prior=return_prior,
                                        training=training, parallel_factor=self.parallel_factor)

    def state_posterior_log_probs(self, inputs, end_hints=None, return_prior=False, training=False,
                                  no_loglik=False):
        return _state_posterior_log_probs_impl(inputs, self.cell, self.reverse_cell, self.bidirectional_rnn,
                                               self.total_prob_rnn, self.total_prob_rnn_rev, end_hints=end_hints,
                                               return_prior=return_prior, training=training, no_loglik=no_loglik,
                                               parallel_factor=self.parallel_factor)

    def state_posterior_probs(self, inputs, end_hints=None, training=False):
        """Posteriors as probabilities (rows sum to 1) and loglik (k,b) fp64: the engine's native
        output, without the exp/log round trip."""
        if _wants_grad(inputs, self.cell):                  # differentiable, like state_posterior_log_probs
            A, pi, E = _graph_inputs(inputs, self.cell, end_hints, training, what="posterior")
            probs = autograd.posterior(A, pi, E, mode=engine.POST_PROB, eps=self.cell.epsilon,
                                       support_only=getattr(self.cell.transitioner, "support_grad", False))
            return probs, autograd.loglik(A, pi, E, eps=self.cell.epsilon)
        A, pi, E = _engine_inputs(inputs, self.cell, end_hints, training)
        return engine.posterior(A, pi, E, mode=engine.POST_PROB, eps=self.cell.epsilon)

    def posterior_decode(self, inputs, state_class=None, num_classes=None, end_hints=None):
        """Posterior decoding -> (label (k,b,L) uint8, conf (k,b,L) fp32, loglik (k,b) fp64): per position the class
        with the largest posterior and that posterior.  state_class maps every state to a class (a sequence or an
        integer tensor; None: every state its own class); a class posterior is the sum over its states, ties go to
        the lowest class.  On a HIP device one engine call (engine.posterior_decode: the (k,b,L,q) posterior is never
        written for models of up to 64 states with the identity map or at most 16 classes — the multi-copy gene
        models of 29 / 43 / 57 states included —, nor for 65..256 states where the per-sequence walk measured
        faster (hmm_posterior_decode_wide; above 128 states only for a GenePredMultiHMMTransitioner, whose A takes the
        walk's sparse step); other models compose the posterior with torch ops); elsewhere the same reduction of a
        step-at-a-time posterior.  Inference only."""
        if _wants_grad(inputs, self.cell):
            raise ValueError("posterior_decode is inference only (labels carry no gradient): call it under "
                             "torch.no_grad(), or train through class_posterior_log_probs / "
                             "state_posterior_log_probs")
        A, pi, E = _engine_inputs(inputs, self.cell, end_hints, False)
        if E.is_cuda:
            sparse = isinstance(self.cell.transitioner, GenePredMultiHMMTransitioner)
            return engine.posterior_decode(A, pi, E, state_class, num_classes, eps=self.cell.epsilon, sparse=sparse)
        table, C = engine.class_table(state_class, num_classes, E.shape[-1])
        gamma, loglik = _posterior_probs_host(A, pi, E, self.cell.epsilon)
        return (*engine.decode_posterior(gamma, table, C), loglik)

    def class_posterior_log_probs(self, inputs, state_class, num_classes=None, end_hints=None, training=False,
                                  log=True):
        """Class posteriors (k,b,L,C): per position the sum of the state posteriors of every class of `state_class` (a
        sequence or an integer tensor of q classes), as logs (log=True; -inf for a class of posterior 0) or
        probabilities — what a model labelled by class is trained on; the trainable counterpart of posterior_decode.
        With gradients wanted: autograd.class_posterior, which takes one fused autograd node (neither the (k,b,L,q)
        posterior nor a gradient of that size is written) for up to 16 states and at most 16 classes where
        hmm_class_posterior_grad_pays says 1, and on the per-sequence walks for 65..256 states and at most 16 classes
        where the transitioner's support_grad asks for them; else state posteriors collapsed by torch ops.  Without
        gradients on a HIP device: for up to 16 states and at most 16 classes the fused forward
        (engine.class_posterior) where hmm_class_posterior_pays says 1; for 65..256 states the fused forward where
        posterior_decode would take its fused call for this model (hmm_posterior_walk_pays, and above 128 states only a
        GenePredMultiHMMTransitioner); else engine.posterior collapsed.  Elsewhere a step-at-a-time posterior
        collapsed."""
        mode = engine.POST_LOG if log else engine.POST_PROB
        if state_class is None:
            raise ValueError("class_posterior_log_probs needs a class table (state_class)")
        if _wants_grad(inputs, self.cell):
            A, pi, E = _graph_inputs(inputs, self.cell, end_hints, training, what="posterior")
            return autograd.class_posterior(A, pi, E, state_class, num_classes, mode=mode, eps=self.cell.epsilon,
                                            support_only=getattr(self.cell.transitioner, "support_grad", False))
        A, pi, E = _engine_inputs(inputs, self.cell, end_hints, training)
        q = E.shape[-1]
        table, C = engine.class_table(state_class, num_classes, q)
        if E.is_cuda:
            lib = engine.lib()
            if C <= 16 and q <= engine.CLASS_MAX_STATES and lib.hmm_class_posterior_pays(*E.shape) == 1:
                prob, logp, _ = engine.class_posterior(A, pi, E, table, C, eps=self.cell.epsilon, prob=not log, log=log)
                return logp if log else prob
            if (C <= 16 and lib.hmm_posterior_walk_min_states() <= q <= lib.hmm_posterior_walk_max_states()
                    and lib.hmm_posterior_walk_pays(*E.shape) == 1
                    and (q <= 128 or isinstance(self.cell.transitioner, GenePredMultiHMMTransitioner))):
                prob, logp, _ = engine.class_posterior_walk(A, pi, E, table, C, eps=self.cell.epsilon, prob=not log,
                                                            log=log)
                return logp if log else prob
            gamma = engine.posterior(A, pi, E, mode=engine.POST_PROB, eps=self.cell.epsilon)[0]
        else:
            gamma = _posterior_probs_host(A, pi, E, self.cell.epsilon)[0]
        P = engine.collapse_posterior(gamma, table, C)
        return torch.log(P) if log else P

    # -- likelihood aggregation -----------------------------------------------------------
    def apply_sequence_weights(self, loglik, indices, aggregate=False):
        """Weights per sequence; aggregate=True: weighted mean over the batch, then mean over
        models.  Under torch.distributed the means run over ALL ranks' sequences via one
        all-reduce of (sum w*loglik, sum w) per model."""
        weights = None
        if self.sequence_weights is not None:
            weights = self.sequence_weights.to(loglik.device)[indices]
            if not aggregate:
                return loglik * weights
        if not aggregate:
            return loglik
        return distributed.aggregate_loglik(loglik, weights).to(torch.float32)

    def compute_prior(self, scaled=True):
        self.cell.recurrent_init()
        prior = self.cell.get_prior_log_density()
        return self._scale_prior(prior) if scaled else prior

    def _scale_prior(self, prior):
        if self.sequence_weights is not None:
            return prior / self.weight_sum.to(prior.device) if torch.is_tensor(prior) else prior / self.weight_sum
        if self.num_seqs is not None:
            return prior / self.num_seqs
        return prior

    def forward(self, inputs, indices=None, training=False):
        """-> loglik (k,b), aggregated loglik (), [prior (k), aux_loss ()]."""
        inputs = inputs.to(torch.float32)
        loglik64 = _loglik_impl(inputs, self.cell, training=training)
        loglik_mean = torch.squeeze(self.apply_sequence_weights(loglik64, indices, aggregate=True))
        loglik = loglik64.to(torch.float32)
        if self.use_prior:
            prior = self._scale_prior(self.cell.get_prior_log_density())
            return loglik, loglik_mean, prior, self.cell.get_aux_loss()
        return loglik, loglik_mean

    def get_config(self):
        return {"cell": self.cell, "num_seqs": self.num_seqs, "use_prior": self.use_prior,
                "sequence_weights": None if self.sequence_weights is None else self.sequence_weights.cpu().numpy(),
                "parallel_factor": self.parallel_factor}

    @classmethod
    def from_config(cls, config):
        return cls(**config)
