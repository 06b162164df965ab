"""Most probable state paths for an HmmCell's parameters (the reference only mentions Viterbi in a
docstring, hmm_layer/MsaHmmCell.py:13; learnMSA, which it ports, has a Viterbi module of this name).

``viterbi(inputs, cell)`` materialises log A, log pi and log E exactly as the layer does for the
forward-backward engine and makes one Viterbi call (include/hmm_engine.h): ``hmm_viterbi`` for up to 64
states — for 17 to 64 states (the two- to four-copy gene models) and the few long sequences where
``hmm_viterbi_scan_pays`` says so, the time-parallel ``hmm_viterbi_scan`` instead, with bit-identical
results —, ``hmm_viterbi_large`` above: every cell the layer serves, up to 4096 states (e.g. the many-copy
gene models and profile HMMs).

``viterbi_sharded(E_slab, cell, group)`` decodes sequences that are cut in TIME across the ranks of a process
group (hmm_layer_amd/seqshard.py: one chromosome-sized sequence on several GPUs), up to 64 states."""
import torch

from . import engine


def viterbi(inputs, cell, end_hints=None, training=False):
    """inputs (k, b, L, s) on a HIP device -> (path (k,b,L) int32, score (k,b) fp64).

    Emissions are clamped at the cell's epsilon before the log, like the forward recursion does
    (hmm_layer/MsaHmmCell.py:87); absent edges (A == 0) become -inf, which the engine treats as
    its "approximately log zero" (-1024)."""
    from .MsaHMMLayer import _engine_inputs
    A, pi, E = _engine_inputs(inputs, cell, end_hints, training)        # fused emitter when it qualifies
    with torch.no_grad():
        logE = torch.log(torch.clamp_min(E, cell.epsilon))
        del E
        logA = torch.log(A)
        logpi = torch.log(torch.clamp_min(pi, cell.epsilon))
    return engine.viterbi(logA.contiguous(), logpi.contiguous(), logE)


def viterbi_sharded(E_slab, cell, group=None):
    """This rank's time slab of emission PROBABILITIES E_slab (k, b, Ls, q) on a HIP device -> (path_slab (k,b,Ls)
    int32, score (k,b) fp64 of the whole sequences).

    Ranks of `group` hold consecutive slabs in rank order (rank 0 owns position 0; slab lengths may differ).  log A,
    log pi and log E are formed exactly as viterbi() forms them (emissions and pi clamped at the cell's epsilon before
    the log), so the ranks' paths put end to end and the score are viterbi()'s on the uncut sequences, bit for bit.
    The caller produces E_slab with whatever halo its emitter needs — the gene emitter's 3-mers read two neighbours
    on each side of a position —; nothing but the slab operators and maps is exchanged here (seqshard.viterbi)."""
    from . import seqshard
    cell.recurrent_init()
    with torch.no_grad():
        E = E_slab.detach().to(torch.float32)
        A = cell.A.detach().to(E.device, torch.float32)
        pi = cell.init_dist.detach().to(E.device, torch.float32).reshape(cell.num_models, cell.max_num_states)
        logE = torch.log(torch.clamp_min(E, cell.epsilon)).contiguous()
        logA = torch.log(A)
        logpi = torch.log(torch.clamp_min(pi, cell.epsilon))
    return seqshard.viterbi(logA.contiguous(), logpi.contiguous(), logE, group=group)
