"""Emission-probability producers of the gene-prediction HMMs (drop-in for the reference's
hmm_layer/gene_pred_hmm_emitter.py): class predictions (and optionally nucleotides) in,
E (k, b, L, q) probabilities out — the tensor the HIP engine consumes.

Interface kept (gene_pred_hmm_emitter.py:61-128, 231-277): ``build(input_shape)``,
``recurrent_init()``, ``make_B()``, ``forward(inputs, end_hints=None, training=False)``,
``get_prior_log_density()``, ``get_aux_loss()``, ``get_config()/from_config()``, parameter
``emission_kernel`` (k, rows, s).

Differences, on purpose: everything is created on / follows the parameters' device; the k-mer
helper does not mutate its input (defect D5 — ``n_mass_compat=True`` reproduces the as-shipped
doubling of N mass in the right-pivot 3-mers).

Embedding emissions (``emit_embeddings=True``, inputs (k, b, L, s + d [+ 5])): one model, diagonal
covariance, one mixture component — the reference's MvnMixture(diag_only=True) with
DefaultDiagBijector(initial_variance), written out in torch ops here (``embedding_log_pdf``) and fused
for inference (``forward_fused``: hmm_gene_emissions, then hmm_embedding_emissions multiplying into E
with the embedding columns read in place) and for training with ``fused_training=True``
(``forward_fused_trainable``: autograd.EmbeddingEmissions, backward hmm_embedding_emissions_grad).
``full_covariance=True`` raises NotImplementedError.

Which kernels serve a model (``GenePredHMMEmitter.fused_routes``): up to 64 states and 32 kernel rows (one and two
copies) hmm_gene_emissions / hmm_gene_emissions_grad; above that, up to 256 states (three to eighteen copies, shared
introns or not), hmm_gene_emissions_wide / hmm_gene_emissions_grad_wide; above 256 states ``forward()`` in torch ops.
With ``emit_embeddings=True`` the embedding factor follows the same borders: hmm_embedding_emissions /
hmm_embedding_emissions_grad up to 64 states and 32 rows, hmm_embedding_emissions_wide /
hmm_embedding_emissions_grad_wide up to 256 states and rows (three to eighteen copies), ``forward()`` above.
With ``trainable_nucleotides_at_exons=True`` one more factor follows on every route: hmm_nucleotide_emissions multiplies
the learned nucleotide distribution of the exon states into E (``forward_fused``), reading the five nucleotide columns
in place; with ``fused_training=True`` it is one more node (autograd.NucleotideEmissions, backward
hmm_nucleotide_emissions_grad), through which ``nuc_emission_kernel`` trains.  One kernel pair serves every model of
up to 256 states.
Four more differences from the as-shipped reference, on purpose:
  * with ``trainable_nucleotides_at_exons=True`` the reference reads ``inputs[..., -5:]`` after ``inputs`` has already
    lost its nucleotide columns (gene_pred_hmm_emitter.py:265-266), so its nucleotide factor is computed from the last
    five class (or embedding) columns.  Here the factor is computed from the nucleotides, the intended meaning:
    acgt = nuc[..., :4] + nuc[..., 4:] / 4, f = acgt . softmax(nuc_emission_kernel) on E0/E1/E2 of every copy and 1/4
    elsewhere.  There is therefore no fixture from the reference for this factor; the tests go by an fp64 restatement.
  * MvnMixture.__init__ copies the parameter with ``torch.tensor(kernel)`` (MvnMixture.py:40), so the
    reference never trains ``embedding_emission_kernel``; here the graph is kept and mu / sigma receive
    gradients.
  * the reference's class_emit einsum omits ``inputs[0]`` with embeddings on
    (gene_pred_hmm_emitter.py:104) and returns an extra leading axis; here the result is (k, b, L, q)
    like every other emitter output.
  * as shipped, MvnMixture.component_log_pdf adds log_det (k1, 1, k2, c) to the transposed distances
    (k1, batch, c, k2) (MvnMixture.py:138-148): with one component this broadcasts to (k1, batch, k2, k2) and
    log_pdf's ``[..., 0]`` gives every row the distance to row 0's mean.  Here row r gets its own distance
    (the diagonal of that tensor); tests/golden/mvn_diag.npz records both.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kmer


class SimpleGenePredHMMEmitter(nn.Module):
    """Class-probability emissions for the 1 + 6*copies state model (Ir, I0-2, E0-2)."""

    def __init__(self, num_models=1, num_copies=1, init=0.0, trainable_emissions=True, emit_embeddings=False,
                 embedding_dim=None, full_covariance=False, embedding_kernel_init="random_normal",
                 initial_variance=1.0, temperature=1.0, share_intron_parameters=True, **kwargs):
        super().__init__(**kwargs)
        if emit_embeddings:
            if full_covariance:
                raise NotImplementedError("embedding emissions cover diagonal covariance only (full_covariance=False)")
            assert embedding_dim is not None and int(embedding_dim) >= 1, "emit_embeddings=True requires embedding_dim"
        else:
            assert embedding_dim is None, "embedding_dim requires emit_embeddings=True"
        self.num_models = num_models
        self.num_copies = num_copies
        self.num_states = 1 + 6 * num_copies
        self.init = init
        self.trainable_emissions = trainable_emissions
        self.emit_embeddings = bool(emit_embeddings)
        self.embedding_dim = int(embedding_dim) if emit_embeddings else None
        self.full_covariance = full_covariance
        self.embedding_kernel_init = embedding_kernel_init
        self.initial_variance = initial_variance
        self.temperature = temperature
        self.share_intron_parameters = share_intron_parameters
        self.emission_kernel = None
        self.embedding_emission_kernel = None
        self.B = None
        self.embedding_mu = self.embedding_sigma = None
        self.built = False

    def kernel_rows(self):
        return self.num_states - 2 * self.num_copies * int(self.share_intron_parameters)

    def build(self, input_shape):
        """input_shape[-1] = s, the number of classes (the embedding columns are not counted)."""
        if self.built:
            return
        s = input_shape[-1]
        if torch.is_tensor(self.init):
            start = self.init.detach().clone().to(torch.float32).reshape(self.num_models, self.kernel_rows(), s)
        else:
            start = torch.full((self.num_models, self.kernel_rows(), s), float(self.init))
        self.emission_kernel = nn.Parameter(start, requires_grad=self.trainable_emissions)
        if self.emit_embeddings:
            assert self.num_models == 1, "embedding emissions support one model"
            shape = (1, self.kernel_rows(), 1, 2 * self.embedding_dim)
            if torch.is_tensor(self.embedding_kernel_init):
                ker = self.embedding_kernel_init.detach().clone().to(torch.float32).reshape(shape)
            elif self.embedding_kernel_init == "random_normal":
                ker = torch.randn(shape)
            else:
                raise ValueError("embedding_kernel_init '%s' not supported" % (self.embedding_kernel_init,))
            self.embedding_emission_kernel = nn.Parameter(ker, requires_grad=True)
        self.built = True

    def recurrent_init(self):
        self.B = self.make_B()
        if self.emit_embeddings:
            self.embedding_mu, self.embedding_sigma = self.make_mvn()

    def make_B(self):
        return F.softmax(self.emission_kernel, dim=-1)

    def make_mvn(self, dtype=None):
        """(mu, sigma), (rows, d) each, with their graph: mu = ker[..., :d], sigma = softplus(ker[..., d:] +
        inverse_softplus(sqrt(initial_variance))) + 1e-5 + 1e-8 (Utility.py:31-42, MvnMixture.py:98-99)."""
        d = self.embedding_dim
        ker = self.embedding_emission_kernel[0, :, 0, :]
        if dtype is not None:
            ker = ker.to(dtype)
        shift = math.log(math.expm1(math.sqrt(float(self.initial_variance))))
        return ker[:, :d], F.softplus(ker[:, d:] + shift) + 1e-5 + 1e-8

    def embedding_log_pdf(self, emb):
        """(..., d) embeddings -> (..., rows) log densities (MvnMixture.component_log_pdf, diag_only)."""
        if self.embedding_mu is None:
            self.recurrent_init()
        mu, sigma = self.embedding_mu, self.embedding_sigma
        diff = emb.unsqueeze(-2) - mu
        md = torch.sum(torch.square(diff) * torch.square(1.0 / sigma), dim=-1)
        log_det = 2 * torch.sum(torch.log(sigma), dim=-1)
        return -0.5 * (self.embedding_dim * math.log(2 * math.pi) + log_det + md)

    def embedding_tables(self, device):
        """(mean, inv_std (rows, d), log_norm (rows)) fp32 for hmm_embedding_emissions: computed from the
        parameter in fp64 and rounded once."""
        with torch.no_grad():
            mu, sigma = self.make_mvn(torch.float64)
            log_norm = -0.5 * self.embedding_dim * math.log(2 * math.pi) - torch.sum(torch.log(sigma), dim=-1)
            return tuple(t.to(device, torch.float32).contiguous() for t in (mu, 1.0 / sigma, log_norm))

    def embedding_tables_with_graph(self, device):
        """embedding_tables with its autograd graph, for training through hmm_embedding_emissions_grad: the same
        fp64 chain from the parameter (softplus, reciprocal, log), cast to fp32 once.  The kernel's three table
        gradients flow back to embedding_emission_kernel through these (rows, d)-sized torch ops."""
        mu, sigma = self.make_mvn(torch.float64)
        log_norm = -0.5 * self.embedding_dim * math.log(2 * math.pi) - torch.sum(torch.log(sigma), dim=-1)
        return tuple(t.to(device, torch.float32).contiguous() for t in (mu, 1.0 / sigma, log_norm))

    def class_emissions(self, inputs, training=False):
        """(k, b, L, s) class probabilities [then d embedding columns] -> (k, b, L, q)."""
        if self.B is None or (self.emit_embeddings and self.embedding_mu is None):
            self.recurrent_init()
        if self.emit_embeddings:
            d = self.embedding_dim
            emit = torch.einsum("...s,kqs->k...q", inputs[0][..., :-d], self.B)
            factor = torch.exp(self.embedding_log_pdf(inputs[0][..., -d:]) / self.temperature).unsqueeze(0)
            if training:
                emit, factor = emit + 1e-10, factor + 1e-10
            emit = emit * factor
        else:
            emit = torch.einsum("...s,kqs->k...q", inputs[0], self.B)
        if self.share_intron_parameters:
            c = self.num_copies
            emit = torch.cat([emit[..., :1 + c], emit[..., 1:1 + c], emit[..., 1:1 + c], emit[..., 1 + c:]], dim=-1)
        return emit

    def apply_end_hints(self, emit, end_hints):
        if end_hints is None:
            return emit
        if emit.shape[-2] == 1:               # one position: it is the first and the last
            return end_hints[..., :1, :] * end_hints[..., 1:, :] * emit
        left = end_hints[..., :1, :] * emit[..., :1, :]
        right = end_hints[..., 1:, :] * emit[..., -1:, :]
        return torch.cat([left, emit[..., 1:-1, :], right], dim=-2)

    def forward(self, inputs, end_hints=None, training=False):
        return self.apply_end_hints(self.class_emissions(inputs, training=training), end_hints)

    def get_prior_log_density(self):
        dev = self.emission_kernel.device if self.emission_kernel is not None else None
        return torch.zeros((1, 1), device=dev)

    def get_aux_loss(self):
        return 0.0

    def get_config(self):
        return {"num_models": self.num_models, "num_copies": self.num_copies, "init": self.init,
                "trainable_emissions": self.trainable_emissions, "emit_embeddings": self.emit_embeddings,
                "embedding_dim": self.embedding_dim, "full_covariance": self.full_covariance,
                "embedding_kernel_init": self.embedding_kernel_init, "initial_variance": self.initial_variance,
                "temperature": self.temperature, "share_intron_parameters": self.share_intron_parameters}

    @classmethod
    def from_config(cls, config):
        return cls(**config)


def assert_codons(codons):
    assert sum(p for _, p in codons) == 1, "codon probabilities must sum to 1: %s" % (codons,)
    for triplet, prob in codons:
        assert len(triplet) == 3 and 0 <= prob <= 1, "bad codon entry: %s" % (codons,)


def make_codon_probs(codons, pivot_left):
    """[(triplet, prob)] -> (1, 1, 64) distribution over 3-mer classes."""
    assert_codons(codons)
    acc = sum(prob * kmer.encode_kmer_string(tri, pivot_left) for tri, prob in codons)
    return acc.reshape(1, 1, 64)


class GenePredHMMEmitter(SimpleGenePredHMMEmitter):
    """1 + 14*copies states: adds START, EI0-2, IE0-2, STOP and 3-mer (codon / splice-site)
    constraints on states E2 .. STOP (gene_pred_hmm_emitter.py:198-217)."""

    def __init__(self, start_codons, stop_codons, intron_begin_pattern, intron_end_pattern, l2_lambda=0.01,
                 nucleotide_kernel_init=None, trainable_nucleotides_at_exons=False, n_mass_compat=False,
                 fused_training=False, **kwargs):
        super().__init__(**kwargs)
        self.num_states = 1 + 14 * self.num_copies
        self.start_codons, self.stop_codons = start_codons, stop_codons
        self.intron_begin_pattern, self.intron_end_pattern = intron_begin_pattern, intron_end_pattern
        self.l2_lambda = l2_lambda
        self.nucleotide_kernel_init = nucleotide_kernel_init
        self.trainable_nucleotides_at_exons = trainable_nucleotides_at_exons
        self.n_mass_compat = n_mass_compat
        self.fused_training = fused_training      # the layer trains through forward_fused_trainable where can_fuse holds
        start = make_codon_probs(start_codons, True)
        stop = make_codon_probs(stop_codons, False)
        ibeg = make_codon_probs(intron_begin_pattern, True)
        iend = make_codon_probs(intron_end_pattern, False)
        anyc = make_codon_probs([("NNN", 1.0)], False)
        not_stop = anyc * (stop == 0).float()
        not_stop = not_stop / not_stop.sum()
        # constrained states in order: E2, START, EI0, EI1, EI2, IE0, IE1, IE2, STOP
        left = [anyc, start, ibeg, ibeg, ibeg, anyc, anyc, anyc, anyc]
        right = [not_stop, anyc, anyc, not_stop, anyc, iend, iend, iend, stop]
        self.start_codon_probs, self.stop_codon_probs = start, stop
        self.intron_begin_codon_probs, self.intron_end_codon_probs = ibeg, iend
        self.any_codon_probs, self.not_stop_codon_probs = anyc, not_stop
        self.register_buffer("codon_probs", torch.cat([torch.cat(left, dim=1), torch.cat(right, dim=1)], dim=0),
                             persistent=False)           # (2, 9, 64)
        self.nuc_emission_kernel = None

    def build(self, input_shape):
        if self.built:
            return
        super().build(input_shape)
        if self.trainable_nucleotides_at_exons:
            assert self.num_models == 1, "trainable nucleotide emissions support one model"
            shape = (self.num_models, 3 * self.num_copies, 4)
            if torch.is_tensor(self.nucleotide_kernel_init):
                start = self.nucleotide_kernel_init.detach().clone().to(torch.float32).reshape(shape)
            else:
                start = torch.zeros(shape)
            self.nuc_emission_kernel = nn.Parameter(start)

    def get_nucleotide_probs(self):
        return torch.softmax(self.nuc_emission_kernel, dim=-1)

    def get_aux_loss(self):
        """l2_lambda * mean over rows of sum_c (scale kernel)^2 with embeddings on
        (gene_pred_hmm_emitter.py:274-275, MvnMixture.py:177-181), else 0."""
        if not self.emit_embeddings:
            return 0.0
        scale_kernel = self.embedding_emission_kernel[..., self.embedding_dim:]
        return self.l2_lambda * torch.mean(torch.sum(torch.square(scale_kernel), dim=-1))

    def codon_emissions(self, nucleotides):
        """(k, b, L, 5) one-hot nucleotides -> (k, b, L, q) factor: 1/4096 for the first
        1 + 5*copies states, left x right 3-mer compatibility for the constrained ones."""
        k, b, L = nucleotides.shape[:3]
        flat = nucleotides.reshape(-1, L, 5)
        left = kmer.make_k_mers(flat, 3, True).reshape(k, b, L, 64)
        right = kmer.make_k_mers(flat, 3, False, n_mass=2 if self.n_mass_compat else 1).reshape(k, b, L, 64)
        tab = self.codon_probs.to(nucleotides.dtype)
        cod = torch.einsum("kbls,qs->kblq", left, tab[0]) * torch.einsum("kbls,qs->kblq", right, tab[1])
        if self.num_copies > 1:
            cod = cod.repeat_interleave(self.num_copies, dim=-1)
        free = torch.full_like(cod[..., :1], 1.0 / 4096.0).expand(*cod.shape[:-1], 1 + 5 * self.num_copies)
        return torch.cat([free, cod], dim=-1)

    def forward(self, inputs, end_hints=None, training=False):
        """(k, b, L, s [+ d] + 5): class probabilities, [embedding,] one-hot nucleotides -> E (k, b, L, q)."""
        nucleotides, classes = inputs[..., -5:], inputs[..., :-5]
        emit = super().forward(classes, end_hints=end_hints, training=training)
        cod = self.codon_emissions(nucleotides)
        if training:
            cod = cod + 1e-7
        full = emit * cod
        if self.trainable_nucleotides_at_exons:
            acgt = nucleotides[..., :4] + nucleotides[..., 4:] / 4
            c = self.num_copies
            nuc = torch.einsum("k...s,kqs->k...q", acgt, self.get_nucleotide_probs())
            quarter = torch.full_like(full[..., :1], 0.25)
            nuc = torch.cat([quarter.expand(*full.shape[:-1], 1 + 3 * c), nuc,
                             quarter.expand(*full.shape[:-1], full.shape[-1] - 1 - 6 * c)], dim=-1)
            full = full * nuc
        return full

    # -- fused inference path (HIP kernels hmm_gene_emissions, hmm_gene_emissions_wide) -------
    def fused_route(self):
        """The route that serves this model without the wide embedding kernels: "gene" (hmm_gene_emissions and its
        backward: q <= 64 and rows <= 32), "wide" (hmm_gene_emissions_wide and its backward: up to 256 states and
        rows, no embeddings) or None.  Kept for its callers; the layer itself goes by fused_routes(), which also
        knows hmm_embedding_emissions_wide."""
        from . import engine
        wide = engine.gene_emissions_routes_wide(self.num_states, self.kernel_rows())
        if wide is None or (wide and self.emit_embeddings):
            return None
        return "wide" if wide else "gene"

    def fused_routes(self):
        """(class route, embedding route) of this model: ("gene" | "wide" | None, None | "mvn" | "mvn_wide").  "gene" /
        "mvn" are hmm_gene_emissions / hmm_embedding_emissions and their backwards (q <= 64 and rows <= 32), "wide" /
        "mvn_wide" the _wide pairs (up to 256 states and rows); the embedding route is None without embeddings.  A
        class route of None means forward() in torch ops (then the embedding route is None too).  The same rules as
        autograd.GeneEmissions and autograd.EmbeddingEmissions (engine.gene_emissions_routes_wide,
        engine.embedding_emissions_routes_wide)."""
        from . import engine
        q, rows = self.num_states, self.kernel_rows()
        wide = engine.gene_emissions_routes_wide(q, rows)
        if wide is None:
            return None, None
        if not self.emit_embeddings:
            return "wide" if wide else "gene", None
        mvn = engine.embedding_emissions_routes_wide(q, rows)
        if mvn is None:
            return None, None
        return "wide" if wide else "gene", "mvn_wide" if mvn else "mvn"

    def can_fuse(self, inputs):
        # one model on a GPU and kernels for the shape (fused_routes): every model of up to 256 states and kernel rows
        # (18 copies), with or without embeddings or the trainable nucleotide factor (hmm_nucleotide_emissions serves
        # the same 256 states); anything larger takes forward()
        return (inputs.is_cuda and inputs.shape[0] == 1 and self.num_models == 1 and self.built
                and self.fused_routes()[0] is not None)

    def state_tables(self, device):
        """(state -> kernel row, state -> codon-table row or -1) as int32 tensors."""
        c = self.num_copies
        n_free = 1 + 5 * c
        if self.share_intron_parameters:      # rows: Ir, I(c), E0..E2 .., states: Ir, I0, I1, I2, rest
            rows = list(range(1 + c)) + list(range(1, 1 + c)) * 2 + list(range(1 + c, self.kernel_rows()))
        else:
            rows = list(range(self.num_states))
        cod = [-1] * n_free + [i // c for i in range(self.num_states - n_free)]
        return (torch.tensor(rows, dtype=torch.int32, device=device),
                torch.tensor(cod, dtype=torch.int32, device=device))

    def nucleotide_table(self, device):
        """state -> row of get_nucleotide_probs()[0] as an int32 tensor: j - (1 + 3c) on the exon states E0/E1/E2 of
        every copy (1 + 3c <= j < 1 + 6c), -1 (free: the factor is 1/4) on every other state."""
        c = self.num_copies
        tab = torch.full((self.num_states,), -1, dtype=torch.int32)
        tab[1 + 3 * c:1 + 6 * c] = torch.arange(3 * c, dtype=torch.int32)
        return tab.to(device)

    def forward_fused(self, inputs, end_hints=None, training=False):
        """Same values as forward() (inference, one model) without the (b,L,64) 3-mer tensors:
        one HIP kernel from class probabilities + nucleotides to E (hmm_gene_emissions, or hmm_gene_emissions_wide
        above 64 states or 32 kernel rows: fused_routes).

        With embeddings, a second kernel (hmm_embedding_emissions, or hmm_embedding_emissions_wide) multiplies the normal-density factor into E,
        reading the d embedding columns in place from `inputs`; the class kernel takes a compact (b, L, s + 5)
        copy of the other columns.  With training=True the reference adds 1e-10 to the class term before the
        product, which the class kernel cannot express: that case takes forward().

        With trainable_nucleotides_at_exons, hmm_nucleotide_emissions then multiplies the nucleotide factor into E in
        place, reading the last five columns of `inputs` where they lie."""
        from . import engine
        with torch.no_grad():
            if self.emit_embeddings and training:
                return self.forward(inputs, end_hints=end_hints, training=True)
            if self.B is None:
                self.recurrent_init()
            row, cod = self.state_tables(inputs.device)
            x = inputs[0].to(torch.float32).contiguous()
            if self.emit_embeddings:
                d = self.embedding_dim
                s = x.shape[-1] - d - 5
                classes = torch.cat([x[..., :s], x[..., s + d:]], dim=-1)
            else:
                classes = x
            route, mvn_route = self.fused_routes()
            kernel = engine.gene_emissions_wide if route == "wide" else engine.gene_emissions
            E = kernel(classes, self.B[0].to(torch.float32).contiguous(),
                       row, self.codon_probs.to(inputs.device, torch.float32).contiguous(), cod,
                       add=1e-7 if training else 0.0, n_mass=2 if self.n_mass_compat else 1)
            if self.emit_embeddings:
                mean, inv_std, log_norm = self.embedding_tables(inputs.device)
                mvn = engine.embedding_emissions_wide if mvn_route == "mvn_wide" else engine.embedding_emissions
                mvn(x, s, d, mean, inv_std, log_norm, row, E=E, inv_temperature=1.0 / float(self.temperature))
            if self.trainable_nucleotides_at_exons:
                engine.nucleotide_emissions(x, x.shape[-1] - 5, self.get_nucleotide_probs()[0].to(torch.float32).contiguous(),
                                            self.nucleotide_table(inputs.device), E=E)
            return self.apply_end_hints(E.unsqueeze(0), end_hints)

    def forward_fused_trainable(self, inputs, end_hints=None, training=False):
        """forward() with its autograd graph, through the HIP kernels: make_B() (softmax, torch), ONE node
        (autograd.GeneEmissions: hmm_gene_emissions forward, hmm_gene_emissions_grad backward, or the _wide pair
        above 64 states or 32 kernel rows), apply_end_hints (torch).  Between forward and backward only the input, B
        and the small tables are kept.

        Difference from forward(): the gradient of the five nucleotide columns of the input is exactly zero.
        One-hot nucleotides are data, and the ``== 1`` test on the N flag is not differentiable anyway; autograd
        through forward() returns small non-zero values there (up to about 3e-2 in fp64 on test-sized inputs).
        A caller who concatenates network output with one-hot nucleotides never sees them.  Needs can_fuse(inputs).

        With embeddings a second node follows (autograd.EmbeddingEmissions: hmm_embedding_emissions forward,
        hmm_embedding_emissions_grad backward, or the _wide pair above 64 states or 32 kernel rows) that multiplies the normal-density factor into E, reading the d
        embedding columns of the input in place; the class node takes the compact (b, L, s + 5) copy of the other
        columns.  The tables come from embedding_tables_with_graph, so embedding_emission_kernel trains.  With
        training=True the reference adds 1e-10 to the class term before the product ((C + 1e-10) (f + 1e-10)
        (cod + 1e-7)): the compact tensor gets one more class column of value 1e-10 and B a column of ones, so
        that C + 1e-10 comes out of the unchanged class kernel (torch.cat's backward drops the column again).
        That needs s + 1 <= 32 classes; above that, and where can_fuse(inputs) does not hold, this is forward().

        With trainable_nucleotides_at_exons one more node follows the class node and the embedding node
        (autograd.NucleotideEmissions: hmm_nucleotide_emissions forward, hmm_nucleotide_emissions_grad backward): it
        multiplies the nucleotide factor into E, reading the five nucleotide columns of the input in place, with
        P = get_nucleotide_probs()[0] and its graph, so nuc_emission_kernel trains.  Where can_fuse(inputs) does not
        hold, that option takes forward() too."""
        from . import autograd
        if self.trainable_nucleotides_at_exons and not self.can_fuse(inputs):
            return self.forward(inputs, end_hints=end_hints, training=training)
        B = self.make_B()[0].to(torch.float32)
        row, cod = self.state_tables(inputs.device)
        x = inputs[0].to(torch.float32)
        kw = dict(add=1e-7 if training else 0.0, n_mass=2 if self.n_mass_compat else 1)
        codon = self.codon_probs.to(inputs.device, torch.float32).contiguous()
        if not self.emit_embeddings:
            E = autograd.gene_emissions(x, B, row, codon, cod, **kw)
            return self.apply_end_hints(self._nucleotide_node(E, x).unsqueeze(0), end_hints)
        d = self.embedding_dim
        s = x.shape[-1] - d - 5
        if (training and s + 1 > 32) or not self.can_fuse(inputs):
            return self.forward(inputs, end_hints=end_hints, training=training)
        parts = [x[..., :s], x[..., s + d:]]
        if training:
            parts.insert(1, torch.full_like(x[..., :1], 1e-10))
            B = torch.cat([B, torch.ones_like(B[:, :1])], dim=-1)
        E = autograd.gene_emissions(torch.cat(parts, dim=-1), B, row, codon, cod, **kw)
        mean, inv_std, log_norm = self.embedding_tables_with_graph(inputs.device)
        E = autograd.embedding_emissions(E, x, mean, inv_std, log_norm, row, s, d,
                                         inv_temperature=1.0 / float(self.temperature),
                                         add=1e-10 if training else 0.0)
        return self.apply_end_hints(self._nucleotide_node(E, x).unsqueeze(0), end_hints)

    def _nucleotide_node(self, E, x):
        """E (b,L,q) times the trainable nucleotide factor (autograd.NucleotideEmissions); E itself without the option."""
        if not self.trainable_nucleotides_at_exons:
            return E
        from . import autograd
        return autograd.nucleotide_emissions(E, x, self.get_nucleotide_probs()[0].to(torch.float32),
                                             self.nucleotide_table(x.device), x.shape[-1] - 5)

    def get_config(self):
        config = super().get_config()
        config.update({"start_codons": self.start_codons, "stop_codons": self.stop_codons,
                       "intron_begin_pattern": self.intron_begin_pattern,
                       "intron_end_pattern": self.intron_end_pattern, "l2_lambda": self.l2_lambda,
                       "nucleotide_kernel_init": self.nucleotide_kernel_init,
                       "trainable_nucleotides_at_exons": self.trainable_nucleotides_at_exons,
                       "n_mass_compat": self.n_mass_compat,           # D5 compatibility switch
                       "fused_training": self.fused_training})
        return config
