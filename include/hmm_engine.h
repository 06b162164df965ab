/*
 * hmm_engine.h — C ABI of the MI355X (gfx950) HMM forward / backward / posterior /
 * Viterbi engine.  Plain pointers and sizes only; every pointer is a DEVICE pointer
 * unless stated otherwise; all calls are asynchronous on `stream` (a hipStream_t passed
 * as void*), re-entrant, and keep no state between calls (the only process-wide settings are
 * the explicit tuning options of hmm_set_option).
 *
 * The reference (sukui-genomics-cn/hmm_layer) has no native boundary: its hot path is a
 * Python loop over HmmCell.forward.  Each entry point below replaces one reference
 * driver; the file:line it replaces is cited per function.  Shapes follow the
 * reference: k = number of models, b = batch, L = sequence length, q = states,
 *   A   (k,q,q)   row-stochastic transition matrices   (transitioner.make_A(),
 *                 hmm_layer/gene_pred_hmm_transitioner.py:99-102)
 *   pi  (k,q)     start distributions                  (make_initial_distribution(), :111-112)
 *   E   (k,b,L,q) emission PROBABILITIES, row-major    (cell.emission_probs(),
 *                 hmm_layer/MsaHmmCell.py:61-71) — the engine applies max(.,eps) itself,
 *                 like the cell does (hmm_layer/MsaHmmCell.py:87-88).
 * All tensors are fp32 and contiguous; log-likelihoods are returned in fp64.
 *
 * Workspace: the caller owns all memory.  Query hmm_workspace_bytes() and pass a
 * device buffer of at least that size (256-byte aligned) to the call.
 *
 * Memory contract (tests/test_memory_contract_gpu.py holds every entry point to it with guard bands around every
 * argument and a workspace of exactly the queried size).  A call
 *   - reads nothing outside its inputs: of a strided input (emb / nuc with ld) only the columns it names;
 *   - writes nothing outside its outputs and the first `workspace_bytes` bytes, as the size query returns them, of the
 *     workspace; of a strided output (demb with ldd) only the columns it names; inputs are never written
 *     (E with multiply = 1 is an output as well);
 *   - writes every element of every output it is asked for (a NULL-able output that is NULL is not asked for);
 *   - does not depend on what the workspace or the outputs held before: a workspace may be reused for any other call,
 *     of any shape, without clearing it.  The one region kept on purpose is what the sequence-sharded protocols leave
 *     in the workspace between their own steps.
 * Alignment of the pointers:
 *   - workspace: 256 bytes;
 *   - 16 bytes: E of hmm_gene_emissions, dx of hmm_gene_emissions_grad and of hmm_gene_emissions_grad_wide (whole
 *     tiles of 16 positions leave as aligned 16-byte pieces), all_ops of hmm_seqshard_posterior and hmm_seqshard_mid_posterior, all_vops of
 *     hmm_seqshard_viterbi_apply and hmm_seqshard_vscan_apply (the hops read the gathered operators' rows as aligned
 *     16-byte pieces);
 *   - every other pointer: the alignment of its element type — 4 bytes for fp32 and int32 tensors (a view such as
 *     E_all + m * b * L * q of an odd-sized model is fine), 8 for fp64 and int64 (loglik, score, partial, slab_vbase).
 *     There the kernels reach caller memory through element accesses, 4-byte-aligned vector types and buffer
 *     descriptors.
 *
 * Streams: to the caller every call is an ordinary in-order operation on `stream` — it starts
 * after everything enqueued there before it, and everything enqueued after it sees its results.
 * Inside, three calls put independent parts of their work on a per-device helper stream, forked
 * from and joined back into `stream` with events: hmm_posterior for q > 64 (the two recursions),
 * hmm_viterbi on large batches (batch groups, HMM_OPT_VGROUPS) and, opt-in, hmm_posterior
 * (HMM_OPT_GROUPS).  They remain capturable into a HIP graph and give identical results when no
 * helper stream can be created (everything then runs in order on `stream`).
 */
#ifndef HMM_ENGINE_H
#define HMM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMM_ENGINE_ABI_VERSION 3

/* error codes (0 = success); hmm_strerror() names them */
#define HMM_OK                 0
#define HMM_ERR_BAD_SHAPE     -1   /* k,b,L,q < 1 */
#define HMM_ERR_Q_UNSUPPORTED -2   /* q above what this build's kernels cover */
#define HMM_ERR_NULL_POINTER  -3
#define HMM_ERR_WORKSPACE     -4   /* workspace too small or misaligned */
#define HMM_ERR_LAUNCH        -5   /* HIP launch error (see hipGetLastError) */
#define HMM_ERR_BAD_ARGUMENT  -6
#define HMM_ERR_NO_DEVICE     -7
#define HMM_ERR_NO_RCCL       -8   /* hmm_loglik_allreduce: the process has no RCCL loaded */

/* The clamp eps.  Every entry point that takes `eps` serves HMM_EPS_MIN <= eps <= HMM_EPS_MAX and refuses anything
 * else — smaller, larger, zero, negative, NaN, infinite — with HMM_ERR_BAD_ARGUMENT, after the null-pointer checks and
 * before the workspace checks.  The lower end is where the kernels' arithmetic stops: a step's normaliser
 * S = sum_j max(E_j, eps) max(R_j, eps) can be as small as q eps^2 (a row of zero emissions on a floored state), the
 * kernels take its reciprocal and logarithm in fp32 with denormals flushed, so eps^2 has to be a normal number
 * (eps >= 2^-63 = 1.08e-19); 1e-18 leaves a factor of 85 above that, and tests/test_eps_sweep_gpu.py holds every
 * output of the 1..64-state kernels to the fp64 oracle there.  The upper end is the largest value that sweep holds them
 * to the oracle at; nothing is known to break above it, it is simply where the evidence ends, and a clamp that carries
 * more than a thousandth of every step's mass is not a rounding guard any more.  The domain is one for the whole
 * library: the entry points for more than 64 states, the per-sequence walks, the class posteriors and the
 * sequence-sharded calls check it too.  All of them accepted any float before (0, negative and NaN included) — this
 * is a deliberate narrowing of the ABI.  The reference's default is 1e-16 (hmm_layer/MsaHmmCell.py:33). */
#define HMM_EPS_MIN 1e-18f
#define HMM_EPS_MAX 1e-3f

/* operations, for hmm_workspace_bytes() */
#define HMM_OP_LOGLIK     0   /* hmm_forward without log_alpha */
#define HMM_OP_FORWARD    1   /* hmm_forward with log_alpha      */
#define HMM_OP_BACKWARD   2
#define HMM_OP_POSTERIOR  3
#define HMM_OP_VITERBI    4

/* output modes of hmm_posterior() */
#define HMM_POST_PROB        0   /* gamma (probabilities, rows sum to 1)                    */
#define HMM_POST_LOG         1   /* log gamma = log alpha + log beta - loglik               */
#define HMM_POST_LOG_NO_LL   2   /* log alpha + log beta (the reference's no_loglik=True)   */

const char *hmm_strerror(int code);
int hmm_abi_version(void);

/*
 * Tuning / test options: explicit, process-wide, read at launch time.  The defaults are the
 * measured best and results depend on nothing outside a call's arguments and these options; the
 * HMM_ENGINE_CHUNK / _FORCE_DENSE / _SCAN2 / _GROUPS / _EXACT environment variables only seed
 * them once, when the first option is read.  hmm_set_option returns the previous value
 * (HMM_ERR_BAD_ARGUMENT for an unknown option).
 */
#define HMM_OPT_CHUNK        0   /* chunk length of the scan (multiple of 16, <= 512); 0 = chosen per shape */
#define HMM_OPT_FORCE_DENSE  1   /* 1: generic kernels even for the compiled gene topologies               */
#define HMM_OPT_SCAN2        2   /* 0: single-level chunk scan                                              */
#define HMM_OPT_GROUPS       3   /* batch groups pipelined on two internal streams (1 = off)               */
#define HMM_OPT_EXACT        4   /* HMM_EXACT_*: routing to the serial exact-clamp kernels (q <= 16)        */
#define HMM_OPT_PGCHUNK      5   /* hmm_posterior_grad in chunks: 0 never, 1 when it pays (default), 2 always  */
#define HMM_OPT_VGROUPS      6   /* hmm_viterbi: batch groups pipelined on an internal stream; 0 = chosen per shape, 1 = off */
#define HMM_OPT_VLARGE       7   /* hmm_viterbi_large: 0 = by q (default), 1 = per-sequence walk, 2 = per-position tiles */
#define HMM_OPT_GLARGE       8   /* hmm_loglik_grad_large and hmm_posterior_grad_large: 0 = by q (default),
                                    1 = per-sequence walk, 2 = per-position GEMMs                            */
#define HMM_OPT_COUNT        9
#define HMM_EXACT_AUTO    0      /* decided on the device (see hmm_posterior)                               */
#define HMM_EXACT_OFF     1      /* always the chunked scan                                                 */
#define HMM_EXACT_ALWAYS  2      /* always the serial kernels                                               */
#define HMM_EXACT_ALWAYS_NARROW 3 /* test hook: as ALWAYS, with the one-sequence-per-wave layout that sequences
                                    of more than 2 GB / 16 need                                              */
int hmm_set_option(int option, int value);
int hmm_get_option(int option);

/* Largest q supported (4096): q <= hmm_scan_max_states() (16) runs the chunked scan kernels,
 * larger models run serial in time with one f32-MFMA GEMM per position (the profile-HMM sizes,
 * e.g. q = 2*512+3 = 1027); in between, up to 64 states: the chunked scan with 32- / 64-state tiles where it
 * pays (17..32 states: every primitive model; 33..64: up to 96 sequences per call), otherwise one wave walks one
 * sequence — with a SPARSE step (each lane gathers its own predecessors / successors) when no state of the model
 * has more than 8 of either, e.g. the multi-copy gene models; decided per model on the device, HMM_OPT_FORCE_DENSE = 1
 * forces the all-candidates step.  Zero entries of A are exact zeros in both steps; the two differ in rounding order only.
 * hmm_viterbi covers q <= hmm_viterbi_max_states() (64) and hmm_viterbi_large every q up to
 * hmm_viterbi_large_max_states() (4096); hmm_loglik_grad covers q <= hmm_grad_max_states() (64) and
 * hmm_loglik_grad_large every q up to hmm_loglik_grad_large_max_states() (4096); hmm_posterior_grad covers
 * q <= hmm_posterior_grad_max_states() (64) and hmm_posterior_grad_large every q up to
 * hmm_posterior_grad_large_max_states() (4096). */
int hmm_max_states(void);
int hmm_scan_max_states(void);
int hmm_viterbi_max_states(void);
int hmm_grad_max_states(void);

/* Time-chunk length the engine will use for (k, b, L): a multiple of 16; 0 for the serial large-q path.  A pure
 * function of the shape (and of HMM_OPT_CHUNK): the forward, backward, log-likelihood and posterior plans of a shape
 * all use it, and so do the gradient plans built on them.  Where the older rule stops at its ceiling of 512 and the
 * forward / backward kernels need more than one round of resident blocks, it is the multiple of 16 in [256, 512] at
 * which the blocks fill the compute units most evenly; hmm_viterbi's plan keeps the older
 * rule there (512). */
int hmm_chunk_len(int k, int b, int L, int q);

/* Diagnostics: what that rule takes the machine to hold, constants of the build (no device needed):
 * compute units (256), resident 4-wave blocks per compute unit of the posterior's forward and backward kernels (2)
 * and of the sparse 15-state chunk reduce (4).  HMM_ERR_BAD_ARGUMENT for another `which`. */
#define HMM_PLAN_CUS             0
#define HMM_PLAN_FORWARD_BLOCKS  1
#define HMM_PLAN_BACKWARD_BLOCKS 2
#define HMM_PLAN_REDUCE_BLOCKS   3
int hmm_plan_capacity(int which);
/* The same read from the current device: its compute units, the occupancy query's blocks per compute unit for the
 * three kernels.  HMM_ERR_NO_DEVICE without one. */
int hmm_plan_capacity_device(int which);

/* Column width (64, 80 or 96) of the GEMM tile the serial large-q path uses for a batch of b
 * sequences per model and q > 64 states (the instantiation is chosen per shape so that the 256 CUs
 * get as even a share of tiles as possible); 0 when q is served by another path. */
int hmm_largeq_tile_cols(int b, int q);

size_t hmm_workspace_bytes(int op, int k, int b, int L, int q);

/*
 * Forward recursion.  Replaces _forward_recursion_impl (hmm_layer/MsaHMMLayer.py:227-282)
 * = BaseRNN time loop (hmm_layer/BaseRNN.py:217-227) over HmmCell.forward
 * (hmm_layer/MsaHmmCell.py:73-106, forward branch :102-103).
 *   log_alpha (k,b,L,q) or NULL : log alpha_t = log alpha_hat_t + sum_{s<=t} log c_s
 *   loglik    (k,b) fp64        : sum_t log c_t
 */
int hmm_forward(const float *A, const float *pi, const float *E,
                int k, int b, int L, int q, float eps,
                float *log_alpha, double *loglik,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward recursion.  Replaces _backward_recursion_impl (hmm_layer/MsaHMMLayer.py:322-381)
 * = the reverse HmmCell (hmm_layer/MsaHmmCell.py:96-100) run over flipped time.
 *   log_beta (k,b,L,q), beta_{L-1} = 1.
 */
int hmm_backward(const float *A, const float *E,
                 int k, int b, int L, int q, float eps,
                 float *log_beta,
                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * State posteriors.  Replaces _state_posterior_log_probs_impl
 * (hmm_layer/MsaHMMLayer.py:422-521) = Bidirectional (hmm_layer/Bidirectional.py:113-164)
 * over the forward and reverse cells + chunk stitching via TotalProbabilityCell
 * (hmm_layer/TotalProbabilityCell.py:30-49, hmm_layer/MsaHMMLayer.py:285-319, 384-419).
 *   out    (k,b,L,q) : per `mode` (HMM_POST_*)
 *   loglik (k,b) fp64 or NULL
 * Posteriors are formed from the scaled per-position variables and renormalised per
 * position, which is algebraically the reference's log alpha + log beta - loglik
 * (hmm_layer/MsaHMMLayer.py:501-514) without its fp32 cancellation.
 *
 * The cell clamps the predicted state MIXTURE at eps every step (hmm_layer/MsaHmmCell.py:87-88); the
 * chunk operators of the scan are the exactly linear products of A diag(max(E, eps)) and know nothing of it.
 * For q <= 64 wherever the chunked scan runs, the engine therefore decides on the device, with no host
 * round trip, which inputs the scan may serve:
 *   - per model: the support of A (entries > eps) must be primitive (irreducible and aperiodic);
 *     reducible or periodic chains, states without incoming edges, all-zero rows (the reference's
 *     as-shipped matrices) and A = I go to serial kernels with the cell's exact step semantics;
 *   - per sequence: the posterior mass of CLAMP-BORN paths — paths through a component that a clamp of either
 *     cell lifted to eps — is exactly what separates the serial recursion from the clamp-free scan (posteriors
 *     and log-likelihood alike).  The in-chunk kernels, which do apply the clamps, sum it per chunk; sequences
 *     above 2e-6 (a tenth of the posteriors' stated tolerance) are recomputed serially — only WINDOWS of chunks
 *     around the ones that carry that mass, grown until the recursion has forgotten it (the cost of a flagged
 *     sequence is its flagged chunks plus the model's forgetting time, not its length), in every entry point:
 *     hmm_posterior; hmm_forward (forward cell's births, weighed with the chunk scan's backward vectors; log alpha
 *     after a window moves with the window's log-likelihood), hmm_backward (the mirror image, weighed with the
 *     forward vectors of a uniform start) and hmm_loglik_grad (forward cell's births).  Windows that grow into
 *     each other, and sequences with more than 16 of them, are redone whole.  Chunks whose operator columns went
 *     through the denormal range (two observations in a row that every path survives at the emission floor only)
 *     count as flagged.
 *     For 17..64 states (the chunked 32- / 64-state scans) the same certificates are summed per chunk — psi in
 *     hmm_posterior, the forward cell's births in hmm_forward (log alpha and the log-likelihood alone), the reverse
 *     cell's in hmm_backward — but a flagged sequence is recomputed WHOLE, there are no windows; a chain whose
 *     operator columns went through the denormal range, or all met an observation they survive at the emission floor
 *     only, is marked by the reduce and its sequence recomputed whole as well.
 * hmm_exact_count() reports how many of the last call's sequences took the serial kernels.
 */
int hmm_posterior(const float *A, const float *pi, const float *E,
                  int k, int b, int L, int q, float eps, int mode,
                  float *out, double *loglik,
                  void *workspace, size_t workspace_bytes, void *stream);

/* Diagnostics of the routing above: reads, from the workspace of a finished q <= 64 call (the
 * caller synchronises first), how many of its k*b sequences were served by the serial exact-clamp
 * kernels.  `op` and the shape are those of the call.  Returns the count or a negative error. */
long long hmm_exact_count(int op, int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
/* The same for a finished hmm_posterior call, q <= 16, in detail:
 *   detail[0] sequences that left the scan (= hmm_exact_count)
 *   detail[1] of those, sequences recomputed in windows (runs of chunks around the flagged ones)
 *   detail[2] the number of such windows
 *   detail[3] sequences recomputed whole because most of their chunks were flagged or because two of their
 *             windows grew into each other (sequences of models routed per model are in detail[0] only)
 *   detail[4] chunks (of hmm_chunk_len positions) the windows walked, their growth until the recursion had
 *             forgotten the clamp-born mass included */
int hmm_exact_detail(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes, long long *detail);
/* The same for the last hmm_forward (HMM_OP_LOGLIK without log alpha, HMM_OP_FORWARD with) or hmm_backward
 * (HMM_OP_BACKWARD) call of this shape: the op selects the workspace layout.  HMM_OP_POSTERIOR = hmm_exact_detail. */
int hmm_exact_detail_op(int op, int k, int b, int L, int q, const void *workspace, size_t workspace_bytes,
                        long long *detail);
/* Test / diagnostic hook: the window table of sequence `seq` after the last call of `op` with this shape (q <= 16):
 * table[34] = count, spare, then (first chunk, chunks) pairs as the window kernels left them; shifts[24] (or null;
 * HMM_OP_FORWARD / HMM_OP_BACKWARD) = 16 per-window log-scale shifts as doubles, then 16 ints (last / first chunks);
 * psi[npsi] (or null) = the certificate's per-chunk sums.  Returns the number of chunks, or an error. */
int hmm_window_table(int op, int k, int b, int L, int q, const void *workspace, size_t workspace_bytes, int seq,
                     int *table, double *shifts, float *psi, int npsi);

/*
 * Posterior decoding, fused: per position the CLASS with the largest posterior and that posterior, without the
 * (k,b,L,q) tensor ever reaching memory — 1 + 4 bytes per position instead of 4 q.  For
 * q <= hmm_posterior_decode_max_states() (16); above, callers compose hmm_posterior with a reduction of their own
 * (hmm_layer_amd.engine.posterior_decode does); 17..64 states have hmm_posterior_decode_mid below.
 *   state_class  HOST pointer, q entries in 0 .. num_classes-1: the class of every state; NULL = the identity map
 *                (every state its own class; num_classes must then equal q).  Read during the call and passed to the
 *                kernels by value: the caller may change or free it at once, and a captured graph keeps the table it
 *                was captured with.
 *   num_classes  1 .. 16
 *   label  (k,b,L) bytes      the class with the largest class posterior, the lowest class index on ties
 *   conf   (k,b,L) or NULL    that class's posterior probability
 *   loglik (k,b) fp64 or NULL as hmm_posterior
 * A, pi, E, eps, the clamp semantics and the routing to the serial kernels are those of hmm_posterior in
 * HMM_POST_PROB mode: the same kernels compute the same gamma row of every position (routed sequences get theirs
 * from the exact serial step), which is then collapsed on chip.  The class posterior is the fp32 sum of gamma over
 * the states of the class, added in increasing state index starting from 0; classes are compared in increasing class
 * index with a strict >, so label is the lowest maximal class.  With the identity map nothing is summed: conf is, bit
 * for bit, the largest entry of hmm_posterior's row and label its lowest index.
 * The workspace is hmm_workspace_bytes(HMM_OP_POSTERIOR, k, b, L, q); hmm_exact_count(HMM_OP_POSTERIOR, ...),
 * hmm_exact_detail and hmm_window_table read the routing of a finished decode call from it as they do for
 * hmm_posterior.  Runs on `stream` alone with no host synchronisation (capturable); repeated calls are bit-identical.
 * Argument checks, before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), q > 16 (HMM_ERR_Q_UNSUPPORTED), NULL
 * among A, pi, E, label, workspace (HMM_ERR_NULL_POINTER), num_classes outside 1..16 or an entry of state_class outside
 * 0..num_classes-1 or state_class NULL with num_classes != q (HMM_ERR_BAD_ARGUMENT), workspace too small or not
 * 256-byte aligned (HMM_ERR_WORKSPACE).
 */
int hmm_posterior_decode_max_states(void);
int hmm_posterior_decode(const float *A, const float *pi, const float *E,
                         int k, int b, int L, int q, float eps,
                         const int *state_class, int num_classes,
                         unsigned char *label, float *conf, double *loglik,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same for 17 <= q <= hmm_posterior_decode_mid_max_states() (64): the two-, three- and four-copy gene models
 * (29 / 43 / 57 states) and any learned dense A of that range.  Arguments, outputs, clamp semantics and routing are
 * those of hmm_posterior_decode, applied to what hmm_posterior(HMM_POST_PROB) computes for these models: the chunked
 * scan (hmm_scan_rows.inc) collapses its staged gamma rows on chip, and the sequences that hmm_posterior routes to the
 * one-wave-per-sequence kernels (hmm_midq.inc: models the device finds non-primitive, sequences the certificate
 * flags, HMM_EXACT_ALWAYS, every sequence of 33..64 states outside the chunked scan's range) are routed here too,
 * to a form of those kernels that stages its gamma rows in LDS and collapses them the same way.
 *   state_class  HOST pointer or NULL, as above; reaches the kernels by value (sixteen 64-bit membership masks)
 *   num_classes  1 .. 16 with a table; q with the identity map (state_class NULL)
 *   label, conf, loglik   as above.  Identity map: conf is bit for bit the largest entry of hmm_posterior's row and
 *                label its lowest index; loglik is bit for bit hmm_posterior's.
 * Workspace: hmm_posterior_decode_mid_workspace_bytes(k, b, L, q) (0: unsupported shape), 256-byte aligned.  Its
 * first hmm_workspace_bytes(HMM_OP_POSTERIOR, k, b, L, q) bytes have exactly hmm_posterior's layout, so
 * hmm_exact_count(HMM_OP_POSTERIOR, ...) reads the routing of a finished call as it does for hmm_posterior.  A
 * PARKING REGION of k*b*L*q floats follows: the serial walk's two waves park alpha_hat (t < L/2) and the backward
 * vector (t >= L/2) there until they meet, where hmm_posterior parks them in `out`.  THE WORKSPACE IS THEREFORE AS
 * LARGE AS THE (k,b,L,q) TENSOR THE CALL AVOIDS WRITING — still less memory than hmm_posterior plus a reduction
 * (gamma, class sums and an argmax), and only walked sequences touch the region; bounding it by device-assigned slots
 * is a follow-up.  The query returns exactly what the call uses.
 * Memory contract: every label and conf element is written; nothing is read from the workspace before the call has
 * written it; label chunks start at arbitrary byte offsets; every offset into E, label and conf is 64-bit.  Runs on
 * `stream` alone with no host synchronisation (capturable); no atomics in the outputs; repeated calls are
 * bit-identical.
 * Argument checks, before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), q < 17 or q > 64
 * (HMM_ERR_Q_UNSUPPORTED), NULL among A, pi, E, label, workspace (HMM_ERR_NULL_POINTER), the class table as for
 * hmm_posterior_decode (HMM_ERR_BAD_ARGUMENT), workspace too small or not 256-byte aligned (HMM_ERR_WORKSPACE).
 * 65..256 states: hmm_posterior_decode_wide below.  Sequence-sharded decode is a follow-up.
 */
int hmm_posterior_decode_mid_max_states(void);
size_t hmm_posterior_decode_mid_workspace_bytes(int k, int b, int L, int q);
int hmm_posterior_decode_mid(const float *A, const float *pi, const float *E,
                             int k, int b, int L, int q, float eps,
                             const int *state_class, int num_classes,
                             unsigned char *label, float *conf, double *loglik,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * Posteriors and fused posterior decoding for hmm_posterior_walk_min_states() (65) <= q <=
 * hmm_posterior_walk_max_states() (256) states by a PER-SEQUENCE WALK (hmm_wideq.inc): the gene models of 5 to 18
 * copies (71 .. 253 states) and any learned A of that range.  hmm_posterior evaluates this range with one GEMM launch
 * per position and direction; here one workgroup walks one sequence, serial in time, with the cell's exact step: the
 * clamp semantics are those of hmm_posterior (max(E, eps), max(pi, eps), the forward clamp of the predicted mixture,
 * the backward max(A r, eps), normaliser logs accumulated in fp64, zero entries of A exact zeros).  There is no
 * certificate and no routing; hmm_exact_count has nothing to report for these calls.  The results agree with
 * hmm_posterior's to rounding order only: no bit-identity is promised across the two evaluations.
 *
 * hmm_posterior_walk: arguments, the three HMM_POST_* modes and outputs (out (k,b,L,q), loglik (k,b) fp64 or NULL)
 * as hmm_posterior.  The two halves of the workgroup walk from both ends and PARK their vectors in `out` until they
 * meet at ceil(L/2); every element of `out` is overwritten.  Workspace: hmm_posterior_walk_workspace_bytes (0:
 * unsupported shape); it has no part that grows with L.
 *
 * Step selection, per model, on the device (no host round trip):
 *   sparse        every state has at most 8 non-zero predecessors and at most 8 non-zero successors, except at most
 *                 2 HUB states of any degree (the intergenic state of a c-copy gene model has c + 1 of each: 19 at 18
 *                 copies).  A state's sum runs over its list in increasing source index, four products then four; a
 *                 hub's sum over ALL states is formed by the whole workgroup half (products summed within each wave
 *                 of 64 states, then the waves in increasing order).
 *   dense, <=128  the row / column of A in registers: four partial sums over the states i = 0, 1, 2, 3 (mod 4) in
 *                 increasing index, added as (s0 + s1) + (s2 + s3).
 *   dense, >128   the same sums with A read from memory at every position: SLOW (q loads per state and position),
 *                 and correct.  It is what a model of 129..256 states outside the sparse rule gets; nothing else is
 *                 substituted for it.  hmm_posterior's GEMMs are the faster evaluation for such a model.
 * HMM_OPT_FORCE_DENSE = 1 forces the dense step.  Normalisers and the row sums of gamma are sums within each wave of
 * 64 states, then over the waves in increasing order.
 *
 * hmm_posterior_decode_wide: arguments and outputs as hmm_posterior_decode_mid (state_class HOST pointer or NULL,
 * num_classes 1..16 with a table, q with the identity map; label (k,b,L) bytes, conf and loglik or NULL).  The class
 * table reaches the kernels by value (sixteen 256-bit membership masks), so a captured graph keeps its table.  The
 * class posterior is the fp32 sum of the gamma row over ALL states in increasing index with weights 0 / 1 (the bits of
 * adding the members alone); classes are compared in increasing index with a strict >.  With the identity map nothing
 * is summed: conf is bit for bit the largest entry of hmm_posterior_walk(HMM_POST_PROB)'s row and label its lowest
 * index.  loglik is bit for bit hmm_posterior_walk's in every mode.
 * Workspace: hmm_posterior_decode_wide_workspace_bytes = the walk's workspace rounded up to 256 bytes, then a PARKING
 * REGION of k*b*L*q floats, addressed like `out`, where the walk parks what hmm_posterior_walk parks in `out` (the
 * same stated contract as hmm_posterior_decode_mid; bounding it by checkpoints is a follow-up).
 *
 * hmm_posterior_walk_pays(k, b, L, q): 1 where the fused decode measured at least 1.25x faster than hmm_posterior
 * followed by a reduction over the (k,b,L,q) tensor (DESIGN, "Decoded output, 65-256 states"), 0 elsewhere and where
 * nothing was measured.  As measured on one MI355X (L = 10 000; 1, 32 and 1024 sequences; the sparse step at 71, 127
 * and 253 states, the dense step at 96 and 128): 1 for k*b <= 1024 sequences, 0 above, whatever L.  The dense step above
 * 128 states was not measured: send only models that take the sparse step there.
 * hmm_layer_amd.engine.posterior_decode asks it; the entry points run wherever they are called.
 *
 * Memory contract: every element of out, label and conf is written; nothing is read from the workspace before the
 * call has written it; label starts at an arbitrary byte offset; every offset into E, out, label, conf and the parking
 * region is 64-bit.  Both calls run on `stream` alone with no helper stream and no host synchronisation (capturable);
 * no atomics in the outputs; repeated calls are bit-identical.
 * Argument checks, before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), q < 65 or q > 256
 * (HMM_ERR_Q_UNSUPPORTED), NULL among A, pi, E, out / label, workspace (HMM_ERR_NULL_POINTER), the mode, respectively
 * the class table as for hmm_posterior_decode_mid (HMM_ERR_BAD_ARGUMENT), workspace too small or not 256-byte aligned
 * (HMM_ERR_WORKSPACE).
 */
int hmm_posterior_walk_min_states(void);
int hmm_posterior_walk_max_states(void);
size_t hmm_posterior_walk_workspace_bytes(int k, int b, int L, int q);
int hmm_posterior_walk_pays(int k, int b, int L, int q);
int hmm_posterior_walk(const float *A, const float *pi, const float *E,
                       int k, int b, int L, int q, float eps, int mode,
                       float *out, double *loglik,
                       void *workspace, size_t workspace_bytes, void *stream);
size_t hmm_posterior_decode_wide_workspace_bytes(int k, int b, int L, int q);
int hmm_posterior_decode_wide(const float *A, const float *pi, const float *E,
                              int k, int b, int L, int q, float eps,
                              const int *state_class, int num_classes,
                              unsigned char *label, float *conf, double *loglik,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Viterbi state paths (max-plus scan).  The reference has none (only a docstring mention,
 * hmm_layer/MsaHmmCell.py:13, and the unused log_A_dense, :46-47); this entry point is what
 * a Viterbi over HmmCell's parameters needs: log A (k,q,q) (transitioner.make_log_A()),
 * log pi (k,q), log E (k,b,L,q) = log of cell.emission_probs() (clamped as the caller sees fit).
 * Scores are Q16 fixed point, Q(x) = rint(clip(x,-1024,1024)*65536), so the chunked scan is
 * bit-identical to the serial recursion; ties take the lowest state index (oracle/viterbi.py).
 *   path  (k,b,L) int32 : most probable state sequence
 *   score (k,b)   fp64  : its log-probability under the quantised model
 */
size_t hmm_viterbi_workspace_bytes(int k, int b, int L, int q);
int hmm_viterbi(const float *logA, const float *logpi, const float *logE,
                int k, int b, int L, int q,
                int32_t *path, double *score,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Viterbi for 1 <= q <= hmm_viterbi_large_max_states() (4096): the same arguments, layouts, error codes and
 * Q16 semantics as hmm_viterbi (bit-identical paths and scores wherever both run).  Two evaluations, chosen by
 * HMM_OPT_VLARGE (0: by q — the walk up to 128 states, tiles above; 1: walk, q <= 1024; 2: tiles):
 *   per-sequence walk   one workgroup per sequence, lane = state; a model whose states have at most 8
 *                       explicit predecessors (entries above the matrix minimum) is stepped sparsely, decided
 *                       per model on the device (HMM_OPT_FORCE_DENSE = 1 forces the all-candidates step);
 *   per-position tiles  one launch per position over the whole batch: rows = sequences, columns = destination
 *                       states, K = source states, integer max-plus with packed (value, index) keys.
 * Workspace: 2*k*b*L*q bytes of 16-bit backpointers plus O(k*b*q + k*q) (hmm_viterbi_large_workspace_bytes is
 * exactly what the call uses, whichever evaluation runs); every offset into logE, path and the backpointers is
 * 64-bit.  Runs on `stream` only, no host synchronisation, capturable into a HIP graph.
 */
int hmm_viterbi_large_max_states(void);
size_t hmm_viterbi_large_workspace_bytes(int k, int b, int L, int q);
int hmm_viterbi_large(const float *logA, const float *logpi, const float *logE,
                      int k, int b, int L, int q,
                      int32_t *path, double *score,
                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Time-parallel Viterbi for 1 <= q <= hmm_viterbi_scan_max_states() (64): the same arguments, layouts, error
 * codes and Q16 semantics as hmm_viterbi (bit-identical paths and scores wherever both run), evaluated by the
 * three-phase chunk scan with q x q max-plus operators in 32-state (q <= 32) or 64-state tiles: reduce (one wave
 * per chunk, lane = start state; a model whose states have at most 8 explicit predecessors is reduced over its
 * predecessors plus the one off-edge candidate, decided per model on the device, HMM_OPT_FORCE_DENSE = 1 forces
 * all q candidates), forward chunk scan, apply (the step of hmm_viterbi's walk from the true entering scores, one
 * backpointer byte per position and state), backward chunk scan, backtrace of every chunk in parallel.  Both
 * chunk scans run in two levels from 32 chunks per sequence on (HMM_OPT_SCAN2 = 0: one level); HMM_OPT_CHUNK
 * forces the chunk length.  It serves FEW LONG sequences: the reduce does about q times the work of the walk.
 *   hmm_viterbi_scan_chunk_len        chunk length the call would use (a multiple of 16, <= 512); 0 for an
 *                                     unsupported shape
 *   hmm_viterbi_scan_pays             1 where the measured rule prefers the scan to hmm_viterbi's
 *                                     walk, else 0; the host wrapper (engine.viterbi) routes by it
 *   hmm_viterbi_scan_workspace_bytes  exactly what the call uses: 64*k*b*L bytes of backpointers plus a QT x QT
 *                                     operator per chunk; 0 for an unsupported shape
 * Argument checks, before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), q > 64 (HMM_ERR_Q_UNSUPPORTED),
 * any NULL pointer (HMM_ERR_NULL_POINTER), workspace too small or not 256-byte aligned (HMM_ERR_WORKSPACE).
 * Every offset into logE, path and the backpointers is 64-bit.  Runs on `stream` only, no host synchronisation,
 * capturable into a HIP graph, deterministic.  hmm_viterbi itself never takes this path.
 */
int hmm_viterbi_scan_max_states(void);
int hmm_viterbi_scan_chunk_len(int k, int b, int L, int q);
int hmm_viterbi_scan_pays(int k, int b, int L, int q);
size_t hmm_viterbi_scan_workspace_bytes(int k, int b, int L, int q);
int hmm_viterbi_scan(const float *logA, const float *logpi, const float *logE,
                     int k, int b, int L, int q,
                     int32_t *path, double *score,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * Fused emission producer of the gene-prediction models.  Replaces GenePredHMMEmitter.forward
 * (hmm_layer/gene_pred_hmm_emitter.py:231-277, class part :93-121) and kmer.make_k_mers
 * (hmm_layer/kmer.py:3-47) for inference with one model:
 *   x           (b,L,s+5)  class probabilities followed by one-hot nucleotides A,C,G,T,N
 *   B           (rows,s)   softmax of the emission kernel (emitter.make_B())
 *   state_row   (q) int    kernel row feeding state j (intron parameter sharing, :115-116)
 *   codon       (2,nc,64)  left / right 3-mer tables (emitter.codon_probs, :198-217)
 *   state_codon (q) int    table row constraining state j, or -1 (free state: `free_value`, 1/4096)
 *   add                    added to the 3-mer factor (1e-7 when training, else 0, :260-261)
 *   n_mass                 1, or 2 to reproduce the reference's doubled N mass in right 3-mers
 *   E           (b,L,q)    emission probabilities, the engine's input.  16-byte aligned (so is dx of
 *                          hmm_gene_emissions_grad and _grad_wide): tiles of 16 positions are stored as aligned
 *                          16-byte pieces.
 * Limits: 1 <= q <= 64, 1 <= rows <= 32, 1 <= s <= 32, 0 <= nc <= 16 (hmm_gene_emissions_wide: 256 states and rows).
 * Table entries out of range never index out of a table.  For this function and hmm_gene_emissions_wide the values
 * below are pinned by tests (tests/test_emitter_sweep_gpu.py); the two backwards read state_row and state_codon
 * through the same two clamps (em_row, em_codon), so the same holds for them by construction:
 *   state_row[j] < 0 reads row 0 of B, state_row[j] >= rows reads row rows - 1;
 *   state_codon[j] < 0 (any negative value, not only -1) makes state j free;
 *   state_codon[j] >= nc reads table row nc - 1;
 *   nc = 0 makes every state free whatever state_codon holds, and codon may then be NULL.
 * The nucleotide columns need not be one-hot: a slot's distribution is its four base columns, plus 1/4 each (n_mass/4
 * in right 3-mers) where the N column is exactly 1; any other value of the N column counts for nothing.
 */
int hmm_gene_emissions(const float *x, int b, int L, int s, const float *B, int rows,
                       const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                       float free_value, float add, int n_mass, float *E, void *stream);

/*
 * Embedding-emission factor of the gene-prediction models (emit_embeddings=True): one diagonal multivariate
 * normal per emission-kernel row, evaluated at every position's embedding and multiplied into (or written as)
 * the emission tensor.  Replaces MvnMixture.log_pdf (hmm_layer/MvnMixture.py:125-149, diag_only, one component)
 * and the exp / product of SimpleGenePredHMMEmitter.forward (hmm_layer/gene_pred_hmm_emitter.py:101-112) for
 * inference with one model:
 *   emb         first embedding float of position 0; position p's d floats start at emb + p * ld (ld >= d).
 *               Read in place: the layer passes x + s with ld = s + d + 5.  Needs 4-byte alignment only.
 *   mean, inv_std (rows,d)  mu and 1 / sigma of every row
 *   log_norm    (rows)      -0.5 d log(2 pi) - sum_c log sigma[r][c]
 *   state_row   (q) int     kernel row feeding state j (entries outside 0..rows-1 are clamped)
 *   f[p][j] = exp(inv_temperature * (log_norm[r] - 0.5 sum_c ((x[p][c] - mean[r][c]) * inv_std[r][c])^2)) + add,
 *             r = state_row[j]
 *   E           (b,L,q)     multiply = 1: E[p][j] *= f[p][j] (read and written once); multiply = 0: E[p][j] = f[p][j]
 * The caller computes inv_std and log_norm from the parameter (in fp64, rounded once).
 * Limits: q <= 64, rows <= 32, d <= hmm_embedding_emissions_max_dim() (every d from 1 up).  Checked before any
 * HIP call, in this order: shape (HMM_ERR_BAD_SHAPE, includes ld < d), limits (HMM_ERR_Q_UNSUPPORTED), any NULL
 * pointer (HMM_ERR_NULL_POINTER), multiply not 0 or 1 (HMM_ERR_BAD_ARGUMENT).
 * Runs on `stream` only, no host synchronisation, no workspace, capturable into a HIP graph; deterministic
 * (no atomics, nothing depends on the grid); every offset into emb and E is 64-bit.
 */
int hmm_embedding_emissions_max_dim(void);
int hmm_embedding_emissions(const float *emb, long long ld, int b, int L, int d,
                            const float *mean, const float *inv_std /* (rows,d) each */,
                            const float *log_norm /* (rows) */,
                            int rows, const int *state_row, int q,
                            float inv_temperature, float add, int multiply,
                            float *E /* (b,L,q) */, void *stream);

/*
 * Backward of hmm_embedding_emissions: what autograd through the reference's ops (MvnMixture.log_pdf, exp, the
 * product with E) computes, from the inputs, the tables and the upstream gradient alone; nothing of size
 * b*L*rows*d is formed.  Arguments as for hmm_embedding_emissions, with g = f - add, r = row(j) = state_row[j]
 * clamped, and
 *   E_in        (b,L,q)     the tensor the forward multiplied into, or NULL for the multiply = 0 forward (E_in = 1)
 *   dE          (b,L,q)     upstream gradient dL/dE_out
 *   dE_in       (b,L,q)     or NULL: dE[p][j] * f[p][r].  Needs E_in; must not alias dE.
 *   demb                    or NULL: position p's d floats at demb + p * ldd (ldd >= d), so the caller can point it
 *                           at the embedding columns of an input-gradient tensor:
 *                           demb[p][c] = -sum_r W[p][r] (x[p][c] - mean[r][c]) inv_std[r][c]^2
 *   dmean, dinv_std (rows,d), dlog_norm (rows)   all three or none; written whole (the caller zeroes nothing):
 *                           dlog_norm[r]   = sum_p W[p][r]
 *                           dmean[r][c]    = sum_p W[p][r] (x[p][c] - mean[r][c]) inv_std[r][c]^2
 *                           dinv_std[r][c] = -sum_p W[p][r] (x[p][c] - mean[r][c])^2 inv_std[r][c]
 *   W[p][r] = inv_temperature * g[p][r] * sum_{j: row(j) = r} dE[p][j] E_in[p][j]   (ascending j; add has no gradient)
 * Everything is evaluated in the difference form ((x - mean) first), like the forward.  Reduction order of the
 * three table gradients: fp32 inside a workgroup (its positions in ascending order per position group, the
 * groups in group order), one partial per workgroup in the workspace, then the partials in workgroup order in
 * fp64, times inv_std^2 / -inv_std in fp64, rounded to fp32 once.  No atomics: repeated calls, and calls for any
 * subset of the outputs, are bit-identical.
 * Limits: q <= 64, rows <= 32, d <= hmm_embedding_emissions_grad_max_dim() (4096; every d from 1 up).  Checked
 * before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE, includes ld < d, and ldd < d with demb given),
 * limits (HMM_ERR_Q_UNSUPPORTED), pointers (HMM_ERR_NULL_POINTER: any input, the workspace, no output at all,
 * one or two of the three table gradients, dE_in without E_in), workspace (HMM_ERR_WORKSPACE: fewer than
 * hmm_embedding_emissions_grad_workspace_bytes bytes, or not 256-byte aligned).  The workspace holds W
 * (b*L x rows rounded up to 4 floats, passed between the two kernels) and at most 1024 workgroup partials of
 * rows * (2 d + 1) floats, at most 16 MiB of them (the grid shrinks as rows * d grows): the partials stop growing
 * with b*L.  The query returns 0 for an unsupported shape.  Runs on `stream` only, no host synchronisation,
 * capturable into a HIP graph; every offset into emb, demb, E_in, dE and dE_in is 64-bit.
 */
int hmm_embedding_emissions_grad_max_dim(void);
size_t hmm_embedding_emissions_grad_workspace_bytes(int b, int L, int d, int rows, int q);
int hmm_embedding_emissions_grad(const float *emb, long long ld, int b, int L, int d,
                                 const float *mean, const float *inv_std, const float *log_norm, int rows,
                                 const int *state_row, int q, float inv_temperature, float add,
                                 const float *E_in /* (b,L,q) or NULL */, const float *dE /* (b,L,q) */,
                                 float *dE_in /* (b,L,q) or NULL */,
                                 float *demb, long long ldd /* or NULL */,
                                 float *dmean, float *dinv_std /* (rows,d) */, float *dlog_norm /* (rows) */,
                                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward of hmm_gene_emissions: what autograd through GenePredHMMEmitter.forward
 * (hmm_layer/gene_pred_hmm_emitter.py:231-277, class part :93-121, kmer.make_k_mers hmm_layer/kmer.py:3-47)
 * computes for the class probabilities and for B, from x, the tables and the upstream gradient alone
 * (the 3-mer factor is recomputed; E is not an input).  Arguments as for hmm_gene_emissions, and
 *   dE          (b,L,q)    upstream gradient dL/dE
 *   dx          (b,L,s+5)  dL/dx, or NULL: class columns sum_j dE*(cod+add)*B[state_row[j]]; the five
 *                          nucleotide columns are written as 0 (one-hot nucleotides are data; autograd
 *                          through the reference's ops yields small non-zero values there)
 *   dB          (rows,s)   dL/dB, or NULL.  Written whole by the call: the caller does not zero it.
 * Limits as for the forward: q <= 64, s <= 32, rows <= 32, nc <= 16.  Checked before any HIP call, in this
 * order: shape (HMM_ERR_BAD_SHAPE), limits (HMM_ERR_Q_UNSUPPORTED), pointers (HMM_ERR_NULL_POINTER: any input,
 * the workspace, or both outputs NULL), workspace (HMM_ERR_WORKSPACE: fewer than
 * hmm_gene_emissions_grad_workspace_bytes bytes, or not 256-byte aligned).  The workspace holds one (rows,s)
 * partial of dB per workgroup; the grid depends on b*L only (at most 1024 workgroups), so the workspace stops
 * growing with b*L.  dB is summed in a fixed order (waves of a workgroup, states of a row, workgroups in fp64):
 * repeated calls give bit-identical results.  hmm_gene_emissions_grad_workspace_bytes returns 0 for an
 * unsupported shape.  Runs on `stream` only, no host synchronisation, capturable into a HIP graph.
 */
size_t hmm_gene_emissions_grad_workspace_bytes(int b, int L, int s, int rows, int q);
int hmm_gene_emissions_grad(const float *x, int b, int L, int s, const float *B, int rows,
                            const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                            float free_value, float add, int n_mass, const float *dE,
                            float *dx /* (b,L,s+5) or NULL */, float *dB /* (rows,s) or NULL */,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * hmm_gene_emissions and hmm_gene_emissions_grad for the gene models of three and more copies (1 + 14 c states:
 * 43, 57, 71 .. 253 for c = 3 .. 18).  Arguments, layouts, add / n_mass / free_value, the exact-zero nucleotide
 * columns of dx and "dB written whole" are exactly those of the two functions above; so are the values (the forward
 * runs the same class-sum chain: where both apply, the results are bit-identical).
 * Limits: 1 <= q <= hmm_gene_emissions_wide_max_states() (256), 1 <= rows <= 256, s <= 32, nc <= 16.  Entries of
 * state_row and state_codon out of range, and nc = 0, mean what they mean for hmm_gene_emissions (above).
 * Checked before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), limits (HMM_ERR_Q_UNSUPPORTED), pointers
 * (HMM_ERR_NULL_POINTER; for the grad: any input, the workspace, or both outputs NULL), workspace
 * (HMM_ERR_WORKSPACE: fewer than hmm_gene_emissions_grad_wide_workspace_bytes bytes, or not 256-byte aligned).
 * The workspace holds one (rows,s) partial of dB per workgroup: at most 1024 workgroups and at most 16 MiB of
 * partials (the grid shrinks as rows * s grows).  The query sizes it for that cap, so it does not depend on b*L, and
 * returns 0 for an unsupported shape.  dx is summed over the groups of 64 states in ascending group order; dB over
 * the waves of a workgroup in wave order, the states of a row in ascending state order, and the workgroups in
 * workgroup order in fp64, rounded once.  No atomics: repeated calls, and calls for one of the two outputs, are
 * bit-identical, and the forward does not depend on the grid.  Runs on `stream` only, no host synchronisation,
 * capturable into a HIP graph; every offset into x, E, dE and dx is 64-bit.
 */
int hmm_gene_emissions_wide_max_states(void);
int hmm_gene_emissions_wide(const float *x, int b, int L, int s, const float *B, int rows,
                            const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                            float free_value, float add, int n_mass, float *E, void *stream);
size_t hmm_gene_emissions_grad_wide_workspace_bytes(int b, int L, int s, int rows, int q);
int hmm_gene_emissions_grad_wide(const float *x, int b, int L, int s, const float *B, int rows,
                                 const int *state_row, const float *codon, int nc, const int *state_codon, int q,
                                 float free_value, float add, int n_mass, const float *dE,
                                 float *dx /* (b,L,s+5) or NULL */, float *dB /* (rows,s) or NULL */,
                                 void *workspace, size_t workspace_bytes, void *stream);

/*
 * hmm_embedding_emissions and hmm_embedding_emissions_grad for the gene models of three and more copies with
 * emit_embeddings=True (43 to 253 states; 37 kernel rows and more).  Arguments, layouts, formulas, multiply 0 / 1,
 * add, inv_temperature, the clamping of state_row entries outside 0..rows-1, ld / ldd (embeddings read in place,
 * demb written in place), the NULL-able arguments and "all three table gradients or none" are exactly those of the
 * two functions above.  Everything is evaluated in the difference form ((x - mean) first).
 * Limits: 1 <= q <= hmm_embedding_emissions_wide_max_states() (256), 1 <= rows <= 256,
 * 1 <= d <= hmm_embedding_emissions_max_dim() (4096; every d from 1 up).  Checked before any HIP call, in this
 * order: shape (HMM_ERR_BAD_SHAPE, includes ld < d, and ldd < d with demb given), limits (HMM_ERR_Q_UNSUPPORTED),
 * pointers (HMM_ERR_NULL_POINTER; for the grad: any input, the workspace, no output at all, one or two of the three
 * table gradients, dE_in without E_in), then multiply not 0 or 1 (forward, HMM_ERR_BAD_ARGUMENT) or the workspace
 * (grad, HMM_ERR_WORKSPACE: fewer than hmm_embedding_emissions_grad_wide_workspace_bytes bytes, or not 256-byte
 * aligned).
 * Forward: the rows are processed in blocks of 32 per tile of 256 positions; per (position, row) the sum over the d
 * columns runs in the order of hmm_embedding_emissions (slices of 16 columns in order, four partial sums per
 * slice), so wherever both functions accept a shape (q <= 64, rows <= 32) the outputs are bit-identical.  Nothing
 * depends on the grid.
 * Backward, reduction orders (all fixed by b*L, d, rows, q and the row map):
 *   Gf[p][r]   the states of row r in ascending state order, fp32;
 *   demb[p][c] the rows in ascending order, one fma each, fp32, negated once;
 *   tables     per block of 32 rows: fp32 inside a workgroup (workgroup x of X takes the tiles of 256 positions x,
 *              x + X, ...; the positions of a tile in ascending order per position group, the groups in group order),
 *              one partial per workgroup in the workspace, then the partials in workgroup order in fp64, times
 *              inv_std^2 / -inv_std in fp64, rounded to fp32 once.
 * No atomics: repeated calls, and calls for any subset of {dE_in, demb, tables}, are bit-identical.
 * The workspace holds W (b*L x rows rounded up to 4 floats) and X = min(tiles, 1024, 16 MiB / partial) workgroup
 * partials of rows * (2 d + 1) floats: at most 16 MiB of partials whatever b*L (the grid shrinks as rows * d grows).
 * The query returns 0 for an unsupported shape.  Both run on `stream` only, without host synchronisation, and are
 * capturable into a HIP graph; every offset into emb, demb, E, E_in, dE and dE_in is 64-bit.
 */
int hmm_embedding_emissions_wide_max_states(void);
int hmm_embedding_emissions_wide(const float *emb, long long ld, int b, int L, int d,
                                 const float *mean, const float *inv_std /* (rows,d) each */,
                                 const float *log_norm /* (rows) */,
                                 int rows, const int *state_row, int q,
                                 float inv_temperature, float add, int multiply,
                                 float *E /* (b,L,q) */, void *stream);
size_t hmm_embedding_emissions_grad_wide_workspace_bytes(int b, int L, int d, int rows, int q);
int hmm_embedding_emissions_grad_wide(const float *emb, long long ld, int b, int L, int d,
                                      const float *mean, const float *inv_std, const float *log_norm, int rows,
                                      const int *state_row, int q, float inv_temperature, float add,
                                      const float *E_in /* (b,L,q) or NULL */, const float *dE /* (b,L,q) */,
                                      float *dE_in /* (b,L,q) or NULL */,
                                      float *demb, long long ldd /* or NULL */,
                                      float *dmean, float *dinv_std /* (rows,d) */, float *dlog_norm /* (rows) */,
                                      void *workspace, size_t workspace_bytes, void *stream);

/*
 * Trainable nucleotide factor of the gene-prediction models (trainable_nucleotides_at_exons=True): a learned
 * 4-way nucleotide distribution on the exon states E0/E1/E2 of every copy, multiplied into (or written as) the
 * emission tensor.  Replaces the acgt einsum, the concatenation with the 1/4 columns and the product of
 * GenePredHMMEmitter.forward (hmm_layer/gene_pred_hmm_emitter.py:224-229, 265-272) for one model:
 *   nuc         first nucleotide float (A) of position 0; position p's five floats A,C,G,T,N start at nuc + p * ld
 *               (ld >= 5).  Read in place: the layer passes x + s (x + s + d with embeddings) with ld = the row
 *               width.  Needs 4-byte alignment only; nothing outside those five floats is read.
 *   P           (rows,4)    softmax of the nucleotide kernel (emitter.get_nucleotide_probs()[0])
 *   state_nuc   (q) int     row of P feeding state j, or < 0 for a free state (f = free_value, 1/4); entries
 *                           >= rows are clamped to rows - 1
 *   acgt[p][a] = nuc[p][a] + nuc[p][4] / 4    (plain arithmetic: no test for N == 1)
 *   f[p][j]    = state_nuc[j] >= 0 ? sum_a acgt[p][a] * P[state_nuc[j]][a] : free_value     (a = 0, 1, 2, 3 in order)
 *   E           (b,L,q)     multiply = 1: E[p][j] *= f[p][j] (read and written once); multiply = 0: E[p][j] = f[p][j]
 * Backward (hmm_nucleotide_emissions_grad), with dE (b,L,q) = dL/dE_out and E_in (b,L,q) the tensor the forward
 * multiplied into (NULL for the multiply = 0 forward: E_in = 1):
 *   dE_in       (b,L,q)     or NULL: dE[p][j] * f[p][j].  Must not alias dE.
 *   dP          (rows,4)    or NULL: sum_p acgt[p][a] * sum_{j: state_nuc[j] = r} dE[p][j] * E_in[p][j].  Written
 *                           whole (the caller zeroes nothing; a row no state points at is 0).
 * Nucleotides are data: there is no gradient for them.  There is no division anywhere, so an all-zero nucleotide
 * row (padding) gives f = 0 and finite gradients.  Reduction order of dP, fixed by b*L, q, rows and state_nuc
 * alone: workgroup x of X = min(tiles of 256 positions, 1024) takes tiles x, x + X, ...; inside it lane (g, j) —
 * state j, position group g of G = 256 / q — adds its positions (g, g + G, ... of every tile) in ascending order
 * in fp32, then element (r, a) of the workgroup's partial is the sum over the states j of row r in ascending
 * order, and per state over g in ascending order; the partials are added in workgroup order in fp64 and rounded
 * once.  No atomics: repeated calls, and calls for either output alone, are bit-identical; the forward does not
 * depend on the grid.
 * Limits: 1 <= q <= hmm_nucleotide_emissions_max_states() (256), 1 <= rows <= 256; one kernel serves every q
 * (E rows need 4-byte alignment only).  Checked before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE:
 * b, L, q or rows < 1, ld < 5), limits (HMM_ERR_Q_UNSUPPORTED), pointers (HMM_ERR_NULL_POINTER; for the grad: any
 * input, the workspace, or both outputs NULL), then multiply not 0 or 1 (forward, HMM_ERR_BAD_ARGUMENT) or the
 * workspace (grad, HMM_ERR_WORKSPACE: fewer than hmm_nucleotide_emissions_grad_workspace_bytes bytes, or not
 * 256-byte aligned).  The workspace holds the X partials of rows * 4 floats (at most 4 MiB): the query returns a
 * multiple of 256 that stops growing with b*L, and 0 for an unsupported shape.  Both run on `stream` only,
 * without host synchronisation, and are capturable into a HIP graph; every offset into nuc, E, E_in, dE and
 * dE_in is 64-bit.
 */
int hmm_nucleotide_emissions_max_states(void);
int hmm_nucleotide_emissions(const float *nuc, long long ld, int b, int L,
                             const float *P /* (rows,4) */, int rows,
                             const int *state_nuc /* (q) */, int q,
                             float free_value, int multiply,
                             float *E /* (b,L,q) */, void *stream);
size_t hmm_nucleotide_emissions_grad_workspace_bytes(int b, int L, int rows, int q);
int hmm_nucleotide_emissions_grad(const float *nuc, long long ld, int b, int L,
                                  const float *P, int rows, const int *state_nuc, int q, float free_value,
                                  const float *E_in /* (b,L,q) or NULL (= ones) */, const float *dE /* (b,L,q) */,
                                  float *dE_in /* (b,L,q) or NULL */, float *dP /* (rows,4) or NULL */,
                                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Per-kernel timing for the roofline report (bench.py): the same computation as
 * hmm_posterior with every kernel launch bracketed by HIP events recorded on `stream`.
 * hmm_profile_read() waits for the recorded events, returns the summed milliseconds and
 * the launch count per kernel (arrays of HMM_KERNEL_COUNT) and resets the profile.
 */
#define HMM_KERNEL_REDUCE   0   /* chunk operators (MFMA matrix-product chain) */
#define HMM_KERNEL_SCAN     1   /* chunk-level prefix / suffix                 */
#define HMM_KERNEL_FORWARD  2   /* in-chunk forward pass, checkpoints          */
#define HMM_KERNEL_BACKWARD 3   /* in-chunk backward pass, posteriors          */
#define HMM_KERNEL_EXACT    4   /* routing + serial exact-clamp kernels (empty launches when nothing is routed) */
#define HMM_KERNEL_COUNT    5
void *hmm_profile_create(void);
void hmm_profile_destroy(void *profile);
int hmm_posterior_profiled(const float *A, const float *pi, const float *E,
                           int k, int b, int L, int q, float eps, int mode,
                           float *out, double *loglik,
                           void *workspace, size_t workspace_bytes, void *stream, void *profile);
int hmm_profile_read(void *profile, double *ms, long long *launches);

/*
 * Weighted log-likelihood aggregate.  Replaces MsaHmmLayer.apply_sequence_weights with
 * aggregate=True (hmm_layer/MsaHMMLayer.py:155-164): for each model the pair
 * (sum_b w*loglik, sum_b w) in fp64.  `weights` (k,b) fp32 or NULL (= ones).
 *   partial (k,2) fp64 device.  The cross-GPU step is one all-reduce(sum) of `partial`
 *   (done by the host wrapper over RCCL); mean over models follows on the host.
 */
int hmm_loglik_partials(const double *loglik, const float *weights, int k, int b,
                        double *partial, void *stream);

/*
 * The cross-GPU step of the same aggregate for hosts that do not have torch.distributed:
 * in-place all-reduce(sum) of `partial` (k,2) fp64 over `comm`, an ncclComm_t (RCCL) the HOST
 * created for its ranks, enqueued on `stream`.  The engine does not link RCCL: it calls the
 * ncclAllReduce of the RCCL library already loaded in the process (HMM_ERR_NO_RCCL if there is
 * none).  Afterwards every rank holds (sum over all ranks' sequences of w*loglik, sum of w) per
 * model; the weighted mean and the mean over models are the host's two divisions
 * (hmm_layer/MsaHMMLayer.py:160-164).
 */
int hmm_loglik_allreduce(void *comm, double *partial, int k, void *stream);

/*
 * Sequence-sharded posteriors: every rank owns one contiguous TIME slab of every sequence
 * (E_slab (k,b,Ls,q), Ls may differ between ranks) — for batches too small to be cut across GPUs.
 * The roles of TotalProbabilityCell.forward (hmm_layer/TotalProbabilityCell.py:30-49) and
 * _get_total_forward/backward_from_chunks (hmm_layer/MsaHMMLayer.py:285-319, 384-419) lifted across
 * devices.  q <= hmm_scan_max_states().  Protocol, R ranks, rank r (slabs in time order):
 *   1. hmm_seqshard_reduce(...)    -> slab_op (k,b,16,16) fp32, slab_exp (k,b,16) int32: the slab's
 *                                     operator per sequence (column n scaled by 2^-exp[n])
 *   2. host: all-gather slab_op / slab_exp over the ranks and lay them out (k,b,R,16,16) / (k,b,R,16); all_ops
 *      16-byte aligned
 *   3. hmm_seqshard_posterior(...) -> out (k,b,Ls,q) per `mode`, loglik (k,b) = the WHOLE sequence's,
 *                                     phi_out (k,b) fp32 or NULL: this slab's share of the sequence's
 *                                     floor-transition bound (see hmm_posterior; +inf when A's support is
 *                                     not primitive).  The host sums phi over ranks; above 1e-6 the
 *                                     sequence needs the unsharded call (serial exact-clamp kernels).
 * seq_start: 1 on the rank that owns position 0 (r == 0), else 0.  The same workspace (same size query)
 * must be passed to steps 1 and 3: the chunk operators stay in it.
 * Only the leading q x q block of an operator and the first q entries of its exponent row are defined
 * (the other rows and columns of the block are zero; the other exponent lanes carry no contract).
 *
 * hmm_seqshard_workspace_bytes: a multiple of 256, non-decreasing in R; 0 for q > hmm_scan_max_states(),
 * for R < 1 and for a bad shape.
 * Argument checks of hmm_seqshard_reduce and hmm_seqshard_posterior, in this order, all before any HIP
 * call (tests/test_seqshard_sweep_cpu.py):
 *   1. q > hmm_scan_max_states()                     HMM_ERR_Q_UNSUPPORTED (-2), ahead of everything, a
 *                                                    bad shape included
 *   2. R < 1                                         HMM_ERR_BAD_ARGUMENT  (-6)
 *   3. k, b, Ls or q < 1 (or k * b > 2^24)           HMM_ERR_BAD_SHAPE     (-1)
 *   4. hmm_seqshard_posterior only: r outside 0 .. R-1, or (seq_start != 0) != (r == 0), then a mode
 *      outside HMM_POST_PROB .. HMM_POST_LOG_NO_LL   HMM_ERR_BAD_ARGUMENT  (-6)
 *   5. a NULL pointer among A, E, slab_op, slab_exp, workspace (reduce) or A, pi, E, all_ops, all_exps,
 *      out, workspace (posterior; loglik and phi_out may be NULL)
 *                                                    HMM_ERR_NULL_POINTER  (-3)
 *   6. workspace_bytes below the size query, or a workspace not aligned to 256 bytes
 *                                                    HMM_ERR_WORKSPACE     (-4)
 */
size_t hmm_seqshard_workspace_bytes(int k, int b, int Ls, int q, int R);
int hmm_seqshard_reduce(const float *A, const float *E, int k, int b, int Ls, int q, float eps, int seq_start,
                        int R, float *slab_op, int *slab_exp,
                        void *workspace, size_t workspace_bytes, void *stream);
int hmm_seqshard_posterior(const float *A, const float *pi, const float *E, int k, int b, int Ls, int q, float eps,
                           int seq_start, const float *all_ops, const int *all_exps, int R, int r, int mode,
                           float *out, double *loglik, float *phi_out,
                           void *workspace, size_t workspace_bytes, void *stream);

/*
 * Sequence-sharded Viterbi: the same cut — every rank owns one contiguous TIME slab of every sequence, logE_slab
 * (k,b,Ls,q) log-probabilities, Ls may differ between ranks — for the most probable path.  Semantics are exactly
 * hmm_viterbi's (Q(x) = rint(clip(x, -1024, 1024) * 65536), lowest-index tie-breaks, entries equal to the matrix
 * minimum are absent edges), and so are the results, bit for bit: integer max-plus is exactly associative.
 * q <= hmm_seqshard_viterbi_max_states() (16 = hmm_scan_max_states()).  Protocol, R ranks, rank r (slabs in time
 * order, rank r owns positions [t_r, t_{r+1})):
 *   1. hmm_seqshard_viterbi_reduce(...) -> slab_vop (k,b,16,16) int32, slab_vbase (k,b,16) int64: the slab's operator
 *                                          per sequence.  slab_vop[j][i] + slab_vbase[i] (i, j < q) is the best Q16
 *                                          score of any path that is in state i at the position before the slab and in
 *                                          state j at the slab's last position, the transition into the slab's first
 *                                          position and all the slab's emissions included; every column i has
 *                                          maximum 0.  With seq_start = 1 every column holds the same vector, the
 *                                          maximum over paths from Q(log pi).  Rows and columns from q on are 0.
 *   2. host: all-gather slab_vop / slab_vbase over the ranks, laid out (k,b,R,16,16) / (k,b,R,16); all_vops 16-byte
 *      aligned
 *   3. hmm_seqshard_viterbi_apply(...)  -> slab_origin (k,b,16) bytes: slab_origin[j] = the state at the position
 *                                          before the slab of the best path into state j at the slab's last position
 *                                          (all 0 for seq_start = 1, never read); final_state (k,b), score (k,b): the
 *                                          WHOLE sequence's lowest-index best last state and its score, the same
 *                                          integers on every rank.  The backpointers stay in the workspace.
 *   4. host: all-gather slab_origin, laid out (k,b,R,16)
 *   5. hmm_seqshard_viterbi_path(...)   -> path (k,b,Ls) int32: this slab's piece of the most probable path
 * seq_start: 1 on the rank that owns position 0 (r == 0), else 0.  logA (k,q,q), logpi (k,q) as for hmm_viterbi, the
 * same on every rank and in steps 1 and 3.  The same workspace, from the same size query, must be passed to steps
 * 1, 3 and 5 with nothing else written to it in between: it holds ALL k models' chunk operators, entering scores,
 * maps and backpointers (8 bytes per position and sequence).  HMM_OPT_FORCE_DENSE, HMM_OPT_CHUNK and HMM_OPT_SCAN2
 * act as for hmm_viterbi and must not change between the steps.  Everything runs in order on `stream` (no helper
 * streams, no batch groups), without host synchronisation: the calls are capturable into a HIP graph.
 *
 * hmm_seqshard_viterbi_workspace_bytes: a multiple of 256, non-decreasing in R; 0 for q > 16, R < 1 or a bad shape.
 * Argument checks, in this order, all before any HIP call:
 *   1. q > hmm_seqshard_viterbi_max_states()         HMM_ERR_Q_UNSUPPORTED (-2), ahead of everything
 *   2. R < 1                                         HMM_ERR_BAD_ARGUMENT  (-6)
 *   3. k, b, Ls or q < 1 (or k * b > 2^24)           HMM_ERR_BAD_SHAPE     (-1)
 *   4. apply / path: r outside 0 .. R-1; apply: (seq_start != 0) != (r == 0)
 *                                                    HMM_ERR_BAD_ARGUMENT  (-6)
 *   5. a NULL pointer among the arguments            HMM_ERR_NULL_POINTER  (-3)
 *   6. workspace_bytes below the size query, or a workspace not aligned to 256 bytes
 *                                                    HMM_ERR_WORKSPACE     (-4)
 */
int hmm_seqshard_viterbi_max_states(void);
size_t hmm_seqshard_viterbi_workspace_bytes(int k, int b, int Ls, int q, int R);
int hmm_seqshard_viterbi_reduce(const float *logA, const float *logpi, const float *logE_slab,
                                int k, int b, int Ls, int q, int seq_start, int R,
                                int *slab_vop, long long *slab_vbase,
                                void *workspace, size_t workspace_bytes, void *stream);
int hmm_seqshard_viterbi_apply(const float *logA, const float *logpi, const float *logE_slab,
                               int k, int b, int Ls, int q, int seq_start,
                               const int *all_vops, const long long *all_vbases, int R, int r,
                               unsigned char *slab_origin, int *final_state, double *score,
                               void *workspace, size_t workspace_bytes, void *stream);
int hmm_seqshard_viterbi_path(int k, int b, int Ls, int q,
                              const unsigned char *all_origins, const int *final_state, int R, int r,
                              int32_t *path,
                              void *workspace, size_t workspace_bytes, void *stream);

/*
 * Sequence-sharded Viterbi for up to 64 states: the protocol of hmm_seqshard_viterbi_* with hmm_viterbi_scan's q x q
 * max-plus operators in tiles of QT = hmm_seqshard_vscan_tile(q) = 32 (q <= 32) or 64 states; every q from 1 to
 * hmm_seqshard_vscan_max_states() (64) is served.  Semantics and results are hmm_viterbi's, bit for bit.  R ranks,
 * rank r owns positions [t_r, t_{r+1}) of every sequence, logE_slab (k,b,Ls,q), Ls may differ between ranks:
 *   1. hmm_seqshard_vscan_reduce(...) -> slab_vop (k,b,QT,QT) int32, slab_vbase (k,b,QT) int64: the slab's operator per
 *                                        sequence.  slab_vop[j][i] + slab_vbase[i] (i, j < q) is the best Q16 score of
 *                                        any path that is in state i at the position before the slab and in state j at
 *                                        the slab's last position, the transition into the slab's first position and
 *                                        all the slab's emissions included; every column i < q has maximum 0.  With
 *                                        seq_start = 1 every column holds the same vector, the maximum over paths from
 *                                        Q(log pi).  Only the leading q x q block and the first q bases are defined;
 *                                        the padding is written on every call: -2^30 in the rows and columns of slab_vop
 *                                        from q on, 0 in the bases from q on.
 *   2. host: all-gather slab_vop / slab_vbase over the ranks, laid out (k,b,R,QT,QT) / (k,b,R,QT); all_vops 16-byte
 *      aligned (the hops read the operators' rows as aligned 16-byte pieces)
 *   3. hmm_seqshard_vscan_apply(...)  -> slab_origin (k,b,QT) bytes: slab_origin[j] = the state at the position before
 *                                        the slab of the best path into state j at the slab's last position (all 0 for
 *                                        seq_start = 1, never read then; 0 from q on); final_state (k,b), score (k,b):
 *                                        the WHOLE sequence's lowest-index best last state and its score, the same
 *                                        integers on every rank.  The backpointers stay in the workspace.
 *   4. host: all-gather slab_origin, laid out (k,b,R,QT)
 *   5. hmm_seqshard_vscan_path(...)   -> path (k,b,Ls) int32: this slab's piece of the most probable path
 * seq_start: 1 on the rank that owns position 0 (r == 0), else 0.  logA (k,q,q), logpi (k,q) as for hmm_viterbi, the
 * same on every rank and in steps 1 and 3.  The same workspace, from the same size query, must be passed to steps
 * 1, 3 and 5 with nothing else written to it in between: it holds ALL k models' chunk operators, entering scores,
 * maps and backpointers (64 bytes per position and sequence).  HMM_OPT_FORCE_DENSE, HMM_OPT_CHUNK and HMM_OPT_SCAN2
 * act as for hmm_viterbi_scan and must not change between the steps.  Everything runs in order on `stream`, without
 * host synchronisation: the calls are capturable into a HIP graph.  Every offset into logE_slab, path and the
 * backpointers is 64-bit.
 *
 * hmm_seqshard_vscan_workspace_bytes: a multiple of 256, non-decreasing in R; 0 for q > 64, R < 1 or a bad shape.
 * hmm_seqshard_vscan_tile: 32 or 64; 0 for q < 1 or q > 64.
 * Argument checks, in this order, all before any HIP call:
 *   1. q > hmm_seqshard_vscan_max_states()           HMM_ERR_Q_UNSUPPORTED (-2), ahead of everything
 *   2. R < 1                                         HMM_ERR_BAD_ARGUMENT  (-6)
 *   3. k, b, Ls or q < 1, k * b > 2^24, or more than 2^31 - 1 chunks
 *                                                    HMM_ERR_BAD_SHAPE     (-1)
 *   4. apply / path: r outside 0 .. R-1; apply: (seq_start != 0) != (r == 0)
 *                                                    HMM_ERR_BAD_ARGUMENT  (-6)
 *   5. a NULL pointer among the arguments            HMM_ERR_NULL_POINTER  (-3)
 *   6. workspace_bytes below the size query, or a workspace not aligned to 256 bytes
 *                                                    HMM_ERR_WORKSPACE     (-4)
 */
int hmm_seqshard_vscan_max_states(void);
int hmm_seqshard_vscan_tile(int q);
size_t hmm_seqshard_vscan_workspace_bytes(int k, int b, int Ls, int q, int R);
int hmm_seqshard_vscan_reduce(const float *logA, const float *logpi, const float *logE_slab,
                              int k, int b, int Ls, int q, int seq_start, int R,
                              int *slab_vop, long long *slab_vbase,
                              void *workspace, size_t workspace_bytes, void *stream);
int hmm_seqshard_vscan_apply(const float *logA, const float *logpi, const float *logE_slab,
                             int k, int b, int Ls, int q, int seq_start,
                             const int *all_vops, const long long *all_vbases, int R, int r,
                             unsigned char *slab_origin, int *final_state, double *score,
                             void *workspace, size_t workspace_bytes, void *stream);
int hmm_seqshard_vscan_path(int k, int b, int Ls, int q,
                            const unsigned char *all_origins, const int *final_state, int R, int r,
                            int32_t *path,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Sequence-sharded posteriors for 17 to 64 states: the protocol of hmm_seqshard_reduce / hmm_seqshard_posterior on
 * the chunked scan that serves hmm_posterior in this range, with operators in tiles of QT = hmm_seqshard_mid_tile(q)
 * = 32 (17..32 states) or 64 (33..64).  Every rank owns one contiguous TIME slab of every sequence, E_slab
 * (k,b,Ls,q), Ls may differ between ranks.  R ranks, rank r (slabs in time order):
 *   1. hmm_seqshard_mid_reduce(...)    -> slab_op (k,b,QT,QT) fp32, slab_exp (k,b,QT) int32: the slab's operator per
 *                                         sequence.  slab_op[i][k] * 2^slab_exp[k] (i, k < q) is the product of the
 *                                         slab's step matrices: i the state at the slab's last position, k the state
 *                                         before the slab (with seq_start = 1 the first position takes no
 *                                         transition).  Every column k < q sums to a value in [0.5, 1), or is all
 *                                         zero.  The padding is written on every call: 0 in the rows and columns of
 *                                         slab_op from q on and in slab_exp from q on.  Never NaN or inf.
 *   2. host: all-gather slab_op / slab_exp over the ranks and lay them out (k,b,R,QT,QT) / (k,b,R,QT); all_ops
 *      16-byte aligned (the hops read the operators' rows as aligned 16-byte pieces)
 *   3. hmm_seqshard_mid_posterior(...) -> out (k,b,Ls,q) per `mode` (HMM_POST_*), loglik (k,b) or NULL = the WHOLE
 *                                         sequence's, the same bits on every rank, phi_out (k,b) fp32 or NULL: this
 *                                         slab's share of the sequence's floor-transition bound (psi of hmm_posterior
 *                                         summed over the slab's chunks, plus 1 for every chunk whose reduce left its
 *                                         mark: operator columns through the denormal range, or an observation that
 *                                         every state survives at the emission floor only; +inf when A's support is
 *                                         not primitive).  The host sums phi over ranks; above 2e-6 the sequence needs
 *                                         the unsharded call (the serial kernels cannot be cut in time).
 * seq_start: 1 on the rank that owns position 0 (r == 0), else 0.  The same workspace (same size query) must be passed
 * to steps 1 and 3 with nothing else written to it in between: the chunk operators and the model verdicts stay in it.
 * The range served is 17 <= q <= 64 (hmm_seqshard_mid_max_states() = 64; up to 16 states: hmm_seqshard_*), every
 * k * b <= 2^24 and every Ls >= 1: hmm_posterior's routing rules for 33..64 states (at most 96 sequences, at least 256
 * positions) do not apply here.  HMM_OPT_CHUNK and HMM_OPT_FORCE_DENSE act as for hmm_posterior and must not change
 * between the steps; HMM_OPT_EXACT is ignored: these calls always run the scan.  Everything runs in order on
 * `stream`, without host synchronisation: the calls are capturable into a HIP graph.
 *
 * hmm_seqshard_mid_workspace_bytes: a multiple of 256, non-decreasing in R; 0 for q outside 17..64, R < 1 or a bad
 * shape.  hmm_seqshard_mid_tile: 32 or 64; 0 for q outside 17..64.
 * Argument checks, in this order, all before any HIP call:
 *   1. q > 64, or q < 17                             HMM_ERR_Q_UNSUPPORTED (-2), ahead of everything
 *   2. R < 1                                         HMM_ERR_BAD_ARGUMENT  (-6)
 *   3. k, b or Ls < 1, or k * b > 2^24               HMM_ERR_BAD_SHAPE     (-1)
 *   4. hmm_seqshard_mid_posterior only: r outside 0 .. R-1, or (seq_start != 0) != (r == 0), then a mode outside
 *      HMM_POST_PROB .. HMM_POST_LOG_NO_LL           HMM_ERR_BAD_ARGUMENT  (-6)
 *   5. a NULL pointer among A, E, slab_op, slab_exp, workspace (reduce) or A, pi, E, all_ops, all_exps, out,
 *      workspace (posterior; loglik and phi_out may be NULL)
 *                                                    HMM_ERR_NULL_POINTER  (-3)
 *   6. workspace_bytes below the size query, or a workspace not aligned to 256 bytes
 *                                                    HMM_ERR_WORKSPACE     (-4)
 */
int hmm_seqshard_mid_max_states(void);
int hmm_seqshard_mid_tile(int q);
size_t hmm_seqshard_mid_workspace_bytes(int k, int b, int Ls, int q, int R);
int hmm_seqshard_mid_reduce(const float *A, const float *E_slab, int k, int b, int Ls, int q, float eps, int seq_start,
                            int R, float *slab_op, int *slab_exp,
                            void *workspace, size_t workspace_bytes, void *stream);
int hmm_seqshard_mid_posterior(const float *A, const float *pi, const float *E_slab, int k, int b, int Ls, int q,
                               float eps, int seq_start, const float *all_ops, const int *all_exps, int R, int r,
                               int mode, float *out, double *loglik, float *phi_out,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gradient of the log-likelihoods (training).  The reference trains by autograd through the
 * Python time loop (hmm_layer/BaseRNN.py:217-227 over HmmCell.forward,
 * hmm_layer/MsaHmmCell.py:73-106); this entry point returns the same derivatives from one
 * forward-backward pass (Baum-Welch expectations), for q <= hmm_grad_max_states():
 *   grad_loglik (k,b) fp32 or NULL (= ones): d loss / d loglik[m][s], the upstream gradient
 *   dA  (k,q,q) : sum_s grad_loglik * d loglik / d A    (= sum_t xi_t(i,j) / A[i][j], dense)
 *   dpi (k,q)   : sum_s grad_loglik * d loglik / d pi   (= sum_s grad_loglik * gamma_0 / pi, whatever E_0 is: a
 *                 sequence whose first emissions are clamped still contributes its gamma_0)
 *   dE  (k,b,L,q): grad_loglik * gamma / E; zero where the cell clamps E below eps
 *   loglik (k,b) fp64 or NULL
 * Entries of E / pi that the cell clamps to eps receive no gradient (torch.maximum semantics).
 * Sums over sequences and time run in a fixed order (fp32 per 16-chain tile, fp64 across tiles):
 * results are deterministic.
 */
size_t hmm_loglik_grad_workspace_bytes(int k, int b, int L, int q);
/* 17..64 states: how many sequences of the last call with this shape the whole-sequence sweeps served (all of
 * them, except for the compiled 29-state two-copy topology on up to 512 sequences, which is computed per chunk of
 * the 32-state scan plan under the routing of hmm_posterior); q <= 16: hmm_exact_count of that call. */
long long hmm_loglik_grad_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
int hmm_loglik_grad(const float *A, const float *pi, const float *E,
                    int k, int b, int L, int q, float eps, const float *grad_loglik,
                    float *dA, float *dpi, float *dE, double *loglik,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same gradient, per chunk of the scan plan, for 1 <= q <= hmm_loglik_grad_scan_max_states() (64): arguments,
 * outputs, clamp semantics and NULL-ability exactly those of hmm_loglik_grad (grad_loglik and loglik may be NULL).
 * hmm_loglik_grad itself evaluates 17..64 states per chunk only for the compiled 29-state topology; every other
 * model of that range walks two whole-sequence sweeps, one wave per sequence.  This entry point is the explicit
 * request to run ANY primitive model of 17..64 states per chunk: the dense reduce and chunk scan of its row width
 * (32 lanes for 17..32 states, 64 for 33..64), the value sweeps, then every chunk sums its own share of dE, dA and
 * the certificate.  Models whose support is not primitive, sequences over the floor-transition certificate
 * (F = eps * sum_t 1 / Sg_t > 2e-6) and sequences a reduce marked are redone by the masked whole-sequence sweeps
 * inside the same call, bit-identical to hmm_loglik_grad's sweeps.  q <= 16 forwards to hmm_loglik_grad (call,
 * workspace query and serial count alike).
 *   hmm_loglik_grad_scan_chunk_len        the chunk length the call would use (a multiple of 16, <= 512; HMM_OPT_CHUNK
 *                                         forces it); 0 for an unsupported shape
 *   hmm_loglik_grad_scan_pays             1 where the measured rule prefers this call to
 *                                         hmm_loglik_grad; 0 for q <= 16, where hmm_loglik_grad already runs per
 *                                         chunk, below 4 chunks, and for every shape the call would refuse
 *   hmm_loglik_grad_scan_workspace_bytes  exactly what the call uses, in 64-bit sizes (the two value arrays of
 *                                         k*b*L*q floats and more); 0 for an unsupported shape
 *   hmm_loglik_grad_scan_serial_count     how many sequences of the LAST call with this shape the whole-sequence
 *                                         sweeps served (synchronous copy from the workspace)
 * Unsupported: L * q * 4 >= 2^31 - 4096 (the kernels' 32-bit row offsets) and k * b > 2^24: HMM_ERR_BAD_SHAPE.
 * Options: HMM_OPT_CHUNK, HMM_OPT_EXACT and HMM_OPT_FORCE_DENSE act as for hmm_posterior's 17..64-state plans;
 * HMM_OPT_PGCHUNK = 2 serves every sequence of an eligible model per chunk, without certificate and marks (tests).
 * Runs on `stream` only, no host synchronisation, capturable into a HIP graph; fixed summation orders (fp32
 * inside a chunk, fp64 across chunks and sequences): repeated calls are bit-identical.
 * Argument checks, before any HIP call and in this order: bad shape -1, q > 64 -2, a NULL A / pi / E / dA / dpi /
 * dE / workspace -3, a small or misaligned (256 bytes) workspace -4.
 */
int hmm_loglik_grad_scan_max_states(void);
int hmm_loglik_grad_scan_chunk_len(int k, int b, int L, int q);
int hmm_loglik_grad_scan_pays(int k, int b, int L, int q);
size_t hmm_loglik_grad_scan_workspace_bytes(int k, int b, int L, int q);
long long hmm_loglik_grad_scan_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
int hmm_loglik_grad_scan(const float *A, const float *pi, const float *E,
                         int k, int b, int L, int q, float eps, const float *grad_loglik,
                         float *dA, float *dpi, float *dE, double *loglik,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same gradient for any 1 <= q <= hmm_loglik_grad_large_max_states() (4096): arguments, outputs and
 * clamp semantics exactly those of hmm_loglik_grad (grad_loglik and loglik may be NULL).  Two evaluations,
 * picked by HMM_OPT_GLARGE (0: by q — the walk up to 128 states, the GEMMs above; 1: walk; 2: GEMMs):
 *   walk   one workgroup per sequence, ceil(q/64) waves, lane = state, A staged in LDS; a forward sweep parks
 *          the unnormalised forward vector (sign bit = the predicted state was clamped) in dE, the backward
 *          sweep overwrites it with w gamma / E and sums row i of xi / A in lane i.  Serves q <= 128: forcing it
 *          above returns HMM_ERR_BAD_ARGUMENT.
 *   GEMMs  per position one f32-MFMA GEMM of the forward recursion, one of the adjoint recursion with an
 *          elementwise pass for dE, and one (q x b)(b x q) product for dA, added into an fp64 accumulator.
 * Under both, position 0 keeps w gamma_0 / eps in its clamped entries of dE until dpi has been summed from that
 * row; they are zeroed afterwards, so dE is 0 wherever E <= eps and dpi loses nothing.
 * The workspace does not depend on L.  Sums run in a fixed order (fp32 within a sequence or a tile, fp64 across
 * sequences and positions): repeated calls return bit-identical results.  Everything runs in order on `stream`.
 * Argument checks, before any HIP call: bad shape -1, q > 4096 -2, a NULL A / pi / E / dA / dpi / dE / workspace
 * -3, a small or misaligned (256 bytes) workspace -4.  workspace_bytes() returns 0 for an unsupported q.
 */
int hmm_loglik_grad_large_max_states(void);
size_t hmm_loglik_grad_large_workspace_bytes(int k, int b, int L, int q);
int hmm_loglik_grad_large(const float *A, const float *pi, const float *E,
                          int k, int b, int L, int q, float eps, const float *grad_loglik,
                          float *dA, float *dpi, float *dE, double *loglik,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * Log-likelihoods and their gradient for hmm_loglik_grad_walk_min_states() (65) <= q <=
 * hmm_loglik_grad_walk_max_states() (256) states by a PER-SEQUENCE WALK WITH THE SPARSE STEP (hmm_gradwq.inc): the
 * training counterpart of hmm_posterior_walk for the gene models of 5 to 18 copies.  One workgroup per sequence,
 * lane = state, two launches (forward sweep, backward sweep), the step of hmm_posterior_walk's sparse form: every
 * state has at most 8 non-zero predecessors and successors except at most two hub states, decided per model on the
 * device.  Derivatives and clamp handling are exactly those of hmm_loglik_grad_large (position 0 included), with
 * ONE DIFFERENCE IN dA: every entry with A[i][j] == 0 is written as an exact 0, where hmm_loglik_grad* return the
 * derivative that autograd through a dense A would give.  Every entry with A[i][j] != 0 gets the same derivative
 * as there.  A transition matrix scattered from per-edge parameters never reads the absent entries.
 *   grad_loglik  (k,b) or NULL (= ones).
 *   dA, dpi, dE  all three, or all three NULL: then the call is the LOG-LIKELIHOOD ALONE (forward sweep only, no
 *                write to any gradient) and loglik is required.  loglik is bit for bit the same in both forms.
 *   loglik       (k,b) fp64 or NULL (with gradients).
 * A MODEL OUTSIDE THE SPARSE RULE (more than two states above degree 8) IS REFUSED ON THE DEVICE: every element of
 * its dA, dpi, dE rows and loglik is NaN, the other models of the call are served, and
 * hmm_loglik_grad_walk_refused(k, b, L, q, workspace, workspace_bytes) copies from the FINISHED call's workspace how
 * many of the k models were refused (it synchronises; negative: an HMM_ERR_* code).  HMM_OPT_FORCE_DENSE does not
 * act on this call.
 * Workspace: hmm_loglik_grad_walk_workspace_bytes (0: unsupported shape or q); it does not grow with L.  Sums run
 * in a fixed order (fp32 within a sequence, fp64 across sequences, normaliser logs in fp64): repeated calls return
 * bit-identical results.  Everything runs in order on `stream`, without host synchronisation: capturable.
 * Argument checks, before any HIP call and in this order: bad shape -1; q < 65 or q > 256 -2; a NULL A / pi / E /
 * workspace, one or two of dA / dpi / dE, or neither gradients nor loglik -3; a small or misaligned (256 bytes)
 * workspace -4.
 * hmm_loglik_grad_walk_pays(k, b, L, q): 1 only where tools/experiments/loglik_grad_walk_time.py measured this call
 * at least 1.25x faster than hmm_loglik_grad_large at its default route; 0 elsewhere, outside the range and wherever
 * nothing was measured.
 */
int hmm_loglik_grad_walk_min_states(void);
int hmm_loglik_grad_walk_max_states(void);
size_t hmm_loglik_grad_walk_workspace_bytes(int k, int b, int L, int q);
int hmm_loglik_grad_walk_pays(int k, int b, int L, int q);
long long hmm_loglik_grad_walk_refused(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
int hmm_loglik_grad_walk(const float *A, const float *pi, const float *E,
                         int k, int b, int L, int q, float eps, const float *grad_loglik,
                         float *dA, float *dpi, float *dE, double *loglik,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * Gradient of a loss on the state posteriors (training through state_posterior_log_probs).  The
 * reference differentiates _state_posterior_log_probs_impl by autograd through its Python loops
 * (hmm_layer/MsaHMMLayer.py:422-521 called with training=True, tests/parallel_rnn_forward.py:70-80);
 * this is that reverse-mode computation as four sweeps per sequence (two value sweeps, two adjoint
 * sweeps; lane = state), for q <= hmm_posterior_grad_max_states() (64):
 *   mode      HMM_POST_PROB (out = gamma) or HMM_POST_LOG (out = log gamma)
 *   grad_out  (k,b,L,q) : d loss / d out
 *   dA (k,q,q), dpi (k,q), dE (k,b,L,q) : d loss / d A, pi, E; clamped entries receive nothing
 * Deterministic (fixed summation order).  q = 1: the posterior is identically 1 and every gradient exactly zero; the
 * call returns zeros without running a sweep (hmm_posterior_grad_serial_count then reports k * b), also for
 * non-finite inputs, which the sweeps of q >= 2 propagate as NaN.
 *
 * For q <= 16 and up to 4096 sequences the sweeps run per chunk of the scan plan, in parallel (the
 * adjoint recursions are affine in the adjoint vector: every chunk's map is measured, the maps are
 * scanned, the sweeps rerun from the true entering vectors; HMM_OPT_PGCHUNK).  Which sequences that
 * path may serve is decided on the device as for hmm_posterior — per model by the support of A, per
 * sequence by the floor-transition bound F = eps * sum_t 1 / <alpha_hat_t, R_t> <= 2e-6 — and in log
 * mode additionally by how much of the upstream gradient sits on states whose posterior is so small
 * that floor paths can matter for THEM: sum |G| min(1, F / gamma) <= 1e-4 sum |G|.  The remaining
 * sequences are redone by whole-sequence sweeps in the same call.  The compiled 29-state two-copy
 * topology is served the same way (rows of 32 lanes, up to 512 sequences); larger batches and other
 * models with q > 16 use the whole-sequence sweeps throughout.  One stated exception, as for
 * hmm_loglik_grad: dA entries of ABSENT edges (A = 0) weigh the adjoint of states that are improbable
 * where the edge would lead to them; across chunk boundaries that adjoint travels through chunk
 * operators whose eps floors are additive, and with emissions of ~1e-10 on the probable path such an
 * entry can be off by a percent (the whole-sequence sweeps, HMM_OPT_PGCHUNK = 0, have them to 1e-6).
 * The reference never reads them: its A is scattered from per-edge parameters.  hmm_posterior_grad_serial_count() reads, from the workspace of
 * a finished call with the same shape (the caller synchronises first), how many sequences those were.
 */
int hmm_posterior_grad_max_states(void);
size_t hmm_posterior_grad_workspace_bytes(int k, int b, int L, int q);
long long hmm_posterior_grad_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
int hmm_posterior_grad(const float *A, const float *pi, const float *E,
                       int k, int b, int L, int q, float eps, int mode, const float *grad_out,
                       float *dA, float *dpi, float *dE,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same gradient, per chunk of the scan plan, for 1 <= q <= hmm_posterior_grad_scan_max_states() (64): arguments,
 * outputs, modes (HMM_POST_PROB, HMM_POST_LOG) and clamp semantics exactly those of hmm_posterior_grad.
 * hmm_posterior_grad itself evaluates 17..64 states per chunk only for the compiled 29-state topology; every other
 * model of that range walks four whole-sequence sweeps, one workgroup per sequence.  This entry point is the
 * explicit request to run ANY primitive model of 17..64 states per chunk: the reduce and chunk scan of its row
 * width (32 lanes for 17..32 states, 64 for 33..64), the two value sweeps per chunk, every chunk's affine adjoint
 * map, a scan of those maps, and the adjoint sweeps again from the true entering vectors.  Models whose support is
 * not primitive, sequences over the floor-transition certificate (F = eps * sum_t 1 / Sg_t > 2e-6), in log mode
 * sequences whose upstream gradient is exposed to the floors (hmm_posterior_grad's rule above) and sequences a
 * reduce marked are redone by the masked whole-sequence sweeps inside the same call, bit-identical to
 * hmm_posterior_grad under HMM_OPT_PGCHUNK = 0.  The exception stated above for dA entries of absent edges holds
 * here as well.  q <= 16 forwards to hmm_posterior_grad (call, workspace query and serial count alike).
 *   hmm_posterior_grad_scan_chunk_len        the chunk length the call would use (17..64 states: a multiple of 16,
 *                                            <= 512; HMM_OPT_CHUNK forces it); 0 for an unsupported shape
 *   hmm_posterior_grad_scan_pays             1 where the measured rule prefers this call to
 *                                            hmm_posterior_grad; 0 for q <= 16, under HMM_OPT_PGCHUNK = 0, where
 *                                            hmm_posterior_grad already runs per chunk, below 4 chunks, and for
 *                                            every shape the call would refuse
 *   hmm_posterior_grad_scan_workspace_bytes  exactly what the call uses, in 64-bit sizes (three arrays of k*b*L*q
 *                                            floats, the chunk operators and more); 0 for an unsupported shape
 *   hmm_posterior_grad_scan_serial_count     how many sequences of the LAST call with this shape the
 *                                            whole-sequence sweeps served (synchronous copy from the workspace)
 * Unsupported: L * q * 4 >= 2^31 - 4096 (the kernels' 32-bit row offsets) and k * b > 2^24: HMM_ERR_BAD_SHAPE.
 * Options: HMM_OPT_CHUNK, HMM_OPT_EXACT and HMM_OPT_FORCE_DENSE act as for hmm_posterior's 17..64-state plans;
 * HMM_OPT_PGCHUNK = 2 serves every sequence of an eligible model per chunk, without certificate and marks (tests).
 * Runs on `stream` only, no host synchronisation; fixed summation orders (fp32 inside a chunk, fp64 across chunks
 * and sequences): repeated calls are bit-identical.
 * Argument checks, before any HIP call and in hmm_posterior_grad's order: k, b, L or q < 1 -1, q > 64 -2, mode not
 * HMM_POST_PROB / HMM_POST_LOG -6, a NULL A / pi / E / grad_out / dA / dpi / dE / workspace -3, an unsupported shape
 * -1, a small or misaligned (256 bytes) workspace -4.
 */
int hmm_posterior_grad_scan_max_states(void);
int hmm_posterior_grad_scan_chunk_len(int k, int b, int L, int q);
int hmm_posterior_grad_scan_pays(int k, int b, int L, int q);
size_t hmm_posterior_grad_scan_workspace_bytes(int k, int b, int L, int q);
long long hmm_posterior_grad_scan_serial_count(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
int hmm_posterior_grad_scan(const float *A, const float *pi, const float *E,
                            int k, int b, int L, int q, float eps, int mode, const float *grad_out,
                            float *dA, float *dpi, float *dE,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same gradient for any 1 <= q <= hmm_posterior_grad_large_max_states() (4096): arguments, outputs, modes and
 * clamp handling exactly those of hmm_posterior_grad (all four clamps pass nothing: max(E, eps), max(pi, eps), the
 * forward cell's clamp of the predicted state and the backward max(A bh, eps)).  The four sweeps of
 * hmm_posterior_grad run serial in time with the cell's exact step, in one of two evaluations picked by
 * HMM_OPT_GLARGE (0: by q — the walk up to 128 states, the GEMMs above; 1: walk; 2: GEMMs):
 *   walk   one workgroup per sequence, ceil(q/64) waves, lane = state, A staged in LDS; two value sweeps store the
 *          forward and backward vectors with their clamp bits, two adjoint sweeps write dE and sum row i of the
 *          sequence's dA in lane i.  Serves q <= 128: forcing it above returns HMM_ERR_BAD_ARGUMENT.
 *   GEMMs  per position one f32-MFMA GEMM for each of the two value recursions and of the two adjoint recursions,
 *          an elementwise pass per adjoint, and two (q x b)(b x q) products for dA into an fp64 accumulator.
 * The workspace grows with L (both value recursions are kept at every position: three k*b*L*q float arrays and
 * k*b*L normalisers, plus per-sequence q x q partials for the walk or O(k b q) and k q^2 doubles for the GEMMs).
 * Sums run in a fixed order (fp32 within a sequence or a tile, fp64 across sequences and positions): repeated
 * calls return bit-identical results.  Everything runs in order on `stream`.
 * Argument checks, before any HIP call: bad shape -1, q > 4096 -2, mode not HMM_POST_PROB / HMM_POST_LOG -6, a NULL
 * A / pi / E / grad_out / dA / dpi / dE / workspace -3, a small or misaligned (256 bytes) workspace -4, the walk
 * forced above 128 states -6.  workspace_bytes() returns 0 for an unsupported shape or q.
 */
int hmm_posterior_grad_large_max_states(void);
size_t hmm_posterior_grad_large_workspace_bytes(int k, int b, int L, int q);
int hmm_posterior_grad_large(const float *A, const float *pi, const float *E,
                             int k, int b, int L, int q, float eps, int mode, const float *grad_out,
                             float *dA, float *dpi, float *dE,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same gradient for hmm_posterior_grad_walk_min_states() (65) <= q <= hmm_posterior_grad_walk_max_states() (256)
 * states by a PER-SEQUENCE WALK WITH THE SPARSE STEP (hmm_postgradwq.inc): the counterpart of hmm_loglik_grad_walk
 * for a loss on the posteriors of the gene models of 5 to 18 copies.  One workgroup per sequence, lane = state, the
 * four sweeps of hmm_posterior_grad_large as four launches with the step of hmm_posterior_walk's sparse form: every
 * state has at most 8 non-zero predecessors and successors except at most two hub states, decided per model on the
 * device.  Arguments, modes (HMM_POST_PROB, HMM_POST_LOG), derivatives and the handling of all four clamps are
 * exactly those of hmm_posterior_grad_large, with ONE DIFFERENCE IN dA, that of hmm_loglik_grad_walk: every entry
 * with A[i][j] == 0 is written as an exact 0; every entry with A[i][j] != 0 gets the derivative
 * hmm_posterior_grad_large gives.
 * A MODEL OUTSIDE THE SPARSE RULE (more than two states above degree 8) IS REFUSED ON THE DEVICE: every element of
 * its dA, dpi and dE rows is NaN, the other models of the call are served, and
 * hmm_posterior_grad_walk_refused(k, b, L, q, workspace, workspace_bytes) copies from the FINISHED call's workspace
 * how many of the k models were refused (it synchronises; negative: an HMM_ERR_* code).  HMM_OPT_FORCE_DENSE does
 * not act on this call.
 * Workspace: hmm_posterior_grad_walk_workspace_bytes (0: unsupported shape or q), exactly what the call uses: two
 * k*b*L*q float arrays (the value recursions with their clamp bits; the two shares of dE meet in the caller's dE,
 * so there is no third) and per-sequence parts that do not grow with L.  No atomics; sums run in a fixed order
 * (fp32 within a sequence, fp64 across sequences): repeated calls return bit-identical results, whatever the
 * workspace held.  Every offset into E, grad_out, dE and the workspace arrays is 64-bit.  Everything runs in order
 * on `stream`, without host synchronisation: capturable.
 * Argument checks, before any HIP call and in this order: bad shape -1; q < 65 or q > 256 -2; mode not
 * HMM_POST_PROB / HMM_POST_LOG -6; a NULL A / pi / E / grad_out / dA / dpi / dE / workspace -3; a small or misaligned
 * (256 bytes) workspace -4.
 * hmm_posterior_grad_walk_pays(k, b, L, q): 1 only where tools/experiments/posterior_grad_walk_time.py measured this
 * call at least 1.25x faster than hmm_posterior_grad_large at its default route; 0 elsewhere, outside the range and
 * wherever nothing was measured.
 */
int hmm_posterior_grad_walk_min_states(void);
int hmm_posterior_grad_walk_max_states(void);
size_t hmm_posterior_grad_walk_workspace_bytes(int k, int b, int L, int q);
int hmm_posterior_grad_walk_pays(int k, int b, int L, int q);
long long hmm_posterior_grad_walk_refused(int k, int b, int L, int q, const void *workspace, size_t workspace_bytes);
int hmm_posterior_grad_walk(const float *A, const float *pi, const float *E,
                            int k, int b, int L, int q, float eps, int mode, const float *grad_out,
                            float *dA, float *dpi, float *dE,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * CLASS POSTERIORS WITH ANALYTIC GRADIENTS for 65 <= q <= 256 states: the trainable counterpart of
 * hmm_posterior_decode_wide.  A model whose states are labelled by class (state_class: HOST pointer to q ints in
 * 0..num_classes-1, REQUIRED; num_classes 1..16) is trained on P_c[t] = sum over the states j of class c of gamma_t[j];
 * no gamma output tensor (k,b,L,q) is written and no upstream gradient of that size is read.  (The forward's workspace
 * still holds a parking region of k*b*L*q floats, below, and the backward's its two arrays of that size.)
 *
 * hmm_class_posterior_walk: the walk of hmm_posterior_walk (same step selection per model, clamp semantics and
 * HMM_OPT_FORCE_DENSE) with a third output policy beside hmm_posterior_decode_wide's: the same staging, masks and
 * class-sum loop (the fp32 sum of the gamma row over ALL states in increasing index with weights 0 / 1), so the sums
 * have the bits hmm_posterior_decode_wide compares — with the same table, out_prob at label is conf and the lowest
 * argmax of out_prob is label.  out_prob (k,b,L,num_classes) gets the sums, out_log (same shape) their logs, within
 * 2 fp32 ulp of log(out_prob) (the fp64 log rounded once; a sum of 0, e.g. an empty class, gives -inf); either may be
 * NULL, not both.  loglik (k,b) fp64 or NULL is bit for bit
 * hmm_posterior_walk's.  The table reaches the kernels by value: a captured graph keeps its table.
 * Workspace: hmm_class_posterior_walk_workspace_bytes = hmm_posterior_decode_wide_workspace_bytes, the PARKING REGION
 * of k*b*L*q floats included, under the same stated contract.  Every element of the outputs given is written; no
 * atomics; repeated calls are bit-identical; every offset is 64-bit; the call runs on `stream` alone (capturable).
 * Argument checks, before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), q < 65 or q > 256
 * (HMM_ERR_Q_UNSUPPORTED), NULL among A, pi, E, state_class, workspace, or both outputs NULL (HMM_ERR_NULL_POINTER),
 * num_classes outside 1..16 or a table entry outside 0..num_classes-1 (HMM_ERR_BAD_ARGUMENT), workspace too small or
 * not 256-byte aligned (HMM_ERR_WORKSPACE).
 *
 * hmm_class_posterior_grad_walk: gradients of a loss on the class posteriors -> dA (k,q,q), dpi (k,q), dE (k,b,L,q),
 * with grad_out (k,b,L,num_classes) the upstream gradient Gc:
 *   HMM_POST_PROB   loss = sum Gc P: hmm_posterior_grad_walk(HMM_POST_PROB) with G[t][j] = Gc[t][class(j)], bit for
 *                   bit.  Gc is read in place: every lane finds its class once and loads Gc[t][class] where the state
 *                   form loads G[t][j].  class_prob is ignored.
 *   HMM_POST_LOG    loss = sum Gc log P.  d loss / d gamma_j = Gc[class(j)] / P[class(j)], so this IS the prob-mode
 *                   adjoint with G'[t][c] = Gc[t][c] / P_c[t], the IEEE fp32 quotient, and G' = 0 where P_c == 0 (an
 *                   empty or exactly-zero class passes nothing).  class_prob (k,b,L,num_classes), REQUIRED, is the
 *                   forward's out_prob; a pre-pass writes G' into the workspace and the adjoints run in prob mode.
 * Everything else is hmm_posterior_grad_walk's: the four sweeps, the edge owners, the fp64 sums over sequences, dA an
 * exact 0 wherever A == 0, refusal of a model outside the sparse rule by NaN in its outputs, no atomics, 64-bit
 * offsets, bit-identical repetition, one stream, capturable.
 * Workspace: hmm_class_posterior_grad_walk_workspace_bytes(k, b, L, q, num_classes) (0: unsupported shape, q or
 * num_classes) = hmm_posterior_grad_walk's layout first, rounded up to 256 bytes, then G' (k*b*L*num_classes floats).
 * hmm_posterior_grad_walk_refused(k, b, L, q, workspace, workspace_bytes) THEREFORE READS THE COUNTER OF A FINISHED
 * hmm_class_posterior_grad_walk CALL as it does hmm_posterior_grad_walk's.
 * Argument checks, before any HIP call and in this order: bad shape -1; q < 65 or q > 256 -2; mode not HMM_POST_PROB /
 * HMM_POST_LOG -6; a NULL A / pi / E / state_class / grad_out / dA / dpi / dE / workspace, or class_prob in
 * HMM_POST_LOG, -3; num_classes outside 1..16 or a table entry outside 0..num_classes-1 -6; a small or misaligned
 * (256 bytes) workspace -4.
 *
 * hmm_class_posterior_walk_pays(k, b, L, q): 1 only where tools/experiments/class_posterior_walk_time.py measured the
 * fused node (both calls) at least 1.25x faster than autograd through hmm_posterior_grad_walk and torch ops over the
 * (k,b,L,q) tensor; 0 elsewhere, outside the range and wherever nothing was measured.  As measured on
 * one MI355X (L = 10 000, 6 classes, log mode): 1 for one model (k = 1) of 71, 127 or 253 states with b = 1024
 * sequences, whatever L (L does not enter, as in hmm_posterior_grad_walk_pays); 0 for every other (k, b, q).
 */
size_t hmm_class_posterior_walk_workspace_bytes(int k, int b, int L, int q);
int hmm_class_posterior_walk_pays(int k, int b, int L, int q);
int hmm_class_posterior_walk(const float *A, const float *pi, const float *E,
                             int k, int b, int L, int q, float eps,
                             const int *state_class, int num_classes,
                             float *out_prob, float *out_log, double *loglik,
                             void *workspace, size_t workspace_bytes, void *stream);
size_t hmm_class_posterior_grad_walk_workspace_bytes(int k, int b, int L, int q, int num_classes);
int hmm_class_posterior_grad_walk(const float *A, const float *pi, const float *E,
                                  int k, int b, int L, int q, float eps, int mode,
                                  const int *state_class, int num_classes, const float *class_prob,
                                  const float *grad_out, float *dA, float *dpi, float *dE,
                                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * CLASS POSTERIORS WITH ANALYTIC GRADIENTS for q <= 16 states: the trainable counterpart of hmm_posterior_decode, with
 * the arguments of the 65..256-state pair above, so that a caller switches by q alone.  THIS PAIR SERVES q <= 16 ONLY:
 * 65..256 states go to hmm_class_posterior_walk / hmm_class_posterior_grad_walk; 17..64 states have no fused class
 * call yet (it needs hmm_posterior_decode_mid's parking region and is a follow-up) and are composed from hmm_posterior /
 * hmm_posterior_grad_scan by the caller.  state_class: HOST pointer to q ints in 0..num_classes-1, REQUIRED (the
 * identity map is hmm_posterior); num_classes 1..16, may exceed q; a class may be empty.
 *
 * hmm_class_posterior: the pipeline and routing of hmm_posterior(HMM_POST_PROB) and hmm_posterior_decode (chunked
 * kernels, windows, exact serial kernels) with a third output policy: the same staging, the same 0/1 weight table by
 * value and the same class-sum loop (fp32 fma(v, w, sum) over the states in increasing index, from 0.0f), so out_prob
 * (k,b,L,num_classes) has the bits hmm_posterior_decode compares: out_prob at label is conf, and the lowest argmax of
 * out_prob is label.  out_log (same shape) is within 2 fp32 ulp of log(out_prob) — the fp64 log rounded once, formed by
 * an elementwise kernel inside the same call — and -inf for a sum of 0.  Either output may be NULL, not both; every
 * element of an output given is written.  loglik (k,b) fp64 or NULL is bit for bit hmm_posterior's.
 * Workspace: hmm_class_posterior_workspace_bytes = hmm_workspace_bytes(HMM_OP_POSTERIOR, ...) (0: unsupported shape or
 * q); there is no parking region, and hmm_exact_count(HMM_OP_POSTERIOR, ...) reads the routing of a finished call.
 * One stream, capturable (the table travels by value: a captured graph keeps its table), no atomics, 64-bit offsets
 * into E and the outputs, bit-identical repetition.
 * Argument checks, before any HIP call, in this order: shape (HMM_ERR_BAD_SHAPE), q > 16 (HMM_ERR_Q_UNSUPPORTED), NULL
 * among A, pi, E, state_class, workspace, or both outputs NULL (HMM_ERR_NULL_POINTER), num_classes outside 1..16 or a
 * table entry outside 0..num_classes-1 (HMM_ERR_BAD_ARGUMENT), workspace too small or not 256-byte aligned
 * (HMM_ERR_WORKSPACE).
 *
 * hmm_class_posterior_grad: gradients of a loss on the class posteriors -> dA (k,q,q), dpi (k,q), dE (k,b,L,q), with
 * grad_out (k,b,L,num_classes) the upstream gradient Gc:
 *   HMM_POST_PROB   loss = sum Gc P: hmm_posterior_grad(HMM_POST_PROB) with G[t][j] = Gc[t][class(j)], bit for bit.
 *                   Gc is read in place: every lane finds its class once and loads Gc[t][class] where the state form
 *                   loads G[t][j].  class_prob is ignored.
 *   HMM_POST_LOG    loss = sum Gc log P: the prob-mode adjoint with G'[t][c] = Gc[t][c] / P_c[t], the IEEE fp32
 *                   quotient, and G' = 0 where P_c == 0.  class_prob (k,b,L,num_classes), REQUIRED, is the forward's
 *                   out_prob; a pre-pass writes G' into the workspace and the adjoints run in prob mode.
 * Routing to the whole-sequence sweeps is hmm_posterior_grad's (model support, F <= 2e-6, HMM_OPT_PGCHUNK); log mode adds
 * the class form of the exposed-weight rule: a sequence is redone whole when
 *   F sum_{P_c >= 1e-8} |Gc| / P_c + sum_{P_c < 1e-8} |Gc|  >  1e-4 sum |Gc|.
 * q = 1 gives exact zeros.  No atomics, 64-bit offsets, bit-identical repetition, one stream, capturable.
 * Workspace: hmm_class_posterior_grad_workspace_bytes(k, b, L, q, num_classes) (0: unsupported shape, q or
 * num_classes) = hmm_posterior_grad's layout first, rounded up to 256 bytes, then G' and the rule's per-sequence sums.
 * hmm_posterior_grad_serial_count(k, b, L, q, workspace, workspace_bytes) THEREFORE READS A FINISHED
 * hmm_class_posterior_grad CALL as it does hmm_posterior_grad's.
 * Argument checks, before any HIP call and in this order: bad shape -1; q > 16 -2; mode not HMM_POST_PROB /
 * HMM_POST_LOG -6; a NULL A / pi / E / state_class / grad_out / dA / dpi / dE / workspace, or class_prob in
 * HMM_POST_LOG, -3; num_classes outside 1..16 or a table entry outside 0..num_classes-1 -6; a small or misaligned
 * (256 bytes) workspace -4.
 *
 * hmm_class_posterior_pays / hmm_class_posterior_grad_pays (k, b, L, q): 1 exactly on the cells
 * tools/experiments/class_posterior_time.py measured at least 1.25x ahead — the forward alone against hmm_posterior +
 * the torch collapse + log, and the fused autograd node (both calls) against the composed one — as recorded in
 * profiles/class_posterior.json; 0 everywhere else, everything not measured included.  As measured on
 * one MI355X (one model, log mode, a label-style gradient with labels uniform over the classes; 7 states with 4
 * classes and 15 states with 5; b x L = 1 x 100 000, 32 x 9 999, 1024 x 10 000, 1024 x 100 000): the forward is 1.39x
 * to 4.79x ahead in all eight cells, which are exactly where hmm_class_posterior_pays is 1 (k = 1; q, b and L as
 * measured); the node is 0.02x to 1.03x — such labels sit on improbable classes and the log rule above redoes their
 * sequences whole, which the composed node's prob-mode state call never does — so hmm_class_posterior_grad_pays is 0
 * everywhere.  Not measured: prob mode, dense gradients, other class counts, b > 1024, k > 1.
 */
int hmm_class_posterior_max_states(void);                       /* 16 */
size_t hmm_class_posterior_workspace_bytes(int k, int b, int L, int q);
int hmm_class_posterior_pays(int k, int b, int L, int q);
int hmm_class_posterior(const float *A, const float *pi, const float *E,
                        int k, int b, int L, int q, float eps,
                        const int *state_class, int num_classes,
                        float *out_prob, float *out_log, double *loglik,
                        void *workspace, size_t workspace_bytes, void *stream);
size_t hmm_class_posterior_grad_workspace_bytes(int k, int b, int L, int q, int num_classes);
int hmm_class_posterior_grad_pays(int k, int b, int L, int q);
int hmm_class_posterior_grad(const float *A, const float *pi, const float *E,
                             int k, int b, int L, int q, float eps, int mode,
                             const int *state_class, int num_classes, const float *class_prob,
                             const float *grad_out, float *dA, float *dpi, float *dE,
                             void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HMM_ENGINE_H */
